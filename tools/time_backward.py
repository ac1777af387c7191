"""Backward tracking timing at the benchmark's size (C3: 4 views x 24 frames x 512x512, 1024 queries, bf16, 4 iterations) with
query frames spread uniformly over the clip:

  (a) forward alone,
  (b) the host composition a user of plain ``forward`` can do: the clip and the time-flipped clip (flipped copies made inside the
      timed call, as a caller would have to), merged on the device,
  (c) forward(backward_tracking=True): one frame store, a time-reversed second window loop.

    python tools/time_backward.py [--out profiles/r06_backward.json] [--reps 15] [--only a|b|c]

Every figure is the median over --reps timed calls (each synchronised on its own, after two warm-up calls), with the min / max
(the protocol of tools/time_grouped.py).  --only times one line alone (e.g. under rocprofv3 --kernel-trace --stats).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvtracker_amd import synth  # noqa: E402
from mvtracker_amd.backward import reversed_layout  # noqa: E402
from mvtracker_amd.tracker import MVTracker  # noqa: E402
from time_grouped import fmt, rec, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--only", choices=["a", "b", "c"], default=None)
    args = ap.parse_args()
    m = MVTracker(hidden_size=256).eval()
    sd = synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.to("cuda")
    m.precision = "bf16"
    V, T, H, W, N = 4, 24, 512, 512, 1024
    clip = synth.make_clip(1234, V=V, T=T, H=H, W=W, N=N)
    clip["query_points"][0, :, 0] = np.random.default_rng(0).integers(0, T, size=N).astype(np.float32)
    a = [torch.from_numpy(clip[k]).cuda() for k in ("rgbs", "depths", "query_points", "intrs", "extrs")]
    qt = a[2][0, :, 0].long()
    lay = reversed_layout(qt.cpu().numpy(), m.S, T)
    reached = torch.zeros(N, dtype=torch.bool)
    reached[torch.from_numpy(lay["order"][:lay["active"]])] = True
    take = ((torch.arange(T, device="cuda")[:, None] < qt[None, :]) & reached.cuda()[None, :])[None]

    def forward():
        return m(*a, iters=4)

    def composition():
        rf = m(*a, iters=4)
        tf, vf = rf["traj_e"], rf["vis_e"]
        q = a[2].clone()
        q[0, :, 0] = (T - 1 - qt).float()
        rb = m(a[0].flip(2), a[1].flip(2), q, a[3].flip(2), a[4].flip(2), iters=4)
        return torch.where(take[..., None], rb["traj_e"].flip(1), tf), torch.where(take, rb["vis_e"].flip(1), vf)

    def backward():
        return m(*a, iters=4, backward_tracking=True)

    lines = dict(a=("forward alone", forward), b=("two forward calls (clip, flipped clip) merged on the host side", composition),
                 c=("forward(backward_tracking=True)", backward))
    res = dict(shape=f"{V} views x {T} frames x {H}x{W}, {N} queries at uniformly drawn frames, bf16, 4 iterations", reps=args.reps,
               statistic="median [min, max] of single synchronised calls, ms", reversed_windows=lay["windows"], lines={})
    for key in ([args.only] if args.only else ["a", "b", "c"]):
        name, fn = lines[key]
        t = timed(fn, args.reps)
        res["lines"][key] = dict(what=name, **rec(t))
        print(f"({key}) {name}: {fmt(t)}", flush=True)
    if args.out and not args.only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
