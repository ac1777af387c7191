"""Streaming session timing and memory at the benchmark's size (C3: 4 views x 512x512, 1024 queries, bf16, 4 iterations), blocks of
S/2 = 6 frames, at T = 24 and T = 96 frames:

  * per-``push`` latency (every push synchronised on its own): median, min, max over the pushes of --reps sessions,
  * the sum over the clip (pushes + finish) beside one ``forward`` call on the whole clip,
  * ``torch.cuda.max_memory_allocated`` of a session and of ``forward``.  The inputs live on the HOST and go to the device block by
    block (session) or whole (forward), so the session's peak holds one block of input, the ring and the chunks it returned.

    python tools/time_streaming.py [--out profiles/r07_streaming.json] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvtracker_amd import synth  # noqa: E402
from mvtracker_amd.tracker import MVTracker  # noqa: E402

KEYS = ("rgbs", "depths", "intrs", "extrs")


def session(m, host, q, block):
    """One session over the host clip; returns (per-push ms, finish ms, the chunks)."""
    T = host["rgbs"].shape[2]
    st = m.open_stream(q, iters=4)
    ts, outs = [], []
    for t in range(0, T, block):
        blk = [host[k][:, :, t:t + block].cuda() for k in KEYS]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs.append(st.push(*blk))
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    outs.append(st.finish())
    torch.cuda.synchronize()
    return ts, (time.perf_counter() - t0) * 1e3, outs


def forward(m, host, q):
    a = {k: host[k].cuda() for k in KEYS}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = m(a["rgbs"], a["depths"], q, a["intrs"], a["extrs"], iters=4)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    p = torch.cuda.max_memory_allocated()
    del out
    return dict(peak_bytes=p, held_before_bytes=base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    m = MVTracker(hidden_size=256).eval()
    sd = synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.to("cuda")
    m.precision = "bf16"
    V, H, W, N = 4, 512, 512, 1024
    block = m.S // 2
    res = dict(shape=f"{V} views x 512x512, {N} queries at frame 0, bf16, 4 iterations, blocks of {block} frames", reps=args.reps,
               statistic="per push: median [min, max] over every push of every repetition, each synchronised on its own, ms; inputs uploaded "
                         "outside the timed region", clips={})
    for T in (24, 96):
        clip = synth.make_clip(1234, V=V, T=T, H=H, W=W, N=N, frame_period=24 if T > 24 else None, rgb_dtype=np.uint8)
        host = {k: torch.from_numpy(clip[k]) for k in KEYS}
        q = torch.from_numpy(clip["query_points"]).cuda()
        for _ in range(2):  # warm-up: weight packing, workspaces, allocator
            session(m, host, q, block)
            forward(m, host, q)
        pushes, totals, fwd = [], [], []
        for _ in range(args.reps):
            ts, tf, _ = session(m, host, q, block)
            pushes += ts
            totals.append(sum(ts) + tf)
            fwd.append(forward(m, host, q)[0])
        mem_s = peak(lambda: session(m, host, q, block)[2])
        mem_f = peak(lambda: forward(m, host, q)[1])
        r = dict(frames=T, pushes_per_session=len(pushes) // args.reps,
                 push_ms=dict(median=round(statistics.median(pushes), 3), min=round(min(pushes), 3), max=round(max(pushes), 3)),
                 session_total_ms=dict(median=round(statistics.median(totals), 3), min=round(min(totals), 3), max=round(max(totals), 3)),
                 forward_ms=dict(median=round(statistics.median(fwd), 3), min=round(min(fwd), 3), max=round(max(fwd), 3)),
                 session_memory=mem_s, forward_memory=mem_f)
        res["clips"][f"T{T}"] = r
        print(f"T = {T}: push {r['push_ms']}, session total {r['session_total_ms']}, forward {r['forward_ms']}; peak memory session "
              f"{mem_s['peak_bytes'] / 2**20:.0f} MiB (held before: {mem_s['held_before_bytes'] / 2**20:.0f}), forward "
              f"{mem_f['peak_bytes'] / 2**20:.0f} MiB", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
