"""Grouped forward timing: single_point evaluation (shape of tools/time_single_point.py: 32 queries, 4 views x 24 frames x 384x512,
bf16) at single_point_group_size G in {1, 4, 8, 16, 32}, and one grouped updater call against G separate calls.

    python tools/time_grouped.py [--out profiles/r05_single_point_grouped.json] [--reps 15] [--only G]

Every figure is the median over --reps timed calls (each synchronised on its own, after two warm-up calls), with the min / max.
--only G times the single_point call at that G alone (e.g. under rocprofv3 --kernel-trace --stats).
"""
import argparse
import json
import os
import sys
import statistics
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvtracker_amd import synth  # noqa: E402
from mvtracker_amd.predictor import EvaluationPredictor  # noqa: E402
from mvtracker_amd.tracker import MVTracker  # noqa: E402


def timed(fn, reps):
    """(median, min, max) ms of one call, over ``reps`` calls each synchronised on its own."""
    fn()
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def fmt(t):
    return f"{t[0]:7.2f} ms [{t[1]:.2f}, {t[2]:.2f}]"


def rec(t):
    return dict(median=round(t[0], 3), min=round(t[1], 3), max=round(t[2], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--only", type=int, default=0)
    ap.add_argument("--queries", type=int, default=32)
    args = ap.parse_args()
    m = MVTracker(hidden_size=256).eval()
    sd = synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.to("cuda")
    m.precision = "bf16"
    nq = args.queries
    clip = synth.make_clip(5, V=4, T=24, H=384, W=512, N=nq)
    a = {k: torch.from_numpy(v).cuda() for k, v in clip.items()}
    pred = EvaluationPredictor(m, interp_shape=None, single_point=True, n_iters=4)
    res = dict(shape="single_point, 4 views x 24 frames x 384x512, bf16, n_iters 4", queries=nq, reps=args.reps,
               statistic="median [min, max] of single synchronised calls, ms", single_point_ms={}, updater={})
    for G in ((args.only,) if args.only else (1, 4, 8, 16, 32)):
        pred.single_point_group_size = G
        t = timed(lambda: pred(rgbs=a["rgbs"], depths=a["depths"], query_points_3d=a["query_points"], intrs=a["intrs"],
                               extrs=a["extrs"]), args.reps)
        res["single_point_ms"][str(G)] = rec(t)
        print(f"single_point G={G:2d}: {fmt(t)} per call", flush=True)
    if args.only:
        return
    # one grouped updater call (G sets of 357 tracks: one query, its local grids, the global support) against G calls
    n = 357
    for G in (1, 4, 8, 32):
        xs = [torch.randn(1, n, m.S, m.updateformer_input_dim, device="cuda") for _ in range(G)]
        sep = timed(lambda: [m.update_former(x) for x in xs], args.reps)
        grp = timed(lambda: m.update_former_grouped(xs), args.reps)
        res["updater"][str(G)] = dict(tracks_per_set=n, separate_ms=rec(sep), grouped_ms=rec(grp))
        print(f"updater G={G:2d} x {n}: separate {fmt(sep)}, grouped {fmt(grp)}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
