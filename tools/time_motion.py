"""Motion mask timing with device events: ``motion_masks`` at the bench clip's shape (4 views x 24 frames x 512 x 512) on uint8 and
float32 frames, window -1 and 2, patch radius 0 and 7, and its three launches on their own.  Median [min, max] of --reps calls after
2 warm-ups; the frames are on the device and every timed window ends in a recorded event that is synchronised on (``motion_masks``'
window includes its one small host read).  Next to the milliseconds: the bytes the design must move ("Motion
masks": the frames read once, the change or diff maps written and read once, the mask written) and the GB/s that makes.

    python tools/time_motion.py [--out profiles/motion.json] [--reps 9]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvtracker_amd import hip, motion  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stat(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def model_bytes(V, T, H, W, esz, all_mode):
    """The bytes of the design: frames read once, the temporal pass's map(s) written and read once, the mask written."""
    maps = V * (1 if all_mode else T - 1) * H * W * 4
    return dict(frames=V * T * 3 * H * W * esz, map_written=maps, map_read=maps, mask=V * T * H * W)


def make_frames(V, T, H, W, seed):
    """uint8: a fixed image per view, 2 % of the pixels redrawn in every frame and a block that moves 4 pixels per frame."""
    rng = np.random.default_rng(seed)
    f = np.repeat(rng.integers(0, 256, (V, 1, 3, H, W), dtype=np.uint8), T, 1)
    for t in range(T):
        hit = rng.random((V, 1, H, W)) < 0.02
        f[:, t] = np.where(hit, rng.integers(0, 256, (V, 3, H, W), dtype=np.uint8), f[:, t])
        f[:, t, :, 100:164, 40 + 4 * t:104 + 4 * t] = 250
    return f


def stages(frames, cfg, iters):
    """The launch sequence of motion_clip, each launch ``iters`` times back to back in its own event window (a single launch is
    tens of microseconds: too short for one window); milliseconds per launch."""
    V, T, _, H, W = frames.shape
    dev = frames.device
    all_mode = cfg.window == -1 or cfg.window >= T - 1
    diff = torch.empty(V, 1 if all_mode else T - 1, H, W, device=dev)
    partial = torch.empty(V * hip.motion_blocks(H, W), T - 1, device=dev, dtype=torch.float64)
    counts = torch.empty(V * (1 if all_mode else T), hip.motion_tiles(H, W), device=dev, dtype=torch.int32)
    static = torch.empty(V, T, H, W, device=dev, dtype=torch.bool)
    rep = torch.empty(T - 1 + V * T, device=dev, dtype=torch.float64)
    launches = dict(
        temporal=lambda: hip.motion_temporal(frames, V, T, H, W, all_mode, diff, partial),
        mask=lambda: hip.motion_mask(diff, V, T, H, W, 0 if all_mode else cfg.window, cfg.patch_radius, cfg.diff_thresh, static, counts),
        report=lambda: hip.motion_report(partial, counts, V, T, H, W, all_mode, rep))
    return {k: timed(lambda: [fn() for _ in range(iters)])[0] / iters for k, fn in launches.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20, help="back-to-back launches per timed window of a single launch")
    ap.add_argument("--shape", type=int, nargs=4, default=[4, 24, 512, 512], metavar=("V", "T", "H", "W"))
    args = ap.parse_args()
    V, T, H, W = args.shape
    res = dict(shape=[V, T, H, W], reps=args.reps,
               statistic=f"median [min, max] of device-event windows after 2 warm-ups, ms; single launches: per launch, {args.iters} back to back "
                         "per window; the frames are on the device", configurations={})
    u8 = torch.from_numpy(make_frames(V, T, H, W, 1)).cuda()
    for name, frames in (("uint8", u8), ("float32", u8.float())):
        for window in (-1, 2):
            for r in (0, 7):
                cfg = motion.MotionMask(window, r, 10.0)
                t = {k: [] for k in ("motion_masks", "temporal", "mask", "report")}
                report = None
                for rep in range(args.reps + 2):
                    row = stages(frames, cfg, args.iters)
                    row["motion_masks"], (_, report) = timed(lambda: motion.motion_masks(frames, cfg))
                    if rep >= 2:
                        for k, v in row.items():
                            t[k].append(v)
                b = model_bytes(V, T, H, W, frames.element_size(), window == -1)
                total = sum(b.values())
                launches = statistics.median([x + y + z for x, y, z in zip(t["temporal"], t["mask"], t["report"])])
                r_ = dict(frames=name, window=window, patch_radius=r, static_fraction=round(float(report.static_fraction.mean()), 4), model_bytes=b,
                          model_megabytes=round(total / 1e6, 1), launches_ms=round(launches, 4), launches_gb_per_s=round(total / launches / 1e6, 1),
                          temporal_gb_per_s=round((b["frames"] + b["map_written"]) / statistics.median(t["temporal"]) / 1e6, 1),
                          mask_gb_per_s=round((b["map_read"] + b["mask"]) / statistics.median(t["mask"]) / 1e6, 1),
                          **{k + "_ms": stat(v) for k, v in t.items()})
                res["configurations"][f"{name}_w{window}_r{r}"] = r_
                print(json.dumps(r_), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
