"""Depth cleaning timing at the workload's own sizes: 4 views x 24 frames at 384x512 and at 512x512, statistical (k = 20, std_ratio 2)
and radius (r = 0.05, min_points 5) mode.  ``clean_depths`` on a clip that is on the device, timed with device events after 2 warm-ups:
median [min, max] of --reps calls, ms per clip and per (view, frame) cloud; and the search launch alone on one chunk of clouds.
With --cpu N, scipy.spatial.cKDTree does the same neighbour search (k nearest / radius count, up to 16 threads) on N of the same clouds on
this host: a CPU baseline for the search and nothing more.

    python tools/time_depth_cleaning.py [--out profiles/r10_depth_cleaning.json] [--reps 5] [--cpu 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvtracker_amd import DepthCleaning, clean, clean_depths, hip, synth  # noqa: E402

V, T = 4, 24
WORKERS = min(16, os.cpu_count() or 1)  # threads of the CPU baseline


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def stat(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu", type=int, default=0, metavar="N", help="clouds to time scipy's cKDTree on (0: skip)")
    args = ap.parse_args()
    modes = {"statistical_k20": DepthCleaning("statistical", nb_neighbors=20, std_ratio=2.0),
             "radius_r0.05_min5": DepthCleaning("radius", radius=0.05, min_points=5)}
    res = dict(views=V, frames=T, reps=args.reps, statistic="median [min, max] of device-event times after 2 warm-ups, ms", configs={})
    for name, (H, W) in {"384x512": (384, 512), "512x512": (512, 512)}.items():
        # (two rendered frames repeated: the clouds' content, not their number, is what repeats)
        clip = synth.make_clip(1234, V=V, T=T, H=H, W=W, N=4, invalid_frac=0.02, frame_period=2)
        depths, intrs, extrs = (torch.from_numpy(clip[k]).cuda() for k in ("depths", "intrs", "extrs"))
        r = dict(height=H, width=W, clouds=V * T, points_per_cloud=H * W)
        for mname, c in modes.items():
            t_clip, keep = [], None
            for rep in range(args.reps + 2):
                ms, (_, keep) = event_ms(lambda: clean_depths(depths, intrs, extrs, c))
                if rep >= 2:
                    t_clip.append(ms)
            valid = int((depths > 0).sum())
            removed = int((~keep & (depths > 0)).sum())
            # the search launch alone, on the first chunk of frames
            nt = max(1, min(T, clean.MAX_CHUNK_POINTS // (V * H * W)))
            kinv, einv = torch.empty(V * T, 9, device="cuda"), torch.empty(V * T, 12, device="cuda")
            hip.invert_cameras(intrs[0].reshape(-1, 9).contiguous(), extrs[0].reshape(-1, 12).contiguous(), kinv, einv, V * T)
            P, C = H * W, V * nt
            xyz = torch.empty(C, P, 4, device="cuda")
            hip.clean_points(depths[0].contiguous(), None, kinv, einv, V, T, 0, nt, H, W, None, None, xyz)
            ntile = (P + 63) // 64
            box, gbox = torch.empty(C, ntile, 8, device="cuda"), torch.empty(C, (ntile + 63) // 64, 8, device="cuda")
            hip.tile_aabb(xyz, P, C, box, (W, H))
            hip.tile_group_aabb(box, P, C, gbox)
            stat_mode = c.mode == hip.CLEAN_STATISTICAL
            vals = torch.empty(C, P, device="cuda", dtype=torch.float32 if stat_mode else torch.int32)
            t_search = []
            for rep in range(args.reps + 2):
                ms, _ = event_ms(lambda: hip.clean_search(xyz, C, P, (W, H), c.mode, c.nb_neighbors, c.radius, c.min_points, box, gbox,
                                                          a_out=vals if stat_mode else None, c_out=None if stat_mode else vals))
                if rep >= 2:
                    t_search.append(ms)
            m = dict(clip_ms=stat(t_clip), per_cloud_ms=round(statistics.median(t_clip) / (V * T), 4), valid_pixels=valid, removed=removed,
                     search_clouds=C, search_ms=stat(t_search), search_per_cloud_ms=round(statistics.median(t_search) / C, 4))
            if args.cpu > 0:
                try:
                    from scipy.spatial import cKDTree
                    t_cpu = []
                    for ci in range(min(args.cpu, C)):
                        x = xyz[ci, :, :3].cpu().numpy().astype(np.float64)
                        x = x[np.isfinite(x).all(1)]
                        t0 = time.perf_counter()
                        tree = cKDTree(x)
                        if stat_mode:
                            tree.query(x, k=c.nb_neighbors, workers=WORKERS)
                        else:
                            tree.query_ball_point(x, c.radius, return_length=True, workers=WORKERS)
                        t_cpu.append((time.perf_counter() - t0) * 1e3)
                    m["cpu_ckdtree_per_cloud_ms"] = stat(t_cpu)  # a CPU baseline on this host (build + query, up to 16 threads), nothing more
                except ImportError:
                    m["cpu_ckdtree_per_cloud_ms"] = None  # not measured: scipy is not importable here
            r[mname] = m
            print(name, mname, json.dumps(m), flush=True)
        res["configs"][name] = r
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
