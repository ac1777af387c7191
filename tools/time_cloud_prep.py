"""Cloud preparation timing on one organised 384 x 512 cloud (a synthetic clip's depth map, unprojected) and on a 1 M-point list (a
bumpy sheet sampled 1024 x 1024, in raster order, passed as an unorganised list): the normals launch ``mvt_normals_estimate`` at
max_nn 30, beside it ``mvt_clean_search`` statistical K = 20 on the same cloud and boxes (the existing self-search: the comparator),
and the three voxel entries, each alone.  HIP events, warm (2 warm-ups, then median [min, max] of --reps calls).

    python tools/time_cloud_prep.py [--out profiles/cloud_prep.json] [--reps 10]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvtracker_amd import hip, synth  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stat(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def organised_cloud(H=384, W=512):
    clip = synth.make_clip(1234, V=1, T=1, H=H, W=W, N=4, invalid_frac=0.02, frame_period=1)
    depths, intrs, extrs = (torch.from_numpy(clip[k]).cuda()[0] for k in ("depths", "intrs", "extrs"))
    kinv, einv = torch.empty(1, 9, device="cuda"), torch.empty(1, 12, device="cuda")
    hip.invert_cameras(intrs.float().reshape(1, 9).contiguous(), extrs.float().reshape(1, 12).contiguous(), kinv, einv, 1)
    xyz = torch.empty(1, H * W, 4, device="cuda")
    hip.clean_points(depths.float().contiguous(), None, kinv, einv, 1, 1, 0, 1, H, W, None, None, xyz)
    return xyz, (W, H)


def sheet_list(n=1024):
    ys, xs = np.meshgrid(np.arange(n) * (10.0 / n), np.arange(n) * (10.0 / n), indexing="ij")
    z = 0.4 * np.sin(1.3 * xs) * np.cos(0.9 * ys) + 0.05 * np.sin(11.0 * xs + 7.0 * ys)
    pts = np.zeros((1, n * n, 4), np.float32)
    pts[0, :, :3] = np.stack([xs, ys, z], -1).reshape(-1, 3)
    return torch.from_numpy(pts).cuda(), (0, 0)


def measure(xyz, grid, radius, voxel, reps):
    P = xyz.shape[1]
    nt = (P + 63) // 64
    box, gbox = torch.empty(1, nt, 8, device="cuda"), torch.empty(1, (nt + 63) // 64, 8, device="cuda")
    hip.tile_aabb(xyz, P, 1, box, grid)
    hip.tile_group_aabb(box, P, 1, gbox)
    nrm, a_out = torch.empty(1, P, 4, device="cuda"), torch.empty(1, P, device="cuda")
    cap = hip.voxel_capacity(P)
    state = torch.zeros(hip.VOXEL_STATE_WORDS, dtype=torch.int64, device="cuda")
    partial = torch.empty(hip.VOXEL_BOUND_BLOCKS * 4, dtype=torch.float64, device="cuda")
    table = torch.empty(cap * hip.VOXEL_SLOT_WORDS, dtype=torch.int64, device="cuda")
    blocks = torch.empty((P + 255) // 256, dtype=torch.int32, device="cuda")
    out = torch.empty(P, 4, device="cuda")
    counts, first, labels, n_out = (torch.empty(n, dtype=torch.int32, device="cuda") for n in (P, P, P, 1))
    steps = {"normals_max_nn30": lambda: hip.normals_estimate(xyz, 1, P, grid, 30, radius, box, gbox, nrm),
             "clean_search_k20": lambda: hip.clean_search(xyz, 1, P, grid, hip.CLEAN_STATISTICAL, 20, 0.0, 0, box, gbox, a_out=a_out),
             "voxel_bounds": lambda: hip.voxel_bounds(xyz[0], P, voxel, partial, state),
             "voxel_insert": lambda: hip.voxel_insert(xyz[0], P, state, table, cap),
             "voxel_emit": lambda: hip.voxel_emit(xyz[0], P, state, table, cap, blocks, out, counts, first, n_out, labels)}
    t = {k: [] for k in steps}
    for rep in range(reps + 2):
        for k, fn in steps.items():
            ms = timed(fn)
            if rep >= 2:
                t[k].append(ms)
    return dict(points=P, valid=int(torch.isfinite(xyz[0, :, 0]).sum()), normals=int(torch.isfinite(nrm[0, :, 0]).sum()), radius=radius, voxel=voxel,
                voxels=int(n_out[0]), status=int(state[hip.VOXEL_STATUS]), **{k + "_ms": stat(v) for k, v in t.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    res = dict(reps=args.reps, statistic="median [min, max] of HIP-event times after 2 warm-ups, ms; one launch sequence per figure", configs={})
    for name, (make, radius, voxel) in {"organised_384x512": (organised_cloud, 0.05, 0.05), "list_1M": (sheet_list, 0.05, 0.05)}.items():
        xyz, grid = make()
        r = measure(xyz, grid, radius, voxel, args.reps)
        res["configs"][name] = r
        print(name, json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
