"""Region clustering timing with device events: ``cluster_points`` at the reference's parameters (eps 0.03, min_samples 12) on seeded
point lists spread over the reference's box (blobs and a haze, 15 000 and 60 000 points), split into its stages, and ``region_masks``
on one frame of a synthetic clip (3 views x 384x512) with a box around a point of the scene.  Median [min, max] of --reps calls
after 2 warm-ups; the inputs are on the device and every timed window ends in a recorded event that is synchronised on.

    python tools/time_region_cluster.py [--out profiles/region_cluster.json] [--reps 9]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvtracker_amd import cluster, hip, synth  # noqa: E402

EPS, MIN_SAMPLES = 0.03, 12


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stat(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def box_cloud(n, seed):
    """n float32 points over the reference's box: three quarters in 6 blobs (sigma 1 to 2 cm), the rest uniform."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(cluster.DEFAULT_BOX)[:, 0], np.asarray(cluster.DEFAULT_BOX)[:, 1]
    centres = rng.uniform(lo, hi, (6, 3))
    k = n * 3 // 4
    which = rng.integers(0, 6, k)
    pts = np.concatenate([centres[which] + rng.normal(size=(k, 3)) * rng.uniform(0.01, 0.02, (6, 1))[which], rng.uniform(lo, hi, (n - k, 3))])
    return pts[rng.permutation(n)].astype(np.float32)


def stages(xyz, M):
    """The launch sequence of cluster_clouds on one point list, each stage in its own event window."""
    dev = xyz.device
    nt = (M + 63) // 64
    box, gbox = torch.empty(1, nt, 8, device=dev), torch.empty(1, (nt + 63) // 64, 8, device=dev)
    core = torch.empty(1, M, device=dev, dtype=torch.uint8)
    parent, root, labels = (torch.empty(1, M, device=dev, dtype=torch.int32) for _ in range(3))
    select = torch.empty(1, M, device=dev, dtype=torch.uint8)
    state = torch.empty(1, hip.CLUSTER_STATE_WORDS, device=dev, dtype=torch.int64)
    r2 = cluster.radius_sq(EPS)
    row = {}
    row["boxes"], _ = timed(lambda: (hip.tile_aabb(xyz, M, 1, box, (0, 0)), hip.tile_group_aabb(box, M, 1, gbox)))
    row["count"], _ = timed(lambda: hip.cluster_count(xyz, 1, M, (0, 0), r2, MIN_SAMPLES, box, gbox, core))
    row["link"], _ = timed(lambda: hip.cluster_link(xyz, 1, M, (0, 0), r2, box, gbox, core, parent, state))
    row["border"], _ = timed(lambda: hip.cluster_border(xyz, 1, M, (0, 0), r2, box, gbox, core, parent, root))
    row["finish"], _ = timed(lambda: hip.cluster_finish(xyz, 1, M, MIN_SAMPLES, core, root, parent, labels, select, state))
    return row, state


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", type=int, nargs="+", default=[15000, 60000])
    args = ap.parse_args()
    res = dict(eps=EPS, min_samples=MIN_SAMPLES, reps=args.reps,
               statistic="median [min, max] of device-event windows after 2 warm-ups, ms; the inputs are on the device", point_lists={}, clips={})
    for n in args.sizes:
        pts = torch.from_numpy(box_cloud(n, 7)).cuda()
        xyz = torch.zeros(1, n, 4, device="cuda")
        xyz[0, :, :3] = pts
        t = {k: [] for k in ("cluster_points", "boxes", "count", "link", "border", "finish")}
        info = None
        for rep in range(args.reps + 2):
            row, _ = stages(xyz, n)
            row["cluster_points"], (_, info) = timed(lambda: cluster.cluster_points(pts, EPS, MIN_SAMPLES, return_info=True))
            if rep >= 2:
                for k, v in row.items():
                    t[k].append(v)
        r = dict(points=n, clusters=info["clusters"], core=info["core"].sum().item() if hasattr(info["core"], "sum") else info["core"],
                 noise=info["noise"], **{k + "_ms": stat(v) for k, v in t.items()})
        res["point_lists"][str(n)] = r
        print("points", n, json.dumps(r), flush=True)
    V, H, W = 3, 384, 512
    clip = synth.make_clip(1234, V=V, T=2, H=H, W=W, N=4, invalid_frac=0.02)
    depths, intrs, extrs = (torch.from_numpy(clip[k]).cuda() for k in ("depths", "intrs", "extrs"))
    from mvtracker_amd import clean
    pts = clean.clean_clip(depths[0], intrs[0], extrs[0], clean.DepthCleaning(), details=True)[3][0, 0]  # view 0, frame 0
    centre = pts[H // 2, W // 2, :3].cpu().numpy().astype(np.float64)
    pose = np.eye(4)
    pose[:3, 3] = centre
    for name, (box, eps) in {"reference_box": (cluster.DEFAULT_BOX, EPS), "one_metre_box": (((-0.5, 0.5),) * 3, EPS)}.items():
        region = cluster.RegionCluster(box, eps, MIN_SAMPLES)
        t, report = [], None
        for rep in range(args.reps + 2):
            ms, (_, report) = timed(lambda: cluster.region_masks(depths[:, :, :1], intrs[:, :, :1], extrs[:, :, :1], pose, region))
            if rep >= 2:
                t.append(ms)
        r = dict(views=V, height=H, width=W, frames=1, candidates=report.candidates.reshape(-1).tolist(), clusters=report.clusters.reshape(-1).tolist(),
                 selected=report.selected.reshape(-1).tolist(), region_masks_ms=stat(t))
        res["clips"][name] = r
        print(name, json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
