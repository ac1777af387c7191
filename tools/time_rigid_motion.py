"""Rigid-motion timing with device events: ``rigid_motion`` (member lists and the fit) at N = 8192 tracks, T = 64 frames, G = 16
objects, its two entries on their own, ``move_points`` at M = 1 M points over T = 24 frames and ``fill_tracks`` on the fit's clip.
Median [min, max] of --reps windows after 2 warm-ups; the inputs are on the device, ``num_objects`` is given (nothing is read back)
and every timed window ends in a recorded event that is synchronised on.  Next to ``mvt_rigid_move``'s milliseconds: the bytes it
must move (16 M for the points and their ids, 12 M T for the output) and the GB/s that makes against the 6.3 TB/s a streaming
kernel achieves on the MI355X (8 TB/s peak).

    python tools/time_rigid_motion.py [--out profiles/rigid_motion.json] [--reps 9]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvtracker_amd import hip, rigid  # noqa: E402

HBM_ACHIEVABLE_GB_S = 6300.0


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


def rotation(axis, angle):
    a = axis / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def moving_objects(T, N, G, seed=0, thr=0.02):
    """G rigid objects of N / G interleaved tracks each, 0.3 units across, noise of 0.1 thresholds, one track in 16 an outlier, 85 %
    of the points visible."""
    rng = np.random.default_rng(seed)
    ids = (np.arange(N) % G).astype(np.int32)
    P = rng.uniform(-0.15, 0.15, size=(N, 3)) + rng.uniform(-1, 1, size=(G, 3))[ids]
    tracks = np.empty((T, N, 3))
    for t in range(T):
        for g in range(G):
            m = ids == g
            Rm = rotation(rng.normal(size=3), 0.02 * t)
            tracks[t, m] = P[m] @ Rm.T + rng.uniform(-0.01, 0.01, size=3) * t
    tracks[1:] += rng.normal(scale=0.1 * thr / np.sqrt(3), size=(T - 1, N, 3))
    out = rng.uniform(size=N) < 1 / 16
    tracks[1:, out] += rng.uniform(3 * thr, 5 * thr, size=(T - 1, int(out.sum()), 1)) / np.sqrt(3)
    return tracks.astype(np.float32), rng.uniform(size=(T, N)) < 0.85, np.zeros(N, np.int32), ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10, help="back-to-back calls per timed window")
    ap.add_argument("--fit-shape", type=int, nargs=3, default=[8192, 64, 16], metavar=("N", "T", "G"))
    ap.add_argument("--move-shape", type=int, nargs=2, default=[1 << 20, 24], metavar=("M", "T"))
    args = ap.parse_args()
    N, T, G = args.fit_shape
    M, Tm = args.move_shape
    tr, vis, qf, ids = (torch.from_numpy(x).cuda() for x in moving_objects(T, N, G))
    opt = rigid.RigidMotion()
    res = rigid.rigid_motion(tr, vis, qf, ids, opt, num_objects=G)
    counts, offsets = torch.empty(G, dtype=torch.int32, device="cuda"), torch.empty(G + 1, dtype=torch.int32, device="cuda")
    members = torch.empty(N, dtype=torch.int32, device="cuda")
    # move_points: the clip's first Tm poses, points of all objects in the reference configuration
    short = rigid.rigid_motion(tr[:Tm].contiguous(), vis[:Tm].contiguous(), qf, ids, opt, num_objects=G)
    pts = torch.rand(M, 3, device="cuda")
    oid = (torch.arange(M, device="cuda") % G).to(torch.int32)
    xf = torch.empty(G, Tm, 3, 4, dtype=torch.float64, device="cuda")
    moved = torch.empty(Tm, M, 3, device="cuda")
    calls = dict(
        rigid_motion=lambda: rigid.rigid_motion(tr, vis, qf, ids, opt, num_objects=G),
        members=lambda: hip.rigid_members(ids, qf, N, G, T, counts, offsets, members, res.reference_frames),
        fit=lambda: hip.rigid_fit(tr, vis, qf, ids, offsets, members, res.reference_frames, T, N, G, opt.inlier_threshold, opt.iterations,
                                  opt.min_points, opt.use_visibility, opt.min_spread, opt.live_before_query, res.poses, res.residual, res.inliers,
                                  res.used, res.inlier_count, res.rmse, res.status),
        fill_tracks=lambda: rigid.fill_tracks(tr, vis, res),
        compose=lambda: hip.rigid_compose(short.poses, short.status, G, Tm, 0, xf),
        move=lambda: hip.rigid_move(pts, oid, xf, M, Tm, G, moved),
        move_points=lambda: rigid.move_points(pts, oid, short, frame=0))
    t = {n: [] for n in calls}
    for rep in range(args.reps + 2):
        row = {n: timed(lambda: [fn() for _ in range(args.iters)])[0] / args.iters for n, fn in calls.items()}
        if rep >= 2:
            for n, v in row.items():
                t[n].append(v)
    move_bytes = 16 * M + 12 * M * Tm
    fill_bytes = T * N * (12 + 12 + 1 + 1 + 1)
    gbs = move_bytes / statistics.median(t["move"]) / 1e6
    out = dict(fit_shape=dict(N=N, T=T, G=G), move_shape=dict(M=M, T=Tm), reps=args.reps,
               statistic=f"median [min, max] of device-event windows after 2 warm-ups, ms per call, {args.iters} calls back to back per window",
               summary=res.summary(), move_model_bytes=move_bytes, move_gb_per_s=round(gbs, 1), hbm_achievable_gb_per_s=HBM_ACHIEVABLE_GB_S,
               move_fraction_of_achievable=round(gbs / HBM_ACHIEVABLE_GB_S, 3),
               fill_gb_per_s=round(fill_bytes / statistics.median(t["fill_tracks"]) / 1e6, 1), **{n + "_ms": stat(v) for n, v in t.items()})
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
