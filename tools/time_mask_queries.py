"""Mask query timing with device events: the entries of mvtracker_amd/masks.py at the bench clip's shape (4 views x 24 frames x
512 x 512) with 6 objects, each seen by every camera under another local id, and their launches on their own.  Median [min, max]
of --reps calls after 2 warm-ups; the clip is on the device and every timed window ends in a recorded event that is synchronised on
(the windows of ``match_mask_ids`` and ``mask_queries`` include their one host read).  Next to the statistics kernel's milliseconds:
the bytes it must move ("Mask queries": every label byte, and the depth of every labelled pixel) and the GB/s
that makes, for masks that cover a tenth of the image and for one label over everything.

    python tools/time_mask_queries.py [--out profiles/mask_queries.json] [--reps 9]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvtracker_amd import hip, masks, synth  # noqa: E402


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


def disc_labels(depths, intrs, extrs, objects, radius):
    """``objects`` discs on the ground around the origin, labelled in world space so that every camera sees the same things; camera v
    calls disc i ``(i + v) % objects + 1``."""
    V, T, _, H, W = depths.shape
    lab = np.zeros((V, T, H, W), np.uint8)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    pix = np.stack([xs, ys, np.ones_like(xs)], -1)
    for v in range(V):
        kinv = np.linalg.inv(intrs[v, 0].astype(np.float64))
        e = np.eye(4)
        e[:3] = extrs[v, 0]
        einv = np.linalg.inv(e)
        for t in range(T):
            cam = (pix @ kinv.T) * depths[v, t, 0][..., None]
            world = cam @ einv[:3, :3].T + einv[:3, 3]
            for i in range(objects):
                a = 2 * np.pi * i / objects
                c = np.array([1.2 * np.cos(a), 1.2 * np.sin(a)])
                hit = ((world[..., :2] - c) ** 2).sum(-1) < radius ** 2
                lab[v, t][hit] = (i + v) % objects + 1
    return lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20, help="back-to-back launches per timed window of a single launch")
    ap.add_argument("--shape", type=int, nargs=4, default=[4, 24, 512, 512], metavar=("V", "T", "H", "W"))
    ap.add_argument("--objects", type=int, default=6)
    args = ap.parse_args()
    V, T, H, W = args.shape
    clip = synth.make_clip(3, V=V, T=T, H=H, W=W, N=1, frame_period=2)
    lab = disc_labels(clip["depths"][0], clip["intrs"][0], clip["extrs"][0], args.objects, 0.45)
    d, k, e = (torch.from_numpy(clip[n]).cuda() for n in ("depths", "intrs", "extrs"))
    res = dict(shape=[V, T, H, W], objects=args.objects, reps=args.reps,
               statistic=f"median [min, max] of device-event windows after 2 warm-ups, ms; single launches: per launch, {args.iters} back to back "
                         "per window; the clip is on the device", configurations={})
    opt = masks.MaskQueries(distance_threshold=0.3, max_points_per_frame=256)
    for name, labels in (("discs", lab), ("one_label", np.ones_like(lab))):
        l8 = torch.from_numpy(labels).cuda()
        c = masks._Clip(l8, d, k, e, None, opt)
        st = masks._statistics(c)
        mt = masks._matching(st, opt)
        tb = st._tables
        ids = torch.empty(V * hip.MASK_LABELS, dtype=torch.int32, device="cuda")
        out = torch.empty(V, T, H, W, dtype=torch.int32, device="cuda")
        g0 = next(g for g, m in mt.members.items() if m)
        m0 = int(mt.object_valid(g0)[0])
        pool, pixel = torch.empty(m0, 3, device="cuda"), torch.empty(m0, dtype=torch.int32, device="cuda")
        count = torch.empty(1, dtype=torch.int32, device="cuda")
        blocks = torch.empty((V * H * W + 255) // 256, dtype=torch.int32, device="cuda")
        launches = dict(
            stats=lambda: hip.mask_stats(c.lab, c.d, None, c.kinv, c.einv, V, T, H, W, opt.min_depth, opt.max_depth, 0.0, tb.stats),
            centroids=lambda: hip.mask_centroids(tb.stats, V, T, 1, tb.centroid),
            match=lambda: hip.mask_match(tb.centroid, V, T, 1, opt.distance_threshold, True, ids, tb.global_id, tb.distance, tb.state),
            relabel=lambda: hip.mask_relabel(c.lab, mt.global_id, V, T, H, W, out),
            pool=lambda: hip.mask_pool(*c.pool_args(0), mt.global_id, g0, pool, pixel, count, blocks))
        calls = dict(
            mask_statistics=lambda: masks.mask_statistics(l8, d, k, e, opt),
            match_mask_ids=lambda: masks.match_mask_ids(st, opt),
            global_masks=lambda: masks.global_masks(l8, mt),
            lift_masks=lambda: masks.lift_masks(l8, d, k, e, 0, matching=mt, options=opt),
            mask_queries=lambda: masks.mask_queries(l8, d, k, e, opt))
        t = {n: [] for n in list(launches) + list(calls)}
        for rep in range(args.reps + 2):
            row = {n: timed(lambda: [fn() for _ in range(args.iters)])[0] / args.iters for n, fn in launches.items()}
            row.update({n: timed(fn)[0] for n, fn in calls.items()})
            if rep >= 2:
                for n, v in row.items():
                    t[n].append(v)
        q, oid, report = masks.mask_queries(l8, d, k, e, opt)
        labelled = int((labels != 0).sum())
        b = dict(labels=labels.size, depth_of_labelled=4 * labelled)
        ms = statistics.median(t["stats"])
        r_ = dict(labels=name, labelled_fraction=round(labelled / labels.size, 4), objects=mt.num_objects, queries=int(q.shape[1]),
                  pools=sum(len(o["frames_used"]) for o in report.objects), stats_model_bytes=b, stats_gb_per_s=round(sum(b.values()) / ms / 1e6, 1),
                  relabel_gb_per_s=round(5 * labels.size / statistics.median(t["relabel"]) / 1e6, 1), **{n + "_ms": stat(v) for n, v in t.items()})
        res["configurations"][name] = r_
        print(json.dumps(r_), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
