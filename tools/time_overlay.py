"""Track overlay timing with device events: ``render_track_overlays`` at the bench clip's shape (4 views x 24 frames x 512 x 512, 1 024
tracks that drift a few pixels per frame, uint8 frames on the device) with the infinite trail, with ``trail=10``, and as a session in
blocks of 4 frames; and the three kinds of launch on their own.  Median [min, max] of --reps calls after 2 warm-ups; every timed window
ends in a recorded event that is synchronised on.  A whole-clip call is 1 projection launch and 2 launches per frame (scatter,
compose); next to the milliseconds stands the share of the time the launches of that sequence would take back to back.

    python tools/time_overlay.py [--out profiles/overlay.json] [--reps 9]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvtracker_amd import hip, overlay, synth  # noqa: E402


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


def make_clip(V, T, H, W, N, seed):
    """Cameras of the synthetic clip; tracks that start on a grid in front of them and drift, a fifth of the points invisible."""
    rng = np.random.default_rng(seed)
    K, E = synth.make_cameras(V, T, H, W)
    start = rng.uniform(-0.8, 0.8, (N, 3)) * np.array([1.0, 1.0, 0.3]) + np.array([0.0, 0.0, 0.4])  # around the point the cameras look at
    vel = rng.normal(0, 0.02, (N, 3))  # about 3 pixels per frame
    tracks = np.stack([start + t * vel + rng.normal(0, 0.002, (N, 3)) for t in range(T)]).astype(np.float32)
    return dict(rgbs=rng.integers(0, 256, (V, T, 3, H, W), dtype=np.uint8), tracks=tracks, visibility=rng.random((T, N)) > 0.2,
                query_frames=(rng.integers(0, 4, N) * (T // 6)).astype(np.int64), intrs=np.asarray(K, np.float32), extrs=np.asarray(E, np.float32))


def launches(c, o, iters):
    """One launch of each kind at the clip's last frame, ``iters`` times back to back in its own event window; ms per launch."""
    V, T, _, H, W = c["rgbs"].shape
    N = c["tracks"].shape[1]
    s = overlay.TrackOverlaySession(c["query_frames"], V, H, W, o)
    pts = torch.empty(T, V, N, 4, dtype=torch.int32, device=c["rgbs"].device)
    out = torch.empty(V, T, 3, s.Hp, s.Wp, dtype=torch.uint8, device=c["rgbs"].device)
    project = lambda: hip.overlay_project(c["tracks"], c["intrs"], c["extrs"], V, T, N, points=pts, pad=o.pad, min_depth=o.min_depth,
                                          query_frames=s.query_frames, frame0=0, lut=s.lut, color_view=o.color_view, Hp=s.Hp, colors=s.colors)
    project()
    draw = lambda: hip.overlay_draw(pts[T - 2], pts[T - 1], c["visibility"][T - 1], s.query_frames, s.colors, V, N, s.M, T - 1, o.linewidth, s.Hp, s.Wp,
                                    s.line_keys, s.marker_keys)
    compose = lambda: hip.overlay_compose(c["rgbs"], V, T, T - 1, H, W, o.pad, s.line_keys, 0, s.marker_keys, out)
    return {k: timed(lambda: [fn() for _ in range(iters)])[0] / iters for k, fn in (("project", project), ("draw", draw), ("compose", compose))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20, help="back-to-back launches per timed window of a single launch")
    ap.add_argument("--shape", type=int, nargs=5, default=[4, 24, 512, 512, 1024], metavar=("V", "T", "H", "W", "N"))
    args = ap.parse_args()
    V, T, H, W, N = args.shape
    c = {k: torch.from_numpy(v).cuda() for k, v in make_clip(V, T, H, W, N, 1).items()}
    a = (c["rgbs"], c["tracks"], c["visibility"], c["query_frames"], c["intrs"], c["extrs"])
    res = dict(shape=[V, T, H, W, N], reps=args.reps, statistic="median [min, max] of device-event windows after 2 warm-ups, ms; single launches: per "
               f"launch, {args.iters} back to back per window; the clip is on the device", cases={})

    def session(o, block):
        s = overlay.open_track_overlay(c["query_frames"], V, H, W, o)
        return [s.push(c["rgbs"][:, t:t + block], c["tracks"][t:t + block], c["visibility"][t:t + block], c["intrs"][:, t:t + block],
                       c["extrs"][:, t:t + block]) for t in range(0, T, block)]

    cases = (("trail_all", overlay.TrackOverlay(), None), ("trail_10", overlay.TrackOverlay(trail=10), None), ("session_blocks_of_4", overlay.TrackOverlay(), 4))
    for name, o, block in cases:
        fn = (lambda: overlay.render_track_overlays(*a, o)[0]) if block is None else (lambda: session(o, block))
        t = {k: [] for k in ("call", "project", "draw", "compose")}
        for rep in range(args.reps + 2):
            row = launches(c, o, args.iters)
            row["call"], video = timed(fn)
            if rep >= 2:
                for k, v in row.items():
                    t[k].append(v)
        video = video if block is None else torch.cat(video, 1)
        drawn = float((video != c["rgbs"]).any(2).float().mean())
        n_project = 1 if block is None else (T + block - 1) // block
        back_to_back = n_project * statistics.median(t["project"]) + T * (statistics.median(t["draw"]) + statistics.median(t["compose"]))
        r = dict(case=name, launches=n_project + 2 * T, drawn_pixel_fraction=round(drawn, 4), ms_per_frame=round(statistics.median(t["call"]) / T, 4),
                 back_to_back_launches_ms=round(back_to_back, 4), **{k + "_ms": stat(v) for k, v in t.items()})
        res["cases"][name] = r
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
