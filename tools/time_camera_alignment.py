"""Camera alignment timing at the workload's own size: 4 views at 384x512, one frame, the rendered scene of the tests
(tests/camera_align_cases.py: a plane and three spheres, view 1's extrinsics off by 1.5 degrees and 4.4 cm), ``sample_stride`` 1 and 2,
the defaults otherwise (cap 0.05, 30 iterations, 2 sweeps).  ``align_cameras`` on a clip that is on the device, timed with device
events after 2 warm-ups: median [min, max] of --reps calls; and one ``mvt_align_correspond`` launch alone (view 1 against the other
three, at the identity, where most queries still search) and one ``mvt_align_solve`` launch.

    python tools/time_camera_alignment.py [--out profiles/r11_camera_alignment.json] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import camera_align_cases as Cs  # noqa: E402
from mvtracker_amd import CameraAlignment, align, align_cameras  # noqa: E402

V, H, W = 4, 384, 512


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
    args = ap.parse_args()
    sc = Cs.scene(V, H, W, T=1)
    ex = Cs.perturbed(sc["extrs"], 1, Cs.rigid(**Cs.PLANTED))
    true = Cs.unproject(sc["depths"], sc["intrs"], sc["extrs"])
    moved = Cs.unproject(sc["depths"], sc["intrs"], ex)
    planted = Cs.displacement(np.eye(4), moved[1], true[1])
    depths, intrs, extrs = (torch.from_numpy(a).cuda() for a in (sc["depths"], sc["intrs"], ex))
    res = dict(views=V, height=H, width=W, frames=1, reps=args.reps, planted_mm=round(1e3 * planted, 3),
               statistic="median [min, max] of device-event times after 2 warm-ups, ms", configs={})
    for stride in (1, 2):
        a = CameraAlignment(sample_stride=stride)
        t_all, c = [], None
        for rep in range(args.reps + 2):
            ms, c = event_ms(lambda: align_cameras(depths, intrs, extrs, a))
            if rep >= 2:
                t_all.append(ms)
        left = Cs.displacement(c.transforms[1].cpu().numpy(), moved[1], true[1])
        st = align.ClipAlignment(depths[0], intrs[0], extrs[0], a)
        run = st.icp(1)
        t_corr, t_solve = [], []
        for rep in range(args.reps + 2):
            ms_c, _ = event_ms(lambda: align.hip.align_correspond(run.src0, run.P, run.grid, run.stride, run.frames, run.D, run.cap2, run.targets,
                                                                  run.istate, run.partial))
            ms_s, _ = event_ms(lambda: align.hip.align_solve(run.partial, run.frames * run.ntq, run.n_queries, True, run.D, run.istate, run.hist,
                                                             run.result, run.sums))
            run.istate.zero_()
            if rep >= 2:
                t_corr.append(ms_c)
                t_solve.append(ms_s)
        m = dict(align_cameras_ms=stat(t_all), queries=int(run.n_queries.item()), query_tiles=run.ntq, target_points=3 * st.P,
                 matched_at_identity=int(run.sums[27].item()), correspond_ms=stat(t_corr), solve_ms=stat(t_solve),
                 iterations=c.iterations.tolist(), fitness=[round(f, 4) for f in c.fitness.tolist()], rmse=[round(f, 5) for f in c.rmse.tolist()],
                 left_mm=round(1e3 * left, 3))
        res["configs"][f"sample_stride_{stride}"] = m
        print(f"sample_stride {stride}", json.dumps(m), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
