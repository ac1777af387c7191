"""Query sampling timing at the benchmark configurations' frame sizes (C2: 3 views x 384x512, C3: 4 views x 512x512), count = 1000,
the evaluator's default region (0, -0.1, 4.2, 2.1): ``sample_queries`` with k-means and with a random draw, and the k-means call
split into pool, statistics + seeding and Lloyd (each stage synchronised on its own), with the iterations to convergence and
the inertia.  Median [min, max] of --reps synchronised calls after 2 warm-ups.  With --sklearn C2 C3 (and sklearn importable) the wall
time of ``KMeans(n_clusters=1000, n_init='auto', random_state=0)`` on one thread over the same pool is measured once beside it.

    python tools/time_query_sampling.py [--out profiles/r08_query_sampling.json] [--reps 15] [--sklearn C2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvtracker_amd import hip, queries, synth  # noqa: E402

COUNT = 1000
REGION = (-0.1, 4.2, 2.1)  # z_min, z_max, radius


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stat(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--sklearn", nargs="*", default=[], metavar="CONFIG", help="configurations to time sklearn on (it takes minutes each)")
    args = ap.parse_args()
    res = dict(count=COUNT, region=dict(z_min=REGION[0], z_max=REGION[1], radius=REGION[2]), reps=args.reps,
               statistic="median [min, max] of synchronised calls after 2 warm-ups, ms; the clip is on the device", configs={})
    for name, (V, H, W) in {"C2": (3, 384, 512), "C3": (4, 512, 512)}.items():
        clip = synth.make_clip(1234, V=V, T=2, H=H, W=W, N=4, invalid_frac=0.02)
        depths, intrs, extrs = (torch.from_numpy(clip[k]).cuda() for k in ("depths", "intrs", "extrs"))
        spec = lambda method: [(0, REGION[0], REGION[1], REGION[2], COUNT, method)]
        d = depths[0].contiguous()
        kinv, einv = torch.empty(V * 2, 9, device="cuda"), torch.empty(V * 2, 12, device="cuda")
        hip.invert_cameras(intrs[0].reshape(-1, 9).contiguous(), extrs[0].reshape(-1, 12).contiguous(), kinv, einv, V * 2)
        t = {k: [] for k in ("sample_kmeans", "sample_random", "pool", "seeding", "lloyd")}
        info = None
        for rep in range(args.reps + 2):
            row = {}
            row["sample_kmeans"], _ = timed(lambda: queries.sample_queries(depths, intrs, extrs, spec("kmeans")))
            row["sample_random"], _ = timed(lambda: queries.sample_queries(depths, intrs, extrs, spec("")))
            row["pool"], pool = timed(lambda: queries.frame_pool(d, kinv, einv, 0, None, 0.9, (0.0, 0.0), REGION[2], REGION[0], REGION[1]))
            w = None

            def seed():
                nonlocal w
                w = queries._km_begin(pool, COUNT, 1e-4)
                queries._km_seed(w, 0)
            row["seeding"], _ = timed(seed)
            row["lloyd"], info = timed(lambda: queries._km_lloyd(w, 300))
            if rep >= 2:
                for k, v in row.items():
                    t[k].append(v)
        r = dict(views=V, height=H, width=W, pixels=V * H * W, pool_points=int(pool.shape[0]), **{k + "_ms": stat(v) for k, v in t.items()},
                 iterations=info["iterations"], converged=info["converged"], inertia=info["inertia"], empty=info["empty"])
        if name in args.sklearn:
            print(f"{name}: sklearn on {pool.shape[0]} points ...", flush=True)
            try:
                from sklearn.cluster import KMeans
                from threadpoolctl import threadpool_limits
                x = pool.cpu().numpy()
                t0 = time.perf_counter()
                with threadpool_limits(limits=1):
                    km = KMeans(n_clusters=COUNT, n_init="auto", random_state=0).fit(x)
                r["sklearn_one_thread_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                r["sklearn_inertia"], r["sklearn_iterations"] = float(km.inertia_), int(km.n_iter_)
            except ImportError:
                r["sklearn_one_thread_ms"] = None  # not measured: sklearn is not importable here
        res["configs"][name] = r
        print(name, json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
