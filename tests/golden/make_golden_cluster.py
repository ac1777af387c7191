"""Writes tests/golden/cluster_dbscan.npz: a handful of float32 clouds (blobs with noise) and the labels
``sklearn.cluster.DBSCAN(eps, min_samples).fit_predict`` gives them at a few settings.  Needs scikit-learn; the tests do not.

    python tests/golden/make_golden_cluster.py

A cloud is rejected, and the next fixed seed tried, when any pair of its points has |d2 - eps^2| <= MARGIN * eps^2 in fp64 at one of
its settings.  The fp32 d2 of two fp32 points differs from the exact value by about 3e-7 relative (three correctly rounded
subtractions, three fused steps); the bar is roughly 30 times that, so the device's fp32 neighbour test and sklearn's agree on every
pair.  Per cloud NAME the file holds NAME_points (M, 3) float32, NAME_eps (S,) float64, NAME_min_samples (S,) int64 and
NAME_labels (S, M) int32.  Data only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cluster_ref  # noqa: E402

MARGIN = 1e-5
SETTINGS = ((0.03, 12), (0.02, 6), (0.03, 3))
CLOUDS = (("blobs300", 300, 3), ("blobs900", 900, 5), ("blobs2500", 2500, 8))


def make_cloud(n, blobs, seed):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-0.15, 0.15, (blobs, 3))
    k = n * 3 // 4
    pts = np.concatenate([centres[rng.integers(0, blobs, k)] + rng.normal(size=(k, 3)) * rng.uniform(0.008, 0.02, (blobs, 1))[rng.integers(0, blobs, k)],
                          rng.uniform(-0.25, 0.25, (n - k, 3))])
    return pts[rng.permutation(n)].astype(np.float32)


def main():
    from sklearn.cluster import DBSCAN
    out = {}
    for name, n, blobs in CLOUDS:
        for seed in range(1000):
            pts = make_cloud(n, blobs, seed)
            if all(cluster_ref.min_pair_gap(pts, eps) > MARGIN for eps, _ in SETTINGS):
                break
        else:
            raise SystemExit(f"no seed gave {name} the margin")
        labels = np.stack([DBSCAN(eps=eps, min_samples=ms).fit_predict(pts) for eps, ms in SETTINGS]).astype(np.int32)
        print(name, "seed", seed, "clusters", (labels.max(1) + 1).tolist(), "noise", (labels < 0).sum(1).tolist())
        out[name + "_points"] = pts
        out[name + "_eps"] = np.array([s[0] for s in SETTINGS], np.float64)
        out[name + "_min_samples"] = np.array([s[1] for s in SETTINGS], np.int64)
        out[name + "_labels"] = labels
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cluster_dbscan.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
