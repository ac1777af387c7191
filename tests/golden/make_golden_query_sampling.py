"""Golden vectors of the evaluator's query sampling for unlabelled clips (reference evaluation/evaluator_3dpt.py:286-388 and
``kmeans_sample``, :42-59), generated in the build container only.  The evaluator module is imported with the stub modules of
make_golden_evaluate3dpt.py (its visualisation / logging imports are absent here and never touched).  The sampling itself sits
inside the evaluator's per-sequence loop, so the pools are produced by the calls that loop makes: ``init_pointcloud_from_rgbd`` on
one frame of all views at stride 1 with the confidence map as the feature map, the confidence threshold, the cylinder.  Data only:
a seeded synthetic clip, a seeded confidence map, the pools, the reference's k-means centres and sklearn's inertia over ten seeds."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")


def _stub(name, **attrs):
    if name in sys.modules:
        return sys.modules[name]
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def _unused(*a, **k):
    raise NotImplementedError("stub: not on the query sampling path")


_stub("imageio")
_stub("rerun")
tb = _stub("torch.utils.tensorboard", SummaryWriter=type("SummaryWriter", (), {}))
import torch.utils  # noqa: E402

torch.utils.tensorboard = tb
pkg = _stub("mvtracker.datasets")
pkg.__path__ = []
_stub("mvtracker.datasets.utils", dataclass_to_cuda_=_unused, transform_scene=_unused)
_stub("easydict", EasyDict=dict)
_stub("mvtracker.utils.visualizer_mp4", log_mp4_track_viz=_unused, MultiViewVisualizer=type("MultiViewVisualizer", (), {}))
_stub("mvtracker.utils.visualizer_rerun", log_pointclouds_to_rerun=_unused, log_tracks_to_rerun=_unused)
import mvtracker.evaluation.evaluator_3dpt as E  # noqa: E402
from sklearn.cluster import KMeans  # noqa: E402
from threadpoolctl import threadpool_limits  # noqa: E402

from mvtracker_amd import synth  # noqa: E402

CLIP_SEED, CONF_SEED, V, T, H, W, K = 47, 48, 2, 3, 37, 53, 64
CONF_THRESHOLD = 0.9
# (t, z_min, z_max, radius): a finite cylinder, no bounds at all, a cylinder that leaves nothing
ROWS = [(0, -0.1, 4.2, 2.1), (1, -np.inf, np.inf, np.inf), (2, -0.1, 4.2, 0.0)]

clip = synth.make_clip(CLIP_SEED, V=V, T=T, H=H, W=W, N=4, invalid_frac=0.02)
conf_np = (np.random.default_rng(CONF_SEED).uniform(size=(1, V, T, 1, H, W)) ** 0.2).astype(np.float32)  # 41 % above 0.9
depths, intrs, extrs, conf = (torch.from_numpy(a) for a in (clip["depths"], clip["intrs"], clip["extrs"], conf_np))

out = {"clip_seed": np.array([CLIP_SEED]), "conf": conf_np, "conf_threshold": np.array([CONF_THRESHOLD]),
       "rows": np.array(ROWS, dtype=np.float64), "k": np.array([K])}
pools = []
for i, (t, zmin, zmax, radius) in enumerate(ROWS):
    xyz, c = E.init_pointcloud_from_rgbd(fmaps=conf[:, :, t:t + 1], depths=depths[:, :, t:t + 1], intrs=intrs[:, :, t:t + 1],
                                         extrs=extrs[:, :, t:t + 1], stride=1, level=0, depth_interp_mode="N/A")
    xyz, c = xyz[0], c[0, :, 0]
    keep = c > CONF_THRESHOLD
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    keep = keep & (x ** 2 + y ** 2 < radius ** 2) & (z >= zmin) & (z <= zmax)
    idx = torch.nonzero(keep)[:, 0]
    out[f"pool{i}_index"] = idx.numpy().astype(np.int64)  # position in the (V, H, W) raster of frame t
    out[f"pool{i}_xyz"] = xyz[idx].numpy().astype(np.float32)
    pools.append(xyz[idx])
assert len(pools[0]) > 4 * K and len(pools[1]) > len(pools[0]) and len(pools[2]) == 0, [len(p) for p in pools]


def inertia64(points, centres):
    d = ((points[:, None, :].astype(np.float64) - centres[None].astype(np.float64)) ** 2).sum(-1)
    return float(d.min(1).sum())


centres = E.kmeans_sample(pools[0], K).numpy()
out["kmeans_centres"] = centres.astype(np.float32)
out["kmeans_inertia"] = np.array([inertia64(pools[0].numpy(), centres)])
with threadpool_limits(limits=1):
    out["sklearn_inertia"] = np.array([float(KMeans(n_clusters=K, n_init="auto", random_state=r).fit(pools[0].numpy()).inertia_)
                                       for r in range(10)])
path = os.path.join(HERE, "query_sampling.npz")
np.savez_compressed(path, **out)
s = out["sklearn_inertia"]
print("query_sampling.npz", os.path.getsize(path) / 1024, "KiB; pools", [len(p) for p in pools], "I_ref", out["kmeans_inertia"][0],
      "sklearn", s.min(), s.max(), "spread", (s.max() - s.min()) / s.min())
