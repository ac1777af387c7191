"""numpy restatement of the query sampling rules, for the tests to check the kernels and the host code against: the candidate pool
of one frame (evaluator_3dpt.py:352-372 on top of init_pointcloud_from_rgbd at stride 1), one Lloyd step in fp64 and the fp64 inertia."""
import numpy as np


def invert_cameras(intrs, extrs):
    """intrs (..., 3, 3), extrs (..., 3, 4) -> K^-1 (..., 3, 3), rows 0..2 of [R|t]^-1 (..., 3, 4): fp64, rounded to fp32."""
    k = np.linalg.inv(intrs.astype(np.float64))
    e = np.zeros(extrs.shape[:-2] + (4, 4))
    e[..., :3, :] = extrs
    e[..., 3, 3] = 1.0
    return k.astype(np.float32), np.linalg.inv(e)[..., :3, :].astype(np.float32)


def frame_points(depths, intrs, extrs, t):
    """World points (V*H*W, 3) fp32 of frame t of depths (V,T,1,H,W) in raster order (view, row, column); pixel centres (x, y)."""
    V, _, _, H, W = depths.shape
    kinv, einv = invert_cameras(intrs[:, t], extrs[:, t])
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    pix = np.stack([xs, ys, np.ones_like(xs)], -1)  # (H,W,3)
    cam = np.einsum("vij,hwj->vhwi", kinv, pix).astype(np.float32) * depths[:, t, 0, :, :, None]
    world = np.einsum("vij,vhwj->vhwi", einv[..., :3], cam).astype(np.float32) + einv[:, None, None, :, 3]
    return world.reshape(V * H * W, 3).astype(np.float32)


def pool_mask(points, depth, conf, conf_threshold, centre, radius, z_min, z_max, radius_inclusive=False):
    """The keep rule on raster-ordered points (n,3) fp32, depth / conf (n,) [conf may be None: depth > 0]; fp32 like torch."""
    valid = conf > np.float32(conf_threshold) if conf is not None else depth > 0
    x = points[:, 0] - np.float32(centre[0])
    y = points[:, 1] - np.float32(centre[1])
    with np.errstate(over="ignore"):
        r2 = (x * x + y * y).astype(np.float32)
        rr = np.float32(float(radius) ** 2)
    inside = (r2 <= rr) if radius_inclusive else (r2 < rr)
    return valid & inside & (points[:, 2] >= np.float32(z_min)) & (points[:, 2] <= np.float32(z_max))


def frame_pool(depths, intrs, extrs, t, conf=None, conf_threshold=0.9, centre=(0.0, 0.0), radius=np.inf, z_min=-np.inf, z_max=np.inf,
               radius_inclusive=False):
    """(raster indices, points) of the pool of frame t; depths / conf (V,T,1,H,W), intrs (V,T,3,3), extrs (V,T,3,4)."""
    pts = frame_points(depths, intrs, extrs, t)
    c = None if conf is None else conf[:, t, 0].reshape(-1)
    keep = pool_mask(pts, depths[:, t, 0].reshape(-1), c, conf_threshold, centre, radius, z_min, z_max, radius_inclusive)
    idx = np.nonzero(keep)[0]
    return idx, pts[idx]


def sq_dists(points, centres):
    return ((points[:, None, :].astype(np.float64) - centres[None].astype(np.float64)) ** 2).sum(-1)


def assign(points, centres):
    """fp64 nearest centre, ties to the lowest index."""
    return np.argmin(sq_dists(points, centres), 1)


def inertia(points, centres):
    return float(sq_dists(points, centres).min(1).sum())


def lloyd_step(points, centres, labels=None):
    """New centres (fp64) = means of the assigned points (an empty cluster keeps its centre), and the counts."""
    labels = assign(points, centres) if labels is None else labels
    k = len(centres)
    counts = np.bincount(labels, minlength=k)
    new = centres.astype(np.float64).copy()
    for c in range(3):
        s = np.bincount(labels, weights=points[:, c].astype(np.float64), minlength=k)
        new[counts > 0, c] = s[counts > 0] / counts[counts > 0]
    return new, counts
