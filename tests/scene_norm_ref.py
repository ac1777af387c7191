"""Numpy fp64 restatement of the reference's scene normalisation (datasets/generic_scene_dataset.py:288-358
``compute_auto_scene_normalization``) and of ``transform_scene`` (datasets/utils.py:210-301): what the two functions compute, in
exact-enough arithmetic, from the same fp32 inputs.  tests/golden/scene_norm.npz records the reference's own fp32 results and their
distance from this restatement (``d_ref``); the device is held to a multiple of that distance."""
import numpy as np

MIN_POINTS = 100


def quantile_parts(sorted_values, q):
    """torch.quantile's default on a float32 tensor: rank = q * (M - 1) with q and the product in fp32, linear interpolation
    between the two neighbouring order statistics.  -> (quantile, lower rank, lower value, upper value)."""
    M = len(sorted_values)
    rank = np.float32(q) * np.float32(M - 1)  # one fp32 multiply
    kb = int(np.floor(rank))
    ka = min(int(np.ceil(rank)), M - 1)
    w = float(rank - np.float32(kb))
    lo, hi = float(sorted_values[kb]), float(sorted_values[ka])
    return lo + w * (hi - lo), kb, lo, hi


def unproject_frame(depth, intr, extr):
    """World points (H*W, 3) fp64 of one view's depth map (H, W): pixel (x, y, 1) through K^-1, times depth, through [R|t]^-1."""
    H, W = depth.shape
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    homog = np.stack([x, y, np.ones_like(x)], -1).reshape(-1, 3).astype(np.float64)
    E = np.eye(4)
    E[:3] = extr.astype(np.float64)
    cam = (np.linalg.inv(intr.astype(np.float64)) @ homog.T).T * depth.reshape(-1, 1).astype(np.float64)
    return (np.linalg.inv(E) @ np.concatenate([cam, np.ones_like(cam[:, :1])], 1).T).T[:, :3]


def auto_scene_normalization(depths, intrs, extrs, conf=None, conf_thresh=4.8, target_radius=6.3, rescale_by_camera_radius=True, frame=0):
    """depths (V,T,1,H,W), intrs (V,T,3,3), extrs (V,T,3,4) [conf as depths; None: valid is depth > 0] -> a dict with scale,
    translate and every intermediate quantity, or RuntimeError with the reference's message."""
    V = depths.shape[0]
    pts = []
    for v in range(V):
        d = depths[v, frame, 0]
        mask = d > 0 if conf is None else (conf[v, frame, 0] > np.float32(conf_thresh)) & (d > 0)
        if mask.sum() < MIN_POINTS:
            continue
        pts.append(unproject_frame(d, intrs[v, frame], extrs[v, frame])[mask.reshape(-1)])
    pts = np.concatenate(pts, 0) if pts else np.zeros((0, 3))
    if len(pts) < MIN_POINTS:
        raise RuntimeError("Too few valid points for normalization.")
    centroid = pts.mean(0)
    zq, z_rank, z_lo, z_hi = quantile_parts(np.sort(pts[:, 2].astype(np.float32)), 0.12)
    # (the reference takes the quantile of the centred z: the same number up to the rounding of one subtraction)
    floor_z = zq - centroid[2]
    out = {"M": len(pts), "centroid": centroid, "floor_z": floor_z, "z_rank": z_rank, "z_lo": z_lo, "z_hi": z_hi,
           "extent": float(np.abs(pts).max())}
    lifted = pts - centroid
    lifted[:, 2] -= floor_z
    if rescale_by_camera_radius:
        # kept from the reference: the translation column of world->camera stands in for the camera centre, and torch.median
        # of an even count is the lower middle value
        c = extrs[:, frame, :, 3].astype(np.float64) - centroid
        c[:, 2] -= floor_z
        dist = np.sort(np.sqrt((c * c).sum(1)))
        radius = float(dist[(len(dist) - 1) // 2])
    else:
        rq, r_rank, r_lo, r_hi = quantile_parts(np.sort(np.sqrt((lifted * lifted).sum(1)).astype(np.float32)), 0.95)
        out.update(r_rank=r_rank, r_lo=r_lo, r_hi=r_hi)
        radius = rq
    out["radius"] = radius
    out["scale"] = target_radius / radius
    t = -out["scale"] * centroid
    t[2] -= out["scale"] * floor_z
    out["translate"] = t
    return out


def rigid_inverse(R, t):
    return R.T, -(R.T @ t)


def transform_scene(scale, R, t, depths=None, extrs=None, query_points=None, tracks=None):
    """X' = t + R (s X): depths * s; extrinsics [Re | s te] [R^T | -R^T t]; rows (.., 4) keep column 0; rows (.., 3) mapped.  fp64."""
    s, R, t = float(scale), np.asarray(R, np.float64), np.asarray(t, np.float64)
    out = [None, None, None, None]
    if depths is not None:
        out[0] = depths.astype(np.float64) * s
    if extrs is not None:
        e = extrs.astype(np.float64)
        Ri, ti = rigid_inverse(R, t)
        rot = e[..., :3] @ Ri
        out[1] = np.concatenate([rot, (e[..., :3] @ ti + s * e[..., 3])[..., None]], -1)
    if query_points is not None:
        q = query_points.astype(np.float64)
        out[2] = np.concatenate([q[..., :1], (s * q[..., 1:]) @ R.T + t], -1)
    if tracks is not None:
        out[3] = (s * tracks.astype(np.float64)) @ R.T + t
    return out


def rel_inf(a, b, magnitude=None):
    """The fixture's relative distance: max |a - b| over ``magnitude`` (default: max |b|)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    m = float(np.abs(b).max()) if magnitude is None else float(magnitude)
    return float(np.abs(a - b).max()) / m if m > 0 else float(np.abs(a - b).max())
