"""numpy restatement of the mask query rules ("Mask queries"), for the tests to check the kernels and the host code
against: rule 1 (valid pixel), rule 2 (integer statistics, fixed point with 20 fractional bits), rule 3 (greedy average-distance
matching in fp64), rule 4 (frames of an object) and rule 5 (pools and the draw).  Points are ``query_sampling_ref.frame_points``.
Options are any object with MaskQueries' attributes."""
from types import SimpleNamespace

import numpy as np
import torch

import query_sampling_ref as Q

L = 256
DEFAULTS = dict(anchor="first", frames_before=3, frames_after=1, min_depth=1e-6, max_depth=10.0, conf_thresh=None, min_pixels=1, match=True,
                distance_threshold=0.15, min_common_frames=1, max_points_per_frame=None, method="random")


def options(**kw):
    return SimpleNamespace(**{**DEFAULTS, **kw})


def valid_pixels(labels, depths, opt, conf=None):
    """Rule 1: labels (V,T,H,W) integers, depths / conf (V,T,1,H,W) fp32 -> (V,T,H,W) bool.  The bounds are compared in fp32."""
    d = depths[:, :, 0]
    with np.errstate(invalid="ignore"):
        ok = (labels != 0) & np.isfinite(d) & (d > np.float32(opt.min_depth)) & (d <= np.float32(opt.max_depth))
        if opt.conf_thresh is not None:
            ok &= conf[:, :, 0] > np.float32(opt.conf_thresh)
    return ok


def clip_points(depths, intrs, extrs, dtype=np.float32):
    """(V,T,H,W,3) world points of every pixel; ``dtype=np.float64`` runs frame_points' arithmetic on fp64 copies of the fp32 inputs
    (the inverted cameras stay the fp32 ones)."""
    V, T, _, H, W = depths.shape
    if dtype == np.float32:
        return np.stack([Q.frame_points(depths, intrs, extrs, t).reshape(V, H, W, 3) for t in range(T)], 1)
    out = np.zeros((V, T, H, W, 3))
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    pix = np.stack([xs, ys, np.ones_like(xs)], -1)
    for t in range(T):
        kinv, einv = (a.astype(np.float64) for a in Q.invert_cameras(intrs[:, t], extrs[:, t]))
        cam = np.einsum("vij,hwj->vhwi", kinv, pix) * depths[:, t, 0, :, :, None].astype(np.float64)
        out[:, t] = np.einsum("vij,vhwj->vhwi", einv[..., :3], cam) + einv[:, None, None, :, 3]
    return out


def statistics(labels, depths, intrs, extrs, opt, conf=None):
    """Rule 2 -> dict(pixels, count, out_of_range (V,T,256) int64, sums (V,T,256,3) int64, centroid (V,T,256,3) fp64)."""
    V, T, H, W = labels.shape
    lab = labels.astype(np.int64)
    ok = valid_pixels(lab, depths, opt, conf)
    pts = clip_points(depths, intrs, extrs)
    with np.errstate(invalid="ignore"):
        in_range = ok & (np.abs(pts) < np.float32(2.0 ** 18)).all(-1)  # (false for NaN and inf)
    q = np.rint(np.where(in_range[..., None], pts, 0).astype(np.float64) * 2 ** 20).astype(np.int64)
    pixels, count, oor = (np.zeros((V, T, L), np.int64) for _ in range(3))
    sums = np.zeros((V, T, L, 3), np.int64)
    for v in range(V):
        for t in range(T):
            l = lab[v, t].reshape(-1)
            pixels[v, t] = np.bincount(l, minlength=L)
            pixels[v, t, 0] = 0
            count[v, t] = np.bincount(l[in_range[v, t].reshape(-1)], minlength=L)
            oor[v, t] = np.bincount(l[(ok & ~in_range)[v, t].reshape(-1)], minlength=L)
            for c in range(3):
                np.add.at(sums[v, t, :, c], l, q[v, t, :, :, c].reshape(-1))
    return dict(pixels=pixels, count=count, out_of_range=oor, sums=sums, centroid=centroids(count, sums, opt.min_pixels))


def centroids(count, sums, min_pixels):
    ok = (count >= min_pixels) & (count > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = sums.astype(np.float64) / count.astype(np.float64)[..., None] * 2.0 ** -20
    return np.where(ok[..., None], c, np.nan)


def pair_distance(centroid, a, b, min_common):
    """Mean over the common frames, added in ascending order; None without enough of them."""
    (v, l), (u, m) = a, b
    s, n = 0.0, 0
    for t in range(centroid.shape[1]):
        p, q = centroid[v, t, l], centroid[u, t, m]
        if not (np.isnan(p[0]) or np.isnan(q[0])):
            s += float(np.sqrt(((p - q) ** 2).sum()))
            n += 1
    return s / n if n >= max(min_common, 1) else None


def matching(centroid, opt):
    """Rule 3 -> dict(global_id (V,256) int32, distance (V,256) fp64, num_objects, members, margin): ``margin`` is the smallest gap
    any decision left -- between the best distance and the threshold, and between the best and the second-best object."""
    V = centroid.shape[0]
    gid = np.full((V, L), -1, np.int32)
    dist = np.full((V, L), np.nan)
    present = [(v, l) for v in range(V) for l in range(L) if not np.isnan(centroid[v, :, l, 0]).all()]
    margin = np.inf
    if not opt.match:
        for v, l in present:
            gid[v, l] = l - 1
        n = max([l for _, l in present], default=0)
    else:
        n = 0
        for v, l in present:
            per_g = {}
            for u, m in present:
                if u < v:
                    d = pair_distance(centroid, (v, l), (u, m), opt.min_common_frames)
                    if d is not None:
                        per_g[gid[u, m]] = min(per_g.get(gid[u, m], np.inf), d)
            ranked = sorted((d, g) for g, d in per_g.items())
            if ranked:
                margin = min(margin, abs(ranked[0][0] - opt.distance_threshold))
                if len(ranked) > 1 and ranked[0][0] < opt.distance_threshold:
                    margin = min(margin, ranked[1][0] - ranked[0][0])
            if ranked and ranked[0][0] < opt.distance_threshold:
                dist[v, l], gid[v, l] = ranked[0]
            else:
                gid[v, l] = n
                n += 1
    members = {g: [(v, l) for v, l in present if gid[v, l] == g] for g in range(n)}
    return dict(global_id=gid, distance=dist, num_objects=n, members=members, margin=margin)


def object_frames(valid, members, opt, T):
    """Rule 4 for one object: valid (T,) -> (anchors, used, skipped)."""
    first = [int(np.nonzero(valid > 0)[0][0])] if (valid > 0).any() else []
    if isinstance(opt.anchor, dict):
        anchors = [opt.anchor[m] for m in members if m in opt.anchor] or first
    elif opt.anchor == "first":
        anchors = first
    else:
        anchors = [int(opt.anchor)]
    frames = set()
    for a in anchors:
        frames |= {t for t in range(a - opt.frames_before, a + opt.frames_after + 1) if 0 <= t <= T - 1}
    frames = sorted(frames)
    return anchors, [t for t in frames if valid[t] > 0], [t for t in frames if valid[t] == 0]


def object_pool(labels, depths, intrs, extrs, opt, gid, g, t, conf=None):
    """Rule 5: (raster indices, points) of the pool of (object g, frame t)."""
    V, T, H, W = labels.shape
    ok = valid_pixels(labels.astype(np.int64), depths, opt, conf)[:, t]
    obj = np.stack([gid[v][labels[v, t].astype(np.int64)] for v in range(V)]) == g
    idx = np.nonzero((ok & obj & (labels[:, t] != 0)).reshape(-1))[0]
    return idx, Q.frame_points(depths, intrs, extrs, t)[idx]


def mask_queries(labels, depths, intrs, extrs, opt, conf=None, seed=0, centres=None):
    """Rules 1-5 -> (rows (N,4) fp32, object_ids (N,) int32, objects (the report's dicts), pools [(g, t, idx, points)]).
    ``centres(pool, k, seed)``: the k-means of the "kmeans" method (the device's, handed in by the test)."""
    V, T, H, W = labels.shape
    st = statistics(labels, depths, intrs, extrs, opt, conf)
    mt = matching(st["centroid"], opt)
    nvalid = st["count"] + st["out_of_range"]
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    rows, ids, objects, pools, k = [], [], [], [], 0
    for g in range(mt["num_objects"]):
        mem = mt["members"][g]
        if not mem:
            continue
        valid = sum((nvalid[v, :, l] for v, l in mem), np.zeros(T, np.int64))
        anchors, used, skipped = object_frames(valid, mem, opt, T)
        ob = dict(object=g, members=mem, anchors=anchors, frames_used=used, frames_skipped=skipped, pool_sizes=[], rows=0)
        for t in used:
            idx, pool = object_pool(labels, depths, intrs, extrs, opt, mt["global_id"], g, t, conf)
            pools.append((g, t, idx, pool))
            ob["pool_sizes"].append(len(pool))
            if opt.max_points_per_frame is not None and len(pool) > opt.max_points_per_frame:
                if opt.method == "random":
                    pool = pool[torch.randperm(len(pool), generator=gen)[:opt.max_points_per_frame].numpy()]
                else:
                    pool = centres(pool, opt.max_points_per_frame, int(seed) + k)
            k += 1
            rows.append(np.concatenate([np.full((len(pool), 1), t, np.float32), pool], 1))
            ids.append(np.full(len(pool), g, np.int32))
            ob["rows"] += len(pool)
        objects.append(ob)
    return np.concatenate(rows), np.concatenate(ids), objects, pools, mt


# ------------------------------------------------------------------------------------------------------------- planted scenes
def exact_scene(V, T, H, W, seed=0):
    """A clip whose unprojection is exact in fp32: focal length 64 (a power of two), an integer principal point, signed-permutation
    rotations, dyadic translations, depths that are multiples of 1/8 in [0.5, 4]: every product and sum of the unprojection is a
    dyadic rational of few bits.  Returns depths (V,T,1,H,W), intrs (V,T,3,3), extrs (V,T,3,4), fp32."""
    rng = np.random.default_rng(seed)
    depths = (rng.integers(4, 33, size=(V, T, 1, H, W)) / 8.0).astype(np.float32)
    intrs = np.zeros((V, T, 3, 3), np.float32)
    intrs[:, :] = np.array([[64.0, 0, W // 2], [0, 64.0, H // 2], [0, 0, 1]], np.float32)
    perms = [np.eye(3), np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0.0]]), np.array([[0, -1, 0], [0, 0, -1], [1, 0, 0.0]]),
             np.array([[-1, 0, 0], [0, 0, 1], [0, 1, 0.0]])]
    extrs = np.zeros((V, T, 3, 4), np.float32)
    for v in range(V):
        extrs[v, :, :, :3] = perms[v % len(perms)]
        extrs[v, :, :, 3] = np.array([0.25 * v, -0.5, 1.0 + 0.125 * v], np.float32)
    return depths, intrs, extrs


def lattice_scene(instances, T, H=16, W=16, focal=32.0):
    """A clip that plants centroids exactly.  Every camera is K = diag(focal, focal, 1), E = [I | 0] and every depth is 1, so pixel
    (x, y) unprojects to (x / focal, y / focal, 1): with a power of two as focal length the labelled pixels lie on a dyadic lattice
    of the plane z = 1, a blob's centroid is the mean of a few lattice points, and centroid differences whose pixel offsets are
    3-4-5 multiples have exact distances.  ``instances[v][l]`` = {frame: (x0, y0, w, h)}: instance l of camera v is that rectangle of
    pixels in that frame.  Returns labels (V,T,H,W) uint8, depths (V,T,1,H,W), intrs (V,T,3,3), extrs (V,T,3,4)."""
    V = len(instances)
    labels = np.zeros((V, T, H, W), np.uint8)
    for v, cam in enumerate(instances):
        for l, frames in cam.items():
            for t, (x0, y0, w, h) in frames.items():
                assert 0 <= t < T and 0 <= x0 and x0 + w <= W and 0 <= y0 and y0 + h <= H and not labels[v, t, y0:y0 + h, x0:x0 + w].any(), (v, l, t)
                labels[v, t, y0:y0 + h, x0:x0 + w] = l
    depths = np.ones((V, T, 1, H, W), np.float32)
    intrs = np.broadcast_to(np.diag([focal, focal, 1.0]).astype(np.float32), (V, T, 3, 3)).copy()
    extrs = np.broadcast_to(np.eye(4, dtype=np.float32)[:3], (V, T, 3, 4)).copy()
    return labels, depths, intrs, extrs
