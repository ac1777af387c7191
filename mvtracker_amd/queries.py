"""Query points for clips without labels, sampled from depth on the device ("Query sampling").

The reference's evaluator does this for every generic dataset (evaluation/evaluator_3dpt.py:286-388): per row of a
``sampling_spec = [(t, z_min, z_max, radius, count, method), ...]`` it unprojects every pixel of frame ``t`` of all views, keeps
the confident points inside a cylinder and draws ``count`` of them, at random (``method == ""``) or as the k-means centres of the
pool (``method == "kmeans"``, sklearn on one CPU thread).  Here the pool is built by ``mvt_query_pool`` (one frame read in place,
order-preserving compaction) and the centres by the ``mvt_kmeans_*`` kernels (greedy k-means++ seeding, Lloyd iterations with
fixed-point integer accumulation: two runs give the same bits).  There is no CPU path.

    q = sample_queries(depths, intrs, extrs, DEFAULT_SPEC, depths_conf=conf)       # (1, N, 4), ready for forward / open_stream
    centres, info = kmeans_centres(points, 1000)
"""
from __future__ import annotations

import math

import torch

from . import hip
from .clip import DepthClip

DEFAULT_SPEC = [(0, -0.1, 4.2, 2.1, 1000, "kmeans")]  # the evaluator's row for unknown datasets (:341-343)
LLOYD_CHUNK = 8  # Lloyd iterations enqueued between two reads of the device's converged flag


def frame_pool(depths, kinv, einv, t, conf=None, conf_threshold=0.9, centre=(0.0, 0.0), radius=math.inf, z_min=-math.inf, z_max=math.inf,
               radius_inclusive=False):
    """Candidate pool of frame ``t``: depths (V,T,1,H,W) fp32 contiguous [conf: the same layout], kinv / einv (V*T, 9 / 12) ->
    (M, 3) points in the reference's order (view, row, column).  One host read (M) at the end."""
    V, T, _, H, W = depths.shape
    dev = depths.device
    n = V * H * W
    pool = torch.empty(n, 3, device=dev)
    count = torch.zeros(1, device=dev, dtype=torch.int32)
    blocks = torch.empty((n + 255) // 256, device=dev, dtype=torch.int32)
    r2 = float(torch.tensor(float(radius) ** 2, dtype=torch.float32))  # the comparison torch makes: fp32 r^2 against fp32(radius ** 2)
    hip.query_pool(depths, conf, kinv, einv, V, T, int(t), H, W, float(conf_threshold), float(centre[0]), float(centre[1]), r2, float(z_min),
                   float(z_max), pool, count, blocks, radius_inclusive=radius_inclusive)
    return pool[:int(count.item())]


def _km_begin(points, count, tol):
    """Workspace of one k-means run + the statistics pass (bounding box, fixed-point scales, stopping threshold)."""
    M, k, dev = points.shape[0], int(count), points.device
    if k < 1 or k > hip.KMEANS_MAX_K:
        raise ValueError(f"count must be in [1, {hip.KMEANS_MAX_K}] (the centres live in LDS), got {k}")
    if M == 0 or k > M:
        raise ValueError(f"k-means needs at least count = {k} points, got {M}")
    w = {"pts": points, "M": M, "k": k,
         "state": torch.zeros(hip.KM_WORDS, device=dev, dtype=torch.int64),
         "centres": torch.empty(k, 3, device=dev),
         "labels": torch.empty(M, device=dev, dtype=torch.int32),
         "acc": torch.zeros(k, 4, device=dev, dtype=torch.int64),
         "min_d2": torch.empty(M, device=dev),
         "partials": torch.empty(hip.KMEANS_MAX_CAND * hip.KMEANS_SEED_BLOCKS, device=dev, dtype=torch.int64),
         "stat": torch.empty(hip.KMEANS_STAT_BLOCKS * 6, device=dev, dtype=torch.float64)}
    hip.kmeans_stats(points, M, float(tol), w["stat"], w["state"])
    return w


def _km_seed(w, seed):
    hip.kmeans_seed(w["pts"], w["M"], w["k"], int(seed), w["min_d2"], w["partials"], w["centres"], w["state"])


def _km_state(w):
    s = w["state"].cpu()
    f = s.view(torch.float64)
    return {"inertia": float(f[hip.KM_INERTIA]), "iterations": int(s[hip.KM_ITER]), "converged": bool(s[hip.KM_CONVERGED]),
            "empty": int(s[hip.KM_EMPTY])}


def _km_lloyd(w, max_iter):
    """Lloyd iterations in chunks of LLOYD_CHUNK (the converged flag is read once per chunk; launches behind it are empty), then
    one assignment against the final centres for the reported labels, inertia and empty clusters."""
    done = 0
    while done < max_iter:
        n = min(LLOYD_CHUNK, max_iter - done)
        hip.kmeans_iterate(w["pts"], w["M"], w["centres"], w["k"], w["labels"], w["acc"], w["state"], n, max_iter)
        done += n
        if _km_state(w)["converged"]:
            break
    run = _km_state(w)
    hip.kmeans_assign(w["pts"], w["M"], w["centres"], w["k"], w["labels"], w["acc"], w["state"], max_iter, final_pass=True)
    hip.kmeans_update(w["centres"], w["k"], w["acc"], w["state"], max_iter, final_pass=True)
    info = _km_state(w)
    info["iterations"], info["converged"] = run["iterations"], run["converged"]
    return info


@hip.guarded
def kmeans_centres(points, count, seed=0, max_iter=300, tol=1e-4):
    """(count, 3) k-means centres of points (N, 3) and info = {inertia, iterations, converged, empty}.  ``len(points) <= count``
    returns the points unchanged (reference :46-47).  Stopping is sklearn's: squared centre shift <= tol * mean variance."""
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be (N, 3), got {tuple(points.shape)}")
    if int(count) < 1:
        raise ValueError(f"count must be at least 1, got {count}")
    if int(max_iter) < 1:
        raise ValueError("max_iter must be at least 1")
    if len(points) == 0:
        raise ValueError("k-means on an empty pool")
    if len(points) <= count:
        return points, {"inertia": 0.0, "iterations": 0, "converged": True, "empty": 0}
    if int(count) > hip.KMEANS_MAX_K:
        raise ValueError(f"count must be at most {hip.KMEANS_MAX_K} (the centres live in LDS), got {count}")
    hip.require_device(points)
    pts = points.to(torch.float32).contiguous()
    if not bool(torch.isfinite(pts).all()):
        raise ValueError("k-means needs finite points")
    w = _km_begin(pts, count, tol)
    _km_seed(w, seed)
    info = _km_lloyd(w, int(max_iter))
    return w["centres"], info


def _region_mask(d, conf, intrs, extrs, t, region, poses):
    """(mask (V,1,1,H,W) bool, RegionReport) of frame t: ``cluster.region_clip`` on that frame alone."""
    from . import cluster
    pose = None
    if region.box is not None:
        p = torch.as_tensor(poses)
        pose = p if p.dim() == 2 else p[t]
    return cluster.region_clip(d[:, t:t + 1], intrs[:, t:t + 1], extrs[:, t:t + 1], pose, region, None if conf is None else conf[:, t:t + 1])


def _region_pool(d, conf, mask, kinv, einv, t, conf_threshold, centre, radius, z_min, z_max, radius_inclusive):
    """``frame_pool`` of frame t with the pixels outside ``mask`` taken out: the frame is copied with depth 0 (and confidence -inf)
    there, so the pool's rule and order are the unrestricted pool's."""
    V, T = d.shape[:2]
    d_t = torch.where(mask, d[:, t:t + 1], torch.zeros((), device=d.device)).contiguous()
    conf_t = None if conf is None else torch.where(mask, conf[:, t:t + 1], torch.full((), -math.inf, device=d.device)).contiguous()
    return frame_pool(d_t, kinv.reshape(V, T, 9)[:, t].contiguous(), einv.reshape(V, T, 12)[:, t].contiguous(), 0, conf_t, conf_threshold, centre,
                      radius, z_min, z_max, radius_inclusive)


@hip.guarded
def sample_queries(depths, intrs, extrs, spec, depths_conf=None, conf_threshold=0.9, centre=(0.0, 0.0), seed=0, radius_inclusive=False,
                   region=None, region_poses=None, region_reports=None, motion=None, rgbs=None, motion_keep="moving", motion_reports=None):
    """Query points (1, N, 4) = (t, x, y, z) in world space for a clip depths (1,V,T,1,H,W), intrs (1,V,T,3,3), extrs (1,V,T,3,4).

    ``spec``: the reference's rows (t, z_min, z_max, radius, count, method).  A row's pool: the pixels of frame t of all views whose
    confidence exceeds ``conf_threshold`` (``depths_conf`` (1,V,T,1,H,W); without it: whose depth is positive) and that lie in the
    cylinder (x-cx)^2 + (y-cy)^2 < radius^2 (``radius_inclusive``: <=, demo.py's rule), z_min <= z <= z_max around ``centre``.
    method "": a seeded permutation of the pool (CPU generator), its first ``count`` rows; "kmeans": the k-means centres, a pool of
    at most ``count`` points whole.  Rows with t >= T or an empty pool are skipped; rows are concatenated in spec order.

    ``region`` (a ``cluster.RegionCluster``) with ``region_poses`` ((4, 4) or (T, 4, 4) world_T_region): a row's pool is restricted,
    before the draw or the k-means, to the pixels of frame t that ``cluster.region_masks`` selects: the largest cluster inside the
    region's box, per view.  The two confidence rules are applied one after the other: which pixels enter the clustered cloud is the
    region's own rule (depth > 0, and with ``region.conf_thresh`` set: conf > region.conf_thresh), so with ``region.conf_thresh``
    None the cluster forms over pixels of any confidence; ``conf_threshold`` then drops pixels from the pool as it does without a
    region.  A frame's mask is computed once, whatever the number of rows that name it; ``region_reports``: a dict that receives
    {t: RegionReport} of those frames.  Without a region nothing of that runs.

    ``motion`` (a ``motion.MotionMask``) with ``rgbs`` (the clip's frames, (1,V,T,3,H,W) or (V,T,3,H,W), uint8 or float): a row's
    pool is restricted, before the draw or the k-means, to the pixels of frame t that ``motion.motion_masks`` calls moving
    (``motion_keep="static"``: static).  With a region as well a pixel must pass both.  The clip's mask is computed once per call,
    whatever the number of rows; ``motion_reports``: a dict that receives {"clip": MotionReport}.  Without ``motion`` nothing of that
    runs."""
    for row in spec:
        if row[5] not in ("", "kmeans"):
            raise NotImplementedError(f"sampling method {row[5]!r} (the reference knows '' and 'kmeans')")
    clip = DepthClip(depths, intrs, extrs, depths_conf, batch="required")
    V, T, H, W, dev = clip.V, clip.T, clip.H, clip.W, clip.dev
    if region is not None:  # (refused before any launch)
        from . import cluster
        if not isinstance(region, cluster.RegionCluster):
            raise ValueError(f"region must be a RegionCluster, got {region!r}")
        if region.box is not None:
            if region_poses is None:
                raise ValueError("a region with a box needs region_poses: (4, 4) or (T, 4, 4) world_T_region")
            cluster.invert_poses(region_poses, T)
    elif region_poses is not None:
        raise ValueError("region_poses without a region")
    frames = None
    if motion is not None:  # (refused before any launch)
        from . import motion as motion_
        if not isinstance(motion, motion_.MotionMask):
            raise ValueError(f"motion must be a MotionMask, got {motion!r}")
        if motion_keep not in ("moving", "static"):
            raise ValueError(f"motion_keep must be 'moving' or 'static', got {motion_keep!r}")
        if rgbs is None:
            raise ValueError("motion needs rgbs: the clip's frames (1, V, T, 3, H, W)")
        frames = motion_.clip_frames(rgbs)
        if (frames.shape[0], frames.shape[1], frames.shape[3], frames.shape[4]) != (V, T, H, W):
            raise ValueError(f"rgbs {tuple(rgbs.shape)} and depths {tuple(depths.shape)} differ in (V, T, H, W)")
    elif rgbs is not None:
        raise ValueError("rgbs without motion")
    d, conf, kinv, einv = clip.d, clip.conf(conf_threshold), clip.kinv, clip.einv
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    out = []
    masks = {}  # frame -> (mask, report): rows that share a frame share the mask
    static = None  # (V,T,H,W) of the whole clip, computed at the first row that needs it
    for i, (t, z_min, z_max, radius, count, method) in enumerate(spec):
        if t >= T:
            continue
        mask = None
        if region is not None:
            if t not in masks:
                masks[t] = _region_mask(d, conf, clip.intrs, clip.extrs, t, region, region_poses)
                if region_reports is not None:
                    region_reports[t] = masks[t][1]
            mask = masks[t][0]
        if motion is not None:
            if static is None:
                static, report = motion_.motion_clip(frames, motion)
                if motion_reports is not None:
                    motion_reports["clip"] = report
            keep = (static[:, t] if motion_keep == "static" else ~static[:, t])[:, None, None]  # (V,1,1,H,W)
            mask = keep if mask is None else mask & keep
        if mask is None:
            pool = frame_pool(d, kinv, einv, t, conf, conf_threshold, centre, radius, z_min, z_max, radius_inclusive)
        else:
            pool = _region_pool(d, conf, mask, kinv, einv, t, conf_threshold, centre, radius, z_min, z_max, radius_inclusive)
        if pool.shape[0] == 0:
            continue
        if method == "":
            pts = pool[torch.randperm(pool.shape[0], generator=g)[:count].to(dev)]
        else:
            pts = kmeans_centres(pool, count, seed=int(seed) + i)[0]
        out.append(torch.cat([torch.full((pts.shape[0], 1), float(t), device=dev), pts], 1))
    if not out:
        raise ValueError("every row of the sampling spec gave an empty pool (frame beyond the clip, no valid depth, or a cylinder that "
                         "holds no point): widen the radius or the z range")
    return torch.cat(out, 0)[None]
