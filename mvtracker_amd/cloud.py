"""Cloud preparation on the device ("Cloud preparation"): PCA normals and voxel downsampling of point clouds, the
two steps the reference takes before every ICP run.

The reference does both with Open3D (conversions/droid/utils/optimization.py ``estimate_normals``:
``estimate_normals(KDTreeSearchParamHybrid(radius=0.05, max_nn=30))``, and ``downsample_pointcloud``: ``voxel_down_sample``); here the
same rules run in ``mvt_tile_aabb`` -> ``mvt_tile_group_aabb`` -> ``mvt_normals_estimate`` and in ``mvt_voxel_bounds`` ->
``mvt_voxel_insert`` -> ``mvt_voxel_emit``.

    normals = estimate_normals(points, radius=0.05, max_nn=30)               # (M, 3); NaN rows where there is no normal
    small, counts, first = voxel_downsample(points, 0.02)                    # one row per occupied voxel, the mean of its points
    T, fitness, rmse = align_point_clouds(source, small, None, 0.05, 30)     # normals of the target estimated on the way

One deviation from Open3D: a point with fewer than 3 neighbours, or whose neighbours are collinear, gets a NaN normal (and so takes
no part in ICP); Open3D leaves (0, 0, 1) there.
"""
from __future__ import annotations

import math

import torch

from . import hip
from .clip import list_cloud


def check_normal_search(radius, max_nn):
    """(radius, max_nn) as the search takes them; radius may be +inf (plain kNN)."""
    if not float(radius) > 0.0:
        raise ValueError(f"radius must be positive (inf: no radius), got {radius!r}")
    if int(max_nn) != max_nn or not 3 <= int(max_nn) <= hip.NORMALS_MAX_NN:
        raise ValueError(f"max_nn must be an integer in 3..{hip.NORMALS_MAX_NN}, got {max_nn!r}")
    return float(radius), int(max_nn)


def normals_of_clouds(xyz, n_clouds, n_points, grid, radius, max_nn, nrm=None, box=None, gbox=None, viewpoint=None, details=False):
    """The points-level entry: clouds xyz (n_clouds, n_points, 4) on the device, NaN rows taking no part; ``grid`` = (w, h) of
    organised clouds or (0, 0).  ``box`` / ``gbox``: the clouds' boxes when the caller has them already (else built here).
    Returns nrm (n_clouds, n_points, 4), with ``details`` also (nbr_idx, nbr_cnt, cov)."""
    radius, max_nn = check_normal_search(radius, max_nn)
    dev = xyz.device
    if box is None:
        box, gbox = hip.cloud_boxes(xyz, n_clouds, n_points, grid)
    if nrm is None:
        nrm = torch.empty(n_clouds, n_points, 4, device=dev)
    idx = cnt = cov = None
    if details:
        idx = torch.empty(n_clouds, n_points, max_nn, dtype=torch.int32, device=dev)
        cnt = torch.empty(n_clouds, n_points, dtype=torch.int32, device=dev)
        cov = torch.empty(n_clouds, n_points, 6, dtype=torch.float64, device=dev)
    hip.normals_estimate(xyz, n_clouds, n_points, grid, max_nn, radius, box, gbox, nrm, viewpoint, idx, cnt, cov)
    return (nrm, idx, cnt, cov) if details else nrm


@hip.guarded
def estimate_normals(points, radius=0.05, max_nn=30, viewpoint=None, return_neighbors=False):
    """Open3D's ``estimate_normals(KDTreeSearchParamHybrid(radius, max_nn))`` on a point list: points (M, 3) on the device ->
    normals (M, 3) fp32, unit eigenvectors of the smallest eigenvalue of the covariance of each point's neighbours (itself and up to
    max_nn - 1 others strictly within radius).  Rows that are not finite, rows with fewer than 3 neighbours and rows whose neighbours
    are collinear come back NaN.  ``viewpoint`` (3 numbers): normals are turned towards it; else the sign is left as it falls.
    ``return_neighbors``: also (indices (M, max_nn) int32 padded with -1, counts (M,) int32, -1 for rows taking no part)."""
    radius, max_nn = check_normal_search(radius, max_nn)
    vp = None
    if viewpoint is not None:
        v = [float(x) for x in (viewpoint.tolist() if isinstance(viewpoint, torch.Tensor) else viewpoint)]
        if len(v) != 3 or not all(math.isfinite(x) for x in v):
            raise ValueError(f"viewpoint must be three finite numbers, got {viewpoint!r}")
        vp = v
    xyz = list_cloud(points)
    M = points.shape[0]
    vpt = None if vp is None else torch.tensor([vp], dtype=torch.float32, device=points.device)
    out = normals_of_clouds(xyz, 1, M, (0, 0), radius, max_nn, viewpoint=vpt, details=return_neighbors)
    if return_neighbors:
        return out[0][0, :, :3], out[1][0], out[2][0]
    return out[0, :, :3]


@hip.guarded
def voxel_downsample(points, voxel_size, return_labels=False):
    """Open3D's ``voxel_down_sample``: points (M, 3) on the device -> ``(points (Mv, 3) fp32, counts (Mv,) int32, first (Mv,) int32)``:
    per occupied voxel of the grid with origin (minimum - voxel_size / 2) the mean of its points, their number and the smallest
    input index among them; rows in ascending ``first``.  Rows that are not finite take no part.  ``return_labels``: also labels
    (M,) int32, the output row of every input point (-1: no part).  The one host read is of Mv, to size the results, and the status
    word beside it."""
    if not (math.isfinite(float(voxel_size)) and float(voxel_size) > 0.0):
        raise ValueError(f"voxel_size must be finite and positive, got {voxel_size!r}")
    xyz = list_cloud(points)[0]
    dev, M = points.device, points.shape[0]
    cap = hip.voxel_capacity(M)
    state = torch.zeros(hip.VOXEL_STATE_WORDS, dtype=torch.int64, device=dev)
    partial = torch.empty(hip.VOXEL_BOUND_BLOCKS * 4, dtype=torch.float64, device=dev)
    table = torch.empty(cap * hip.VOXEL_SLOT_WORDS, dtype=torch.int64, device=dev)
    blocks = torch.empty((M + 255) // 256, dtype=torch.int32, device=dev)
    out = torch.empty(M, 4, device=dev)
    counts = torch.empty(M, dtype=torch.int32, device=dev)
    first = torch.empty(M, dtype=torch.int32, device=dev)
    labels = torch.empty(M, dtype=torch.int32, device=dev) if return_labels else None
    tail = torch.zeros(2, dtype=torch.int64, device=dev)  # (Mv, status): one read
    n_out = tail[:1].view(torch.int32)[:1]
    hip.voxel_bounds(xyz, M, float(voxel_size), partial, state)
    hip.voxel_insert(xyz, M, state, table, cap)
    hip.voxel_emit(xyz, M, state, table, cap, blocks, out, counts, first, n_out, labels)
    tail[1:] = state[hip.VOXEL_STATUS:hip.VOXEL_STATUS + 1]
    mv, status = tail.tolist()  # the one host read
    if status & hip.VOXEL_RANGE:
        raise ValueError(f"voxel_size {voxel_size!r} is too small for this cloud: more than 2^21 cells along an axis")
    if status:
        raise hip.HipError(f"voxel table full (status {status})")
    res = (out[:mv, :3], counts[:mv], first[:mv])
    return res + (labels,) if return_labels else res
