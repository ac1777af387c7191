"""Depth cleaning on the device ("Depth cleaning"): statistical or radius outlier removal of every (view, frame)
cloud, so that flying pixels at depth edges do not become neighbours of the tracks that pass near them.

The reference's demo does this for display only (``--clean_pointcloud``: utils/visualizer_rerun.py ``_clean_point_cloud_with_open3d``,
Open3D's ``remove_statistical_outlier`` / ``remove_radius_outlier`` on each (view, frame) cloud); here the same rules run in
``mvt_clean_points`` -> ``mvt_tile_aabb`` -> ``mvt_tile_group_aabb`` -> ``mvt_clean_search`` -> ``mvt_clean_mask`` with no host read.

    c = DepthCleaning("statistical", nb_neighbors=20, std_ratio=2.0)               # the reference's pc_clean_cfg keys and defaults
    depths_clean, keep = clean_depths(depths, intrs, extrs, c, depths_conf=conf)   # depths_clean = where(keep, depths, 0)
    out = predictor(rgbs=..., depths=..., ..., depth_cleaning=c)                   # cleaned before normalisation and resize
    keep = clean_point_cloud(points, c)                                            # an unorganised (M, 3) cloud
"""
from __future__ import annotations

import math

import torch

from . import hip
from .clip import DepthClip, list_cloud

METHODS = ("statistical", "radius")
MAX_CHUNK_POINTS = 1 << 23  # padded points searched per launch sequence: under 22 bytes of workspace each, 176 MiB in all


class DepthCleaning:
    """The reference's ``pc_clean_cfg``: ``method`` "statistical" (``nb_neighbors``, ``std_ratio``) or "radius" (``radius``,
    ``min_points``), and which pixels enter a cloud at all: ``conf_thresh`` (with a confidence map: conf > conf_thresh) and the
    reference's ``sphere_radius_crop`` (``sphere_radius`` around ``sphere_center``, strict)."""

    def __init__(self, method="statistical", nb_neighbors=20, std_ratio=2.0, radius=0.05, min_points=5, conf_thresh=None, sphere_radius=None,
                 sphere_center=(0.0, 0.0, 0.0)):
        if method not in METHODS:
            raise ValueError(f"method must be one of {METHODS}, got {method!r}")
        if int(nb_neighbors) != nb_neighbors or not 1 <= int(nb_neighbors) <= hip.CLEAN_MAX_K:
            raise ValueError(f"nb_neighbors must be an integer in 1..{hip.CLEAN_MAX_K}, got {nb_neighbors!r}")
        if not math.isfinite(float(std_ratio)):
            raise ValueError(f"std_ratio must be finite, got {std_ratio!r}")
        if not (math.isfinite(float(radius)) and float(radius) > 0.0):
            raise ValueError(f"radius must be finite and positive, got {radius!r}")
        if int(min_points) != min_points or int(min_points) < 0:
            raise ValueError(f"min_points must be an integer >= 0, got {min_points!r}")
        if conf_thresh is not None and not math.isfinite(float(conf_thresh)):
            raise ValueError(f"conf_thresh must be finite, got {conf_thresh!r}")
        if sphere_radius is not None and not (math.isfinite(float(sphere_radius)) and float(sphere_radius) > 0.0):
            raise ValueError(f"sphere_radius must be finite and positive, got {sphere_radius!r}")
        centre = tuple(float(v) for v in sphere_center)
        if len(centre) != 3 or not all(math.isfinite(v) for v in centre):
            raise ValueError(f"sphere_center must be three finite numbers, got {sphere_center!r}")
        self.method = method
        self.nb_neighbors, self.std_ratio = int(nb_neighbors), float(std_ratio)
        self.radius, self.min_points = float(radius), int(min_points)
        self.conf_thresh = None if conf_thresh is None else float(conf_thresh)
        self.sphere_radius = None if sphere_radius is None else float(sphere_radius)
        self.sphere_center = centre

    def __repr__(self):
        return (f"DepthCleaning(method={self.method!r}, nb_neighbors={self.nb_neighbors}, std_ratio={self.std_ratio}, radius={self.radius}, "
                f"min_points={self.min_points}, conf_thresh={self.conf_thresh}, sphere_radius={self.sphere_radius}, "
                f"sphere_center={self.sphere_center})")

    @property
    def mode(self):
        return hip.CLEAN_STATISTICAL if self.method == "statistical" else hip.CLEAN_RADIUS

    @property
    def sphere(self):
        return None if self.sphere_radius is None else (*self.sphere_center, self.sphere_radius)


def _check(cleaning):
    if not isinstance(cleaning, DepthCleaning):
        raise ValueError(f"cleaning must be a DepthCleaning, got {cleaning!r}")
    return cleaning


def search_clouds(xyz, n_clouds, n_points, grid, cleaning):
    """The points-level entry: clouds xyz (n_clouds, n_points, 4) on the device, NaN rows taking no part; ``grid`` = (w, h) of an
    organised cloud (multiples of 8, w * h = n_points) or (0, 0) for a point list.  Returns (values, state, keep), all on the device:
    values (n_clouds, n_points) = the mean neighbour distance a (fp32, statistical) or the neighbour count c (int32, radius),
    state (n_clouds, 4) fp64 = (M, mu, sigma, thr), keep (n_clouds, n_points) uint8."""
    c = _check(cleaning)
    dev = xyz.device
    box, gbox = hip.cloud_boxes(xyz, n_clouds, n_points, grid)
    stat = c.mode == hip.CLEAN_STATISTICAL
    values = torch.empty(n_clouds, n_points, device=dev, dtype=torch.float32 if stat else torch.int32)
    hip.clean_search(xyz, n_clouds, n_points, grid, c.mode, c.nb_neighbors, c.radius, c.min_points, box, gbox,
                     a_out=values if stat else None, c_out=None if stat else values)
    state = torch.empty(n_clouds, 4, device=dev, dtype=torch.float64)
    keep = torch.empty(n_clouds, n_points, device=dev, dtype=torch.uint8)
    hip.clean_mask(values if stat else None, None if stat else values, n_clouds, n_points, c.mode, c.std_ratio, c.min_points, state, keep)
    return values, state, keep


def clean_clip(depths, intrs, extrs, cleaning, depths_conf=None, details=False):
    """``clean_depths`` without the ``where``: the bool keep mask of the shape of ``depths``; with ``details`` also the per-pixel
    search values (V,T,H,W), the cloud states (V,T,4) and the clouds' points (V,T,H,W,4)."""
    c = _check(cleaning)
    clip = DepthClip(depths, intrs, extrs, depths_conf)
    V, T, H, W, dev = clip.V, clip.T, clip.H, clip.W, clip.dev
    Hp, Wp, P = clip.padded_grid()
    keep = torch.empty(V, T, H, W, device=dev, dtype=torch.bool)
    vals = states = pts = None
    if details:
        vals = torch.empty(V, T, H, W, device=dev, dtype=torch.float32 if c.mode == hip.CLEAN_STATISTICAL else torch.int32)
        states = torch.empty(V, T, 4, device=dev, dtype=torch.float64)
        pts = torch.empty(V, T, H, W, 4, device=dev)
    for t0, nt in clip.frame_chunks(MAX_CHUNK_POINTS):  # frames per launch sequence: bounded workspace
        xyz = clip.clouds(t0, nt, c.conf_thresh, c.sphere)
        v_, s_, k_ = search_clouds(xyz, V * nt, P, (Wp, Hp), c)
        keep[:, t0:t0 + nt] = clip.crop(k_, nt) != 0
        if details:
            vals[:, t0:t0 + nt] = clip.crop(v_, nt)
            states[:, t0:t0 + nt] = s_.reshape(V, nt, 4)
            pts[:, t0:t0 + nt] = clip.crop(xyz, nt)
    keep = clip.rebatch(keep.reshape(V, T, 1, H, W))
    return (keep, vals, states, pts) if details else keep


@hip.guarded
def clean_depths(depths, intrs, extrs, cleaning, depths_conf=None):
    """Outlier removal of every (view, frame) cloud of a clip.  depths (V,T,1,H,W) or (1,V,T,1,H,W) with intrs / extrs (and
    ``depths_conf``) of the same rank, as ``EvaluationPredictor.forward`` takes them.  A pixel is valid when its depth is finite and
    > 0, its confidence exceeds ``cleaning.conf_thresh`` (both given) and its point lies inside the sphere crop (given); the valid
    pixels of one depth map are one cloud, searched against itself.  Returns ``(depths_clean, keep)``: ``keep`` bool of the shape of
    ``depths`` (False on pixels that are not valid), ``depths_clean = where(keep, depths, 0)``.  The inputs are not written."""
    keep = clean_clip(depths, intrs, extrs, cleaning, depths_conf)
    return torch.where(keep, depths, torch.zeros((), dtype=depths.dtype, device=depths.device)), keep


@hip.guarded
def clean_point_cloud(points, cleaning):
    """The reference function's own signature on an unorganised cloud: points (M, 3) on the device -> keep (M,) bool.  Rows with a
    coordinate that is not finite take no part and come back False."""
    c = _check(cleaning)
    xyz = list_cloud(points, empty_ok=True)
    M = points.shape[0]
    if M == 0:
        return torch.zeros(0, dtype=torch.bool, device=points.device)
    return search_clouds(xyz, 1, M, (0, 0), c)[2][0] != 0
