"""Region clustering on the device ("Region clustering"): DBSCAN of point clouds and the box-and-cluster rule that
says which points belong to the thing at a pose, so that queries can be put "on the gripper" or "on the object near this pose".

The reference does this per (camera, frame) cloud on the CPU (conversions/droid/mark_gripper_points.py ``classify_gripper_points``:
an oriented box around the end effector's pose, ``sklearn.cluster.DBSCAN(eps=0.03, min_samples=12)`` on the points inside, the
largest cluster); here the same rules run in ``mvt_clean_points`` -> ``mvt_cluster_crop`` -> ``mvt_tile_aabb`` ->
``mvt_tile_group_aabb`` -> ``mvt_cluster_count`` -> ``mvt_cluster_link`` -> ``mvt_cluster_border`` -> ``mvt_cluster_finish`` with
no host read on the way.  The labels are sklearn's, numbering included: they are a function of the cloud alone.

    region = RegionCluster()                                                          # the reference's box, eps and min_samples
    labels = cluster_points(points, eps=0.03, min_samples=12)                         # (M,) int32, -1 = noise
    on_it = select_region_points(points, world_T_gripper, region)                     # (M,) bool, the reference function
    mask, report = region_masks(depths, intrs, extrs, poses, region)                  # per (view, frame) cloud
    q = sample_queries(depths, intrs, extrs, spec, region=region, region_poses=poses)

One deviation from the reference: the clouds are clustered in world coordinates, not in the region's frame.  A rigid motion changes
distances by rounding only.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import hip
from .clip import DepthClip, list_cloud

DEFAULT_BOX = ((-0.08, 0.08), (-0.07, 0.07), (-0.04, 0.18))  # the reference's GRIPPER_BOUNDS (metres, the end effector's frame)
MAX_CHUNK_POINTS = 1 << 23  # padded points clustered per launch sequence: under 31 bytes of workspace each, 260 MB in all
STATE_FIELDS = ("candidates", "core", "clusters", "chosen", "chosen_size", "noise", "fallback", "status")
FALLBACKS = {0: "", hip.CLUSTER_FEW: "few", hip.CLUSTER_NONE: "none", hip.CLUSTER_EMPTY: "empty"}


class RegionCluster:
    """``classify_gripper_points``' parameters: ``box`` = ((xlo, xhi), (ylo, yhi), (zlo, zhi)) in the region's frame (None: no crop),
    DBSCAN's ``eps`` and ``min_samples``, and which pixels of a depth map enter a cloud at all: ``conf_thresh`` (with a confidence
    map: conf > conf_thresh)."""

    def __init__(self, box=DEFAULT_BOX, eps=0.03, min_samples=12, conf_thresh=None):
        if box is not None:
            try:
                b = tuple((float(lo), float(hi)) for lo, hi in box)
            except (TypeError, ValueError):
                raise ValueError(f"box must be three (lo, hi) pairs or None, got {box!r}") from None
            if len(b) != 3 or not all(math.isfinite(lo) and math.isfinite(hi) and lo < hi for lo, hi in b):
                raise ValueError(f"box must be three finite (lo, hi) pairs with lo < hi, got {box!r}")
            box = b
        self.box = box
        self.eps, self.min_samples = check_dbscan(eps, min_samples)
        if conf_thresh is not None and not math.isfinite(float(conf_thresh)):
            raise ValueError(f"conf_thresh must be finite, got {conf_thresh!r}")
        self.conf_thresh = None if conf_thresh is None else float(conf_thresh)

    def __repr__(self):
        return f"RegionCluster(box={self.box}, eps={self.eps}, min_samples={self.min_samples}, conf_thresh={self.conf_thresh})"

    @property
    def bounds(self):
        return None if self.box is None else tuple(v for pair in self.box for v in pair)


def check_dbscan(eps, min_samples):
    if not (math.isfinite(float(eps)) and float(eps) > 0.0):
        raise ValueError(f"eps must be finite and positive, got {eps!r}")
    if int(min_samples) != min_samples or not 1 <= int(min_samples) < (1 << 30):
        raise ValueError(f"min_samples must be an integer >= 1, got {min_samples!r}")
    return float(eps), int(min_samples)


def _check(region):
    if not isinstance(region, RegionCluster):
        raise ValueError(f"region must be a RegionCluster, got {region!r}")
    return region


def radius_sq(eps):
    """The neighbour test's threshold: fp32(eps * eps), rounded once on the host."""
    return float(torch.tensor(float(eps) ** 2, dtype=torch.float32))


def invert_poses(poses, n=None):
    """world_T_region (4, 4) or (n, 4, 4) -> region_T_world (n, 3, 4) fp32 on the host: inverted in fp64, rounded once."""
    p = torch.as_tensor(np.asarray(poses.detach().cpu() if isinstance(poses, torch.Tensor) else poses, dtype=np.float64))
    if tuple(p.shape) == (4, 4):
        p = p[None].expand(1 if n is None else n, 4, 4)
    if p.dim() != 3 or tuple(p.shape[1:]) != (4, 4) or (n is not None and p.shape[0] != n):
        raise ValueError(f"poses must be (4, 4) or ({'T' if n is None else n}, 4, 4) world_T_region, got {tuple(p.shape)}")
    if not bool(torch.isfinite(p).all()):
        raise ValueError("poses must be finite")
    try:
        inv = torch.linalg.inv(p.contiguous())
    except RuntimeError as e:
        raise ValueError(f"poses must be invertible: {e}") from None
    return inv[:, :3].to(torch.float32).contiguous()


def cluster_clouds(xyz, n_clouds, n_points, grid, eps, min_samples, region_T_world=None, bounds=None):
    """The points-level entry: clouds xyz (n_clouds, n_points, 4) on the device, NaN rows taking no part; ``grid`` = (w, h) of
    organised clouds or (0, 0).  With ``region_T_world`` (n_clouds, 3, 4) fp32 on the device and ``bounds`` the clouds are cropped
    first, IN PLACE.  Returns dict(labels int32, select uint8, core uint8: (n_clouds, n_points); state (n_clouds, 8) int64), all on
    the device and none of them read here."""
    eps, min_samples = check_dbscan(eps, min_samples)
    dev = xyz.device
    if bounds is not None:
        hip.cluster_crop(xyz, n_clouds, n_points, region_T_world, bounds)
    box, gbox = hip.cloud_boxes(xyz, n_clouds, n_points, grid)
    r2 = radius_sq(eps)
    core = torch.empty(n_clouds, n_points, device=dev, dtype=torch.uint8)
    parent = torch.empty(n_clouds, n_points, device=dev, dtype=torch.int32)
    root = torch.empty(n_clouds, n_points, device=dev, dtype=torch.int32)
    labels = torch.empty(n_clouds, n_points, device=dev, dtype=torch.int32)
    select = torch.empty(n_clouds, n_points, device=dev, dtype=torch.uint8)
    state = torch.empty(n_clouds, hip.CLUSTER_STATE_WORDS, device=dev, dtype=torch.int64)
    hip.cluster_count(xyz, n_clouds, n_points, grid, r2, min_samples, box, gbox, core)
    hip.cluster_link(xyz, n_clouds, n_points, grid, r2, box, gbox, core, parent, state)
    hip.cluster_border(xyz, n_clouds, n_points, grid, r2, box, gbox, core, parent, root)
    hip.cluster_finish(xyz, n_clouds, n_points, min_samples, core, root, parent, labels, select, state)  # (parent: now the workspace)
    return {"labels": labels, "select": select, "core": core, "state": state}


def check_status(state):
    """Raises when a union-find loop of the device gave up (it never does on a cloud the entries accept); state on the host."""
    bad = torch.nonzero(state.reshape(-1, hip.CLUSTER_STATE_WORDS)[:, hip.CLUSTER_STATUS])
    if bad.numel():
        raise hip.HipError(f"region clustering: a union-find loop exceeded its bound in cloud {int(bad[0])}")


def _info(row):
    return {k: int(v) for k, v in zip(STATE_FIELDS, row.tolist())}


@hip.guarded
def cluster_points(points, eps=0.03, min_samples=12, return_info=False):
    """``sklearn.cluster.DBSCAN(eps, min_samples).fit_predict`` on a point list: points (M, 3) on the device -> labels (M,) int32,
    -1 for noise and for rows that are not finite.  ``return_info``: also a dict of the cloud's state row (candidates, core,
    clusters, chosen, chosen_size, noise, fallback, status) plus ``core`` (M,) bool."""
    eps, min_samples = check_dbscan(eps, min_samples)
    xyz = list_cloud(points, empty_ok=True)
    M = points.shape[0]
    if M == 0:
        labels = torch.zeros(0, dtype=torch.int32, device=points.device)
        info = dict(_info(torch.tensor([0, 0, 0, -1, 0, 0, hip.CLUSTER_EMPTY, 0])), core=torch.zeros(0, dtype=torch.bool, device=points.device))
        return (labels, info) if return_info else labels
    r = cluster_clouds(xyz, 1, M, (0, 0), eps, min_samples)
    state = r["state"].cpu()
    check_status(state)
    if return_info:
        return r["labels"][0], dict(_info(state[0]), core=r["core"][0] != 0)
    return r["labels"][0]


@hip.guarded
def select_region_points(points, pose, region=None):
    """The reference function's own signature: points (M, 3) in world space on the device, ``pose`` (4, 4) world_T_region ->
    (M,) bool, True on the points of the largest cluster inside the region's box (all points in the box when there are fewer than
    min_samples of them or no cluster forms)."""
    c = RegionCluster() if region is None else _check(region)
    xyz = list_cloud(points, empty_ok=True)
    M = points.shape[0]
    if M == 0:
        return torch.zeros(0, dtype=torch.bool, device=points.device)
    rtw = invert_poses(pose, 1).to(points.device) if c.box is not None else None
    r = cluster_clouds(xyz, 1, M, (0, 0), c.eps, c.min_samples, rtw, c.bounds)
    check_status(r["state"].cpu())
    return r["select"][0] != 0


class RegionReport:
    """Per (view, frame) figures of ``region_masks``: int64 arrays (V, T) ``candidates`` (points inside the box), ``core``,
    ``clusters``, ``chosen`` (id of the largest cluster, -1 without one), ``chosen_size``, ``noise``, ``fallback`` (0 none, 1 few
    candidates, 2 no cluster, 3 empty), ``status`` and ``selected`` (pixels of the mask)."""

    def __init__(self, states, selected):
        s = np.asarray(states, np.int64)
        for i, k in enumerate(STATE_FIELDS):
            setattr(self, k, s[..., i].copy())
        self.selected = np.asarray(selected, np.int64)

    def summary(self):
        n = self.candidates.size
        fb = {name: int((self.fallback == code).sum()) for code, name in FALLBACKS.items() if code}
        return (f"{n} clouds: {int(self.selected.sum())} points selected of {int(self.candidates.sum())} in the box, "
                f"{float(self.clusters.mean()) if n else 0.0:.2f} clusters per cloud, fallbacks few {fb['few']} none {fb['none']} empty {fb['empty']}")

    def table(self):
        head = f"{'view':>4} {'frame':>5} {'in box':>8} {'core':>8} {'clusters':>8} {'chosen':>6} {'size':>8} {'noise':>8} {'selected':>8} fallback"
        rows = [head]
        V, T = self.candidates.shape
        for v in range(V):
            for t in range(T):
                rows.append(f"{v:>4} {t:>5} {self.candidates[v, t]:>8} {self.core[v, t]:>8} {self.clusters[v, t]:>8} {self.chosen[v, t]:>6} "
                            f"{self.chosen_size[v, t]:>8} {self.noise[v, t]:>8} {self.selected[v, t]:>8} {FALLBACKS[int(self.fallback[v, t])]}")
        return "\n".join(rows)


def region_clip(depths, intrs, extrs, poses, region, depths_conf=None, details=False):
    """``region_masks`` whose ``details`` stay in clip rank: (mask bool of the shape of ``depths``, RegionReport); with ``details``
    also the labels (V,T,H,W) int32, the core flags (V,T,H,W) bool and the cropped clouds' points (V,T,H,W,4)."""
    c = _check(region)
    clip = DepthClip(depths, intrs, extrs, depths_conf)
    V, T, H, W, dev = clip.V, clip.T, clip.H, clip.W, clip.dev
    rtw = None
    if c.box is not None:
        if poses is None:
            raise ValueError("a region with a box needs poses: (4, 4) or (T, 4, 4) world_T_region")
        rtw = invert_poses(poses, T)  # (T, 3, 4) on the host
    Hp, Wp, P = clip.padded_grid()
    mask = torch.empty(V, T, H, W, device=dev, dtype=torch.bool)
    states = torch.empty(V, T, hip.CLUSTER_STATE_WORDS, device=dev, dtype=torch.int64)
    labels = cores = pts = None
    if details:
        labels = torch.empty(V, T, H, W, device=dev, dtype=torch.int32)
        cores = torch.empty(V, T, H, W, device=dev, dtype=torch.bool)
        pts = torch.empty(V, T, H, W, 4, device=dev)
    for t0, nt in clip.frame_chunks(MAX_CHUNK_POINTS):  # frames per launch sequence: bounded workspace
        xyz = clip.clouds(t0, nt, c.conf_thresh)
        m = None if rtw is None else rtw[t0:t0 + nt][None].expand(V, nt, 3, 4).reshape(V * nt, 3, 4).contiguous().to(dev)  # cloud = v * nt + t
        r = cluster_clouds(xyz, V * nt, P, (Wp, Hp), c.eps, c.min_samples, m, c.bounds)
        mask[:, t0:t0 + nt] = clip.crop(r["select"], nt) != 0
        states[:, t0:t0 + nt] = r["state"].reshape(V, nt, hip.CLUSTER_STATE_WORDS)
        if details:
            labels[:, t0:t0 + nt] = clip.crop(r["labels"], nt)
            cores[:, t0:t0 + nt] = clip.crop(r["core"], nt) != 0
            pts[:, t0:t0 + nt] = clip.crop(xyz, nt)
    tail = torch.cat([states.reshape(V * T, -1), mask.reshape(V * T, -1).sum(1, keepdim=True)], 1).cpu()  # the one host read
    check_status(tail[:, :hip.CLUSTER_STATE_WORDS])
    report = RegionReport(tail[:, :hip.CLUSTER_STATE_WORDS].reshape(V, T, -1).numpy(), tail[:, -1].reshape(V, T).numpy())
    mask = clip.rebatch(mask.reshape(V, T, 1, H, W))
    return (mask, report, labels, cores, pts) if details else (mask, report)


@hip.guarded
def region_masks(depths, intrs, extrs, poses, region, depths_conf=None, details=False):
    """Which pixels lie on the thing at ``poses``: depths (V,T,1,H,W) or (1,V,T,1,H,W) with intrs / extrs (and ``depths_conf``) of
    the same rank, ``poses`` (4, 4) or (T, 4, 4) world_T_region.  A pixel is valid when its depth is finite and > 0 and its
    confidence exceeds ``region.conf_thresh`` (both given); the valid pixels of one depth map whose points lie strictly inside the
    region's box are one cloud, clustered on its own, and its largest cluster is the mask (every point in the box when there are
    fewer than ``min_samples`` or no cluster forms).  Returns ``(mask, report)``: ``mask`` bool of the shape of ``depths``, ``report``
    a RegionReport.  The inputs are not written."""
    return region_clip(depths, intrs, extrs, poses, region, depths_conf, details)
