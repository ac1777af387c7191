"""Rigid object motion on the device ("Rigid motion"): from the tracks of segmented objects, one rigid pose per
object and frame, the tracks that do not move with their object, occluded points put where their object says they are, and dense
object points carried through the clip.

    res = predictor(rgbs, depths, q, intrs, extrs, query_groups=ids, rigid_motion=RigidMotion())
    motion = predictor.last_rigid_motion                       # or rigid_motion(traj_e[0], vis_e[0], q[0, :, 0].int(), ids)
    filled, where = fill_tracks(res["traj_e"][0], res["vis_e"][0], motion)
    pts, oid, _ = lift_masks(labels, depths, intrs, extrs, frame=3)
    moved = move_points(pts, oid, motion, frame=3)             # (T,M,3): the objects' dense points in every frame

The rules (``mvt_rigid_members`` / ``mvt_rigid_fit`` / ``mvt_rigid_compose`` / ``mvt_rigid_move`` / ``mvt_rigid_fill``):

* ``object_ids[i]`` in [0, G) names track i's object; any other id (-1) means none: the track takes no part, its ``residual`` is
  NaN and its ``inliers`` False.  ``G = num_objects``, or the largest id + 1 when that is None -- reading that maximum is the one
  host read of ``rigid_motion``.
* Object g's reference frame ``r_g`` is the largest query frame of its members (clamped to the clip), so that every member is live
  from it on; ``P_i = tracks[r_g, i]``, ``Q_i(t) = tracks[t, i]`` and ``poses[g, t]`` maps the reference configuration to frame t:
  ``Q ~ R P + t``.  An object without members has ``reference_frames = -1`` and status 1 everywhere.
* Member i has base weight 1 at frame t when ``t >= query_frames[i]`` (or ``live_before_query``, for tracks of a backward-tracking
  call), with ``use_visibility`` when it is visible at t and at ``r_g``, and when ``P_i`` and ``Q_i(t)`` are finite.
* The fit is the weighted Kabsch solution: centroids, ``H = sum w (Q - qbar)(P - pbar)^T``, the PROPER rotation that maximises
  ``tr(R^T H)`` (the reference's ``align_umeyama`` with its sign on the smallest singular direction; ``procrustes_analysis``, which
  negates a row of R, is not followed: that is not the optimum), ``t = qbar - R pbar``; fp64 throughout, rounded to fp32 once.
* Iteration 0 uses the base weights, each of the ``iterations - 1`` refits ``base and residual of the previous fit <=
  inlier_threshold``.  A refit that keeps fewer than ``min_points`` members, or a degenerate set, is dropped and the previous fit
  stands.
* ``status``: 0 fitted; 1 fewer than ``min_points`` base members; 2 degenerate: the second-largest eigenvalue of the weighted
  covariance of P over the weight sum is below ``min_spread^2`` (collinear or coincident members).  Where it is not 0 the pose,
  ``rmse`` and the members' ``residual`` are NaN.
* ``residual`` = ``|R P_i + t - Q_i|`` of the fit that stood, for every member, live or not; ``inliers = base and residual <=
  inlier_threshold``; ``used = sum base``; ``rmse`` over the inliers.

Repeatability: all sums are fp64 in a fixed order, so two runs give the same bits, and the results of a frame depend only on that
frame's rows and the reference frame's rows -- a later streaming session can push frame blocks and get the bits of the whole clip.
There is no CPU path.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from . import hip

STATUS_NAMES = {hip.RIGID_OK: "ok", hip.RIGID_TOO_FEW: "too few", hip.RIGID_DEGENERATE: "degenerate"}
REPLACE = {"occluded": hip.RIGID_FILL_OCCLUDED, "outliers": hip.RIGID_FILL_OUTLIERS}


def _int(name, v, lo, hi=None):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer)) or int(v) != v or int(v) < lo or (hi is not None and int(v) > hi):
        raise ValueError(f"{name} must be an integer in [{lo}, {'inf' if hi is None else hi}], got {v!r}")
    return int(v)


@dataclass(frozen=True)
class RigidMotion:
    """``inlier_threshold``: a member moves with its object when it lies within this distance (scene units) of where the pose puts
    it.  ``iterations``: fits per (object, frame), the first on all live members, the others on the inliers of the one before.
    ``min_points``: members a fit needs (at least 3).  ``use_visibility``: only members visible at the frame and at the reference
    frame enter a fit.  ``min_spread``: the extent (standard deviation along their second axis) the members' reference points
    need; below it the object is degenerate.  ``live_before_query``: members also count before their query frame."""
    inlier_threshold: float = 0.02
    iterations: int = 3
    min_points: int = 4
    use_visibility: bool = True
    min_spread: float = 1e-3
    live_before_query: bool = False

    def __post_init__(self):
        set_ = lambda k, v: object.__setattr__(self, k, v)
        for k in ("inlier_threshold", "min_spread"):
            v = getattr(self, k)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)) or float(v) < 0:
                raise ValueError(f"{k} must be finite and not negative, got {v!r}")
            set_(k, float(v))
        set_("iterations", _int("iterations", self.iterations, 1, hip.RIGID_MAX_ITERATIONS))
        set_("min_points", _int("min_points", self.min_points, 3))
        for k in ("use_visibility", "live_before_query"):
            if not isinstance(getattr(self, k), bool):
                raise ValueError(f"{k} must be a bool, got {getattr(self, k)!r}")


def _check(options):
    if not isinstance(options, RigidMotion):
        raise ValueError(f"options must be a RigidMotion, got {options!r}")
    return options


def _readback(t):
    """The one host read of ``rigid_motion``: the largest object id, when ``num_objects`` is not given."""
    return int(t.item())


def _ints(name, t, n, dev):
    """(n,) integers on ``dev`` -> int32, contiguous."""
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.shape[0] != n or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"{name} must be ({n},) integers, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__} "
                         f"{getattr(t, 'dtype', '')}")
    if t.device != dev:
        raise ValueError(f"{name} on {t.device}, tracks on {dev}")
    return t.to(torch.int32).contiguous()


def _tracks(tracks, visibility):
    if not isinstance(tracks, torch.Tensor) or tracks.dim() != 3 or tracks.shape[2] != 3 or tracks.dtype != torch.float32 or min(tracks.shape) < 1:
        raise ValueError(f"tracks must be (T, N, 3) fp32, got {tuple(tracks.shape) if isinstance(tracks, torch.Tensor) else tracks!r} "
                         f"{getattr(tracks, 'dtype', '')}")
    T, N = tracks.shape[:2]
    if not isinstance(visibility, torch.Tensor) or tuple(visibility.shape) != (T, N) or visibility.dtype != torch.bool:
        raise ValueError(f"visibility must be ({T}, {N}) bool, got {tuple(visibility.shape) if isinstance(visibility, torch.Tensor) else visibility!r} "
                         f"{getattr(visibility, 'dtype', '')}")
    if visibility.device != tracks.device:
        raise ValueError(f"visibility on {visibility.device}, tracks on {tracks.device}")
    if T > hip.RIGID_MAX_FRAMES:
        raise ValueError(f"at most {hip.RIGID_MAX_FRAMES} frames per call, got {T}")
    return tracks.contiguous(), visibility.contiguous(), T, N


class RigidMotionResult:
    """On the device: ``poses`` (G,T,4,4) fp32, ``reference_frames`` (G,) int32, ``inliers`` (T,N) bool, ``residual`` (T,N) fp32,
    ``used`` / ``inlier_count`` / ``status`` (G,T) int32, ``rmse`` (G,T) fp32; ``options``, and the ``query_frames`` / ``object_ids``
    (int32) the call was made with, which ``fill_tracks`` reads.  ``summary()`` and ``table()`` read the (G,T) tables back."""

    def __init__(self, options, query_frames, object_ids, G, T, N, dev):
        self.options, self.query_frames, self.object_ids = options, query_frames, object_ids
        self.num_objects, self.num_frames, self.num_tracks = G, T, N
        self.poses = torch.empty(G, T, 4, 4, device=dev)
        self.reference_frames = torch.empty(G, dtype=torch.int32, device=dev)
        self.inliers = torch.empty(T, N, dtype=torch.bool, device=dev)
        self.residual = torch.empty(T, N, device=dev)
        self.used, self.inlier_count, self.status = (torch.empty(G, T, dtype=torch.int32, device=dev) for _ in range(3))
        self.rmse = torch.empty(G, T, device=dev)

    def _host(self):
        return {k: getattr(self, k).cpu().numpy() for k in ("reference_frames", "used", "inlier_count", "status", "rmse")}

    def summary(self):
        h = self._host()
        G, T = self.num_objects, self.num_frames
        ok = h["status"] == hip.RIGID_OK
        worst = float(np.nanmax(h["rmse"])) if np.isfinite(h["rmse"]).any() else float("nan")
        dropped = int((h["used"] - h["inlier_count"])[ok].sum())
        return (f"{G} objects x {T} frames: {int(ok.sum())} poses, {int((h['status'] == hip.RIGID_TOO_FEW).sum())} with too few members, "
                f"{int((h['status'] == hip.RIGID_DEGENERATE).sum())} degenerate; {dropped} of {int(h['used'][ok].sum())} live track points "
                f"do not move with their object (threshold {self.options.inlier_threshold:g}), worst rmse {worst:.4g}")

    def table(self):
        h = self._host()
        rows = [f"{'object':>6} {'ref':>4} {'frames ok':>9} {'too few':>7} {'degen.':>6} {'used':>8} {'inliers':>8} {'mean rmse':>10} {'max rmse':>10}"]
        for g in range(self.num_objects):
            s, e = h["status"][g], h["rmse"][g]
            ok = s == hip.RIGID_OK
            fin = e[np.isfinite(e)]
            mean, top = (f"{fin.mean():.5f}", f"{fin.max():.5f}") if fin.size else ("-", "-")
            rows.append(f"{g:>6} {int(h['reference_frames'][g]):>4} {int(ok.sum()):>9} {int((s == hip.RIGID_TOO_FEW).sum()):>7} "
                        f"{int((s == hip.RIGID_DEGENERATE).sum()):>6} {int(h['used'][g][ok].sum()):>8} {int(h['inlier_count'][g][ok].sum()):>8} "
                        f"{mean:>10} {top:>10}")
        return "\n".join(rows)


@hip.guarded
def rigid_motion(tracks, visibility, query_frames, object_ids, options=RigidMotion(), num_objects=None):
    """tracks (T,N,3) fp32, visibility (T,N) bool, query_frames (N,) integers, object_ids (N,) integers (-1: no object) ->
    ``RigidMotionResult``.  Two entries (six launches); with ``num_objects`` nothing is read back."""
    opt = _check(options)
    tracks, visibility, T, N = _tracks(tracks, visibility)
    dev = tracks.device
    qf, ids = _ints("query_frames", query_frames, N, dev), _ints("object_ids", object_ids, N, dev)
    if num_objects is None:
        G = max(_readback(ids.max()) + 1, 0)
    else:
        G = _int("num_objects", num_objects, 0, hip.RIGID_MAX_OBJECTS)
    if G > hip.RIGID_MAX_OBJECTS:
        raise ValueError(f"at most {hip.RIGID_MAX_OBJECTS} objects, got ids up to {G - 1}")
    res = RigidMotionResult(opt, qf, ids, G, T, N, dev)
    if G == 0:  # no object at all: nothing to fit
        res.residual.fill_(float("nan"))
        res.inliers.fill_(False)
        return res
    hip.require_device(tracks)
    counts = torch.empty(G, dtype=torch.int32, device=dev)
    offsets = torch.empty(G + 1, dtype=torch.int32, device=dev)
    members = torch.empty(N, dtype=torch.int32, device=dev)
    hip.rigid_members(ids, qf, N, G, T, counts, offsets, members, res.reference_frames)
    hip.rigid_fit(tracks, visibility, qf, ids, offsets, members, res.reference_frames, T, N, G, opt.inlier_threshold, opt.iterations, opt.min_points,
                  opt.use_visibility, opt.min_spread, opt.live_before_query, res.poses, res.residual, res.inliers, res.used, res.inlier_count,
                  res.rmse, res.status)
    return res


def _motion(motion):
    if not isinstance(motion, RigidMotionResult):
        raise ValueError(f"motion must be a RigidMotionResult, got {motion!r}")
    return motion


def move_points(points, point_objects, motion, frame=None):
    """points (M,3) fp32 of the objects ``point_objects`` (M,) integers -> (T,M,3) fp32: every point in every frame.  ``frame=None``:
    the points are in their object's reference configuration, the output is ``pose[g,t] p``; ``frame=f``: they were observed at frame
    f (``lift_masks(..., frame=f)``), the output is ``pose[g,t] pose[g,f]^-1 p``, the product formed in fp64 once per (g, t).
    NaN for a point of no object and where the pose at t (with ``frame=f`` also the one at f) has a status other than 0."""
    m = _motion(motion)
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError(f"points must be (M, 3) fp32, got {tuple(points.shape) if isinstance(points, torch.Tensor) else points!r} "
                         f"{getattr(points, 'dtype', '')}")
    M, dev, G, T = points.shape[0], m.poses.device, m.num_objects, m.num_frames
    if points.device != dev:
        raise ValueError(f"points on {points.device}, the motion on {dev}")
    ids = _ints("point_objects", point_objects, M, dev)
    if frame is not None:
        frame = _int("frame", frame, 0, T - 1)
    out = torch.empty(T, M, 3, device=dev)
    if M == 0:
        return out
    if G == 0:
        return out.fill_(float("nan"))
    with hip.device_guard(points):
        hip.require_device(points)
        xf = torch.empty(G, T, 3, 4, dtype=torch.float64, device=dev)
        hip.rigid_compose(m.poses, m.status, G, T, frame, xf)
        hip.rigid_move(points.contiguous(), ids, xf, M, T, G, out)
    return out


def fill_tracks(tracks, visibility, motion, replace=("occluded",)):
    """-> (tracks_filled (T,N,3) fp32, filled (T,N) bool).  Where a member of an object has a status-0 pose and is live, its point
    becomes ``pose P_i`` if it is not visible (``"occluded"`` in ``replace``) or not an inlier (``"outliers"``); everything else
    keeps its bits.  ``tracks`` and ``visibility`` are those ``motion`` was computed from."""
    m = _motion(motion)
    if isinstance(replace, str):
        replace = (replace,)
    replace = tuple(replace)
    if not replace or any(r not in REPLACE for r in replace):
        raise ValueError(f'replace must name "occluded" and / or "outliers", got {replace!r}')
    tracks, visibility, T, N = _tracks(tracks, visibility)
    if (T, N) != (m.num_frames, m.num_tracks) or tracks.device != m.poses.device:
        raise ValueError(f"tracks ({T}, {N}, 3) on {tracks.device} are not those of the motion: ({m.num_frames}, {m.num_tracks}, 3) on "
                         f"{m.poses.device}")
    out = torch.empty_like(tracks)
    filled = torch.empty(T, N, dtype=torch.bool, device=tracks.device)
    if m.num_objects == 0:
        return out.copy_(tracks), filled.fill_(False)
    with hip.device_guard(tracks):
        hip.require_device(tracks)
        hip.rigid_fill(tracks, visibility, m.inliers, m.query_frames, m.object_ids, m.reference_frames, m.poses, m.status, T, N, m.num_objects,
                       sum(REPLACE[r] for r in set(replace)), m.options.live_before_query, out, filled)
    return out, filled
