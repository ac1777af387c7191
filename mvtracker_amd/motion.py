"""Motion masks on the device ("Motion masks"): which pixels of a clip are static background and which move, and
how many leading frames pass before anything moves.

The reference has the detector inside its depth pipeline (mvtracker/datasets/generic_scene_dataset.py
``_static_bg_mask_from_window``: frame-to-frame absolute differences, channel mean, a ``max_pool3d`` over a temporal window and a
(2r+1)^2 patch, a threshold) and its frame-level sibling in demo.py (``_detect_static_prefix_frames``).  Here the pool's closed form
runs in ``mvt_motion_temporal`` -> ``mvt_motion_mask`` -> ``mvt_motion_report``: every frame is read once, the mask is the
reference's bit for bit, and nothing is read back for it.

    static, report = motion_masks(rgbs)                                   # (V,T,H,W) bool, MotionReport
    static, report = motion_masks(rgbs, MotionMask(window=2, patch_radius=3, diff_thresh=10 / 255))
    report.static_prefix_frames()                                         # [0, 1, ...]: the frames before anything moves
    q = sample_queries(depths, intrs, extrs, spec, motion=MotionMask(), rgbs=rgbs)   # queries on what moves

One deviation from the reference: ``boundary_mean_diff`` is summed in fp64 (exact on integer frames) where the reference sums in fp32.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from . import hip


@dataclass(frozen=True)
class MotionMask:
    """``_static_bg_mask_from_window``'s parameters, with its defaults: ``window`` frames to either side of a frame whose boundaries
    count (-1: the whole clip), ``patch_radius`` r of the (2r+1)^2 patch, ``diff_thresh`` in the frames' own units (10.0 for 0..255
    frames, 10 / 255 for 0..1 frames): a pixel is static when the largest channel-mean difference in its window and patch is below it."""
    window: int = -1
    patch_radius: int = 7
    diff_thresh: float = 10.0

    def __post_init__(self):
        w, r = self.window, self.patch_radius
        if isinstance(w, bool) or int(w) != w or not (int(w) == -1 or int(w) >= 1):
            raise ValueError(f"window must be -1 (the whole clip) or an integer >= 1, got {w!r}")
        if isinstance(r, bool) or int(r) != r or not 0 <= int(r) <= hip.MOTION_MAX_RADIUS:
            raise ValueError(f"patch_radius must be an integer in [0, {hip.MOTION_MAX_RADIUS}], got {r!r}")
        if not math.isfinite(float(self.diff_thresh)):
            raise ValueError(f"diff_thresh must be finite, got {self.diff_thresh!r}")
        object.__setattr__(self, "window", int(w))
        object.__setattr__(self, "patch_radius", int(r))
        object.__setattr__(self, "diff_thresh", float(self.diff_thresh))


def _check(motion):
    if not isinstance(motion, MotionMask):
        raise ValueError(f"motion must be a MotionMask, got {motion!r}")
    return motion


class MotionReport:
    """Figures of ``motion_masks``: ``static_fraction`` (V, T) fp64, the share of static pixels per (view, frame), and
    ``boundary_mean_diff`` (T-1,) fp64, the mean absolute difference of frames b and b + 1 over views, channels and pixels
    (demo.py ``_detect_static_prefix_frames``' ``diffs``)."""

    def __init__(self, static_fraction, boundary_mean_diff):
        self.static_fraction = np.asarray(static_fraction, np.float64)
        self.boundary_mean_diff = np.asarray(boundary_mean_diff, np.float64)

    def static_prefix_frames(self, diff_threshold=0.5, max_frames=10):
        """The demo's rule: frame 0, then frame i + 1 while ``boundary_mean_diff[i] <= diff_threshold`` and fewer than ``max_frames``
        are taken, stopping at the first failure.  The threshold is in the frames' own units (the demo's 0.5 is for 0..255 frames)."""
        frames = [0]
        for i, delta in enumerate(self.boundary_mean_diff):
            if float(delta) <= diff_threshold and len(frames) < max_frames:
                frames.append(i + 1)
            else:
                break
        return frames

    def summary(self):
        V, T = self.static_fraction.shape
        d = self.boundary_mean_diff
        peak = f"largest mean frame difference {float(d.max()):.4g} at boundary {int(d.argmax())}" if d.size else "a single frame"
        return (f"{V} views x {T} frames: {100.0 * float(self.static_fraction.mean()):.1f} % of the pixels static "
                f"(per view {', '.join(f'{100.0 * f:.1f}' for f in self.static_fraction.mean(1))}), {peak}")

    def table(self):
        V, T = self.static_fraction.shape
        rows = [f"{'frame':>5} {'mean diff':>10} " + " ".join(f"{'static v' + str(v):>10}" for v in range(V))]
        for t in range(T):
            delta = f"{self.boundary_mean_diff[t - 1]:>10.4f}" if t else f"{'':>10}"
            rows.append(f"{t:>5} {delta} " + " ".join(f"{self.static_fraction[v, t]:>10.4f}" for v in range(V)))
        return "\n".join(rows)


def clip_frames(rgbs):
    """rgbs (1,V,T,3,H,W) or (V,T,3,H,W), uint8 or float -> (V,T,3,H,W) contiguous, uint8 as it is and every float type as fp32."""
    if rgbs.dim() == 6:
        if rgbs.shape[0] != 1:
            raise ValueError(f"rgbs must be (V, T, 3, H, W) or (1, V, T, 3, H, W), got {tuple(rgbs.shape)}")
        rgbs = rgbs[0]
    if rgbs.dim() != 5 or rgbs.shape[2] != 3 or min(rgbs.shape) < 1:
        raise ValueError(f"rgbs must be (V, T, 3, H, W) or (1, V, T, 3, H, W), got {tuple(rgbs.shape)}")
    if rgbs.dtype != torch.uint8 and not rgbs.dtype.is_floating_point:
        raise ValueError(f"rgbs must be uint8 or float, got {rgbs.dtype}")
    return (rgbs if rgbs.dtype == torch.uint8 else rgbs.to(torch.float32)).contiguous()


def motion_clip(frames, motion):
    """``motion_masks`` on checked frames (V,T,3,H,W): (static (V,T,H,W) bool, MotionReport).  Three launches and one host read."""
    V, T, _, H, W = frames.shape
    dev = frames.device
    if T == 1:  # the reference's rule: a single frame is static, and there is no boundary
        return torch.ones(V, T, H, W, dtype=torch.bool, device=dev), MotionReport(np.ones((V, 1)), np.zeros(0))
    if V * T > 65535:
        raise ValueError(f"{V} views x {T} frames are too many for one call (the limit is 65535 images)")
    hip.require_device(frames)
    all_mode = motion.window == -1 or motion.window >= T - 1  # every frame's window holds every boundary: one map, pooled once
    blocks, tiles = hip.motion_blocks(H, W), hip.motion_tiles(H, W)
    diff = torch.empty(V, 1 if all_mode else T - 1, H, W, device=dev)
    partial = torch.empty(V * blocks, T - 1, device=dev, dtype=torch.float64)
    counts = torch.empty(V * (1 if all_mode else T), tiles, device=dev, dtype=torch.int32)
    static = torch.empty(V, T, H, W, device=dev, dtype=torch.bool)
    rep = torch.empty(T - 1 + V * T, device=dev, dtype=torch.float64)
    hip.motion_temporal(frames, V, T, H, W, all_mode, diff, partial)
    hip.motion_mask(diff, V, T, H, W, 0 if all_mode else motion.window, motion.patch_radius, motion.diff_thresh, static, counts)
    hip.motion_report(partial, counts, V, T, H, W, all_mode, rep)
    r = rep.cpu().numpy()  # the one host read
    return static, MotionReport(r[T - 1:].reshape(V, T) / float(H * W), r[:T - 1] / float(V * 3 * H * W))


@hip.guarded
def motion_masks(rgbs, motion=MotionMask()):
    """Static-background mask of a clip: rgbs (V,T,3,H,W) or (1,V,T,3,H,W), uint8 or float (uint8 frames go to the kernel as they
    are and give the bits of the same frames as float32).  Returns ``(static, report)``: ``static`` (V,T,H,W) bool on the device,
    True where the largest frame-to-frame difference (mean over channels) within ``motion.window`` frames and ``motion.patch_radius``
    pixels is below ``motion.diff_thresh``; ``report`` a MotionReport.  The input is not written."""
    return motion_clip(clip_frames(rgbs), _check(motion))
