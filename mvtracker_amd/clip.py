"""The checked inputs of the depth-clip features: one front end for every module that takes ``depths`` with
``intrs`` / ``extrs`` (cleaning, clustering, alignment, reprojection, scene normalisation, query sampling, mask queries), and one for
the point lists they take beside it.  Host code only: every launch goes through ``hip.<name>``, looked up at call time.

    clip = DepthClip(depths, intrs, extrs, depths_conf)                 # every shape and rank check; nothing allocated or launched
    Hp, Wp, P = clip.padded_grid()
    for t0, nt in clip.frame_chunks(MAX_CHUNK_POINTS):
        xyz = clip.clouds(t0, nt, conf_thresh)                          # (V * nt, P, 4): cloud v * nt + t
        keep[:, t0:t0 + nt] = clip.crop(search(xyz), nt) != 0
    return clip.rebatch(keep)
"""
from __future__ import annotations

from functools import cached_property

import torch

from . import hip

MAX_POINTS = (1 << 31) - 64  # points of one cloud: the launches index them with 32 bits


def frames_per_chunk(V, T, P, max_points):
    """Frames per launch sequence of V clouds of P points a frame: at most ``max_points`` points (the workspace bound) and 65535
    clouds (the launch grid's), at least one frame."""
    return max(1, min(T, max_points // (V * P), 65535 // V))


class DepthClip:
    """depths (V,T,1,H,W) with intrs (V,T,3,3), extrs (V,T,3,4) and ``depths_conf`` like depths or None, checked.  ``batch``:
    "either" takes them as they are or all with a leading batch of 1, "required" only with it.  Keeps ``V, T, H, W, dev, batched``
    and the tensors in clip rank as the caller gave them (``depths, intrs, extrs, depths_conf``); everything converted or computed
    (``d``, ``K``, ``E``, ``conf``, ``kinv`` / ``einv``) is made when first asked for."""

    def __init__(self, depths, intrs, extrs, depths_conf=None, batch="either"):
        self.batched = batch == "required" or depths.dim() == 6
        lead = (1,) if self.batched else ()
        if depths.dim() != 5 + len(lead) or tuple(depths.shape[:len(lead)]) != lead or depths.shape[-3] != 1:
            want = "depths must be (1, V, T, 1, H, W)" if batch == "required" else "depths must be (V, T, 1, H, W) or (1, V, T, 1, H, W)"
            raise ValueError(f"{want}, got {tuple(depths.shape)}")
        V, T, _, H, W = depths.shape[-5:]
        if tuple(intrs.shape) != lead + (V, T, 3, 3) or tuple(extrs.shape) != lead + (V, T, 3, 4):
            raise ValueError(f"intrs / extrs must be {lead + (V, T, 3, 3)} / {lead + (V, T, 3, 4)}, got {tuple(intrs.shape)} / {tuple(extrs.shape)}")
        if depths_conf is not None and tuple(depths_conf.shape) != tuple(depths.shape):
            raise ValueError(f"depths_conf must have the shape of depths, got {tuple(depths_conf.shape)}")
        hip.require_device(depths)
        self.V, self.T, self.H, self.W, self.dev = V, T, H, W, depths.device
        self.depths, self.intrs, self.extrs, self.depths_conf = (self.squeeze(t) for t in (depths, intrs, extrs, depths_conf))

    def squeeze(self, x):
        """A tensor of the call in clip rank: without the leading batch where the clip came with one."""
        return x[0] if (self.batched and x is not None) else x

    def rebatch(self, x):
        """A result in the rank of the inputs: with the leading batch where the clip came with one."""
        return x[None] if self.batched else x

    @cached_property
    def d(self):
        """depths (V,T,1,H,W) fp32 contiguous."""
        return self.depths.to(torch.float32).contiguous()

    @cached_property
    def K(self):
        """intrs (V,T,9) fp32 contiguous."""
        return self.intrs.to(torch.float32).reshape(self.V, self.T, 9).contiguous()

    @cached_property
    def E(self):
        """extrs (V,T,12) fp32 contiguous."""
        return self.extrs.to(torch.float32).reshape(self.V, self.T, 12).contiguous()

    @cached_property
    def _conf32(self):
        return self.depths_conf.to(torch.float32).contiguous()

    def conf(self, thresh):
        """The confidence map (V,T,1,H,W) fp32 contiguous for a rule ``conf > thresh``; None without a map or without a threshold."""
        return None if (self.depths_conf is None or thresh is None) else self._conf32

    @cached_property
    def _inverse(self):
        n = self.V * self.T
        kinv = torch.empty(n, 9, device=self.dev)
        einv = torch.empty(n, 12, device=self.dev)
        hip.invert_cameras(self.K.reshape(n, 9), self.E.reshape(n, 12), kinv, einv, n)
        return kinv, einv

    kinv = property(lambda self: self._inverse[0], doc="inverse intrinsics (V*T, 9): one launch, at the first request for either")
    einv = property(lambda self: self._inverse[1], doc="camera-to-world extrinsics (V*T, 12)")

    def padded_grid(self):
        """(Hp, Wp, P = Hp * Wp): the grid of one cloud, padded to multiples of 8 (the 8 x 8 tiles of the cloud searches)."""
        Hp, Wp = (self.H + 7) // 8 * 8, (self.W + 7) // 8 * 8
        if Hp * Wp >= MAX_POINTS:
            raise ValueError(f"a cloud of {Hp} x {Wp} points is too large (the limit is 2^31 per launch)")
        return Hp, Wp, Hp * Wp

    def frame_chunks(self, max_points):
        """(t0, nt) of the clip's frames in runs of ``frames_per_chunk``."""
        step = frames_per_chunk(self.V, self.T, self.padded_grid()[2], max_points)
        return [(t0, min(step, self.T - t0)) for t0 in range(0, self.T, step)]

    def clouds(self, t0, nt, conf_thresh, sphere=None):
        """The padded clouds of frames [t0, t0 + nt): xyz (V * nt, P, 4), cloud v * nt + t, NaN rows where a pixel is not valid
        (depth finite and > 0, conf > conf_thresh with both given, inside ``sphere`` = (cx, cy, cz, radius) when given)."""
        xyz = torch.empty(self.V * nt, self.padded_grid()[2], 4, device=self.dev)
        hip.clean_points(self.d, self.conf(conf_thresh), self.kinv, self.einv, self.V, self.T, t0, nt, self.H, self.W, conf_thresh, sphere, xyz)
        return xyz

    def crop(self, x, nt):
        """Per-point results x (V * nt, P, ...) of ``clouds(t0, nt, ..)`` as images (V, nt, H, W, ...), the padding cut off."""
        Hp, Wp, _ = self.padded_grid()
        return x.reshape(self.V, nt, Hp, Wp, *x.shape[2:])[:, :, :self.H, :self.W]


def list_cloud(points, what="points", empty_ok=False):
    """A point list (M, 3) on the device as one cloud (1, M, 4) fp32: rows with a coordinate that is not finite become NaN rows,
    which take no part in any search; w = 0."""
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{what} must be (M, 3), got {tuple(points.shape)}")
    M = points.shape[0]
    if M == 0 and not empty_ok:
        raise ValueError(f"{what} is empty")
    if M >= MAX_POINTS:
        raise ValueError(f"{M} points are too many (the limit is 2^31 per launch)")
    hip.require_device(points)
    p = points.to(torch.float32)
    xyz = torch.zeros(1, M, 4, device=points.device)
    xyz[0, :, :3] = torch.where(torch.isfinite(p).all(1, keepdim=True), p, torch.full((), float("nan"), device=points.device))
    return xyz
