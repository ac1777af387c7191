"""Scene normalisation on the device ("Scene normalisation"): the step between a clip in the user's own units and
a scene of the size the weights were trained on (floor near z = 0, cameras about 6 units from the centre).

The reference does this in its dataset for every generic scene (datasets/generic_scene_dataset.py:288-358
``compute_auto_scene_normalization``, applied with datasets/utils.py:210-301 ``transform_scene``).  Here ``mvt_scene_stats`` reads
the normalisation frame in place and leaves the kept count, the centroid and the two quantiles on the device (exact order
statistics by radix select, no sort), and ``mvt_scene_apply`` / ``mvt_scene_tracks`` apply X' = t + R (s X) or undo it.

    T = auto_scene_normalization(depths, intrs, extrs, depths_conf=conf)           # a SceneTransform
    out = predictor(rgbs=..., depths=..., ..., scene_transform=T)                  # or scene_transform="auto"; tracks come back
    d, e, q, _ = T.apply(depths=depths, extrs=extrs, query_points=queries)         # in the caller's world
    tracks = T.restore_tracks(traj_in_model_space)
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import hip
from .clip import DepthClip

MIN_POINTS = 100  # a view with fewer valid pixels is left out; fewer kept points in all is an error (reference :314-315, :330-331)
FLOOR_QUANTILE, RADIUS_QUANTILE = 0.12, 0.95


class SceneTransform:
    """X' = translation + rotation @ (scale * X) (``transform_scene``'s definition), as small host numbers."""

    def __init__(self, scale, rotation=None, translation=(0.0, 0.0, 0.0)):
        self.scale = float(scale)
        self.rotation = np.eye(3) if rotation is None else np.array(torch.as_tensor(rotation).detach().cpu().numpy(), dtype=np.float64)
        self.translation = np.array(torch.as_tensor(translation).detach().cpu().numpy(), dtype=np.float64).reshape(-1)
        if not (math.isfinite(self.scale) and self.scale > 0.0):
            raise ValueError(f"scale must be finite and positive, got {self.scale}")
        if self.rotation.shape != (3, 3) or self.translation.shape != (3,):
            raise ValueError(f"rotation must be 3x3 and translation 3, got {self.rotation.shape} and {self.translation.shape}")
        if not (np.isfinite(self.rotation).all() and np.isfinite(self.translation).all()):
            raise ValueError("rotation and translation must be finite")
        if np.abs(self.rotation @ self.rotation.T - np.eye(3)).max() > 1e-3:  # the reference's assert (utils.py:233-238)
            raise ValueError("The rotation matrix should be orthonormal.")

    def __repr__(self):
        return f"SceneTransform(scale={self.scale!r}, rotation={self.rotation.tolist()!r}, translation={self.translation.tolist()!r})"

    def __eq__(self, other):
        return (isinstance(other, SceneTransform) and self.scale == other.scale and np.array_equal(self.rotation, other.rotation)
                and np.array_equal(self.translation, other.translation))

    def params(self):
        """(s, R row-major, t): the 13 numbers the kernels take."""
        return [self.scale, *self.rotation.reshape(-1).tolist(), *self.translation.tolist()]

    def inverse(self):
        """X = R^T (X' - t) / s, in the same form: scale 1/s, rotation R^T, translation -R^T t / s."""
        rt = self.rotation.T
        return SceneTransform(1.0 / self.scale, rt, -(rt @ self.translation) / self.scale)

    def apply(self, depths=None, extrs=None, query_points=None, tracks=None):
        """(depths, extrs, query_points, tracks) transformed, on the device, ``None`` where nothing was given.  depths (..., H, W)
        are multiplied by the scale, extrs (..., 3, 4) right-multiplied by the rigid inverse with their translation scaled,
        query_points (..., 4) and tracks (..., 3) mapped; a leading batch dimension of 1 is kept as it is."""
        first = next((t for t in (depths, extrs, query_points, tracks) if t is not None), None)
        if first is None:
            return None, None, None, None
        if extrs is not None and tuple(extrs.shape[-2:]) != (3, 4):
            raise ValueError(f"extrs must be (..., 3, 4), got {tuple(extrs.shape)}")
        if query_points is not None and query_points.shape[-1] != 4:
            raise ValueError(f"query points must be (..., 4), got {tuple(query_points.shape)}")
        if tracks is not None and tracks.shape[-1] != 3:
            raise ValueError(f"tracks must be (..., 3), got {tuple(tracks.shape)}")
        with hip.device_guard(first):
            hip.require_device(first)
            f32 = lambda t: None if t is None or t.numel() == 0 else t.to(torch.float32).contiguous()
            d, e, q, tr = f32(depths), f32(extrs), f32(query_points), f32(tracks)
            do, eo, qo = (None if t is None else torch.empty_like(t) for t in (d, e, q))
            p = self.params()
            if d is not None or e is not None or q is not None:
                hip.scene_apply(p, d, do, e, eo, q, qo)
            tro = None
            if tr is not None:
                tro = torch.empty_like(tr)
                hip.scene_tracks(p, tr, tro)
            keep = lambda src, out: out if out is not None else (None if src is None else src.to(torch.float32))  # (an empty tensor)
            return keep(depths, do), keep(extrs, eo), keep(query_points, qo), keep(tracks, tro)

    def restore_tracks(self, traj):
        """Tracks of the transformed scene back in the caller's world."""
        return self.inverse().apply(tracks=traj)[3]


def scene_statistics(depths, intrs, extrs, depths_conf=None, conf_thresh=4.8, frame=0, radius_quantile=None):
    """The pool statistics of frame ``frame`` as the kernels leave them, still on the device: (state int64 (SN_WORDS,), the frame's
    world->camera translation columns (V, 3) fp64).  Inputs as ``forward`` takes them (1,V,T,...)."""
    clip = DepthClip(depths, intrs, extrs, depths_conf, batch="required")
    V, T, H, W, dev = clip.V, clip.T, clip.H, clip.W, clip.dev
    if not 0 <= int(frame) < T:
        raise ValueError(f"frame {frame} outside the clip of {T} frames")
    state = torch.empty(hip.SN_WORDS, device=dev, dtype=torch.int64)
    keys = torch.empty(V * H * W, device=dev, dtype=torch.int32)
    partial = torch.empty(hip.SCENE_BLOCKS * 3, device=dev, dtype=torch.float64)
    iws = torch.empty(hip.SELECT_WS_WORDS + V, device=dev, dtype=torch.int32)
    hip.scene_stats(clip.d, clip.conf(conf_thresh), clip.kinv, clip.einv, V, T, int(frame), H, W, float(conf_thresh), MIN_POINTS, FLOOR_QUANTILE,
                    radius_quantile, keys, partial, iws, state)
    return state, clip.E[:, int(frame), 3::4].to(torch.float64)


def read_statistics(state):
    """The state words as a dict of host numbers (one read)."""
    s = state.cpu()
    f = s.view(torch.float64)
    return {"M": int(s[hip.SN_M]), "centroid": f[hip.SN_CENTROID:hip.SN_CENTROID + 3].numpy().copy(), "z_quantile": float(f[hip.SN_Z_QUANTILE]),
            "floor_z": float(f[hip.SN_FLOOR]), "z_lo": float(f[hip.SN_Z_LO]), "z_hi": float(f[hip.SN_Z_HI]), "z_rank": int(s[hip.SN_Z_RANK]),
            "radius_quantile": float(f[hip.SN_R_QUANTILE]), "r_lo": float(f[hip.SN_R_LO]), "r_hi": float(f[hip.SN_R_HI]),
            "r_rank": int(s[hip.SN_R_RANK]), "nonfinite": int(s[hip.SN_NONFINITE])}


@hip.guarded
def auto_scene_normalization(depths, intrs, extrs, depths_conf=None, conf_thresh=4.8, target_radius=6.3, rescale_by_camera_radius=True, frame=0):
    """The reference's ``compute_auto_scene_normalization`` (its defaults; this project's argument order, as ``sample_queries``):
    unproject the valid pixels of frame ``frame`` of every view with at least 100 of them, centre the cloud, lift its 12 % z quantile
    to z = 0, and rescale so that the median camera distance (``rescale_by_camera_radius``) or the 95 % radius quantile of the cloud
    becomes ``target_radius``.  Returns a ``SceneTransform`` with the identity rotation.  One host read, at the end.

    Kept from the reference as it is: the "camera centres" are the translation columns of the world->camera extrinsics (not the
    centres -R^T t), the median of an even number of views is the lower one (``torch.median``), and a quantile's rank is
    ``q * (M - 1)`` rounded to fp32."""
    state, cam_t = scene_statistics(depths, intrs, extrs, depths_conf, conf_thresh, frame,
                                    None if rescale_by_camera_radius else RADIUS_QUANTILE)
    # the one read: the state's words as doubles (the integers are read back from their bits) and the cameras' translation columns
    host = torch.cat([state.view(torch.float64), cam_t.reshape(-1)]).cpu()
    st = read_statistics(host[:hip.SN_WORDS].view(torch.int64))
    if st["M"] < MIN_POINTS:
        raise RuntimeError("Too few valid points for normalization.")
    if st["nonfinite"]:
        raise ValueError(f"{st['nonfinite']} valid pixels of frame {frame} have a depth that is not finite")
    centroid, floor_z = st["centroid"], st["floor_z"]
    if rescale_by_camera_radius:
        c = host[hip.SN_WORDS:].numpy().reshape(-1, 3) - centroid
        c[:, 2] -= floor_z
        dist = np.sort(np.sqrt((c * c).sum(1)))
        radius = float(dist[(len(dist) - 1) // 2])  # torch.median: the lower of the two middle values
    else:
        radius = st["radius_quantile"]
    scale = float(target_radius) / radius if radius > 0.0 else math.inf
    translate = -scale * centroid
    translate[2] -= scale * floor_z
    if not (math.isfinite(scale) and scale > 0.0 and np.isfinite(translate).all()):
        raise ValueError(f"scene normalisation gave scale {scale} and translation {translate.tolist()} (centroid {centroid.tolist()}, "
                         f"floor {floor_z}, radius {radius})")
    return SceneTransform(scale, None, translate)
