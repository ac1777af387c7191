"""Track overlays on the device ("Track overlays"): the tracker's world-space tracks drawn into every view's frames.

The reference draws on the CPU with OpenCV (mvtracker/utils/visualizer_mp4.py ``Visualizer.visualize`` -> ``draw_tracks_on_video`` ->
``_draw_pred_tracks``: one ``cv2.line`` per (frame, older frame, track), O(T^2 N) calls per view with the infinite trail, which is why it
caps the picture at 36 tracks).  Here ``mvt_overlay_project`` projects a block of frames into every view, and per frame
``mvt_overlay_draw`` scatters the N * V new segments and markers as 64-bit keys (order << 24 | rgb, kept by an atomic maximum: the
painter's last writer whatever the order of arrival) and ``mvt_overlay_compose`` reads the frame once and writes the picture once.  The
line keys persist from frame to frame, so the work is O(T N) segments per view and a clip may arrive in blocks.

    video, colors = render_track_overlays(rgbs, tracks, visibility, query_frames, intrs, extrs)      # (V,T,3,H,W) uint8, (N,3) uint8
    video, colors = render_track_overlays(rgbs, tracks, None, query_frames, intrs, extrs, TrackOverlay(trail=10, pad=16, min_depth=0.05))
    sheet = stack_views(video)                                                                      # (T,3,V*Hp,Wp), views along the height
    session = open_track_overlay(query_frames, V, H, W, TrackOverlay())                              # for callers of open_stream
    block = session.push(rgbs_block, tracks_block, visibility_block, intrs_block, extrs_block)      # the bits of the whole-clip call
    xyz = project_tracks(tracks, intrs, extrs)                                                      # (V,T,N,3): pixel x, pixel y, camera z

Lines, discs and rings are integer primitives without anti-aliasing (the header states them); DESIGN lists the deviations from the
reference and what is out of scope.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Union

import torch

from . import hip
from .motion import clip_frames

# matplotlib's gist_rainbow, 256 entries, each channel rint(lut * 255) (no entry lies on a tie), as 256 x (r, g, b) bytes
GIST_RAINBOW = bytes.fromhex(
    "ff0029ff0023ff001eff0019ff0013ff000eff0009ff0003ff0200ff0700ff0d00ff1200ff1800ff1d00ff2200ff2800ff2d00ff3300ff3800ff3d00ff4300ff"
    "4800ff4e00ff5300ff5800ff5e00ff6300ff6900ff6e00ff7300ff7900ff7e00ff8400ff8900ff8e00ff9400ff9900ff9f00ffa400ffa900ffaf00ffb400ffba"
    "00ffbf00ffc400ffca00ffcf00ffd500ffda00ffe000ffe500ffea00fff000fff500fffb00feff00f9ff00f3ff00eeff00e8ff00e3ff00deff00d8ff00d3ff00"
    "cdff00c8ff00c3ff00bdff00b8ff00b2ff00adff00a8ff00a2ff009dff0097ff0092ff008dff0087ff0082ff007cff0077ff0072ff006cff0067ff0061ff005c"
    "ff0056ff0051ff004cff0046ff0041ff003bff0036ff0031ff002bff0026ff0020ff001bff0016ff0010ff000bff0005ff0000ff0000ff0500ff0b00ff1000ff"
    "1600ff1b00ff2000ff2600ff2b00ff3000ff3600ff3b00ff4100ff4600ff4b00ff5100ff5600ff5b00ff6100ff6600ff6c00ff7100ff7600ff7c00ff8100ff86"
    "00ff8c00ff9100ff9700ff9c00ffa100ffa700ffac00ffb100ffb700ffbc00ffc200ffc700ffcc00ffd200ffd700ffdc00ffe200ffe700ffed00fff200fff700"
    "fffd00fcff00f6ff00f1ff00ecff00e6ff00e1ff00dbff00d6ff00d0ff00cbff00c6ff00c0ff00bbff00b5ff00b0ff00aaff00a5ff00a0ff009aff0095ff008f"
    "ff008aff0084ff007fff0079ff0074ff006fff0069ff0064ff005eff0059ff0053ff004eff0049ff0043ff003eff0038ff0033ff002dff0028ff0023ff001dff"
    "0018ff0012ff000dff0007ff0002ff0400ff0900ff0e00ff1400ff1900ff1f00ff2400ff2a00ff2f00ff3400ff3a00ff3f00ff4500ff4a00ff5000ff5500ff5a"
    "00ff6000ff6500ff6b00ff7000ff7600ff7b00ff8100ff8600ff8b00ff9100ff9600ff9c00ffa100ffa700ffac00ffb100ffb700ffbc00ffc200ffc700ffcd00"
    "ffd200ffd700ffdd00ffe200ffe800ffed00fff300fff800fffe00ffff00fbff00f6ff00f0ff00ebff00e5ff00e0ff00daff00d5ff00d0ff00caff00c5ff00bf")


def rainbow_index(y: int, Hp: int) -> int:
    """Row of GIST_RAINBOW for a track whose query-frame point has the integer row ``y`` in a picture ``Hp`` high: what
    ``cmap(Normalize(0, Hp)(y))`` picks."""
    return min(255, max(0, (int(y) * 256) // int(Hp)))


def _int_in(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or int(v) != v or not lo <= int(v) <= hi:
        raise ValueError(f"{name} must be an integer in [{lo}, {hi}], got {v!r}")
    return int(v)


@dataclass(frozen=True, eq=False)
class TrackOverlay:
    """How tracks are drawn.  ``trail``: the reference's ``tracks_leave_trace`` (-1: every segment since the query frame, 0: no lines,
    L: the last L segments); ``linewidth`` 1..8 (markers have the radius 2 * linewidth); ``pad`` 0..64: the reference's ``pad_value``, a
    white border of that many pixels, the tracks shifted by it; ``colors``: ``"rainbow"`` (gist_rainbow by the track's row at its query
    frame in view ``color_view``) or an (N, 3) uint8 tensor; ``min_depth``: None (the reference: no depth test, points behind a camera
    are drawn mirrored) or a depth a point's camera z must exceed to be drawn; ``max_tracks``: draw only the first M tracks."""
    trail: int = -1
    linewidth: int = 2
    pad: int = 0
    colors: Union[str, torch.Tensor] = "rainbow"
    color_view: int = 0
    min_depth: Optional[float] = None
    max_tracks: Optional[int] = None

    def __post_init__(self):
        object.__setattr__(self, "trail", _int_in("trail", self.trail, -1, hip.OVERLAY_MAX_INDEX))
        object.__setattr__(self, "linewidth", _int_in("linewidth", self.linewidth, 1, hip.OVERLAY_MAX_LINEWIDTH))
        object.__setattr__(self, "pad", _int_in("pad", self.pad, 0, hip.OVERLAY_MAX_PAD))
        object.__setattr__(self, "color_view", _int_in("color_view", self.color_view, 0, 1 << 15))
        c = self.colors
        if isinstance(c, torch.Tensor):
            if c.dtype != torch.uint8 or c.dim() != 2 or c.shape[1] != 3 or c.shape[0] < 1:
                raise ValueError(f"colors must be \"rainbow\" or an (N, 3) uint8 tensor, got {tuple(c.shape)} {c.dtype}")
        elif not (isinstance(c, str) and c == "rainbow"):
            raise ValueError(f"colors must be \"rainbow\" or an (N, 3) uint8 tensor, got {c!r}")
        if self.min_depth is not None:
            if isinstance(self.min_depth, bool) or not isinstance(self.min_depth, (int, float)) or not math.isfinite(float(self.min_depth)):
                raise ValueError(f"min_depth must be None or a finite number, got {self.min_depth!r}")
            object.__setattr__(self, "min_depth", float(self.min_depth))
        if self.max_tracks is not None:
            object.__setattr__(self, "max_tracks", _int_in("max_tracks", self.max_tracks, 1, hip.OVERLAY_MAX_INDEX))


def _check(overlay):
    if not isinstance(overlay, TrackOverlay):
        raise ValueError(f"overlay must be a TrackOverlay, got {overlay!r}")
    return overlay


def _check_cameras(tracks, intrs, extrs, V=None):
    """tracks (T, N, 3), intrs (V, T, 3, 3), extrs (V, T, 3, 4) as contiguous fp32; ValueError for anything else."""
    if not (isinstance(tracks, torch.Tensor) and tracks.dim() == 3 and tracks.shape[2] == 3 and tracks.shape[0] >= 1 and tracks.shape[1] >= 1):
        raise ValueError(f"tracks must be (T, N, 3), got {tuple(getattr(tracks, 'shape', ()))}")
    T, N = tracks.shape[:2]
    if not (isinstance(intrs, torch.Tensor) and intrs.dim() == 4 and intrs.shape[0] >= 1 and tuple(intrs.shape[1:]) == (T, 3, 3)):
        raise ValueError(f"intrs must be (V, {T}, 3, 3), got {tuple(getattr(intrs, 'shape', ()))}")
    if V is not None and intrs.shape[0] != V:
        raise ValueError(f"intrs must be ({V}, {T}, 3, 3), got {tuple(intrs.shape)}")
    V = intrs.shape[0]
    if not (isinstance(extrs, torch.Tensor) and tuple(extrs.shape) == (V, T, 3, 4)):
        raise ValueError(f"extrs must be ({V}, {T}, 3, 4), got {tuple(getattr(extrs, 'shape', ()))}")
    if N >= hip.OVERLAY_MAX_INDEX or T >= hip.OVERLAY_MAX_INDEX or V * T * N >= 1 << 31:
        raise ValueError(f"{V} views x {T} frames x {N} tracks are too many for one call (tracks and frames < 2^20, their product < 2^31)")
    return tuple(a.to(torch.float32).contiguous() for a in (tracks, intrs, extrs))


@hip.guarded
def project_tracks(tracks, intrs, extrs):
    """tracks (T, N, 3) world points, intrs (V, T, 3, 3), extrs (V, T, 3, 4) -> (V, T, N, 3) fp32: pixel x, pixel y, camera z.  The
    reference's ``world_space_to_pixel_xy_and_camera_z`` for every view in one launch (fp32, no fused multiply-add)."""
    tracks, intrs, extrs = _check_cameras(tracks, intrs, extrs)
    hip.require_device(tracks)
    (T, N), V = tracks.shape[:2], intrs.shape[0]
    xyz = torch.empty(V, T, N, 3, device=tracks.device)
    hip.overlay_project(tracks, intrs, extrs, V, T, N, xyz=xyz)
    return xyz


@hip.guarded
def track_pixels(tracks, intrs, extrs, pad=0, min_depth=None):
    """The integer points the overlay draws with: (V, T, N, 3) int32 (x, y, valid) -- ``project_tracks``, clipped to [-1e4, 1e4],
    plus ``pad``, truncated toward zero; invalid (and then 0, 0) where x or y is NaN or, with ``min_depth``, not z > min_depth."""
    o = TrackOverlay(pad=pad, min_depth=min_depth)
    tracks, intrs, extrs = _check_cameras(tracks, intrs, extrs)
    hip.require_device(tracks)
    (T, N), V = tracks.shape[:2], intrs.shape[0]
    pts = torch.empty(T, V, N, 4, device=tracks.device, dtype=torch.int32)
    hip.overlay_project(tracks, intrs, extrs, V, T, N, points=pts, pad=o.pad, min_depth=o.min_depth)
    return pts.permute(1, 0, 2, 3)[..., :3].contiguous()


class TrackOverlaySession:
    """``open_track_overlay``: ``push`` draws a block of consecutive frames (numbered from 0 over the pushes) and returns its overlay;
    the concatenated blocks are the bits of ``render_track_overlays`` on the whole clip.  ``colors`` (N, 3) uint8 on the device holds a
    track's colour once its query frame was pushed (zeros before).  Scratch: two key planes per view, whatever the clip's length."""

    def __init__(self, query_frames, num_views, height, width, overlay):
        o = _check(overlay)
        if not (isinstance(query_frames, torch.Tensor) and query_frames.dim() == 1 and query_frames.numel() >= 1):
            raise ValueError(f"query_frames must be (N,), got {tuple(getattr(query_frames, 'shape', ()))}")
        if query_frames.dtype == torch.bool or query_frames.dtype.is_complex:
            raise ValueError(f"query_frames must hold frame numbers, got {query_frames.dtype}")
        V, H, W = (_int_in(n, v, 1, 1 << 20) for n, v in (("num_views", num_views), ("height", height), ("width", width)))
        N = query_frames.numel()
        Hp, Wp = H + 2 * o.pad, W + 2 * o.pad
        if Hp > hip.OVERLAY_MAX_SIDE or Wp > hip.OVERLAY_MAX_SIDE or V * Hp * Wp >= 1 << 31:
            raise ValueError(f"a padded picture of {Hp} x {Wp} in {V} views is too large (sides <= {hip.OVERLAY_MAX_SIDE}, views x pixels < 2^31)")
        if N >= hip.OVERLAY_MAX_INDEX or V * N >= 1 << 27:
            raise ValueError(f"{N} tracks in {V} views are too many (tracks < 2^20, views x tracks < 2^27)")
        if o.color_view >= V:
            raise ValueError(f"color_view {o.color_view} is not one of the {V} views")
        if isinstance(o.colors, torch.Tensor) and o.colors.shape[0] != N:
            raise ValueError(f"colors must be ({N}, 3), one row per track, got {tuple(o.colors.shape)}")
        hip.require_device(query_frames)
        dev = query_frames.device
        self.overlay, self.V, self.H, self.W, self.N, self.Hp, self.Wp = o, V, H, W, N, Hp, Wp
        self.M = N if o.max_tracks is None else min(N, o.max_tracks)
        # (the reference's .long() of the queries' time column; a track is drawn from max(query frame, 0) on)
        self.query_frames = query_frames.to(torch.int64).clamp(0, hip.OVERLAY_MAX_INDEX).to(torch.int32).contiguous()
        if isinstance(o.colors, torch.Tensor):
            self.lut, self.colors = None, o.colors.to(dev).contiguous().clone()
        else:
            self.lut = torch.frombuffer(bytearray(GIST_RAINBOW), dtype=torch.uint8).reshape(256, 3).to(dev)
            self.colors = torch.zeros(N, 3, dtype=torch.uint8, device=dev)
        self.line_keys = torch.zeros(V, Hp, Wp, dtype=torch.int64, device=dev) if o.trail != 0 else None
        self.marker_keys = torch.zeros(V, Hp, Wp, dtype=torch.int64, device=dev)
        self.last_points = None  # (V, N, 4) int32: the points of the last pushed frame, the start of the next frame's segments
        self.frames = 0

    @torch.no_grad()
    def push(self, rgbs_block, tracks_block, visibility_block, intrs_block, extrs_block):
        """rgbs (V, b, 3, H, W) uint8 or float, tracks (b, N, 3), visibility (b, N) bool or None, intrs (V, b, 3, 3), extrs
        (V, b, 3, 4) of the next b frames -> (V, b, 3, H + 2 pad, W + 2 pad) uint8.  Everything is checked before the first launch."""
        o, V, N = self.overlay, self.V, self.N
        with hip.device_guard(self.marker_keys):
            frames = clip_frames(rgbs_block)
            b = frames.shape[1]
            if tuple(frames.shape) != (V, b, 3, self.H, self.W):
                raise ValueError(f"rgbs must be ({V}, b, 3, {self.H}, {self.W}), got {tuple(frames.shape)}")
            tracks, intrs, extrs = _check_cameras(tracks_block, intrs_block, extrs_block, V)
            if tuple(tracks.shape) != (b, N, 3):
                raise ValueError(f"tracks must be ({b}, {N}, 3), got {tuple(tracks.shape)}")
            vis = visibility_block
            if vis is not None:
                if not (isinstance(vis, torch.Tensor) and tuple(vis.shape) == (b, N)) or vis.dtype.is_floating_point:
                    raise ValueError(f"visibility must be None or ({b}, {N}) bool, got {tuple(getattr(vis, 'shape', ()))} {getattr(vis, 'dtype', None)}")
                vis = (vis != 0).contiguous()
            if self.frames + b >= hip.OVERLAY_MAX_INDEX:
                raise ValueError(f"frame numbers must stay below {hip.OVERLAY_MAX_INDEX}")
            for a in (frames, tracks, intrs, extrs) + (() if vis is None else (vis,)):
                hip.require_device(a)
            dev = frames.device
            pts = torch.empty(b + 1, V, N, 4, dtype=torch.int32, device=dev)  # slot 0: the frame before the block
            if self.last_points is not None:
                pts[0] = self.last_points
            hip.overlay_project(tracks, intrs, extrs, V, b, N, points=pts[1:], pad=o.pad, min_depth=o.min_depth, query_frames=self.query_frames,
                                frame0=self.frames, lut=self.lut, color_view=o.color_view, Hp=self.Hp, colors=self.colors)
            out = torch.empty(V, b, 3, self.Hp, self.Wp, dtype=torch.uint8, device=dev)
            for j in range(b):
                t = self.frames + j
                lines = o.trail != 0 and t >= 1
                hip.overlay_draw(pts[j] if lines else None, pts[j + 1], None if vis is None else vis[j], self.query_frames, self.colors, V, N, self.M,
                                 t, o.linewidth, self.Hp, self.Wp, self.line_keys if lines else None, self.marker_keys)
                first = 0 if o.trail < 0 else max(0, t - o.trail)
                hip.overlay_compose(frames, V, b, j, self.H, self.W, o.pad, self.line_keys, first, self.marker_keys, out)
            self.last_points = pts[b]
            self.frames += b
            return out


@hip.guarded
def open_track_overlay(query_frames, num_views, height, width, overlay=TrackOverlay()):
    """A ``TrackOverlaySession`` for ``num_views`` views of ``height`` x ``width`` frames and the N tracks whose query frames are
    ``query_frames`` (N,): for callers of ``open_stream`` who kept their frames (a stream's tracks arrive one window after their
    frames).  N is fixed here."""
    return TrackOverlaySession(query_frames, num_views, height, width, overlay)


@hip.guarded
def render_track_overlays(rgbs, tracks, visibility, query_frames, intrs, extrs, overlay=TrackOverlay()):
    """rgbs (V, T, 3, H, W) uint8 or float (a leading batch axis of 1 is dropped), tracks (T, N, 3) world points, visibility (T, N)
    bool or None, query_frames (N,), intrs (V, T, 3, 3), extrs (V, T, 3, 4) -> ``(video, colors)``: video (V, T, 3, H + 2 pad,
    W + 2 pad) uint8 with the tracks drawn by the reference's rules, colors (N, 3) uint8, both on the device.  One ``push`` of a
    session; the inputs are not written."""
    _check(overlay)
    frames = clip_frames(rgbs)
    V, _, _, H, W = frames.shape
    session = TrackOverlaySession(query_frames, V, H, W, overlay)
    return session.push(frames, tracks, visibility, intrs, extrs), session.colors


def stack_views(video):
    """(V, T, 3, Hp, Wp) -> (T, 3, V * Hp, Wp): the views under each other, as the reference's MultiViewVisualizer stacks them."""
    if video.dim() != 5:
        raise ValueError(f"video must be (V, T, 3, Hp, Wp), got {tuple(video.shape)}")
    return torch.cat(list(video.unbind(0)), dim=2)
