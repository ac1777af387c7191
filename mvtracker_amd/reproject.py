"""Reprojection check on the device ("Reprojection check"): every view is rendered from the other views' depth
maps with an order-independent z-buffer and the render is scored against the view's own frame and own depth map, so that a camera
correction (``align_cameras``) can be judged by something other than the optimiser's own fitness.

The reference does this on the host (conversions/droid/reproject_depth_into_videos.py ``render_dense_pointcloud``, then
conversions/droid/debug/compare_photometric_error.py: MSE, PSNR, MAE, SSIM of "ICP" against "no ICP"); here the same rules run in
``mvt_reproject_clear`` -> ``mvt_reproject_splat_depths`` -> ``mvt_reproject_resolve`` -> ``mvt_photometric_score`` with one
readback, of the score records.

    color, depth, index = render_point_cloud(points, colors, intr, extr, H, W)             # the reference function, on the device
    color, depth, index = reproject_views(rgbs, depths, intrs, extrs, frames=(0,))         # (V,F,3,H,W), (V,F,1,H,W), (V,F,H,W)
    report = reprojection_report(rgbs, depths, intrs, extrs, ReprojectionCheck())          # .mse .psnr .ssim .depth_close_fraction ..
    out = predictor(rgbs=..., depths=..., ..., camera_alignment=a, reprojection_check=ReprojectionCheck())
    print(compare_reports(predictor.last_reprojection_report_before, predictor.last_reprojection_report))
"""
from __future__ import annotations

import math

import torch

from . import hip
from .clip import DepthClip

SOURCES = ("others", "all")
SPLATS = (1, 3, 5)
MAX_RUN_PIXELS = 1 << 24  # z-buffer words per run of frames: 128 MiB of keys


def _check_render(min_depth, splat):
    if not (math.isfinite(float(min_depth)) and float(min_depth) >= 0.0):
        raise ValueError(f"min_depth must be finite and >= 0, got {min_depth!r}")
    if splat not in SPLATS:
        raise ValueError(f"splat must be one of {SPLATS}, got {splat!r}")
    return float(min_depth), int(splat)


def _check_frames(frames):
    try:
        fr = tuple(frames)
    except TypeError:
        raise ValueError(f"frames must be a sequence of frame indices, got {frames!r}") from None
    if not fr or any(int(f) != f or int(f) < 0 for f in fr) or len(set(int(f) for f in fr)) != len(fr):
        raise ValueError(f"frames must be distinct integers >= 0, at least one, got {frames!r}")
    return tuple(int(f) for f in fr)


class ReprojectionCheck:
    """``frames`` that are rendered and scored; ``sources``: "others" (a view is rendered from every other view: the leave-one-out
    the alignment itself uses) or "all" (from every view, what the reference script renders); ``min_depth``: a point is drawn only
    when its depth in the target camera exceeds it; ``splat``: 1, 3 or 5, the side of the depth-tested sprite a point is drawn as;
    ``depth_tol``: a rendered depth within this of the view's own depth counts as close, in the caller's units; ``conf_thresh``: with
    a confidence map only pixels with conf > conf_thresh are sources."""

    def __init__(self, frames=(0,), sources="others", min_depth=0.01, splat=1, depth_tol=0.05, conf_thresh=None):
        self.frames = _check_frames(frames)
        if sources not in SOURCES:
            raise ValueError(f"sources must be one of {SOURCES}, got {sources!r}")
        self.min_depth, self.splat = _check_render(min_depth, splat)
        if not (math.isfinite(float(depth_tol)) and float(depth_tol) >= 0.0):
            raise ValueError(f"depth_tol must be finite and >= 0, got {depth_tol!r}")
        if conf_thresh is not None and not math.isfinite(float(conf_thresh)):
            raise ValueError(f"conf_thresh must be finite, got {conf_thresh!r}")
        self.sources, self.depth_tol = sources, float(depth_tol)
        self.conf_thresh = None if conf_thresh is None else float(conf_thresh)

    def __repr__(self):
        return (f"ReprojectionCheck(frames={self.frames}, sources={self.sources!r}, min_depth={self.min_depth}, splat={self.splat}, "
                f"depth_tol={self.depth_tol}, conf_thresh={self.conf_thresh})")


def _check(check):
    if not isinstance(check, ReprojectionCheck):
        raise ValueError(f"check must be a ReprojectionCheck, got {check!r}")
    return check


@hip.guarded
def render_point_cloud(points, colors, intr, extr, height, width, min_depth=0.01, splat=1):
    """The reference's ``render_dense_pointcloud`` on the device: points (M,3) and colors (M,3) uint8 through the camera intr (3,3),
    extr (3,4) (world -> camera).  Returns ``(color (3,H,W) uint8, depth (H,W) fp32, index (H,W) int32)``: per pixel the nearest
    point's colour, its depth (0: no point) and its row (-1: no point)."""
    min_depth, splat = _check_render(min_depth, splat)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be (M, 3), got {tuple(points.shape)}")
    if tuple(colors.shape) != tuple(points.shape) or colors.dtype != torch.uint8:
        raise ValueError(f"colors must be uint8 of the shape of points, got {colors.dtype} {tuple(colors.shape)}")
    if tuple(intr.shape) != (3, 3) or tuple(extr.shape) != (3, 4):
        raise ValueError(f"intr / extr must be (3, 3) / (3, 4), got {tuple(intr.shape)} / {tuple(extr.shape)}")
    H, W = int(height), int(width)
    if H < 1 or W < 1 or H * W >= 1 << 31:
        raise ValueError(f"height and width must be positive with fewer than 2^31 pixels, got {height!r} x {width!r}")
    hip.require_device(points)
    dev = points.device
    M = points.shape[0]
    if M >= 1 << 31:
        raise ValueError(f"{M} points are too many (the limit is 2^31 per launch)")
    color = torch.zeros(3, H, W, dtype=torch.uint8, device=dev)
    depth = torch.zeros(H, W, device=dev)
    index = torch.full((H, W), -1, dtype=torch.int32, device=dev)
    if M == 0:
        return color, depth, index
    keys = torch.empty(H * W, dtype=torch.int64, device=dev)
    hip.reproject_clear(keys, H * W)
    hip.reproject_splat_points(points.to(torch.float32).contiguous(), M, 1, intr.to(torch.float32).reshape(1, 9).contiguous(),
                               extr.to(torch.float32).reshape(1, 12).contiguous(), H, W, min_depth, splat, keys)
    hip.reproject_resolve(keys, 1, H, W, index, depth, color, colors=colors.contiguous())
    return color, depth, index


def reproject_clip(rgbs, depths, intrs, extrs, frames=None, sources="others", min_depth=0.01, splat=1, depths_conf=None, conf_thresh=None):
    """``reproject_views`` whose results stay in clip rank: (V,F,3,H,W), (V,F,1,H,W), (V,F,H,W) with or without the leading batch."""
    min_depth, splat = _check_render(min_depth, splat)
    if sources not in SOURCES:
        raise ValueError(f"sources must be one of {SOURCES}, got {sources!r}")
    clip = DepthClip(depths, intrs, extrs, depths_conf)
    V, T, H, W, dev = clip.V, clip.T, clip.H, clip.W, clip.dev
    if tuple(rgbs.shape) != tuple(depths.shape[:-3]) + (3, H, W):
        raise ValueError(f"rgbs must be {tuple(depths.shape[:-3]) + (3, H, W)}, got {tuple(rgbs.shape)}")
    fr = tuple(range(T)) if frames is None else _check_frames(frames)
    if max(fr) >= T:
        raise ValueError(f"frames {fr} reach past the clip's {T} frames")
    if not 1 <= V <= hip.REPROJECT_MAX_TARGETS:
        raise ValueError(f"the reprojection takes 1..{hip.REPROJECT_MAX_TARGETS} views, got {V}")
    if sources == "others" and V < 2:
        raise ValueError('sources="others" needs at least 2 views')
    if V * H * W >= 1 << 31:
        raise ValueError(f"{V} views of {H} x {W} pixels are too large (the limit is 2^31 source pixels)")
    F, HW = len(fr), H * W
    d, conf = clip.d, clip.conf(conf_thresh)
    c = clip.squeeze(rgbs)
    c = c.contiguous() if c.dtype == torch.uint8 else c.to(torch.float32).contiguous()
    kinv, einv = clip.kinv, clip.einv
    idx = torch.tensor(fr, dtype=torch.long, device=dev)
    Kf = clip.K.index_select(1, idx).transpose(0, 1).contiguous()  # (F, V, 9): the target cameras of a frame are contiguous rows
    Ef = clip.E.index_select(1, idx).transpose(0, 1).contiguous()
    color = torch.empty(V, F, 3, H, W, dtype=torch.uint8, device=dev)
    depth = torch.empty(V, F, 1, H, W, device=dev)
    index = torch.empty(V, F, H, W, dtype=torch.int32, device=dev)
    step = max(1, min(F, MAX_RUN_PIXELS // (V * HW)))  # frames per run: bounded workspace
    keys = torch.empty(step, V, HW, dtype=torch.int64, device=dev)
    views = list(range(V))
    for f0 in range(0, F, step):
        nf = min(step, F - f0)
        hip.reproject_clear(keys, nf * V * HW)
        for j in range(nf):
            fi = f0 + j
            hip.reproject_splat_depths(d, conf, kinv, einv, V, T, fr[fi], H, W, conf_thresh, views, Kf[fi], Ef[fi], sources == "others", min_depth,
                                       splat, keys[j])
            # target v of frame fi is image v * F + fi of the outputs
            hip.reproject_resolve(keys[j], V, H, W, index.reshape(-1)[fi * HW:], depth.reshape(-1)[fi * HW:], color.reshape(-1)[fi * 3 * HW:],
                                  target_stride=F, rgbs=c, V=V, T=T, t=fr[fi])
    return color, depth, index


@hip.guarded
def reproject_views(rgbs, depths, intrs, extrs, frames=None, sources="others", min_depth=0.01, splat=1, depths_conf=None, conf_thresh=None):
    """Every view of a clip rendered from the views' depth maps.  rgbs (V,T,3,H,W) uint8 or float (0..255), depths (V,T,1,H,W),
    intrs (V,T,3,3), extrs (V,T,3,4), or all with a leading batch of 1, as ``clean_depths`` takes them.  ``frames``: the frames
    rendered (None: all); ``sources`` "others" / "all".  A source pixel is valid as in ``clean_depths`` (depth finite and > 0,
    conf > conf_thresh when both are given).  Returns ``(color (V,F,3,H,W) uint8, depth (V,F,1,H,W) fp32 with 0 = nothing drawn,
    index (V,F,H,W) int32)``: ``index = view * H * W + y * W + x`` of the source pixel that won, -1 where nothing was drawn: a
    cross-view correspondence map.  With the batch the outputs carry it too."""
    out = reproject_clip(rgbs, depths, intrs, extrs, frames, sources, min_depth, splat, depths_conf, conf_thresh)
    return tuple(o[None] for o in out) if depths.dim() == 6 else out


class ReprojectionReport:
    """The scores of every (view, frame) pair: ``records`` (V,F,SCORE_WORDS) int64 words on the host, as ``mvt_photometric_score``
    wrote them.  The figures are (V,F) fp64 tensors: ``coverage``; ``mse = SSE / (3 N)``, ``psnr = 10 log10(255^2 / mse)`` (inf at
    mse = 0), ``mae``, ``ssim`` over all pixels and ``mse_covered`` .. ``ssim_covered`` over the pixels the render covers (NaN when
    there is none); ``depth_pixels``: covered pixels with a valid own depth, ``depth_close_fraction``: the share of them within
    ``depth_tol``, ``depth_mae`` / ``depth_mae_close``: the mean |rendered - own| depth over them / over the close ones."""

    FIGURES = ("coverage", "mse", "psnr", "mae", "ssim", "mse_covered", "psnr_covered", "mae_covered", "ssim_covered", "depth_pixels",
               "depth_close_fraction", "depth_mae", "depth_mae_close")

    def __init__(self, records, frames, check=None):
        if records.dim() != 3 or records.shape[2] != hip.SCORE_WORDS or records.dtype != torch.int64 or records.shape[1] != len(frames):
            raise ValueError(f"records must be (V, {len(frames)}, {hip.SCORE_WORDS}) int64, got {records.dtype} {tuple(records.shape)}")
        self.records, self.frames, self.check = records.cpu().contiguous(), tuple(frames), check

    def _int(self, word):
        return self.records[..., word].to(torch.float64)

    def _dbl(self, word):
        return self.records.view(torch.float64)[..., word]

    @staticmethod
    def _psnr(mse):
        return torch.where(mse == 0, torch.full_like(mse, float("inf")), 10.0 * torch.log10(255.0 ** 2 / mse))

    coverage = property(lambda s: s._int(hip.SCORE_COVERED) / s._int(hip.SCORE_N))
    mse = property(lambda s: s._int(hip.SCORE_SSE) / (3.0 * s._int(hip.SCORE_N)))
    mae = property(lambda s: s._int(hip.SCORE_SAE) / (3.0 * s._int(hip.SCORE_N)))
    ssim = property(lambda s: s._dbl(hip.SCORE_SSIM) / s._int(hip.SCORE_N))
    psnr = property(lambda s: s._psnr(s.mse))
    mse_covered = property(lambda s: s._int(hip.SCORE_SSE_COV) / (3.0 * s._int(hip.SCORE_COVERED)))
    mae_covered = property(lambda s: s._int(hip.SCORE_SAE_COV) / (3.0 * s._int(hip.SCORE_COVERED)))
    ssim_covered = property(lambda s: s._dbl(hip.SCORE_SSIM_COV) / s._int(hip.SCORE_COVERED))
    psnr_covered = property(lambda s: s._psnr(s.mse_covered))
    depth_pixels = property(lambda s: s._int(hip.SCORE_N_DEPTH))
    depth_close_fraction = property(lambda s: s._int(hip.SCORE_N_CLOSE) / s._int(hip.SCORE_N_DEPTH))
    depth_mae = property(lambda s: s._dbl(hip.SCORE_DEPTH_SAE) / s._int(hip.SCORE_N_DEPTH))
    depth_mae_close = property(lambda s: s._dbl(hip.SCORE_DEPTH_SAE_CLOSE) / s._int(hip.SCORE_N_CLOSE))

    def summary(self):
        """Per view, the mean and the (population) standard deviation over the frames of every figure, by the rules of the
        reference's ``compare_videos``: infinite PSNRs are left out of the PSNR mean and deviation, which are 0 when none is left.
        Returns ``{figure: (mean (V,), std (V,))}`` fp64 plus ``"frame_count"``."""
        out = {"frame_count": len(self.frames)}
        for name in self.FIGURES:
            val = getattr(self, name)
            if name.startswith("psnr"):
                keep = torch.isfinite(val)
                n = keep.sum(1)
                v0 = torch.where(keep, val, torch.zeros_like(val))
                mean = torch.where(n > 0, v0.sum(1) / n.clamp(min=1), torch.zeros_like(v0[:, 0]))
                var = torch.where(keep, (val - mean[:, None]) ** 2, torch.zeros_like(val)).sum(1) / n.clamp(min=1)
                out[name] = (mean, torch.where(n > 0, var.sqrt(), torch.zeros_like(mean)))
            else:
                out[name] = (val.mean(1), val.std(1, unbiased=False))
        return out

    def table(self, label="reprojection"):
        """The reference's report table: one row per view with the mean MSE, PSNR, SSIM and MAE over the frames, and the depth columns."""
        s = self.summary()
        lines = [f"{'View':<8} {'Type':<14} {'MSE':>12} {'PSNR':>12} {'SSIM':>12} {'MAE':>12} {'Coverage':>10} {'DepthClose':>11} {'DepthMAE':>10}",
                 "-" * 108]
        for v in range(self.records.shape[0]):
            lines.append(f"{v:<8} {label:<14} {float(s['mse'][0][v]):>12.2f} {float(s['psnr'][0][v]):>12.2f} {float(s['ssim'][0][v]):>12.4f} "
                         f"{float(s['mae'][0][v]):>12.2f} {float(s['coverage'][0][v]):>10.4f} {float(s['depth_close_fraction'][0][v]):>11.4f} "
                         f"{float(s['depth_mae'][0][v]):>10.4f}")
        return "\n".join(lines)


def compare_reports(before, after):
    """The reference's improvement summary as a string: per view the change of the mean figures from ``before`` to ``after``, signed
    so that positive is better (MSE and MAE fall, PSNR, SSIM and the close-depth share rise)."""
    a, b = after.summary(), before.summary()
    lines = [f"{'View':<8} {'dMSE':>12} {'dPSNR':>12} {'dSSIM':>12} {'dMAE':>12} {'dDepthClose':>12}", "-" * 74]
    for v in range(after.records.shape[0]):
        lines.append(f"{v:<8} {float(b['mse'][0][v] - a['mse'][0][v]):>12.2f} {float(a['psnr'][0][v] - b['psnr'][0][v]):>12.2f} "
                     f"{float(a['ssim'][0][v] - b['ssim'][0][v]):>12.4f} {float(b['mae'][0][v] - a['mae'][0][v]):>12.2f} "
                     f"{float(a['depth_close_fraction'][0][v] - b['depth_close_fraction'][0][v]):>12.4f}")
    return "\n".join(lines)


def score_renders(color, depth, index, rgbs, depths, frames, depth_tol):
    """The score records (V,F,SCORE_WORDS) int64 on the device of renders (V,F,..) against frames ``frames`` of a clip."""
    V, F = index.shape[:2]
    H, W = index.shape[-2:]
    if H < 6 or W < 6:
        raise ValueError(f"the SSIM window needs images of at least 6 x 6 pixels, got {H} x {W}")
    idx = torch.tensor(frames, dtype=torch.long, device=index.device)
    real = rgbs if rgbs.dtype == torch.uint8 else rgbs.to(torch.float32)
    real = real.index_select(1, idx).contiguous()                  # (V,F,3,H,W): the views' own frames
    own = depths.to(torch.float32).index_select(1, idx).contiguous()  # (V,F,1,H,W): the views' own depth maps
    scores = torch.empty(V, F, hip.SCORE_WORDS, dtype=torch.int64, device=index.device)
    hip.photometric_score(color, real, index, depth, own, V * F, H, W, depth_tol, scores)
    return scores


@hip.guarded
def reprojection_report(rgbs, depths, intrs, extrs, check, depths_conf=None):
    """Renders every view of the clip from the other views (``check.sources``) at ``check.frames`` and scores each render against
    the view's own frame and depth map.  Inputs as ``reproject_views`` takes them.  Returns a ``ReprojectionReport``; the records
    are read back once, the inputs are not written."""
    ck = _check(check)
    if min(depths.shape[-2:]) < 6:  # (before the render: nothing is launched for a clip the scores refuse)
        raise ValueError(f"the SSIM window needs images of at least 6 x 6 pixels, got {depths.shape[-2]} x {depths.shape[-1]}")
    color, depth, index = reproject_clip(rgbs, depths, intrs, extrs, ck.frames, ck.sources, ck.min_depth, ck.splat, depths_conf, ck.conf_thresh)
    if depths.dim() == 6:  # (a leading batch of 1 on both: the render has checked it)
        rgbs, depths = rgbs[0], depths[0]
    scores = score_renders(color, depth, index, rgbs, depths, ck.frames, ck.depth_tol)
    return ReprojectionReport(scores.cpu(), ck.frames, ck)
