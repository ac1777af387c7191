"""CPU stand-ins for the reprojection entries of mvtracker_amd.hip (reproject_clear, reproject_splat_depths, reproject_splat_points,
reproject_resolve, photometric_score), on top of tests/hip_mock_align.py: the host code of mvtracker_amd/reproject.py and the
predictor's wiring run on CPU tensors.  The fake entries follow the kernels' rules (the source pixels and their points through the
mocked clean_points, the key layout, the strided outputs of resolve) and call the restatement tests/reproject_ref.py for the
arithmetic; ``calls`` lists the entries called, in order, and ``splats`` the (frame, exclude_self, splat) of every clip splat."""
import numpy as np
import torch

import hip_mock_align
import hip_mock_clean
import reproject_ref as R

calls = []
splats = []


def _keys(keys):
    return keys.reshape(-1).numpy().view(np.uint64)


def reproject_clear(keys, n):
    calls.append("reproject_clear")
    assert keys.dtype == torch.int64 and keys.numel() >= n
    keys.reshape(-1)[:n] = -1


def reproject_splat_depths(depths, conf, kinv, einv, V, T, t, H, W, conf_thresh, target_views, intrs, extrs, exclude_self, min_depth, splat,
                           keys):
    calls.append("reproject_splat_depths")
    splats.append((t, bool(exclude_self), splat))
    Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
    xyz = torch.empty(V, Hp * Wp, 4)
    n = len(hip_mock_clean.calls)
    hip_mock_clean.clean_points(depths, conf, kinv, einv, V, T, t, 1, H, W, conf_thresh, None, xyz)
    del hip_mock_clean.calls[n:]  # (the real entry unprojects in its own kernel: no clean_points call)
    pts = xyz.reshape(V, Hp, Wp, 4)[:, :H, :W, :3].numpy()
    flat = np.arange(V * H * W).reshape(V, H * W)
    k = _keys(keys)
    K, E = intrs.reshape(-1, 3, 3).numpy(), extrs.reshape(-1, 3, 4).numpy()
    for j, tv in enumerate(target_views):
        for sv in range(V):
            if exclude_self and sv == tv:
                continue
            p = pts[sv].reshape(-1, 3)
            m = np.isfinite(p).all(1)
            R.splat_keys(k[j * H * W:(j + 1) * H * W], p[m], flat[sv][m], K[j], E[j], H, W, min_depth, splat)


def reproject_splat_points(points, M, n_targets, intrs, extrs, H, W, min_depth, splat, keys):
    calls.append("reproject_splat_points")
    k = _keys(keys)
    K, E = intrs.reshape(-1, 3, 3).numpy(), extrs.reshape(-1, 3, 4).numpy()
    for j in range(n_targets):
        R.splat_keys(k[j * H * W:(j + 1) * H * W], points.reshape(-1, 3)[:M].numpy(), np.arange(M), K[j], E[j], H, W, min_depth, splat)


def reproject_resolve(keys, n_targets, H, W, index, depth, color, target_stride=1, rgbs=None, V=0, T=0, t=0, colors=None):
    calls.append("reproject_resolve")
    assert (rgbs is None) != (colors is None)
    HW = H * W
    k = _keys(keys)
    if colors is not None:
        cols = colors.numpy()
    else:
        cols = R.to_u8(rgbs.reshape(V, T, 3, H, W)[:, t].numpy()).transpose(0, 2, 3, 1).reshape(V * HW, 3)
    for j in range(n_targets):
        c, d, i = R.resolve(k[j * HW:(j + 1) * HW], H, W, cols)
        o = j * target_stride * HW
        index.reshape(-1)[o:o + HW] = torch.from_numpy(i.reshape(-1))
        depth.reshape(-1)[o:o + HW] = torch.from_numpy(d.reshape(-1).copy())
        color.reshape(-1)[3 * o:3 * o + 3 * HW] = torch.from_numpy(c.reshape(-1))


def photometric_score(a, b, index, depth, target_depth, n, H, W, depth_tol, scores, partial=None):
    from mvtracker_amd import hip
    calls.append("photometric_score")
    if H < 6 or W < 6:
        raise hip.HipError("mvt_photometric_score failed with code 1 (arguments rejected)")
    A, B = a.reshape(n, 3, H, W).numpy(), b.reshape(n, 3, H, W).numpy()
    I, D, Z = index.reshape(n, H, W).numpy(), depth.reshape(n, H, W).numpy(), target_depth.reshape(n, H, W).numpy()
    out = scores.reshape(n, R.WORDS)
    for j in range(n):
        out[j] = torch.from_numpy(R.record_words(R.score(A[j], B[j], I[j], D[j], Z[j], depth_tol)))


def install(monkeypatch):
    import sys
    from mvtracker_amd import hip
    hip_mock_align.install(monkeypatch)
    me = sys.modules[__name__]
    del calls[:]
    del splats[:]
    for name in "reproject_clear reproject_splat_depths reproject_splat_points reproject_resolve photometric_score".split():
        monkeypatch.setattr(hip, name, getattr(me, name))
