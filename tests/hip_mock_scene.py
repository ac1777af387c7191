"""CPU stand-ins for the scene normalisation entries of mvtracker_amd.hip (select_kth, scene_stats, scene_apply, scene_tracks), on
top of tests/hip_mock.py: the host code of mvtracker_amd/scene.py and the predictor's wiring run on CPU tensors.  The mocks follow
the kernels' rules (validity, per-view minimum, fp32 unprojection through hip_mock.unproject, fp32 rank, fp64 arithmetic rounded
once) with torch ops; ``calls`` lists the entries called, in order."""
import numpy as np
import torch

import hip_mock

calls = []


def select_kth(values, n, k, out, workspace):
    calls.append("select_kth")
    out[0] = torch.sort(values.reshape(-1)[:n]).values[k]


def _quantile(sorted_values, q):
    M = len(sorted_values)
    rank = np.float32(q) * np.float32(M - 1)
    kb = int(np.floor(rank))
    lo, hi = float(sorted_values[kb]), float(sorted_values[min(kb + 1, M - 1)])
    return lo + float(rank - np.float32(kb)) * (hi - lo), kb, lo, hi


def scene_stats(depths, conf, kinv, einv, V, T, t, H, W, conf_thresh, min_points, q_floor, q_radius, keys, partial, iws, state):
    from mvtracker_amd import hip
    calls.append("scene_stats")
    ds = depths.reshape(V, T, H, W).permute(1, 0, 2, 3).contiguous()
    xyz = torch.empty(T, V, H, W, 4)
    hip_mock.unproject(ds, kinv, einv, xyz, V, T, H, W, 1, 0)
    d = ds[t]
    valid = d > 0 if conf is None else (conf.reshape(V, T, H, W)[:, t] > np.float32(conf_thresh)) & (d > 0)
    valid = valid & (valid.reshape(V, -1).sum(1) >= min_points)[:, None, None]
    pts = xyz[t][..., :3][valid].double()
    state.zero_()
    f = state.view(torch.float64)
    state[hip.SN_M] = M = pts.shape[0]
    state[hip.SN_NONFINITE] = int((valid & ~torch.isfinite(d)).sum())
    if M == 0:
        return
    c = pts.mean(0)
    f[hip.SN_CENTROID:hip.SN_CENTROID + 3] = c
    q, kb, lo, hi = _quantile(torch.sort(pts[:, 2].float()).values.numpy(), q_floor)
    f[hip.SN_Z_QUANTILE], f[hip.SN_FLOOR], f[hip.SN_Z_LO], f[hip.SN_Z_HI] = q, q - float(c[2]), lo, hi
    state[hip.SN_Z_RANK] = kb
    if q_radius is not None:
        lifted = pts - c
        lifted[:, 2] -= q - float(c[2])
        q, kb, lo, hi = _quantile(torch.sort(lifted.norm(dim=1).float()).values.numpy(), q_radius)
        f[hip.SN_R_QUANTILE], f[hip.SN_R_LO], f[hip.SN_R_HI] = q, lo, hi
        state[hip.SN_R_RANK] = kb


def _xf(params):
    p = torch.tensor([float(v) for v in params], dtype=torch.float64)
    return float(p[0]), p[1:10].reshape(3, 3), p[10:13]


def _points(x, s, R, t):
    return ((s * x.double()) @ R.T + t).float()


def scene_apply(params, depths=None, depths_out=None, extrs=None, extrs_out=None, queries=None, queries_out=None):
    calls.append("scene_apply")
    s, R, t = _xf(params)
    if depths is not None:
        depths_out.copy_((depths.double() * s).float())
    if extrs is not None:
        e = extrs.reshape(-1, 3, 4).double()
        rot = e[:, :, :3] @ R.T
        extrs_out.reshape(-1, 3, 4).copy_(torch.cat([rot, (s * e[:, :, 3] - rot @ t)[..., None]], -1).float())
    if queries is not None:
        q = queries.reshape(-1, 4)
        queries_out.reshape(-1, 4).copy_(torch.cat([q[:, :1], _points(q[:, 1:], s, R, t)], 1))


def scene_tracks(params, tracks, out):
    calls.append("scene_tracks")
    out.reshape(-1, 3).copy_(_points(tracks.reshape(-1, 3), *_xf(params)))


def install(monkeypatch):
    import sys
    from mvtracker_amd import hip
    hip_mock.install(monkeypatch)
    me = sys.modules[__name__]
    del calls[:]
    for name in "select_kth scene_stats scene_apply scene_tracks".split():
        monkeypatch.setattr(hip, name, getattr(me, name))
