"""CPU stand-ins for the depth cleaning entries of mvtracker_amd.hip (clean_points, clean_search, clean_mask), on top of
tests/hip_mock_scene.py: the host code of mvtracker_amd/clean.py and the predictor's wiring run on CPU tensors.  The fake entries
follow the kernels' rules (validity, fp32 unprojection through hip_mock.unproject, padding to whole 8x8 patches, NaN points) and call
the restatement tests/cloud_clean_ref.py for the search and the statistics; ``calls`` lists the entries called, in order."""
import numpy as np
import torch

import cloud_clean_ref as R
import hip_mock
import hip_mock_scene

calls = []


def clean_points(depths, conf, kinv, einv, V, T, t0, nt, H, W, conf_thresh, sphere, xyz):
    calls.append("clean_points")
    Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
    ds = depths.reshape(V, T, H, W).permute(1, 0, 2, 3).contiguous()
    pts = torch.empty(T, V, H, W, 4)
    hip_mock.unproject(ds, kinv, einv, pts, V, T, H, W, 1, 0)
    pts = pts.permute(1, 0, 2, 3, 4)[:, t0:t0 + nt].numpy()  # (V, nt, H, W, 4)
    d = depths.reshape(V, T, H, W)[:, t0:t0 + nt].numpy()
    c = None if conf is None else conf.reshape(V, T, H, W)[:, t0:t0 + nt].numpy()
    ok = R.valid_pixels(d, c, conf_thresh) & np.isfinite(pts[..., :3]).all(-1)
    if sphere is not None:
        ok &= R.sphere_inside(pts, sphere[:3], sphere[3])
    out = np.full((V, nt, Hp, Wp, 4), np.nan, np.float32)
    out[..., 3] = 0
    out[:, :, :H, :W, :3] = np.where(ok[..., None], pts[..., :3], np.nan)
    xyz.reshape(V * nt, Hp * Wp, 4).copy_(torch.from_numpy(out.reshape(V * nt, Hp * Wp, 4)))


def clean_search(xyz, Cn, Pn, grid, mode, K, radius, min_points, box, gbox, a_out=None, c_out=None):
    from mvtracker_amd import hip
    calls.append("clean_search")
    assert grid == (0, 0) or (grid[0] % 8 == 0 and grid[1] % 8 == 0 and grid[0] * grid[1] == Pn)
    x = xyz.reshape(Cn, Pn, 4).numpy()
    for ci in range(Cn):
        if mode == hip.CLEAN_STATISTICAL:
            a_out.reshape(Cn, Pn)[ci] = torch.from_numpy(R.clean_cloud(x[ci], "statistical", K, 0.0)["a32"])
        else:
            c = R.clean_cloud(x[ci], "radius", radius=radius, min_points=min_points)["c"]
            c_out.reshape(Cn, Pn)[ci] = torch.from_numpy(np.minimum(c, min_points + 1).astype(np.int32))


def clean_mask(a, c, Cn, Pn, mode, std_ratio, min_points, state, keep):
    from mvtracker_amd import hip
    calls.append("clean_mask")
    state.zero_()
    for ci in range(Cn):
        if mode == hip.CLEAN_STATISTICAL:
            ai = a.reshape(Cn, Pn)[ci].numpy().astype(np.float64)
            ok = ~np.isnan(ai)
            st = R.statistics(ai[ok], std_ratio)
            k = np.zeros(Pn, bool)
            k[ok] = st["keep"]
            state.reshape(Cn, 4)[ci] = torch.tensor([st["M"], st["mu"], st["sigma"], st["thr"]], dtype=torch.float64)
        else:
            cc = c.reshape(Cn, Pn)[ci].numpy()
            k = cc > min_points
            state.reshape(Cn, 4)[ci, 0] = float((cc >= 0).sum())
        keep.reshape(Cn, Pn)[ci] = torch.from_numpy(k.astype(np.uint8))


def install(monkeypatch):
    import sys
    from mvtracker_amd import hip
    hip_mock_scene.install(monkeypatch)
    me = sys.modules[__name__]
    del calls[:]
    for name in "clean_points clean_search clean_mask".split():
        monkeypatch.setattr(hip, name, getattr(me, name))
