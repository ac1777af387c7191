"""Seeded inputs of the depth cleaning tests (tests/test_cloud_clean_host.py, tests/test_gpu_cloud_clean.py).

Lattice clouds: coordinates are integers / 4 within +-64, so every fp32 d2 is exact whatever the contraction; a raster of a bumpy
surface with planted NaN rows, duplicate pairs (a = 0 at K = 2) and points 50 units off the surface, and the same points in a seeded
random order, where image neighbours mean nothing.  Rendered clouds: a synth clip with 20 flying pixels per (view, frame)."""
import numpy as np

LATTICE_SHAPES = [(8, 8), (9, 17), (24, 40), (72, 96)]
KS = (1, 2, 16, 17, 20, 64)


def lattice_cloud(H, W, seed=0):
    """(H*W, 3) float32 raster, NaN rows where the point is not valid."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    row, col = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    z = 1.5 * np.sin(0.37 * col) + 1.2 * np.cos(0.23 * row) + 0.5 * np.sin(0.11 * col * row)
    pts = np.stack([(col - W // 2) / 4.0, (row - H // 2) / 4.0, np.round(4.0 * z) / 4.0], -1).reshape(-1, 3)
    n = H * W
    order = rng.permutation(n)
    n_dup, n_off, n_bad = max(1, n // 16), max(1, n // 50), max(1, n // 32)
    src, dst = order[:n_dup], order[n_dup:2 * n_dup]
    pts[dst] = pts[src]  # duplicate pairs
    off = order[2 * n_dup:2 * n_dup + n_off]
    pts[off, 2] += 50.0  # far off the surface
    bad = order[2 * n_dup + n_off:2 * n_dup + n_off + n_bad]
    pts[bad] = np.nan
    assert np.nanmax(np.abs(pts)) <= 64 and np.array_equal(np.nan_to_num(pts * 4), np.round(np.nan_to_num(pts * 4)))
    return pts.astype(np.float32)


def permuted(pts, seed=0):
    return pts[np.random.default_rng(seed + 77).permutation(len(pts))]


def organised(pts, H, W):
    """The raster padded with NaN points to whole 8x8 patches: ((Hp*Wp, 4) float32, (Wp, Hp), index of every input row)."""
    Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
    out = np.full((Hp, Wp, 4), np.nan, np.float32)
    out[..., 3] = 0
    out[:H, :W, :3] = pts.reshape(H, W, 3)
    idx = (np.arange(H)[:, None] * Wp + np.arange(W)[None, :]).reshape(-1)
    return out.reshape(-1, 4), (Wp, Hp), idx


def linear(pts):
    out = np.zeros((len(pts), 4), np.float32)
    out[:, :3] = pts
    return out


def flying_clip(n_flying=20):
    """synth.make_clip(7, V=3, T=2, H=37, W=53, N=4, invalid_frac=0.02) with, in every (view, frame) depth map, the depth of
    ``n_flying`` seeded valid pixels multiplied by a factor in [0.5, 0.8] (one default_rng(0) for the whole clip)."""
    from mvtracker_amd import synth
    clip = synth.make_clip(7, V=3, T=2, H=37, W=53, N=4, invalid_frac=0.02)
    d = clip["depths"].copy()
    rng = np.random.default_rng(0)
    planted = np.zeros(d.shape, bool)
    for v in range(d.shape[1]):
        for t in range(d.shape[2]):
            flat = d[0, v, t, 0].reshape(-1)
            pick = rng.choice(np.flatnonzero(flat > 0), n_flying, replace=False)
            flat[pick] *= rng.uniform(0.5, 0.8, n_flying).astype(np.float32)
            planted[0, v, t, 0].reshape(-1)[pick] = True
    clip["depths"] = d
    clip["planted"] = planted
    return clip
