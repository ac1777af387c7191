"""Inputs of the camera alignment tests (tests/test_camera_align_host.py, tests/test_gpu_camera_align.py).

Rendered scene: the ground plane z = 0 and three spheres, rendered exactly (no jitter, no view-dependent distortion: the views agree
on every surface to fp32 rounding) from synth.make_cameras' ring; depth is invalid (0) beyond 5.9.  synth.make_clip is not usable
here: it distorts every ray by a view-dependent +-2 %, up to 7 cm of disagreement between views.
Dyadic clouds: coordinates in multiples of 1/4 (targets) and 1/32 (sources), so every fp32 d2 and every fp64 sum is exact."""
import numpy as np

SPHERES = (((0.4, 0.3, 0.6), 0.6), ((-0.9, 0.5, 0.35), 0.35), ((0.2, -1.0, 0.45), 0.45))
FAR = 5.9
NORMAL_MAX_EDGE = 0.3  # at 48 x 64 most grid neighbours are more than max_distance (5 cm) apart: that default leaves 860 of 6 556 normals
PLANTED = dict(angle_deg=1.5, axis=(0.3, -0.5, 0.8), translation=(0.03, -0.02, 0.025))
# a second view's error of the same size (43 mm mean displacement): only for the host test that shows why two at once are left out
PLANTED_2 = dict(angle_deg=-1.0, axis=(0.7, 0.2, -0.4), translation=(-0.02, 0.03, 0.015))


def render_depth(intr, extr, H, W):
    """z-depth (H, W) float64 of the scene through one camera, 0 where nothing is hit within FAR."""
    R, tv = extr[:, :3], extr[:, 3]
    c = -R.T @ tv
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dc = np.stack([(xs - intr[0, 2]) / intr[0, 0], (ys - intr[1, 2]) / intr[1, 1], np.ones_like(xs)], -1)
    dw = dc @ R
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = np.where(dw[..., 2] < -1e-9, -c[2] / dw[..., 2], np.inf)
    a = (dw * dw).sum(-1)
    for centre, radius in SPHERES:
        oc = c - np.asarray(centre)
        b = 2 * (dw * oc).sum(-1)
        disc = b * b - 4 * a * ((oc * oc).sum() - radius ** 2)
        ls = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
        lam = np.minimum(lam, np.where(ls > 0, ls, np.inf))
    return np.where(lam < FAR, lam, 0.0)


def scene(V, H, W, T=2):
    """dict(depths (1,V,T,1,H,W), intrs (1,V,T,3,3), extrs (1,V,T,3,4)) float32; static over T."""
    from mvtracker_amd import synth
    intrs, extrs = synth.make_cameras(V, T, H, W)
    depths = np.zeros((V, T, 1, H, W), np.float32)
    for v in range(V):
        depths[v, :, 0] = render_depth(intrs[v, 0], extrs[v, 0], H, W)
    return dict(depths=depths[None], intrs=intrs[None].astype(np.float32), extrs=extrs[None].astype(np.float32))


def rigid(angle_deg, axis, translation):
    """4x4 fp64: rotation by angle about the axis through the origin (Rodrigues), then the translation."""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    th = np.deg2rad(angle_deg)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    G = np.eye(4)
    G[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    G[:3, 3] = translation
    return G


def perturbed(extrs, view, G):
    """extrs (1,V,T,3,4) with view's cameras replaced by E G: its unprojected points move by inv(G), so the correction sought is G."""
    out = extrs.astype(np.float64).copy()
    E = out[0, view]
    out[0, view] = E[..., :3] @ G[:3, :] + np.concatenate([np.zeros((3, 3)), E[0, :, 3:]], 1)
    return out.astype(np.float32)


def unproject(depths, intrs, extrs):
    """World points (V,T,H,W,3) fp64 of a clip (batch dim stripped inside), NaN where the depth is not valid."""
    d, K, E = depths[0, :, :, 0].astype(np.float64), intrs[0].astype(np.float64), extrs[0].astype(np.float64)
    V, T, H, W = d.shape
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    pix = np.stack([xs, ys, np.ones_like(xs)], -1)
    out = np.full((V, T, H, W, 3), np.nan)
    for v in range(V):
        for t in range(T):
            cam = (pix @ np.linalg.inv(K[v, t]).T) * d[v, t][..., None]
            out[v, t] = (cam - E[v, t, :, 3]) @ E[v, t, :, :3]
            out[v, t][~(d[v, t] > 0)] = np.nan
    return out


def displacement(D, moved, true):
    """Mean distance between D applied to the points ``moved`` and the points ``true`` (both (..., 3), NaN rows skipped)."""
    D = np.asarray(D, np.float64)
    ok = np.isfinite(moved).all(-1) & np.isfinite(true).all(-1)
    return float(np.linalg.norm(moved[ok] @ D[:3, :3].T + D[:3, 3] - true[ok], axis=-1).mean())


def organised_clouds(points):
    """points (V,T,H,W,3) -> ([V][T] of (Hp*Wp, 4) float32 padded to whole 8x8 patches, (Wp, Hp))."""
    V, T, H, W, _ = points.shape
    Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
    out = np.full((V, T, Hp, Wp, 4), np.nan, np.float32)
    out[..., 3] = 0
    out[:, :, :H, :W, :3] = points
    return [[out[v, t].reshape(-1, 4) for t in range(T)] for v in range(V)], (Wp, Hp)


# ------------------------------------------------------------------------------------------------------------------ dyadic clouds
def dyadic_target(H, W, seed=0, axis_normals=False):
    """(H*W, 3) float32 raster with coordinates in multiples of 1/4 (a bumpy surface over a regular x, y lattice; some NaN rows) and
    (H*W, 3) float32 normals: unit vectors, or with ``axis_normals`` one of +-e_x, +-e_y, +-e_z; some NaN rows (no valid normal)."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    row, col = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    z = 1.5 * np.sin(0.37 * col + seed) + 1.2 * np.cos(0.23 * row) + 0.5 * np.sin(0.11 * col * row)
    pts = np.stack([(col - W // 2) / 4.0, (row - H // 2) / 4.0, np.round(4.0 * z) / 4.0], -1).reshape(-1, 3)
    n = H * W
    if axis_normals:
        nrm = np.zeros((n, 3))
        nrm[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1.0, 1.0], n)
    else:
        nrm = rng.standard_normal((n, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    order = rng.permutation(n)
    pts[order[:max(1, n // 32)]] = np.nan
    nrm[order[max(1, n // 32):max(2, n // 16)]] = np.nan
    return pts.astype(np.float32), nrm.astype(np.float32)


SHIFT = (1 / 16, 1 / 32, -1 / 16)


def dyadic_source(target, count, seed=0):
    """``count`` rows drawn (with repetition when count exceeds them) from the target's raster, shifted by SHIFT: every d2 to a
    lattice point is a multiple of 2^-10 and no two candidates tie (the shift breaks the lattice's symmetries)."""
    rng = np.random.default_rng(seed + 5)
    rows = np.resize(rng.permutation(np.flatnonzero(np.isfinite(target).all(1))), count)
    return (target[rows] + np.asarray(SHIFT, np.float32)).astype(np.float32)


def linear(pts):
    out = np.zeros((len(pts), 4), np.float32)
    out[:, :3] = pts
    return out
