"""CPU restatement of the reprojection check (include/mvtracker_hip.h, "Reprojection check") with numpy and scipy.

The rendering rule is reproduced BIT FOR BIT: the projection is fp64 with every product, sum and quotient written out element by
element (never a matmul, which a BLAS may contract into fused multiply-adds), and the z-buffer is ``np.minimum.at`` on the 64-bit
keys (bits of the fp32 depth) << 32 | index.  The scores: integer words exact, SSIM with ``scipy.ndimage.correlate1d(mode="mirror")``
(reflect-101) in fp64.  SSIM's OpenCV parameters are restated by specification (DESIGN): no cv2 is available to record a fixture."""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
WORDS = 16
(N, COVERED, SSE, SAE, SSE_COV, SAE_COV, SSIM, SSIM_COV, N_DEPTH, N_CLOSE, DEPTH_SAE, DEPTH_SAE_CLOSE) = range(12)
C1, C2 = 6.5025, 58.5225


def project(points, intr, extr, H, W, min_depth=0.01):
    """(drawn (M,) bool, u, v (M,) int64, depth bits (M,) uint32) of fp32 points (M,3) through fp32 intr (3,3), extr (3,4)."""
    X = np.asarray(points, np.float32)
    K, E = np.asarray(intr, np.float32).astype(np.float64), np.asarray(extr, np.float32).astype(np.float64)
    x, y, z = (X[:, i].astype(np.float64) for i in range(3))
    with np.errstate(all="ignore"):
        c = [((E[r, 0] * x + E[r, 1] * y) + E[r, 2] * z) + E[r, 3] for r in range(3)]
        uf = (c[0] * K[0, 0]) / c[2] + K[0, 2]
        vf = (c[1] * K[1, 1]) / c[2] + K[1, 2]
        ok = np.isfinite(X).all(1) & (c[2] > np.float64(np.float32(min_depth)))
        ok &= np.isfinite(uf) & np.isfinite(vf) & (np.abs(uf) < 2.0 ** 31) & (np.abs(vf) < 2.0 ** 31)
        u = np.where(ok, uf, 0.0).astype(np.int64)  # truncation toward zero
        v = np.where(ok, vf, 0.0).astype(np.int64)
        ok &= (u >= 0) & (u < W) & (v >= 0) & (v < H)
        zbits = np.where(ok, c[2], 1.0).astype(np.float32).view(np.uint32)
    return ok, u, v, zbits


def splat_keys(keys, points, indices, intr, extr, H, W, min_depth=0.01, splat=1):
    """Draws points (M,3) with the source indices (M,) into the key image keys (H*W,) uint64, in place."""
    ok, u, v, zb = project(points, intr, extr, H, W, min_depth)
    key = (zb.astype(np.uint64) << np.uint64(32)) | np.asarray(indices).astype(np.uint64)
    r = splat // 2
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            px, py = u + dx, v + dy
            m = ok & (px >= 0) & (px < W) & (py >= 0) & (py < H)
            np.minimum.at(keys, (py * W + px)[m], key[m])
    return keys


def resolve(keys, H, W, colors):
    """keys (H*W,) -> (color (3,H,W) uint8, depth (H,W) fp32, index (H,W) int32); colors (n,3) uint8 by source index."""
    empty = keys == EMPTY
    idx = np.where(empty, 0, keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    depth = np.where(empty, np.uint32(0), (keys >> np.uint64(32)).astype(np.uint32)).astype(np.uint32).view(np.float32)
    color = np.where(empty[:, None], 0, np.asarray(colors, np.uint8)[idx]).astype(np.uint8)
    return color.T.reshape(3, H, W).copy(), depth.reshape(H, W), np.where(empty, -1, idx).astype(np.int32).reshape(H, W)


def render_points(points, colors, intr, extr, H, W, min_depth=0.01, splat=1):
    """The list form: (color, depth, index) of points (M,3) fp32 with colors (M,3) uint8; the index is the row."""
    keys = np.full(H * W, EMPTY, np.uint64)
    splat_keys(keys, points, np.arange(len(points)), intr, extr, H, W, min_depth, splat)
    return resolve(keys, H, W, colors)


def to_u8(img):
    """The 8-bit values of a frame: uint8 as it is, a float x as min(max(rint(x), 0), 255) with NaN -> 0."""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return img
    with np.errstate(invalid="ignore"):
        return np.clip(np.nan_to_num(np.rint(img.astype(np.float32)), nan=0.0, posinf=255.0, neginf=0.0), 0, 255).astype(np.uint8)


def render_views(points, valid, rgbs_t, intrs_t, extrs_t, sources="others", min_depth=0.01, splat=1):
    """The clip form on one frame: points (V,H,W,3) fp32 WITH THE DEVICE'S BITS (mvt_clean_points), valid (V,H,W) bool, the frame's
    rgbs_t (V,3,H,W), cameras intrs_t (V,3,3), extrs_t (V,3,4) -> color (V,3,H,W), depth (V,H,W), index (V,H,W).  Index = v H W + pixel."""
    V, H, W, _ = points.shape
    flat = np.arange(V * H * W).reshape(V, H * W)
    cols = to_u8(rgbs_t).transpose(0, 2, 3, 1).reshape(V * H * W, 3)
    out = []
    for tv in range(V):
        keys = np.full(H * W, EMPTY, np.uint64)
        for sv in range(V):
            if sources == "others" and sv == tv:
                continue
            m = valid[sv].reshape(-1) & np.isfinite(points[sv].reshape(-1, 3)).all(1)
            splat_keys(keys, points[sv].reshape(-1, 3)[m], flat[sv][m], intrs_t[tv], extrs_t[tv], H, W, min_depth, splat)
        out.append(resolve(keys, H, W, cols))
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def gaussian_taps():
    w = np.exp(-((np.arange(11) - 5.0) ** 2) / 4.5)
    return w / w.sum()


def grey(img_u8):
    """OpenCV's 8-bit BGR2GRAY on planar (3,H,W) R, G, B."""
    r, g, b = (img_u8[i].astype(np.int64) for i in range(3))
    return ((4899 * r + 9617 * g + 1868 * b + 8192) >> 14).astype(np.float64)


def ssim_map(a_u8, b_u8):
    """The reference's compute_ssim map (H,W) fp64."""
    from scipy.ndimage import correlate1d
    w = gaussian_taps()

    def blur(x):
        return correlate1d(correlate1d(x, w, axis=1, mode="mirror"), w, axis=0, mode="mirror")

    x, y = grey(a_u8), grey(b_u8)
    mu1, mu2 = blur(x), blur(y)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = blur(x * x) - mu1_sq, blur(y * y) - mu2_sq, blur(x * y) - mu12
    return ((2 * mu12 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))


def score(a, b, index, depth, target_depth, depth_tol):
    """One pair's record: a dict word -> Python int / float.  a, b (3,H,W) uint8 or float; index, depth, target_depth (H,W)."""
    a8, b8 = to_u8(a).astype(np.int64), to_u8(b).astype(np.int64)
    H, W = index.shape
    cov = index >= 0
    d = a8 - b8
    se, ae = (d * d).sum(0), np.abs(d).sum(0)
    sm = ssim_map(to_u8(a), to_u8(b))
    zt = np.asarray(target_depth, np.float32)
    with np.errstate(invalid="ignore"):
        dv = cov & np.isfinite(zt) & (zt > 0)
    dd = np.abs(np.asarray(depth, np.float32).astype(np.float64) - zt.astype(np.float64))
    close = dv & (dd <= np.float64(np.float32(depth_tol)))
    return {N: H * W, COVERED: int(cov.sum()), SSE: int(se.sum()), SAE: int(ae.sum()), SSE_COV: int(se[cov].sum()), SAE_COV: int(ae[cov].sum()),
            SSIM: float(sm.sum()), SSIM_COV: float(sm[cov].sum()), N_DEPTH: int(dv.sum()), N_CLOSE: int(close.sum()),
            DEPTH_SAE: float(dd[dv].sum()), DEPTH_SAE_CLOSE: float(dd[close].sum())}


def record_words(rec):
    """The 16 int64 words of a record dict, doubles by their bits."""
    out = np.zeros(WORDS, np.int64)
    for k, v in rec.items():
        out[k] = np.float64(v).view(np.int64) if k in (SSIM, SSIM_COV, DEPTH_SAE, DEPTH_SAE_CLOSE) else v
    return out
