"""A plain restatement of the track-overlay drawing rule (include/mvtracker_hip.h, DESIGN section 8 "Track overlays") in numpy and
Python integers: a sequential painter that redraws every frame from scratch, every primitive in the stated order, the later one
overwriting the earlier.  Its algorithm is not the device's (no keys, no persistent line layer, no atomics).  Shared by
tests/test_overlay_host.py, tests/hip_mock_overlay.py and tests/test_gpu_overlay.py."""
import numpy as np

F = np.float32


def project(tracks, intrs, extrs):
    """tracks (T,N,3), intrs (V,T,3,3), extrs (V,T,3,4) -> px, py, z (V,T,N) float32: the stated operation sequence, one rounding each."""
    x, y, z = (tracks[None, :, :, k].astype(F) for k in range(3))
    E, K = extrs.astype(F)[:, :, None], intrs.astype(F)[:, :, None]  # (V,T,1,3,4), (V,T,1,3,3)
    with np.errstate(all="ignore"):
        c = [((E[..., r, 0] * x + E[..., r, 1] * y) + E[..., r, 2] * z) + E[..., r, 3] for r in range(3)]
        h = [(K[..., r, 0] * c[0] + K[..., r, 1] * c[1]) + K[..., r, 2] * c[2] for r in range(3)]
        return h[0] / h[2], h[1] / h[2], c[2]


def integer_points(px, py, z, pad=0, min_depth=None):
    """-> x, y (int64, 0 where invalid), valid (bool): clip to [-1e4, 1e4] (a NaN stays), + pad in float32, truncate toward zero."""
    with np.errstate(all="ignore"):
        valid = ~(np.isnan(px) | np.isnan(py))
        if min_depth is not None:
            valid &= z > F(min_depth)
        cx = np.clip(px, F(-1e4), F(1e4)) + F(pad)
        cy = np.clip(py, F(-1e4), F(1e4)) + F(pad)
        x = np.where(valid, np.trunc(np.where(valid, cx, 0)), 0).astype(np.int64)
        y = np.where(valid, np.trunc(np.where(valid, cy, 0)), 0).astype(np.int64)
    return x, y, valid


def _box(x0, x1, y0, y1, Hp, Wp):
    x0, x1, y0, y1 = max(x0, 0), min(x1, Wp - 1), max(y0, 0), min(y1, Hp - 1)
    if x0 > x1 or y0 > y1:
        return np.zeros((0, 0), np.int64), np.zeros((0, 0), np.int64)
    return np.meshgrid(np.arange(x0, x1 + 1, dtype=np.int64), np.arange(y0, y1 + 1, dtype=np.int64))


def stroke(a, b, w, Hp, Wp):
    """Pixels (ys, xs) of the stroke of width w from a to b, clipped to the picture.  int64: every term stays below 2.4e18."""
    (ax, ay), (bx, by) = (int(a[0]), int(a[1])), (int(b[0]), int(b[1]))
    h = (w + 1) // 2
    X, Y = _box(min(ax, bx) - h, max(ax, bx) + h, min(ay, by) - h, max(ay, by) + h, Hp, Wp)
    dx, dy = bx - ax, by - ay
    L2 = dx * dx + dy * dy
    ex, ey = X - ax, Y - ay
    q = ex * dx + ey * dy
    at_a = 4 * (ex * ex + ey * ey) <= w * w
    at_b = 4 * ((X - bx) ** 2 + (Y - by) ** 2) <= w * w
    side = 4 * (ex * dy - ey * dx) ** 2 <= w * w * L2
    m = np.where(q <= 0, at_a, np.where(q >= L2, at_b, side))
    return Y[m], X[m]


def disc(c, R, Hp, Wp):
    X, Y = _box(c[0] - R, c[0] + R, c[1] - R, c[1] + R, Hp, Wp)
    m = (X - int(c[0])) ** 2 + (Y - int(c[1])) ** 2 <= R * R
    return Y[m], X[m]


def ring(c, R, Hp, Wp):
    X, Y = _box(c[0] - R - 1, c[0] + R + 1, c[1] - R - 1, c[1] + R + 1, Hp, Wp)
    d4 = 4 * ((X - int(c[0])) ** 2 + (Y - int(c[1])) ** 2)
    m = ((2 * R - 1) ** 2 <= d4) & (d4 <= (2 * R + 1) ** 2)
    return Y[m], X[m]


def to_u8(frames):
    """uint8 as it is; float clamped to [0, 255] and truncated, NaN -> 0."""
    if frames.dtype == np.uint8:
        return frames
    with np.errstate(all="ignore"):
        f = np.where(np.isnan(frames), 0, frames)
        return np.trunc(np.clip(f, 0, 255)).astype(np.uint8)


def rainbow_colors(lut, x, y, valid, query_frames, color_view, pad, Hp):
    """(N,3) uint8: lut[min(255, max(0, y * 256 // Hp))] with y of the track's query frame in view color_view (pad if invalid);
    zeros for a track whose query frame is beyond the clip."""
    T, N = y.shape[1:]
    out = np.zeros((N, 3), np.uint8)
    for n in range(N):
        q = max(int(query_frames[n]), 0)
        if q < T:
            yy = int(y[color_view, q, n]) if valid[color_view, q, n] else pad
            out[n] = lut[min(255, max(0, (yy * 256) // Hp))]
    return out


def frame_ops(t, x, y, valid, visibility, query_frames, trail, w, Hp, Wp, M):
    """The primitives of frame t of ONE view in painter's order: dicts(kind 'line' | 'disc' | 'ring', s, i, ys, xs); x, y, valid (T,N)."""
    ops = []
    if trail != 0 and t >= 1:
        for s in range(0 if trail < 0 else max(0, t - trail), t):
            for i in range(M):
                if s < query_frames[i] or not (valid[s, i] and valid[s + 1, i]):
                    continue
                a, b = (int(x[s, i]), int(y[s, i])), (int(x[s + 1, i]), int(y[s + 1, i]))
                if a == (0, 0) or b == (0, 0):
                    continue
                ys, xs = stroke(a, b, w, Hp, Wp)
                ops.append(dict(kind="line", s=s, i=i, ys=ys, xs=xs))
    for i in range(M):
        if query_frames[i] > t or not valid[t, i] or x[t, i] == 0 or y[t, i] == 0:
            continue
        c = (int(x[t, i]), int(y[t, i]))
        vis = True if visibility is None else bool(visibility[t, i])
        ys, xs = disc(c, 2 * w, Hp, Wp) if vis else ring(c, 2 * w, Hp, Wp)
        ops.append(dict(kind="disc" if vis else "ring", s=t, i=i, ys=ys, xs=xs))
    return ops


def render(rgbs, tracks, visibility, query_frames, intrs, extrs, lut=None, trail=-1, linewidth=2, pad=0, colors="rainbow", color_view=0,
           min_depth=None, max_tracks=None, reverse=False, ops_out=None):
    """-> video (V,T,3,Hp,Wp) uint8, colors (N,3) uint8.  ``reverse``: paint every frame's primitives in the opposite order (a
    picture that depends on the order must change).  ``ops_out``: a dict that receives {(v, t): the frame's primitives}."""
    V, T, _, H, W = rgbs.shape
    N = tracks.shape[1]
    Hp, Wp = H + 2 * pad, W + 2 * pad
    M = N if max_tracks is None else min(N, max_tracks)
    qf = np.maximum(np.asarray(query_frames).astype(np.int64), 0)
    x, y, valid = integer_points(*project(tracks, intrs, extrs), pad, min_depth)
    cols = rainbow_colors(lut, x, y, valid, qf, color_view, pad, Hp) if isinstance(colors, str) else np.asarray(colors, np.uint8)
    video = np.full((V, T, 3, Hp, Wp), 255, np.uint8)
    video[:, :, :, pad:pad + H, pad:pad + W] = to_u8(rgbs)
    for v in range(V):
        for t in range(T):
            ops = frame_ops(t, x[v], y[v], valid[v], visibility, qf, trail, linewidth, Hp, Wp, M)
            if ops_out is not None:
                ops_out[(v, t)] = ops
            for op in (reversed(ops) if reverse else ops):
                video[v, t, :, op["ys"], op["xs"]] = cols[op["i"]]
    return video, cols
