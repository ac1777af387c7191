"""Plain numpy restatements of the rules of csrc/knn_corr.hip, for tests/test_gpu_corr_exact.py -- TEST INFRASTRUCTURE ONLY.

Every function states one rule of the kernel file on exact inputs (integer lattice points, integer feature rows, window
coordinates that are multiples of 0.25) in int64 / float64 arithmetic, independent of oracle/ and of tests/hip_mock.py.  A rule
takes ``fault=`` to plant one named mistake; the probes of the test module show that each planted mistake changes the expected
result on the test's own inputs, i.e. that those inputs can see it.

    lt              a candidate survives for d2 <  thr instead of d2 <= thr            (sim_scan)
    tie_high        equal distances are won by the higher index                        (ref_select)
    seg_off         a segment boundary one tile late                                   (ref_scan_keys)
    swap_decode     the patch decode reads the tile number column-major                (tile_points)
    no_lower_clamp  the frame is min(f, T-1) only; a negative frame wraps              (frame_linear)
    ring_no_base    the ring slot is f mod R                                           (slot_ring)
    drop_last_row   the last texel row of the window patch is not loaded               (ref_window)
    swap_axes       the bilinear fractions of x and y are exchanged                    (ref_window)
    perm_dup        the workgroup permutation folds two XCD lanes onto one             (wg_order)
"""
import zlib

import numpy as np

KEY_MAX = -1  # 0xFFFFFFFFFFFFFFFF read as int64 (torch has no uint64 arithmetic)
BIG = 1 << 40  # stands for "no distance": above every lattice d2 (< 2^24)


def rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------ tiles and boxes

def tile_points(P, grid=(0, 0), fault=None):
    """(ntiles, 64): the point that lane l of tile t reads; >= P behind the end of a linear cloud.  grid = (w, h) per view."""
    nt = (P + 63) // 64
    t, l = np.arange(nt)[:, None], np.arange(64)[None, :]
    gw, gh = grid
    if gw == 0:
        return t * 64 + l
    tpr, tph = gw // 8, gh // 8
    v, r = t // (tpr * tph), t % (tpr * tph)
    if fault == "swap_decode":
        tx, ty = r // tph, r % tph
    else:
        ty, tx = r // tpr, r % tpr
    return (v * gh + ty * 8 + (l >> 3)) * gw + tx * 8 + (l & 7)


def ref_boxes(xyz, grid=(0, 0), fault=None):
    """xyz (T, P, 4) fp32 -> (T, ntiles, 8): lo.xyz over non-NaN coordinates, count of all-finite points, hi.xyz, 0."""
    T, P, _ = xyz.shape
    tp = tile_points(P, grid, fault)
    valid = (tp < P)[None]
    pts = xyz[:, np.minimum(tp, P - 1), :3]
    skip = np.isnan(pts) | ~valid[..., None]
    box = np.zeros((T, tp.shape[0], 8), np.float32)
    box[..., 0:3] = np.where(skip, np.inf, pts).min(2)
    box[..., 4:7] = np.where(skip, -np.inf, pts).max(2)
    box[..., 3] = (np.isfinite(pts).all(3) & valid).sum(2)
    return box


def ref_group_boxes(box):
    T, nt, _ = box.shape
    ng = (nt + 63) // 64
    g = np.zeros((T, ng, 8), np.float32)
    for i in range(ng):
        b = box[:, 64 * i:64 * i + 64]
        g[:, i, 0:3] = b[..., 0:3].min(1)
        g[:, i, 4:7] = b[..., 4:7].max(1)
        g[:, i, 3] = b[..., 3].astype(np.float64).sum(1)
    return g


# ------------------------------------------------------------------ kNN on the lattice

def d2_int(cloud, q):
    """Exact squared distances (N, P) int64 and the all-finite flag (P,).  cloud (P, >=3) fp32 lattice (NaN / inf allowed)."""
    c3 = cloud[:, :3]
    fin = np.isfinite(c3).all(1)
    c = np.where(fin[:, None], c3, 0).astype(np.int64)
    d = c[None] - q[:, None, :3].astype(np.int64)
    d2 = (d * d).sum(2)
    assert int(d2.max()) < 1 << 24
    return d2, fin


def make_keys(d2, idx):
    """(bits(float32(d2)) << 32) | index; BIG -> KEY_MAX."""
    bits = d2.astype(np.float32).view(np.int32).astype(np.int64)
    return np.where(d2 >= BIG, KEY_MAX, (bits << 32) | idx)


def seed_threshold(cloud, q, seed, dims=(0, 0, 0, 0)):
    """(N,) first threshold of a seeded scan: the largest d2 over the query's seed points (a coarse seed (v, y, x) stands for the
    fine point (v, 2y, 2x)); BIG where a seed point is not finite."""
    P = cloud.shape[0]
    si = seed.astype(np.int64)
    cw, ch, fw, fh = dims
    if cw > 0:
        v, rem = si // (cw * ch), si % (cw * ch)
        si = (v * fh + 2 * (rem // cw)) * fw + 2 * (rem % cw)
    si = np.clip(si, 0, P - 1)
    d2, fin = d2_int(cloud, q)
    return np.where(fin[si].all(1), np.take_along_axis(d2, si, 1).max(1), BIG)


def ref_select(cloud, q, K, lo=0, hi=None, fault=None, thr=None):
    """The K smallest (d2, index) keys among points [lo, hi): (N, K) int64, ascending, KEY_MAX-padded.  thr (N,): a seeded scan's
    first threshold -- no candidate beyond it is ever listed (the merged result is the same: a valid seed bounds the K-th distance)."""
    P = cloud.shape[0]
    hi = P if hi is None else min(hi, P)
    d2, fin = d2_int(cloud, q)
    idx = np.arange(lo, hi)
    d2s = np.where(fin[lo:hi][None], d2[:, lo:hi], BIG)
    if thr is not None:
        d2s = np.where(d2s > thr[:, None], BIG, d2s)
    tb = np.broadcast_to(-idx if fault == "tie_high" else idx, d2s.shape)
    order = np.lexsort((tb, d2s), axis=-1)[:, :K]
    keys = make_keys(np.take_along_axis(d2s, order, 1), idx[order])
    pad = np.full((q.shape[0], K - keys.shape[1]), KEY_MAX, np.int64)
    return np.concatenate([keys, pad], 1)


def segments(P, nseg, fault=None):
    """Point ranges of the nseg scan segments of a linear cloud."""
    nt = (P + 63) // 64
    tper = (nt + nseg - 1) // nseg
    sh = 1 if fault == "seg_off" else 0
    return [((g * tper + (sh if g else 0)) * 64, min(((g + 1) * tper + (sh if g + 1 < nseg else 0)) * 64, P)) for g in range(nseg)]


def ref_scan_keys(cloud, q, K, nseg, fault=None, thr=None):
    """(N, nseg, K) per-segment key lists (linear tiles)."""
    return np.stack([ref_select(cloud, q, K, a, b, fault, thr) for a, b in segments(cloud.shape[0], nseg, fault)], 1)


def ref_merge(keys, K, P):
    """(N, E) key lists -> (N, K) int32 indices: unsigned order, padding ties by position, index clamped to P-1."""
    u = keys.view(np.uint64)
    order = np.argsort(u, axis=1, kind="stable")[:, :K]
    idx = np.take_along_axis(keys, order, 1) & 0xFFFFFFFF
    return np.minimum(idx, P - 1).astype(np.int32)


def ref_knn(cloud, q, K, fault=None):
    return ref_merge(ref_select(cloud, q, K, fault=fault), K, cloud.shape[0])


def sim_scan(cloud, q, K, grid=(0, 0), seed=None, fault=None):
    """The thresholded scan restated: candidates in tile order survive for d2 <= thr, the list is cut back to the entries within
    its K-th distance when it passes 64, a seed only sets the first threshold.  -> (N, K) int32."""
    P = cloud.shape[0]
    d2, fin = d2_int(cloud, q)
    tp = tile_points(P, grid)
    out = np.empty((q.shape[0], K), np.int32)
    for n in range(q.shape[0]):
        thr = BIG
        if seed is not None:
            s = np.clip(seed[n], 0, P - 1)
            thr = int(d2[n, s].max()) if fin[s].all() else BIG
        ld, li = np.empty(0, np.int64), np.empty(0, np.int64)
        for tile in tp:
            c = tile[tile < P]
            c = c[fin[c]]
            keep = d2[n, c] < thr if fault == "lt" else d2[n, c] <= thr
            ld, li = np.concatenate([ld, d2[n, c][keep]]), np.concatenate([li, c[keep]])
            if len(ld) > 64:
                thr = int(np.sort(ld)[K - 1])
                ld, li = ld[ld <= thr], li[ld <= thr]
        o = np.lexsort((li, ld))[:K]
        out[n] = np.concatenate([li[o], np.full(K - len(o), P - 1)])
    return out


# ------------------------------------------------------------------ slot -> frame

def frame_linear(frame0, s, step, T, fault=None):
    f = frame0 + s * step
    if fault == "no_lower_clamp":
        return min(f, T - 1) % T  # what a Python index does with a negative frame
    return min(max(f, 0), T - 1)


def slot_ring(frame0, s, step, ring, fault=None):
    base, R, lo, hi = ring
    f = min(max(frame0 + s * step, lo), hi)
    return f % R if fault == "ring_no_base" else (f - base) % R


# ------------------------------------------------------------------ gather-dot

def clamp_idx(idx, P):
    i = idx.astype(np.int64) & 0xFFFFFFFF
    return np.where(i >= P, P - 1, i)


def ref_gather_dot(xyz, fvec, idx, targets, coords, slots, groups=1, add_offset=True, add_xyz=False):
    """xyz (F, P, 4), fvec (F, P, C), idx (N, S, K), targets (N, S, C), coords (N, S, 3), slots[s] = store slot of window slot s
    -> (N, S, K, groups + 3 add_offset + 3 add_xyz) float64: grouped dots / sqrt(C / groups), offsets, neighbour coordinates."""
    N, S, K = idx.shape
    P, C = fvec.shape[1], fvec.shape[2]
    i = clamp_idx(idx, P)
    out = []
    for s in range(S):
        nf = fvec[slots[s]][i[:, s]].astype(np.float64).reshape(N, K, groups, C // groups)
        tg = targets[:, s].astype(np.float64).reshape(N, 1, groups, C // groups)
        parts = [(nf * tg).sum(3) / np.sqrt(C / groups)]
        nx = xyz[slots[s]][i[:, s]][..., :3].astype(np.float64)
        if add_offset:
            parts.append(nx - coords[:, s, None].astype(np.float64))
        if add_xyz:
            parts.append(nx)
        out.append(np.concatenate(parts, 2))
    return np.stack(out, 1)


# ------------------------------------------------------------------ window correlation

def ref_window(fmap, targets, coords, N, level, r, fault=None):
    """fmap (BS, h, w, C), targets (BS*N, C), coords (BS*N, 2) level-0 pixels -> (BS*N, (2r+1)^2) float64: the target dotted with
    the zero-padded bilinear sample at (x + a - r, y + b - r) / sqrt(C), output a * (2r+1) + b (first index along x)."""
    BS, h, w, C = fmap.shape
    win, side = 2 * r + 1, 2 * r + 2
    out = np.zeros((targets.shape[0], win * win))
    f64 = fmap.astype(np.float64)
    for row in range(targets.shape[0]):
        cx, cy = float(coords[row, 0]) / 2 ** level, float(coords[row, 1]) / 2 ** level
        x0, y0 = int(np.floor(cx)), int(np.floor(cy))
        ax, ay = cx - x0, cy - y0
        if fault == "swap_axes":
            ax, ay = ay, ax
        dm = f64[row // N] @ targets[row].astype(np.float64)
        xs, ys = x0 - r + np.arange(side), y0 - r + np.arange(side)
        okx, oky = (xs >= 0) & (xs < w), (ys >= 0) & (ys < h)
        if fault == "drop_last_row":
            oky[-1] = False
        patch = np.zeros((side, side))
        patch[np.ix_(oky, okx)] = dm[np.ix_(ys[oky], xs[okx])]
        v = (1 - ay) * ((1 - ax) * patch[:-1, :-1] + ax * patch[:-1, 1:]) + ay * ((1 - ax) * patch[1:, :-1] + ax * patch[1:, 1:])
        out[row] = v.T.reshape(-1) / np.sqrt(C)  # v[b, a] -> a * win + b
    return out


def wg_order(BS, N, fault=None):
    """Workgroup (4 rows each) that block id i of window_corr_levels works on; identity where the XCD order is not taken."""
    nblk = (BS * N + 3) // 4
    ident = np.arange(nblk)
    pf, rem = N // 4, BS % 8
    total = BS * pf
    if not (N % 4 == 0 and nblk == total and total % 8 == 0 and (rem * pf) % 8 == 0):
        return ident, "row"
    xcd, j = ident % (4 if fault == "perm_dup" else 8), ident // 8
    whole = (BS // 8) * pf
    a = ((j // pf) * 8 + xcd) * pf + j % pf
    u = xcd * (rem * pf // 8) + (j - whole)
    b = ((BS - rem) + u // pf) * pf + u % pf
    return np.where(j < whole, a, b), ("whole" if rem == 0 else "leftover")
