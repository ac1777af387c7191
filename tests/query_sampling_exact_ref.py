"""Integer restatement of query sampling's k-means ("Query sampling"; include/mvtracker_hip.h, mvt_kmeans_*) in numpy and
Python integers, for tests/test_gpu_query_sampling_exact.py.  It is written from the specification and knows nothing of workgroups,
tiles or waves: the device's result must not depend on them.

Lattice clouds.  Every coordinate is origin + n / 256 with an integer n in [0, 1024] and origin a multiple of 8 (0, 8, 1024), all
exact in fp32.  A difference of two coordinates is then m / 256 with |m| <= 2^10, its square m^2 / 2^16 with m^2 <= 2^20, and a
squared distance at most 3 * 2^20 < 2^24 units of 2^-16: exact in fp32 in any order of addition, with or without fused
multiply-add.  scale and scale2 are powers of two, so (x - lo) * scale and d2 * scale2 are exact in fp64 and their truncation to
an integer is the same integer everywhere.  ``assert_lattice`` checks the conditions of a cloud.
"""
import math

import numpy as np

MASK = (1 << 64) - 1
UNITS = 256  # lattice steps per coordinate unit
N_MAX = 1024  # largest lattice index
MAX_CAND = 10  # MVT_KMEANS_MAX_CAND


# ------------------------------------------------------------------------------------------------------------------ clouds
def from_lattice(n, origin=0):
    """Lattice indices (M, 3) -> fp32 points origin + n / 256."""
    n = np.asarray(n, np.int64)
    assert n.min() >= 0 and n.max() <= N_MAX and origin % 8 == 0
    return (float(origin) + n.astype(np.float64) / UNITS).astype(np.float32)


def assert_lattice(p, origin=0):
    """The exactness conditions of the module docstring, for points (M, 3) fp32."""
    p = np.asarray(p)
    assert p.dtype == np.float32 and p.ndim == 2 and p.shape[1] == 3
    n = (p.astype(np.float64) - origin) * UNITS
    assert np.array_equal(n, np.floor(n)) and n.min() >= 0 and n.max() <= N_MAX
    assert 3 * N_MAX ** 2 < 2 ** 24  # the largest squared distance, in units of 2^-16, is an integer fp32 holds
    assert (float(origin) + N_MAX / UNITS) * UNITS < 2 ** 24  # and so is every coordinate, in units of 1/256


def blobs(M, seed, origin=0, nblobs=3, sigma=40.0):
    """M lattice points around ``nblobs`` seeded centres (sigma in lattice steps), clipped to the lattice."""
    rng = np.random.default_rng(seed)
    c = rng.integers(200, 825, size=(nblobs, 3))
    n = c[rng.integers(0, nblobs, size=M)] + np.rint(rng.normal(0.0, sigma, size=(M, 3))).astype(np.int64)
    return from_lattice(np.clip(n, 0, N_MAX), origin)


def duplicates(M, locations, seed, origin=0):
    """M points at ``locations`` distinct lattice places, every place taken at least once."""
    rng = np.random.default_rng(seed)
    loc = rng.choice(N_MAX + 1, size=(locations, 3), replace=False)
    which = np.concatenate([np.arange(locations), rng.integers(0, locations, size=M - locations)])
    return from_lattice(loc[rng.permutation(which)], origin)


def separated(sizes, seed, origin=0, spread=6):
    """One blob per entry of ``sizes`` near the nodes of a coarse grid, each moved by up to 60 lattice steps so that no point is
    equidistant from two blobs (gaps of 250 steps or more, every blob within +-spread steps of its place), shuffled."""
    rng = np.random.default_rng(seed)
    grid = np.array([(x, y, z) for x in (128, 512, 896) for y in (128, 512, 896) for z in (128, 512, 896)])
    place = grid[rng.choice(len(grid), size=len(sizes), replace=False)] + rng.integers(-60, 61, size=(len(sizes), 3))
    n = np.concatenate([place[i] + rng.integers(-spread, spread + 1, size=(s, 3)) for i, s in enumerate(sizes)])
    return from_lattice(n[rng.permutation(len(n))], origin)


# ------------------------------------------------------------------------------------------------------------------ statistics
def _pow2_floor(x):
    return math.ldexp(1.0, math.frexp(x)[1] - 1)  # 2^floor(log2 x)


def stats(p, tol=1e-4):
    """-> dict(lo, hi (3,) fp64, scale, scale2, tol_ref, m2).  A value gets qmax = min(2^40, 2^62 / M) levels; scale =
    2^floor(log2(qmax / extent)), scale2 the same of the squared box diagonal; both 1.0 when the extent is 0.  tol_ref = fp32(tol) x
    the mean over axes of the two-pass fp64 variance; m2 = the mean over axes of E[(x - lo)^2] (the size of the device's terms)."""
    x = np.asarray(p, np.float32).astype(np.float64)
    M = len(x)
    lo, hi = x.min(0), x.max(0)
    ext, diag2 = float((hi - lo).max()), float(((hi - lo) ** 2).sum())
    qmax = min(2.0 ** 40, 2.0 ** 62 / M)
    ok = ext > 0.0
    mean = x.sum(0) / M
    var = ((x - mean) ** 2).sum(0) / M
    return dict(lo=lo, hi=hi, scale=_pow2_floor(qmax / ext) if ok else 1.0, scale2=_pow2_floor(qmax / diag2) if ok else 1.0,
                tol_ref=float(np.float32(tol)) * float(var.sum()) / 3.0, m2=float((((x - lo) ** 2).sum(0) / M).sum()) / 3.0)


# ------------------------------------------------------------------------------------------------------------------ seeding
def mix64(z):
    """splitmix64's finaliser on Python integers."""
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def draw64(seed, step, cand):
    return mix64((mix64(seed & MASK) + (step << 8) + cand) & MASK)


def ntrials(k):
    return min(MAX_CAND, 2 + int(math.floor(math.log(k))))


def _d2(x, c):
    """Squared distances of fp64 rows x (M, 3) to one point c (3,): exact for lattice points."""
    d = x - c
    return d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]


def _q(d2, scale2):
    return np.floor(d2 * scale2).astype(np.int64)  # d2 * scale2 <= 2^40: exact in fp64


def seed(p, k, seed, scale2, mutant=None):
    """Greedy k-means++ -> dict(idx (k,) chosen point indices, cands [per step: the candidate indices], winners [per step: the
    winning candidate's number], pots [per step: the potential after it, a Python int], min_d2 (M,) fp32 folded over centres
    0 .. k-2 (inf for k = 1)).  mutant: None, "cand0", "uniform" or "tile_base" (the planted bugs of the issue)."""
    x = np.asarray(p, np.float32).astype(np.float64)
    M, nt = len(x), ntrials(k)
    cands = [(draw64(seed, 0, 0) * M) >> 64]
    min_d2 = np.full(M, np.inf)
    out = dict(idx=[], cands=[], winners=[], pots=[])
    for step in range(k):
        if step > 0:
            min_d2 = np.minimum(min_d2, _d2(x, x[out["idx"][-1]]))
        vs = [_q(np.minimum(min_d2, _d2(x, x[c])), scale2) for c in cands]
        pots = [int(v.sum()) for v in vs]
        w = 0 if mutant == "cand0" else min(range(len(cands)), key=lambda c: (pots[c], c))
        pot = pots[w]
        out["idx"].append(cands[w])
        out["cands"].append(list(cands))
        out["winners"].append(w)
        out["pots"].append(pot)
        if step + 1 == k:
            break
        cs = np.cumsum(vs[w])
        nxt = []
        for t in range(nt):
            r = draw64(seed, step + 1, t)
            uniform = (r * M) >> 64
            if pot == 0 or mutant == "uniform":
                nxt.append(uniform)
                continue
            target = (r * pot) >> 64
            i = int(np.searchsorted(cs, target, side="right"))  # the first point whose inclusive running sum exceeds the target
            if mutant == "tile_base":  # the running sum restarted at the 1024-point tile of the right answer
                t0 = i // 1024 * 1024
                local = np.cumsum(vs[w][t0:t0 + 1024])
                j = int(np.searchsorted(local, target, side="right"))
                i = t0 + j if j < len(local) else uniform
            nxt.append(i)
        cands = nxt
    out["idx"] = np.asarray(out["idx"], np.int64)
    out["min_d2"] = min_d2.astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------------------------ Lloyd
def assign(p, centres, st):
    """-> dict(labels (M,) int32: argmin of the fp64 squared distance, the lowest index on a tie; acc (k, 4) int64: sums of
    floor((x - lo) * scale) and counts; inertia: the integer sum of floor(d2 * scale2); best, second (M,) fp64 squared distances).
    With lattice centres every d2 is exact and so are the labels and the inertia; the sums are exact for any centres."""
    x = np.asarray(p, np.float32).astype(np.float64)
    c = np.asarray(centres, np.float32).astype(np.float64)
    M, k = len(x), len(c)
    labels, best, second = np.empty(M, np.int64), np.empty(M), np.full(M, np.inf)
    if k <= 16:
        d = np.stack([_d2(x, c[j]) for j in range(k)], 1)
        labels[:] = d.argmin(1)
        if k > 1:
            second[:] = np.partition(d, 1, axis=1)[:, 1]
        best[:] = d.min(1)
    else:
        rows = max(1, (1 << 21) // k)
        for i0 in range(0, M, rows):
            dd = x[i0:i0 + rows, None, :] - c[None, :, :]
            d = dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1] + dd[..., 2] * dd[..., 2]
            labels[i0:i0 + rows] = d.argmin(1)
            part = np.partition(d, 1, axis=1)
            best[i0:i0 + rows], second[i0:i0 + rows] = part[:, 0], part[:, 1]
    q = np.floor((x - st["lo"]) * st["scale"]).astype(np.int64)  # (x - lo) * scale <= 2^40: exact in fp64
    acc = np.zeros((k, 4), np.int64)
    if k <= 16:
        for j in range(k):
            m = labels == j
            acc[j, :3], acc[j, 3] = q[m].sum(0), m.sum()
    else:
        for col in range(3):
            np.add.at(acc[:, col], labels, q[:, col])
        acc[:, 3] = np.bincount(labels, minlength=k)
    return dict(labels=labels.astype(np.int32), acc=acc, inertia=int(_q(best, st["scale2"]).sum()), best=best, second=second)


def update(centres, acc, st):
    """-> (new centres (k, 3) fp32 = fp32(lo + sum / (count * scale)) in fp64, empty clusters keeping theirs; the number of empty
    clusters; the fp64 sum of squared shifts)."""
    old = np.asarray(centres, np.float32)
    acc = np.asarray(acc, np.int64)
    cnt = acc[:, 3]
    full = cnt > 0
    new = old.copy()
    new[full] = (st["lo"] + acc[full, :3].astype(np.float64) / (cnt[full, None].astype(np.float64) * st["scale"])).astype(np.float32)
    d = new.astype(np.float64) - old.astype(np.float64)
    return new, int((~full).sum()), float((d * d).sum())


def lloyd(p, centres, st, max_iter=300):
    """Lloyd iterations from ``centres`` with tol = 0 -> [per iteration dict(labels, centres (after the update), shift, empty,
    margin)], ending with the iteration whose shift is 0.0 (the labels repeated).  margin: the smallest (second - best) / second."""
    c, out = np.asarray(centres, np.float32), []
    for _ in range(max_iter):
        a = assign(p, c, st)
        c, empty, shift = update(c, a["acc"], st)
        with np.errstate(invalid="ignore", divide="ignore"):
            margin = float(np.where(a["second"] > 0, (a["second"] - a["best"]) / a["second"], 0.0).min())
        out.append(dict(labels=a["labels"], centres=c, shift=shift, empty=empty, margin=margin))
        if shift == 0.0:
            break
    return out
