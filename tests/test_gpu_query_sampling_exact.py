"""Query sampling to the bit: mvt_query_pool and the mvt_kmeans_* kernels against tests/query_sampling_exact_ref.py.

GPU tests (`-m gpu`) go through the entries of mvtracker_amd.hip; the tests without the marker are the CPU-only checks of the
probes themselves.  Every output and workspace tensor is poisoned before a launch (NaN, -1 labels, 0x5A.. state words).

A. Pool.  The pool is `torch.equal` to the rows mvt_unproject writes at stride 1, level 0 for the kept pixels, in raster order;
   membership is recomputed on the host from those device coordinates with torch fp32 operations.  `count` and the whole
   `block_counts` (exclusive prefix of the per-256-pixel counts) are exact.  Shapes of 256, 257 and 700 workgroups (the scan's
   chunk 1, 2 and 3), eight keep patterns driven through the confidence map, planted boundaries on kinv = I, einv = [I | 0].
B. Statistics.  LO / HI / SCALE / SCALE2 bit-equal, the counters zeroed out of the poison, KM_TOL within a derived bar.
C. Seeding.  Chosen points, potential, candidate words and the min_d2 workspace equal the reference's for every case of CASES.
   A target that EQUALS a prefix boundary cannot be planted: the draw is a hash of (seed, step, candidate), so the test cannot
   choose the target; what the cases cover is listed by the CPU checks (winners other than candidate 0, draws in the second tile of
   a two-tile block and beyond a tile's first 256 points, the three mutants caught).
D. One assignment and one update from planted lattice centres: labels, acc, the integer inertia, centres, KM_* words.
E. Control flow (early return, final pass, iterate(16) = 2 x iterate(8)) and a whole run followed iteration by iteration.

Every comparison is torch.equal, np.array_equal or integer equality, except KM_TOL and KM_SHIFT (bars derived at their tests).
"""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import query_sampling_exact_ref as X  # noqa: E402

gpu = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
INF = float("inf")
POISON = 0x5A5A5A5A5A5A5A5A
BIG = 2 ** 22 + 1  # two 1024-point tiles per seeding workgroup (2049 workgroups), the assign and stats grids at their caps


def _hip():
    from mvtracker_amd import hip
    return hip


def t_(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------------------------------------ clouds
@functools.lru_cache(maxsize=None)
def big():
    """2^22 + 1 lattice points whose first two rows are the lattice's corners: every prefix of two or more rows has extent 4.0."""
    n = np.round((X.blobs(BIG, 21).astype(np.float64)) * X.UNITS).astype(np.int64)
    n[0], n[1] = 0, X.N_MAX
    return X.from_lattice(n)


@functools.lru_cache(maxsize=None)
def cloud(name):
    if name == "big":
        return big()
    if name == "dup":
        return X.duplicates(600, 3, 5)
    if name == "sep":
        return X.separated((64, 128, 256, 512, 128, 64), 9, origin=8)
    kind, M, origin = name.split(":")
    assert kind == "blobs"
    return X.blobs(int(M), 100 + int(M) % 97, origin=int(origin))


@functools.lru_cache(maxsize=None)
def stats_of(name, M=None):
    p = cloud(name)
    return X.stats(p if M is None else p[:M])


# ------------------------------------------------------------------------------------------------------------------ device helpers
def workspace(pts_np, k, tol=1e-4, stats=True):
    hip = _hip()
    M = len(pts_np)
    w = dict(pts=t_(pts_np), M=M, k=k,
             state=torch.full((hip.KM_WORDS,), POISON, dtype=torch.int64, device=DEV),
             centres=torch.full((k, 3), NAN, device=DEV),
             labels=torch.full((M,), -1, dtype=torch.int32, device=DEV),
             acc=torch.zeros(k, 4, dtype=torch.int64, device=DEV),  # an input of the assignment: zero on entry
             min_d2=torch.full((M,), NAN, device=DEV),
             partials=torch.full((hip.KMEANS_MAX_CAND * hip.KMEANS_SEED_BLOCKS,), POISON, dtype=torch.int64, device=DEV),
             stat=torch.full((hip.KMEANS_STAT_BLOCKS * 6,), NAN, dtype=torch.float64, device=DEV))
    if stats:
        hip.kmeans_stats(w["pts"], M, float(tol), w["stat"], w["state"])
    return w


def state_of(w):
    torch.cuda.synchronize()
    s = w["state"].cpu().numpy().copy()
    return s, s.view(np.float64)


def snapshot(w):
    torch.cuda.synchronize()
    return {k: w[k].clone() for k in ("state", "centres", "labels", "acc")}


def unchanged(w, snap, keys=("state", "centres", "labels", "acc")):
    torch.cuda.synchronize()
    return all(np.array_equal(bits(w[k].cpu().numpy()), bits(snap[k].cpu().numpy())) for k in keys)


# ================================================================================================================== A. pool
# name -> (V, H, W): 256, 257 and 700 workgroups of 256 pixels (700 = 3 * 233 + 1: the last thread's chunk of the scan is partial)
SHAPES = {"nb256": (1, 256, 256), "nb257": (1, 241, 272), "nb700": (2, 279, 321)}
PATTERNS = ["all", "none", "last", "first", "lane63", "wg_first", "hashed", "empty_runs"]


def keep_pattern(name, n):
    i = np.arange(n, dtype=np.uint64)
    nb = (n + 255) // 256
    hashed = ((i * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)) & np.uint64(1) == 1
    if name == "all":
        return np.ones(n, bool)
    if name == "none":
        return np.zeros(n, bool)
    if name == "last":
        return i == n - 1
    if name == "first":
        return i == 0
    if name == "lane63":
        return i % 64 == 63
    if name == "wg_first":
        return i % 256 == 0
    if name == "hashed":
        return hashed
    blk = (i // 256).astype(np.int64)
    return hashed & ~((blk >= nb // 3) & (blk < nb // 3 + 7)) & ~((blk >= nb // 2) & (blk < nb // 2 + 3)) & (blk < nb - 5)


def test_keep_patterns_are_what_they_say():
    for shape, (V, H, W) in SHAPES.items():
        n = V * H * W
        nb = (n + 255) // 256
        assert nb == int(shape[2:]) and (nb % 3 != 0 or nb <= 512)
        per = {p: np.add.reduceat(keep_pattern(p, n).astype(np.int64), np.arange(0, n, 256)) for p in PATTERNS}
        assert per["all"].sum() == n and per["none"].sum() == 0 and per["last"].sum() == 1 and per["last"][-1] == 1 and per["first"][0] == 1
        assert (per["lane63"][:-1] == 4).all() and (per["wg_first"] == 1).all()
        assert 0.45 * n < per["hashed"].sum() < 0.55 * n and (per["hashed"] > 0).all()
        e = per["empty_runs"] == 0
        assert e[nb // 3:nb // 3 + 7].all() and e[nb // 2:nb // 2 + 3].all() and e[-5:].all() and e.sum() == 15 and per["empty_runs"][-6] > 0


def cameras(V, T, H, W, seed):
    """Seeded pinhole cameras (V,T,3,3), (V,T,3,4), another pose and focal length for every (view, frame) -> kinv, einv on the device."""
    hip = _hip()
    rng = np.random.default_rng(seed)
    intrs, extrs = np.zeros((V, T, 3, 3), np.float32), np.zeros((V, T, 3, 4), np.float32)
    for v in range(V):
        for t in range(T):
            f = W * rng.uniform(0.7, 1.1)
            intrs[v, t] = [[f, 0, W / 2 + rng.uniform(-3, 3)], [0, f * rng.uniform(0.95, 1.05), H / 2 + rng.uniform(-3, 3)], [0, 0, 1]]
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            extrs[v, t, :, :3] = q * np.sign(np.linalg.det(q))
            extrs[v, t, :, 3] = rng.uniform(-1, 1, size=3)
    n = V * T
    kinv, einv = torch.full((n, 9), NAN, device=DEV), torch.full((n, 12), NAN, device=DEV)
    hip.invert_cameras(t_(intrs.reshape(n, 9)), t_(extrs.reshape(n, 12)), kinv, einv, n)
    return kinv, einv


def unprojected_rows(depths, kinv, einv, t):
    """The (V*H*W, 3) rows mvt_unproject writes for frame t at stride 1, level 0, in (view, row, column) order."""
    hip = _hip()
    V, T, _, H, W = depths.shape
    ds = depths[:, :, 0].permute(1, 0, 2, 3).contiguous()
    xyz = torch.full((T, V, H, W, 4), NAN, device=DEV)
    hip.unproject(ds, kinv, einv, xyz, V, T, H, W, 1, 0)
    return xyz[t].reshape(-1, 4)[:, :3].contiguous()


def run_pool(depths, conf, kinv, einv, t, thr=0.5, x0=0.0, y0=0.0, r2=INF, zmin=-INF, zmax=INF, inclusive=False, flags=None):
    hip = _hip()
    V, T, _, H, W = depths.shape
    n = V * H * W
    pool = torch.full((n, 3), NAN, device=DEV)
    count = torch.full((1,), -77, dtype=torch.int32, device=DEV)
    blocks = torch.full(((n + 255) // 256,), -77, dtype=torch.int32, device=DEV)
    hip.query_pool(depths, conf, kinv, einv, V, T, t, H, W, thr, x0, y0, r2, zmin, zmax, pool, count, blocks, radius_inclusive=inclusive,
                   flags=flags)
    torch.cuda.synchronize()
    return pool, count, blocks


def check_pool(depths, conf, kinv, einv, t, rows=None, **kw):
    """One pool call against the membership recomputed from the device's own fp32 coordinates; returns the kept raster indices."""
    V, T, _, H, W = depths.shape
    n = V * H * W
    rows = unprojected_rows(depths, kinv, einv, t) if rows is None else rows
    x, y, z = rows.unbind(1)
    r2v = (x - kw.get("x0", 0.0)) ** 2 + (y - kw.get("y0", 0.0)) ** 2  # torch: two rounded squares, one rounded sum
    r2 = kw.get("r2", INF)
    inside = (r2v <= r2 if kw.get("inclusive") else r2v < r2) & (z >= kw.get("zmin", -INF)) & (z <= kw.get("zmax", INF))
    valid = conf[:, t].reshape(-1) > kw.get("thr", 0.5) if conf is not None else depths[:, t].reshape(-1) > 0
    keep = valid & inside
    pool, count, blocks = run_pool(depths, conf, kinv, einv, t, **kw)
    m = int(keep.sum())
    assert int(count[0]) == m
    assert torch.equal(pool[:m], rows[keep])
    assert bool(torch.isnan(pool[m:]).all())  # rows from M on are not written
    per = torch.nn.functional.pad(keep.to(torch.int64), (0, (-n) % 256)).reshape(-1, 256).sum(1)
    assert torch.equal(blocks.to(torch.int64), torch.cumsum(per, 0) - per)
    return torch.nonzero(keep).reshape(-1).cpu().numpy()


@functools.lru_cache(maxsize=None)
def pool_scene(shape):
    V, H, W = SHAPES[shape]
    rng = np.random.default_rng(V * H * W)
    depths = t_(rng.uniform(0.5, 4.0, size=(V, 1, 1, H, W)).astype(np.float32))
    kinv, einv = cameras(V, 1, H, W, seed=H)
    return depths, kinv, einv, unprojected_rows(depths, kinv, einv, 0)


@gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_pool_keep_patterns_and_scan_shapes(shape, pattern):
    depths, kinv, einv, rows = pool_scene(shape)
    keep = keep_pattern(pattern, rows.shape[0])
    conf = t_(keep.astype(np.float32)).reshape(depths.shape)
    idx = check_pool(depths, conf, kinv, einv, 0, rows=rows)
    assert np.array_equal(idx, np.flatnonzero(keep))  # geometry plays no part


@gpu
@pytest.mark.parametrize("t", [0, 2])
@pytest.mark.parametrize("with_conf", [True, False])
def test_pool_geometry_three_frames(t, with_conf):
    """T = 3 with another depth map and camera for every frame, a finite cylinder off the axis and a z range; 1961 pixels per view."""
    V, T, H, W = 2, 3, 37, 53
    rng = np.random.default_rng(7)
    d = rng.uniform(0.5, 4.0, size=(V, T, 1, H, W)).astype(np.float32)
    d[rng.random(d.shape) < 0.03] = 0.0
    d[rng.random(d.shape) < 0.01] = NAN
    d[rng.random(d.shape) < 0.01] = -1.0
    depths = t_(d)
    conf = t_((rng.integers(0, 5, size=d.shape) / 4.0).astype(np.float32)) if with_conf else None
    kinv, einv = cameras(V, T, H, W, seed=3)
    kept = {}
    for inclusive in (False, True):
        kept[inclusive] = check_pool(depths, conf, kinv, einv, t, thr=0.5, x0=0.25, y0=-0.5, r2=float(np.float32(1.7) ** 2), zmin=-1.0, zmax=1.5,
                                     inclusive=inclusive)
    assert 50 < len(kept[False]) < V * H * W - 50
    other = check_pool(depths, conf, kinv, einv, 1, thr=0.5, x0=0.25, y0=-0.5, r2=float(np.float32(1.7) ** 2), zmin=-1.0, zmax=1.5)
    assert not np.array_equal(other, kept[False])  # frame 1 is another frame


def planted(depth=None, conf=None, H=8, W=8):
    """kinv = I, einv = [I | 0]: pixel (x, y) at depth d is the point (x d, y d, d) exactly."""
    d = np.ones((1, 1, 1, H, W), np.float32) if depth is None else np.asarray(depth, np.float32).reshape(1, 1, 1, H, W)
    kinv = t_(np.eye(3, dtype=np.float32).reshape(1, 9))
    einv = t_(np.eye(3, 4, dtype=np.float32).reshape(1, 12))
    return t_(d), (None if conf is None else t_(np.asarray(conf, np.float32).reshape(1, 1, 1, H, W))), kinv, einv


def pool_pixels(depths, conf, kinv, einv, **kw):
    """-> the set of (x, y) the pool kept, read back from the points themselves (depth 1: the point is (x, y, 1))."""
    pool, count, _ = run_pool(depths, conf, kinv, einv, 0, **kw)
    return {(int(p[0]), int(p[1])) for p in pool[:int(count[0])].cpu().numpy()}


@gpu
def test_pool_planted_boundaries():
    hip = _hip()
    ring = {(3, 4), (4, 3), (0, 5), (5, 0)}  # x^2 + y^2 = 25 exactly
    inner = {(x, y) for x in range(8) for y in range(8) if x * x + y * y < 25}
    d, _, kinv, einv = planted()
    assert pool_pixels(d, None, kinv, einv, r2=25.0) == inner
    assert pool_pixels(d, None, kinv, einv, r2=25.0, inclusive=True) == inner | ring
    every = {(x, y) for x in range(8) for y in range(8)}
    assert pool_pixels(d, None, kinv, einv) == every  # infinite radius and z range
    assert pool_pixels(d, None, kinv, einv, zmin=1.0, zmax=1.0) == every  # z_min == z == z_max is kept
    up, down = float(np.nextafter(np.float32(1), np.float32(2))), float(np.nextafter(np.float32(1), np.float32(0)))
    assert pool_pixels(d, None, kinv, einv, zmin=up) == set() and pool_pixels(d, None, kinv, einv, zmax=down) == set()
    # conf == threshold is dropped (strict); validity with a map is the map alone
    conf = np.full((8, 8), 0.5, np.float32)
    conf[2, 3], conf[0, 0] = 0.75, 0.25
    assert pool_pixels(*planted(conf=conf), thr=0.5) == {(3, 2)}
    # depth 0, a negative and a NaN depth: dropped without a map; with a map only the NaN is (its coordinates fail every test)
    dd = np.ones((8, 8), np.float32)
    dd[1, 1], dd[2, 2], dd[3, 3] = 0.0, -1.0, NAN
    assert pool_pixels(*planted(depth=dd)) == every - {(1, 1), (2, 2), (3, 3)}
    d, c, kinv, einv = planted(depth=dd, conf=np.ones((8, 8), np.float32))
    pool, count, _ = run_pool(d, c, kinv, einv, 0)
    rows = pool[:int(count[0])].cpu().numpy()
    assert len(rows) == 63 and np.array_equal(rows[9], [0, 0, 0]) and np.array_equal(rows[18], [-2, -2, -1]) and np.array_equal(rows[27], [4, 3, 1])
    d, c, kinv, einv = planted(depth=dd, conf=np.ones((8, 8), np.float32))
    assert int(run_pool(d, c, kinv, einv, 0, zmin=0.5)[1][0]) == 61  # (the z test still applies to the points a map lets through)
    # an unknown flag bit is refused before any launch
    d, _, kinv, einv = planted()
    with pytest.raises(hip.HipError, match="arguments rejected"):
        run_pool(d, None, kinv, einv, 0, flags=2)
    with pytest.raises(hip.HipError, match="arguments rejected"):
        run_pool(d, None, kinv, einv, 0, flags=hip.POOL_RADIUS_INCLUSIVE | 4)
    pool = torch.full((64, 3), NAN, device=DEV)
    count, blocks = torch.full((1,), -77, dtype=torch.int32, device=DEV), torch.full((1,), -77, dtype=torch.int32, device=DEV)
    with pytest.raises(hip.HipError, match="arguments rejected"):
        hip.query_pool(d, None, kinv, einv, 1, 1, 0, 8, 8, 0.5, 0.0, 0.0, INF, -INF, INF, pool, count, blocks, flags=2)
    torch.cuda.synchronize()
    assert bool(torch.isnan(pool).all()) and int(count[0]) == -77 and int(blocks[0]) == -77


# ================================================================================================================== B. statistics
def _stats_cloud(name):
    if name == "identical":
        return np.repeat(X.blobs(1, 3), 300, 0)
    if name == "degenerate_axis":
        p = X.blobs(1000, 4).copy()
        p[:, 2] = p[0, 2]
        return p
    if name == "origin1024":
        return cloud("blobs:5003:1024")
    if name == "min_first_max_last":  # 1000 = 3 * 256 + 232: the last point sits in a partial workgroup
        n = np.random.default_rng(6).integers(1, X.N_MAX, size=(1000, 3))
        n[0], n[-1] = 0, X.N_MAX
        return X.from_lattice(n)
    M = int(name[1:])
    return big()[:M] if M > 257 else X.blobs(M, M)


STATS = ["M1", "M255", "M256", "M257", "M262145", f"M{2 ** 22}", f"M{BIG}", "identical", "degenerate_axis", "origin1024", "min_first_max_last"]


def test_the_sum_budget_moves_the_scale_between_2_to_the_22_and_one_more():
    a, b = stats_of("big", 2 ** 22), stats_of("big")
    assert (a["hi"] - a["lo"]).max() == 4.0 and (b["hi"] - b["lo"]).max() == 4.0
    assert a["scale"] == 2.0 ** 38 and b["scale"] == 2.0 ** 37  # 2^62 / M falls below 2^40 at M = 2^22 + 1
    one = X.stats(_stats_cloud("identical"))
    assert one["scale"] == 1.0 and one["scale2"] == 1.0 and one["tol_ref"] == 0.0 and one["m2"] == 0.0
    for name, origin in (("big", 0), ("dup", 0), ("sep", 8), ("blobs:5003:0", 0), ("blobs:5003:1024", 1024), ("blobs:20011:8", 8)):
        X.assert_lattice(cloud(name), origin)
    s = X.stats(_stats_cloud("min_first_max_last"))
    assert s["lo"].tolist() == [0.0] * 3 and s["hi"].tolist() == [4.0] * 3


@gpu
@pytest.mark.parametrize("name", STATS)
def test_statistics(name):
    """KM_TOL's bar, 1e-12 x tol x m2 with m2 the mean over axes of E[(x - lo)^2], is derived, not measured: the device adds fp64
    terms (x - lo) and (x - lo)^2 along a strided loop of at most 16 steps per lane, a 6-step wave tree, 4 waves, at most 16 partials
    per lane of the last wave and another tree -- at most about 64 roundings of 2^-53 = 1.1e-16 each, relative to a sum whose size
    m2 measures; the variance is the difference of two such terms (E[d^2] and mean^2 <= E[d^2]), so its absolute error is below
    2 x 64 x 1.1e-16 x m2 = 1.4e-14 m2 per axis and the bar leaves a factor of roughly 50 (the fp64 two-pass reference's own error
    is of the same small size)."""
    hip = _hip()
    p = _stats_cloud(name)
    tol = 1e-4
    ref = X.stats(p, tol)
    w = workspace(p, 1, tol)
    s, f = state_of(w)
    assert np.array_equal(bits(f[hip.KM_LO:hip.KM_LO + 3]), bits(ref["lo"])) and np.array_equal(bits(f[hip.KM_HI:hip.KM_HI + 3]), bits(ref["hi"]))
    assert f[hip.KM_SCALE] == ref["scale"] and f[hip.KM_SCALE2] == ref["scale2"]
    for word in (hip.KM_ITER, hip.KM_CONVERGED, hip.KM_EMPTY, hip.KM_INERTIA, hip.KM_INERTIA_ACC, hip.KM_SHIFT, hip.KM_POT):
        assert s[word] == 0, word
    assert (s[hip.KM_CAND:] == POISON).all()  # not the statistics' words
    bar = 1e-12 * float(np.float32(tol)) * ref["m2"]
    print(f"{name}: M {len(p)} scale 2^{math.log2(ref['scale']):.0f} scale2 2^{math.log2(ref['scale2']):.0f} tol {f[hip.KM_TOL]:.17g} "
          f"ref {ref['tol_ref']:.17g} |diff| {abs(f[hip.KM_TOL] - ref['tol_ref']):.3e} bar {bar:.3e}")
    assert abs(f[hip.KM_TOL] - ref["tol_ref"]) <= bar


# ================================================================================================================== C. seeding
# name -> (cloud, M, k, seed).  The seeds are chosen so that the CPU checks below hold (test_seed_cases_cover_what_they_claim).
CASES = {
    "1x1": ("blobs:5003:0", 1, 1, 0),
    "257x2": ("blobs:5003:0", 257, 2, 0),
    "1024x3": ("blobs:5003:0", 1024, 3, 0),  # exactly one tile
    "1025x8": ("blobs:5003:0", 1025, 8, 0),
    "1025x8_seed1": ("blobs:5003:0", 1025, 8, 1),
    "1025x8_seed2^63": ("blobs:5003:0", 1025, 8, 2 ** 63),
    "1025x8_seed-1": ("blobs:5003:0", 1025, 8, -1),
    "5003x7": ("blobs:5003:0", 5003, 7, 0),
    "5003x64": ("blobs:5003:0", 5003, 64, 0),
    "5003x7_origin1024": ("blobs:5003:1024", 5003, 7, 0),
    "20011x1000": ("blobs:20011:8", 20011, 1000, 0),  # ntrials = 8
    "4200x4096": ("blobs:5003:0", 4200, 4096, 0),  # ntrials = 10 = MVT_KMEANS_MAX_CAND, k at its limit
    "big_x3": ("big", BIG, 3, 0),  # two tiles per workgroup, 2049 workgroups
    "duplicates": ("dup", 600, 5, 7),  # the potential reaches 0: uniform draws and winner 0 from then on
}


def case_points(name):
    c, M, k, seed = CASES[name]
    return cloud(c)[:M], k, seed, stats_of(c, M)["scale2"]


@functools.lru_cache(maxsize=None)
def seed_ref(name, mutant=None):
    p, k, seed, scale2 = case_points(name)
    return X.seed(p, k, seed, scale2, mutant)


def test_hash_and_trial_count():
    assert X.mix64(0) == 0xE220A8397B1DCDAF and X.mix64(1) == 0x910A2DEC89025CC1  # splitmix64's first outputs for the seeds 0 and 1
    assert X.draw64(-1, 0, 0) == X.draw64(2 ** 64 - 1, 0, 0) != X.draw64(2 ** 63, 0, 0)
    assert [X.ntrials(k) for k in (1, 2, 3, 7, 8, 64, 1000, 2980, 2981, 4096)] == [2, 2, 3, 3, 4, 6, 8, 9, 10, 10]


@pytest.mark.parametrize("name", list(CASES))
def test_seed_cases_cover_what_they_claim(name):
    p, k, seed, scale2 = case_points(name)
    r = seed_ref(name)
    assert len(r["idx"]) == k and all(len(c) == (1 if s == 0 else X.ntrials(k)) for s, c in enumerate(r["cands"]))
    if k > 1:
        assert any(w != 0 for w in r["winners"]), "every winner is candidate 0: choose another seed"
    if name == "duplicates":
        assert r["pots"][1] > 0 and r["pots"][2] == 0 and r["pots"][-1] == 0 and r["winners"][3:] == [0, 0]
        assert len(np.unique(p[r["idx"][:3]], axis=0)) == 3
    else:
        assert len(np.unique(r["idx"])) == k and all(a > b for a, b in zip(r["pots"], r["pots"][1:]))
    if name == "big_x3":
        drawn = np.array([c for cs in r["cands"][1:] for c in cs])
        assert (drawn % 2048 >= 1024).any() and (drawn % 1024 >= 256).any() and (drawn >= 2048).any()
        assert not np.array_equal(seed_ref(name, "tile_base")["idx"], r["idx"])
    if name in ("5003x7", "5003x64"):
        for mutant in ("cand0", "uniform", "tile_base"):
            assert not np.array_equal(seed_ref(name, mutant)["idx"], r["idx"]), mutant
    if name == "4200x4096":
        assert X.ntrials(k) == X.MAX_CAND


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_seeding(name):
    hip = _hip()
    p, k, seed, _ = case_points(name)
    r = seed_ref(name)
    w = workspace(p, k)
    sd = seed & X.MASK
    hip.kmeans_seed(w["pts"], w["M"], k, sd - 2 ** 64 if sd >= 2 ** 63 else sd, w["min_d2"], w["partials"], w["centres"], w["state"])
    s, f = state_of(w)
    got = w["centres"].cpu().numpy()
    first_wrong = next((i for i in range(k) if not np.array_equal(bits(got[i]), bits(p[r["idx"][i]]))), None)
    print(f"{name}: M {len(p)} k {k} potential {int(s[hip.KM_POT])} (ref {r['pots'][-1]}), first centre that differs: {first_wrong}")
    assert first_wrong is None
    assert int(s[hip.KM_POT]) == r["pots"][-1]
    last = r["cands"][-1]
    assert s[hip.KM_CAND:hip.KM_CAND + len(last)].tolist() == last
    assert (s[hip.KM_CAND + len(last):] == POISON).all()
    assert np.array_equal(bits(w["min_d2"].cpu().numpy()), bits(r["min_d2"]))


# ================================================================================================================== D. assign, update
FAR = (0, 63, 64, 255, 256)  # (and k - 1): an empty cluster in every wave and in the strided loop of the one-workgroup update


def planted_centres(p, k, seed, far=True):
    """k lattice centres: distinct points of the cloud, and at FAR and k - 1 (where k > 8) centres 8192 + j lattice steps up every
    axis, far outside the cloud.  A far centre's d2 is beyond 2^24 units and rounds in fp32; it only has to lose every comparison,
    and it does by a wide factor (no point is assigned to it, so it enters neither the sums nor the inertia)."""
    rng = np.random.default_rng(seed)
    c = p[rng.choice(len(p), size=k, replace=False)].copy()
    if far and k > 8:
        for j in sorted({j for j in FAR + (k - 1,) if j < k}):
            c[j] = p.min(0) + np.float32((8192 + j) / X.UNITS)
    return c


ASSIGN = [(k, M) for k in (1, 7, 255, 256, 257, 1024, 1025, 4096) for M in sorted({k + 3, 5003}) if M >= k]


def assign_case(k, M):
    p = cloud("blobs:5003:0")[:M]
    return p, planted_centres(p, k, seed=k + M)


def run_assign_update(p, c, ref_st):
    """One assignment and one update on the device against the reference; returns (labels, acc before the update)."""
    hip = _hip()
    k = len(c)
    a = X.assign(p, c, ref_st)
    new, empty, shift = X.update(c, a["acc"], ref_st)
    w = workspace(p, k)
    w["centres"].copy_(torch.from_numpy(c))
    hip.kmeans_assign(w["pts"], w["M"], w["centres"], k, w["labels"], w["acc"], w["state"])
    s, f = state_of(w)
    labels, acc = w["labels"].cpu().numpy(), w["acc"].cpu().numpy().copy()
    assert np.array_equal(labels, a["labels"])
    assert np.array_equal(acc, a["acc"])
    assert int(s[hip.KM_INERTIA_ACC]) == a["inertia"] and s[hip.KM_ITER] == 0
    hip.kmeans_update(w["centres"], k, w["acc"], w["state"])
    s, f = state_of(w)
    assert np.array_equal(bits(w["centres"].cpu().numpy()), bits(new))
    assert f[hip.KM_INERTIA] == a["inertia"] / ref_st["scale2"]  # an integer below 2^62 over a power of two
    assert s[hip.KM_EMPTY] == empty and s[hip.KM_ITER] == 1 and s[hip.KM_INERTIA_ACC] == 0
    assert int(w["acc"].abs().max()) == 0
    # KM_SHIFT: at most 3 k <= 12288 non-negative fp64 terms added in an order the reference does not know: any order is within
    # (n - 1) x 2^-53 < 1.4e-12 relative of the exact sum, so two orders differ by less than 2.8e-12 < 1e-11
    print(f"k {k} M {len(p)}: empty {empty}, inertia {a['inertia']}, shift {f[hip.KM_SHIFT]:.17g} ref {shift:.17g}")
    assert abs(f[hip.KM_SHIFT] - shift) <= 1e-11 * shift
    return labels, acc, empty


def test_assign_cases_are_exact_in_the_reference():
    p, c = assign_case(257, 5003)
    a = X.assign(p, c, stats_of("blobs:5003:0"))
    near = np.delete(np.arange(257), [0, 63, 64, 255, 256])
    far2 = ((p[:, None, :].astype(np.float64) - c[None, [0, 63, 64, 255, 256]].astype(np.float64)) ** 2).sum(2).min()
    assert far2 > 100 * a["best"].max() and not np.isin(a["labels"], [0, 63, 64, 255, 256]).any() and len(near) == 252
    assert a["acc"][:, 3].sum() == 5003 and a["inertia"] > 0
    d2 = a["best"] * 2.0 ** 16
    assert np.array_equal(d2, np.floor(d2)) and d2.max() < 2 ** 24  # integers of 2^-16 that fp32 holds


@gpu
@pytest.mark.parametrize("k,M", ASSIGN)
def test_assign_and_update(k, M):
    p, c = assign_case(k, M)
    _, _, empty = run_assign_update(p, c, X.stats(p))
    assert k <= 8 or empty >= len({j for j in FAR + (k - 1,) if j < k})


@gpu
def test_assign_at_the_grid_cap():
    p = big()
    c = X.from_lattice([[300, 300, 300], [700, 500, 400], [400, 800, 700]])
    run_assign_update(p, c, stats_of("big"))


def tie_case():
    """Point 0 moved to the lattice's corner, everything else at 64 steps or more from it; centres 2 and 5 at distance 2 steps from
    the corner along two axes (an exact tie: 2 wins), centres 1 and 4 identical (4 stays empty)."""
    n = np.round(cloud("blobs:5003:0").astype(np.float64) * X.UNITS).astype(np.int64)
    n = np.clip(n, 64, X.N_MAX)
    n[0] = 0
    p = X.from_lattice(n)
    c = p[[10, 20, 30, 40, 50, 60, 70]].copy()
    c[2], c[5] = X.from_lattice([[2, 0, 0]])[0], X.from_lattice([[0, 0, 2]])[0]
    c[4] = c[1]
    return p, c


def test_tie_case_has_its_ties():
    p, c = tie_case()
    a = X.assign(p, c, X.stats(p))
    assert a["labels"][0] == 2 and a["best"][0] == a["second"][0] == 4 / 65536
    assert (a["labels"] == 1).sum() > 0 and (a["labels"] == 4).sum() == 0 and a["acc"][4, 3] == 0
    assert (a["best"][a["labels"] == 1] == a["second"][a["labels"] == 1]).all()


@gpu
def test_assign_ties_go_to_the_lower_index():
    p, c = tie_case()
    labels, acc, empty = run_assign_update(p, c, X.stats(p))
    assert labels[0] == 2 and (labels == 4).sum() == 0 and empty >= 1


@gpu
def test_lds_and_global_accumulation_agree():
    """k = 1024 adds the sums up in LDS first, k = 1025 (one far centre more) adds to global memory directly."""
    p = cloud("blobs:5003:0")
    c = planted_centres(p, 1024, seed=77)
    far = (p.min(0) + np.float32(40.0))[None]
    la, aa, _ = run_assign_update(p, c, X.stats(p))
    lb, ab, _ = run_assign_update(p, np.concatenate([c, far]), X.stats(p))
    assert np.array_equal(la, lb) and np.array_equal(aa, ab[:1024]) and (ab[1024] == 0).all()


# ================================================================================================================== E. control flow
def lloyd_ready(tol=1e-4):
    """(5003, 7) after statistics and seeding, labels and acc as a fresh run has them."""
    hip = _hip()
    p = cloud("blobs:5003:0")
    w = workspace(p, 7, tol)
    hip.kmeans_seed(w["pts"], w["M"], 7, 0, w["min_d2"], w["partials"], w["centres"], w["state"])
    return p, w


@gpu
@pytest.mark.parametrize("why", ["converged", "max_iter"])
def test_a_finished_run_is_left_untouched(why):
    hip = _hip()
    p, w = lloyd_ready()
    max_iter = 5
    if why == "converged":
        w["state"][hip.KM_CONVERGED] = 1
    else:
        w["state"][hip.KM_ITER] = max_iter
    w["acc"].fill_(123456789)  # (not a state an assignment would leave: it must not be read, added to or cleared)
    snap = snapshot(w)
    args = (w["pts"], w["M"], w["centres"], 7, w["labels"], w["acc"], w["state"])
    hip.kmeans_assign(*args, max_iter)
    assert unchanged(w, snap)
    hip.kmeans_update(w["centres"], 7, w["acc"], w["state"], max_iter)
    assert unchanged(w, snap)
    hip.kmeans_iterate(*args, 3, max_iter)
    assert unchanged(w, snap) and int(w["labels"].max()) == -1
    if why == "max_iter":  # ITER > max_iter as well
        w["state"][hip.KM_ITER] = max_iter + 1
        snap = snapshot(w)
        hip.kmeans_iterate(*args, 2, max_iter)
        assert unchanged(w, snap)


@gpu
@pytest.mark.parametrize("why", ["converged", "max_iter"])
def test_final_pass_runs_regardless_and_changes_only_its_words(why):
    hip = _hip()
    p, w = lloyd_ready()
    st = X.stats(p)
    if why == "converged":
        w["state"][hip.KM_CONVERGED] = 1
    else:
        w["state"][hip.KM_ITER] = 5
    w["state"][hip.KM_SHIFT] = 0x3FF8000000000000  # 1.5: a final pass reports no shift
    c = w["centres"].cpu().numpy()
    a = X.assign(p, c, st)
    before, _ = state_of(w)
    snap = snapshot(w)
    hip.kmeans_assign(w["pts"], w["M"], w["centres"], 7, w["labels"], w["acc"], w["state"], 5, final_pass=True)
    s, f = state_of(w)
    assert np.array_equal(w["labels"].cpu().numpy(), a["labels"]) and np.array_equal(w["acc"].cpu().numpy(), a["acc"])
    assert int(s[hip.KM_INERTIA_ACC]) == a["inertia"]
    assert np.array_equal(np.delete(s, hip.KM_INERTIA_ACC), np.delete(before, hip.KM_INERTIA_ACC)) and unchanged(w, snap, ("centres",))
    hip.kmeans_update(w["centres"], 7, w["acc"], w["state"], 5, final_pass=True)
    s, f = state_of(w)
    assert np.array_equal(w["acc"].cpu().numpy(), a["acc"])  # left holding the sums
    assert f[hip.KM_INERTIA] == a["inertia"] / st["scale2"] and s[hip.KM_EMPTY] == int((a["acc"][:, 3] == 0).sum()) and s[hip.KM_INERTIA_ACC] == 0
    changed = [hip.KM_INERTIA, hip.KM_EMPTY, hip.KM_INERTIA_ACC]
    assert np.array_equal(np.delete(s, changed), np.delete(before, changed)) and unchanged(w, snap, ("centres",))


@gpu
def test_sixteen_iterations_are_two_calls_of_eight():
    hip = _hip()
    runs = []
    for calls in ((16,), (8, 8)):
        p, w = lloyd_ready()
        for n in calls:
            hip.kmeans_iterate(w["pts"], w["M"], w["centres"], 7, w["labels"], w["acc"], w["state"], n, 300)
        runs.append(snapshot(w))
        s, _ = state_of(w)
        assert 1 <= s[hip.KM_ITER] <= 16
    assert all(np.array_equal(bits(runs[0][k].cpu().numpy()), bits(runs[1][k].cpu().numpy())) for k in runs[0])


WHOLE = {6: 0, 2: 8}  # k -> seed of the run on the separated cloud (6 blobs): two iterations at k = 6, three at k = 2


@functools.lru_cache(maxsize=None)
def whole_run(k):
    p = cloud("sep")
    st = X.stats(p, 0.0)
    sr = X.seed(p, k, WHOLE[k], st["scale2"])
    return p, st, sr, X.lloyd(p, p[sr["idx"]], st)


@pytest.mark.parametrize("k", list(WHOLE))
def test_the_whole_run_can_be_followed_exactly(k):
    """At every reference iteration every point's best and second-best squared distances differ by more than 1e-3 relative; the
    device's fp32 distances carry a relative error of a few 2^-24, so its labels are the reference's and the run can be followed
    to the bit.  The final centres of the k = 6 run are dyadic (every blob has a power-of-two size), which makes the fp64 squared
    distances of the final pass exact and its inertia an integer the reference knows."""
    p, st, sr, its = whole_run(k)
    assert st["tol_ref"] == 0.0 and 2 <= len(its) < 50 and its[-1]["shift"] == 0.0 and all(i["shift"] > 0 for i in its[:-1])
    assert all(i["margin"] > 1e-3 for i in its), [i["margin"] for i in its]
    assert np.array_equal(its[-1]["labels"], its[-2]["labels"]) and all(i["empty"] == 0 for i in its)
    if k == 6:
        c = its[-1]["centres"].astype(np.float64) * 2.0 ** 17
        assert np.array_equal(c, np.floor(c)) and sorted(np.bincount(its[-1]["labels"]).tolist()) == [64, 64, 128, 128, 256, 512]


@gpu
@pytest.mark.parametrize("k", list(WHOLE))
def test_whole_run_iteration_by_iteration(k):
    hip = _hip()
    p, st, sr, its = whole_run(k)
    w = workspace(p, k, tol=0.0)
    hip.kmeans_seed(w["pts"], w["M"], k, WHOLE[k], w["min_d2"], w["partials"], w["centres"], w["state"])
    torch.cuda.synchronize()
    assert np.array_equal(bits(w["centres"].cpu().numpy()), bits(p[sr["idx"]]))
    for n, it in enumerate(its + its[-1:] * 2):  # two calls more: a converged run stays where it is
        hip.kmeans_iterate(w["pts"], w["M"], w["centres"], k, w["labels"], w["acc"], w["state"], 1, 300)
        s, f = state_of(w)
        done = n >= len(its) - 1
        assert np.array_equal(bits(w["centres"].cpu().numpy()), bits(it["centres"])), n
        assert np.array_equal(w["labels"].cpu().numpy(), it["labels"]), n
        assert s[hip.KM_ITER] == min(n + 1, len(its)) and s[hip.KM_CONVERGED] == int(done) and s[hip.KM_EMPTY] == 0
        assert (f[hip.KM_SHIFT] == 0.0) == done
        assert abs(f[hip.KM_SHIFT] - it["shift"]) <= 1e-11 * it["shift"]  # (the bar of the update test: at most 3 k fp64 terms)


@gpu
def test_kmeans_centres_returns_the_followed_run():
    from mvtracker_amd import queries
    p, st, sr, its = whole_run(6)
    c, info = queries.kmeans_centres(t_(p), 6, seed=WHOLE[6], tol=0.0)
    a = X.assign(p, its[-1]["centres"], st)
    assert np.array_equal(bits(c.cpu().numpy()), bits(its[-1]["centres"]))
    assert info == {"inertia": a["inertia"] / st["scale2"], "iterations": len(its), "converged": True, "empty": 0}
