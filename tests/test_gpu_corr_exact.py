"""The kNN search and the two correlation operators of csrc/knn_corr.hip on inputs whose right answer is exact.

GPU tests (`-m gpu`) go through `mvtracker_amd.hip`; the tests without the marker are the CPU-only checks of the reference
restatement (tests/corr_exact_ref.py) against oracle/, of the mocks against that restatement, and of the probes.  Every output
buffer is poisoned before the launch (NaN; the sentinels SENT_I / SENT_K for index and key buffers), gets a padded leading
dimension where the entry has one and a guard row behind the last one, and whatever the kernel must not write has to stay poisoned.

Exact inputs.  Points and queries are integers in [-1000, 1000]: a squared distance is an integer below 2^24, so
fma(dz,dz,fma(dy,dy,dx*dx)) is that integer in fp32 and the expected key is (bits(float32(d2)) << 32) | index from int64
arithmetic.  Feature rows, targets and maps are integers in [-3, 3] (exact in bf16): at C <= 256 a dot is an integer of magnitude
<= 2304 in any order.  Window coordinates are multiples of 0.25 in level-0 pixels and there are at most 4 levels, so the
fractions are multiples of 2^-5 and the four-term blend is exact in fp32.  Where the divisor sqrt(C / groups) is a power of two the
comparison is torch.equal; elsewhere |err| <= 2^-22 |ref| against the fp64 quotient (one rounding of sqrtf and one of the
division, 2^-24 each, doubled for a division that is not correctly rounded); a dot off by one is >= 1/2304 relative.

A. tile and group boxes          B. every kNN entry point (shapes, orders, seeds, short frames, refusals)
C. the slot-to-frame map through every entry that takes one, linear and ring
D. gather-dot with planted indices, both store paths, the options form      E. the 1-NN gather
F. window correlation, radius 1..7, and the XCD workgroup permutation with every row compared
G. on the inputs of B..F the mocks of tests/hip_mock.py and tests/hip_mock_ring.py give the kernels' results on CPU copies (bit
   for bit for indices, keys of linear tiles, features, offsets and power-of-two scales; within the bar elsewhere), and the probes:
   each fault of corr_exact_ref planted into the restatement changes the expected result of its section on that section's inputs.

The scans run 2 queries per wave with tile boxes and 8 without; MVT_KNN_Q, read once per process, overrides that.
`knn_queries_per_wave` / `knn_kernels` restate the choice; tests/test_gpu_tuning_switches.py runs B in a child process per value.
"""
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

import corr_exact_ref as R
import hip_mock
import hip_mock_ring
from oracle import mvt_oracle as O

gpu = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
SENT_I = -7777  # no point index
SENT_K = 0x5555555555555555  # no key: its low word is no index of a cloud below 2^30 points, its high word no lattice distance
BAR = 2.0 ** -22

MOCK = types.SimpleNamespace(name="mock", **{n: getattr(hip_mock, n) for n in (
    "tile_aabb tile_group_aabb knn_scan knn_merge knn_search knn_scan_levels knn_merge_levels knn_search_levels corr_gather_dot "
    "corr_gather_dot_opts knn1_gather window_corr").split()}, **{n: getattr(hip_mock_ring, n) for n in (
        "knn_scan_ring knn_search_ring knn_scan_levels_ring knn_search_levels_ring corr_gather_dot_ring corr_gather_dot_opts_ring "
        "knn1_gather_ring").split()})


@pytest.fixture(scope="module")
def hip():
    from mvtracker_amd import hip as h
    assert torch.cuda.is_available()
    return h


def T_(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


def lattice(r, *shape):
    return r.integers(-1000, 1001, shape).astype(np.float32)


def small(r, *shape):
    return r.integers(-3, 4, shape).astype(np.float32)


def cloud4(p3):
    return np.concatenate([p3, np.zeros(p3.shape[:-1] + (1,), np.float32)], -1)


def exact_scale(c_per_group):
    return c_per_group in (1, 4, 16, 64, 256)


def assert_values(got, ref64, exact, what):
    """got fp32 numpy against the fp64 reference: equal where the divisor is a power of two, within the bar elsewhere."""
    if exact:
        assert np.array_equal(got, ref64.astype(np.float32)), what
    else:
        err = np.abs(got.astype(np.float64) - ref64)
        assert np.all(err <= BAR * np.abs(ref64)), (what, float(err.max()))


# ================================================================== A: tile and group boxes

BOX_SHAPES = [(16, (0, 0)), (64, (0, 0)), (65, (0, 0)), (133, (0, 0)), (1000, (0, 0)), (3 * 16 * 24, (24, 16)), (72 * 64, (72, 64))]


@functools.lru_cache(maxsize=None)
def box_cloud(P, grid):
    r = R.rng("box", P, grid)
    xyz = cloud4(lattice(r, 2, P, 3))
    tp = R.tile_points(P, grid)
    xyz[0, 3, 1] = NAN  # one NaN coordinate: the point's other coordinates still count for lo / hi, the point not for .w
    xyz[0, 5, 0] = np.inf  # counts for hi, not for .w
    xyz[1, 7, 2] = -np.inf
    last = tp[-1][tp[-1] < P]
    xyz[1, last, :3] = NAN  # an all-NaN tile (the partial last tile of a linear cloud)
    return xyz


def run_boxes(lib, dev, xyz, grid):
    T, P = xyz.shape[:2]
    nt = (P + 63) // 64
    box = torch.full((T * nt + 1, 8), NAN, device=dev)
    lib.tile_aabb(T_(xyz, dev), P, T, box, grid)
    assert bool(torch.isnan(box[T * nt:]).all())
    return box[:T * nt].reshape(T, nt, 8).cpu().numpy()


@gpu
@pytest.mark.parametrize("P,grid", BOX_SHAPES)
def test_tile_boxes(hip, P, grid):
    xyz = box_cloud(P, grid)
    got = run_boxes(hip, DEV, xyz, grid)
    ref = R.ref_boxes(xyz, grid)
    assert np.array_equal(got, ref)  # (+-inf compare equal to themselves; no NaN is expected anywhere)
    assert not np.isnan(got).any() and np.all(got[..., 7] == 0)


def group_records(ntiles):
    r = R.rng("gbox", ntiles)
    box = np.zeros((2, ntiles, 8), np.float32)
    box[..., 0:3] = lattice(r, 2, ntiles, 3)
    box[..., 4:7] = box[..., 0:3] + r.integers(0, 50, (2, ntiles, 3))
    box[..., 3] = r.integers(0, 65, (2, ntiles))
    box[0, 1, 0:3], box[0, 1, 4:7], box[0, 1, 3] = np.inf, -np.inf, 0  # an all-NaN tile's record
    box[1, ntiles - 1, 4] = np.inf
    return box


@gpu
@pytest.mark.parametrize("ntiles", [3, 64, 65, 72, 130])
def test_group_boxes(hip, ntiles):
    box = group_records(ntiles)
    ng = (ntiles + 63) // 64
    P = ntiles * 64 - 17  # (a partial last tile: the group kernel takes the tile count from P)
    g = torch.full((2 * ng + 1, 8), NAN, device=DEV)
    hip.tile_group_aabb(T_(box, DEV), P, 2, g)
    assert bool(torch.isnan(g[2 * ng:]).all())
    got = g[:2 * ng].reshape(2, ng, 8).cpu().numpy()
    assert np.array_equal(got, R.ref_group_boxes(box))
    m = torch.full((2, ng, 8), NAN)
    hip_mock.tile_group_aabb(torch.from_numpy(box), P, 2, m)
    assert np.array_equal(m.numpy(), got)


@pytest.mark.parametrize("ntiles", [3, 64, 65, 72, 130])
def test_group_boxes_mock_is_the_rule(ntiles):
    box = group_records(ntiles)
    m = torch.full((2, (ntiles + 63) // 64, 8), NAN)
    hip_mock.tile_group_aabb(torch.from_numpy(box), ntiles * 64, 2, m)
    assert np.array_equal(m.numpy(), R.ref_group_boxes(box))


def test_probe_swapped_patch_decode():
    for P, grid in BOX_SHAPES:
        xyz = box_cloud(P, grid)
        same = np.array_equal(R.ref_boxes(xyz, grid, fault="swap_decode"), R.ref_boxes(xyz, grid))
        assert same == (grid[0] == 0), (P, grid)  # every patch shape sees it
        tp = R.tile_points(P, grid)
        assert np.array_equal(np.sort(tp[tp < P]), np.arange(P))  # the decode visits every point once


# ================================================================== B: kNN

KCase = types.SimpleNamespace


def kcase(name, xyz, coords, K, nseg=1, grid=(0, 0), boxed=True, gbox=False, seed=None, seed_dims=(0, 0, 0, 0), fr=(0, 1), ring=None,
          slots=None):
    S = coords.shape[1]
    T = xyz.shape[0]
    if slots is None:
        slots = [R.frame_linear(fr[0], s, fr[1], T) for s in range(S)]
    return KCase(name=name, xyz=xyz, coords=coords, K=K, nseg=nseg, grid=grid, boxed=boxed, gbox=gbox, seed=seed,
                 seed_k=0 if seed is None else seed.shape[2], seed_dims=seed_dims, fr=fr, ring=ring, T=T, slots=slots)


def accepted(P, K, nseg):
    nt = (P + 63) // 64
    return nseg * K <= 64 and P >= K and -(-nt // nseg) * (nseg - 1) < nt


def expect_idx(c, fault=None):
    return np.stack([R.ref_knn(c.xyz[c.slots[s]], c.coords[:, s], c.K, fault) for s in range(c.coords.shape[1])], 1)


def expect_keys(c, nseg, fault=None):
    """Per-segment key lists: the segment's K nearest -- of a seeded scan, those within the seed's threshold (a seed may only prune:
    what lies beyond the largest seed distance is never listed, and the list is KEY_MAX-padded instead)."""
    out = []
    for s in range(c.coords.shape[1]):
        cloud, q = c.xyz[c.slots[s]], c.coords[:, s]
        thr = None if c.seed is None else R.seed_threshold(cloud, q, c.seed[:, s], c.seed_dims)
        out.append(R.ref_scan_keys(cloud, q, c.K, nseg, fault, thr))
    return np.stack(out, 1)


def run_knn(lib, dev, c, entry):
    """One entry point on one case -> {name: cpu tensor}; 'scan*' give key lists (N, S, nseg, K) and merged indices."""
    F_, P = c.xyz.shape[:2]
    N, S = c.coords.shape[:2]
    K, rows = c.K, N * S
    xyz, coords = T_(c.xyz, dev), T_(c.coords, dev)
    nt = (P + 63) // 64
    box = gbox = None
    if c.boxed or entry.startswith("search"):
        box = torch.zeros(F_, nt, 8, device=dev)
        lib.tile_aabb(xyz, P, F_, box, c.grid)
        if c.gbox:
            gbox = torch.zeros(F_, (nt + 63) // 64, 8, device=dev)
            lib.tile_group_aabb(box, P, F_, gbox)
    seed = None if c.seed is None else T_(c.seed, dev)
    where, sfx = (c.ring, "_ring") if c.ring else (c.T, "")
    f0, step = c.fr
    out = {}

    def bufs(nseg):
        return (torch.full(((rows + 1) * nseg * K,), SENT_K, dtype=torch.int64, device=dev),
                torch.full(((rows + 1) * K,), SENT_I, dtype=torch.int32, device=dev))

    def take(tag, keys, idx, nseg):
        if keys is not None:
            assert bool((keys[rows * nseg * K:] == SENT_K).all()), tag
            out[tag + "keys"] = keys[:rows * nseg * K].cpu().reshape(N, S, nseg, K)
        assert bool((idx[rows * K:] == SENT_I).all()), tag
        out[tag + "idx"] = idx[:rows * K].cpu().reshape(N, S, K)

    if entry == "scan":
        keys, idx = bufs(c.nseg)
        getattr(lib, "knn_scan" + sfx)(xyz, P, coords, N, S, f0, step, where, K, c.nseg, keys, seed_idx=seed, seed_k=c.seed_k,
                                       seed_dims=c.seed_dims, box=box, grid=c.grid)
        lib.knn_merge(keys[:rows * c.nseg * K], N, S, K, c.nseg, P, idx[:rows * K])
        take("scan.", keys, idx, c.nseg)
    elif entry == "search":
        _, idx = bufs(1)
        getattr(lib, "knn_search" + sfx)(xyz, P, coords, N, S, f0, step, where, K, idx[:rows * K], box, grid=c.grid, gbox=gbox, seed_idx=seed,
                                         seed_k=c.seed_k, seed_dims=c.seed_dims)
        take("search.", None, idx, 1)
    elif entry == "scan_levels":
        lv, held = [], []
        for nseg in (c.nseg, 1):
            keys, idx = bufs(nseg)
            held.append((keys, idx, nseg))
            lv.append(dict(xyz=xyz, P=P, keys=keys, nseg=nseg, seed_idx=seed, box=box, grid=c.grid, idx_out=idx[:rows * K]))
        getattr(lib, "knn_scan_levels" + sfx)(lv, coords, N, S, f0, step, where, K, seed_k=c.seed_k)
        lib.knn_merge_levels([dict(l, keys=l["keys"][:rows * l["nseg"] * K]) for l in lv], N, S, K)
        for i, (keys, idx, nseg) in enumerate(held):
            take(f"scan_levels{i}.", keys, idx, nseg)
    elif entry == "search_levels":
        lv, held = [], []
        for i in range(2):
            _, idx = bufs(1)
            sd = seed
            if seed is not None and c.seed_k == K:  # in place: idx_out aliases seed_idx
                idx[:rows * K] = seed.reshape(-1)
                sd = idx[:rows * K]
            held.append(idx)
            lv.append(dict(xyz=xyz, P=P, seed_idx=sd, box=box, grid=c.grid, idx_out=idx[:rows * K], gbox=gbox if i == 0 else None))
        getattr(lib, "knn_search_levels" + sfx)(lv, coords, N, S, f0, step, where, K, c.seed_k)
        for i, idx in enumerate(held):
            take(f"search_levels{i}.", None, idx, 1)
    else:
        raise KeyError(entry)
    return out


ENTRIES = ("scan", "search", "scan_levels", "search_levels")
KNN_Q_COMPILED = (1, 2, 4, 8)


def knn_queries_per_wave(boxes, q_env=None):
    """knn_corr.hip: queries per wave of the scan kernels; q_env = MVT_KNN_Q as atoi reads it (0: unset; default: this process's).
    A value outside KNN_Q_COMPILED has no kernel: the entries refuse."""
    if q_env is None:
        m = re.match(r"\s*[+-]?\d+", os.environ.get("MVT_KNN_Q", ""))
        q_env = int(m.group()) if m else 0
    return q_env if q_env else (2 if boxes else 8)


def knn_kernels(c, q_env=None):
    """{(kernel, Q, with tile boxes)} that the entries of case c launch (run_knn: the search entries always get boxes, a levels
    scan has them when every level does)."""
    kern = {"scan": "knn_scan_kernel", "search": "knn_scan_kernel", "scan_levels": "knn_scan_levels_kernel", "search_levels": "knn_search_levels_kernel"}
    out = set()
    for e in entries_of(c):
        boxes = bool(c.boxed) or e.startswith("search")
        out.add((kern[e], knn_queries_per_wave(boxes, q_env), boxes))
    return out


def entries_of(c):
    return tuple(e for e in ENTRIES if not (e.endswith("levels") and c.seed_dims[0]))  # (the levels forms take no coarse seed)


def check_knn(c, res, who):
    want = expect_idx(c)
    for name, t in res.items():
        if name.endswith("idx"):
            assert np.array_equal(t.numpy(), want), (who, c.name, name)
        elif c.grid == (0, 0):  # with patch tiles a segment is a range of patches: only the merged indices are defined
            assert np.array_equal(t.numpy(), expect_keys(c, t.shape[2])), (who, c.name, name)


def check_case(lib, dev, c, mock_on=None):
    for e in entries_of(c):
        res = run_knn(lib, dev, c, e)
        check_knn(c, res, getattr(lib, "name", "hip"))
        if mock_on is not None:
            m = run_knn(MOCK, "cpu", c, e)
            for name, t in res.items():
                if name.endswith("idx") or c.grid == (0, 0):
                    assert torch.equal(t, m[name]), (c.name, name)


KNN_P = (16, 63, 64, 65, 133, 1000, 4608)


@functools.lru_cache(maxsize=None)
def shape_cases(P):
    out = []
    for K in (1, 5, 16):
        for nseg in (1, 2, 4):
            if not accepted(P, K, nseg):
                continue
            N = (1, 3, 9)[len(out) % 3]
            r = R.rng("shape", P, K, nseg)
            xyz, coords = cloud4(lattice(r, 2, P, 3)), lattice(r, N, 2, 3)
            for boxed in (False, True):
                out.append(kcase(f"P{P}K{K}n{nseg}N{N}{'b' if boxed else 'f'}", xyz, coords, K, nseg, boxed=boxed, gbox=boxed and P > 4096))
    assert P != 133 or any(c.K == 16 and c.nseg == 2 for c in out)
    return out


MODES = {"free": dict(P=1100, grid=(0, 0), boxed=False, nseg=2, gbox=False, straddle=576, N=9),
         "boxed": dict(P=1100, grid=(0, 0), boxed=True, nseg=2, gbox=False, straddle=576, N=3),
         "patch": dict(P=1152, grid=(24, 16), boxed=True, nseg=2, gbox=False, straddle=576, N=3),
         "group": dict(P=4608, grid=(72, 64), boxed=True, nseg=1, gbox=True, straddle=4096, N=3)}
ORDERS = ("desc", "asc", "same", "ties")
TIE_OFFSETS = np.array([[50, 0, 0], [-50, 0, 0], [0, 50, 0], [0, -50, 0], [0, 0, 50], [0, 0, -50], [30, 40, 0], [0, -30, 40], [40, 0, -30]])


def order_cloud(kind, P, K, q0, visit, straddle, r):
    """(P, 3) lattice cloud laid out along the visiting order ``visit`` as seen from the query q0."""
    pts = lattice(r, P, 3)
    if kind in ("desc", "asc"):
        d2 = ((pts.astype(np.int64) - q0.astype(np.int64)) ** 2).sum(1)
        o = np.argsort(d2, kind="stable")
        seq = pts[o[::-1] if kind == "desc" else o]
    elif kind == "same":
        seq = np.broadcast_to(pts[:1], (P, 3)).copy()
    else:  # 500 far ties; K-1 nearer points; a run of ties at the K-th distance over the tile / segment boundary at ``straddle``
        seq = q0 + np.where(np.abs(pts) < 100, 100, pts) * 0.6  # the rest: farther than the tie run on the first axis alone
        seq = np.trunc(seq).astype(np.float32)
        seq[:500] = q0 + [300, 0, 0]
        a = straddle - 40
        seq[a:a + K - 1] = q0 + np.stack([np.arange(1, K), np.zeros(K - 1), np.zeros(K - 1)], 1)
        n = straddle + 100 - (a + K - 1)
        seq[a + K - 1:straddle + 100] = q0 + TIE_OFFSETS[np.arange(n) % len(TIE_OFFSETS)]
    cloud = np.empty((P, 3), np.float32)
    cloud[visit] = seq
    assert np.abs(cloud).max() <= 1000
    return cloud


@functools.lru_cache(maxsize=None)
def order_case(kind, mode, K=16):
    m = MODES[mode]
    r = R.rng("order", kind, mode, K)
    P, N = m["P"], m["N"]
    coords = lattice(r, N, 2, 3)
    coords[0] = r.integers(-300, 301, (2, 3))
    visit = R.tile_points(P, m["grid"]).reshape(-1)
    visit = visit[visit < P]
    xyz = cloud4(np.stack([order_cloud(kind, P, K, coords[0, s], visit, m["straddle"], r) for s in range(2)]))
    return kcase(f"{kind}/{mode}", xyz, coords, K, m["nseg"], m["grid"], m["boxed"], m["gbox"])


def true_seed(cloud, q, K, high_ties=True):
    """The K nearest of each query, taking the HIGHEST indices of a tie at the K-th distance: the lower ones still have to win."""
    d2, fin = R.d2_int(cloud, q)
    d2 = np.where(fin[None], d2, R.BIG)
    out = np.empty((q.shape[0], K), np.int32)
    for n in range(q.shape[0]):
        kth = np.sort(d2[n])[K - 1]
        inner = np.flatnonzero(d2[n] < kth)
        tie = np.flatnonzero(d2[n] == kth)
        out[n] = np.concatenate([inner, tie[len(tie) - (K - len(inner)):] if high_ties else tie[:K - len(inner)]])
    return out


SEEDS = ("true", "far", "k64", "nan", "dims")


@functools.lru_cache(maxsize=None)
def seed_case(kind, K=16):
    base = order_case("ties", "patch" if kind == "dims" else "boxed", K)
    xyz, coords = base.xyz.copy(), base.coords
    N, S = coords.shape[:2]
    P = xyz.shape[1]
    r = R.rng("seed", kind, K)
    if kind == "nan":
        xyz[:, 700, :3] = NAN
    per = lambda f: np.stack([f(xyz[s], coords[:, s]) for s in range(S)], 1).astype(np.int32)
    dims = (0, 0, 0, 0)
    if kind in ("true", "nan"):
        seed = per(lambda c, q: true_seed(c, q, K))
        if kind == "nan":
            seed[:, :, K // 2] = 700
    elif kind == "far":
        seed = per(lambda c, q: np.argsort(np.where(R.d2_int(c, q)[1][None], R.d2_int(c, q)[0], -1), axis=1)[:, -K:])
    elif kind == "k64":
        seed = np.stack([r.permutation(P)[:64] for _ in range(N * S)]).reshape(N, S, 64).astype(np.int32)
    else:  # coarse (v, y, x) of a 12 x 8 grid per view -> fine (v, 2y, 2x) of the 24 x 16 grid
        seed = np.stack([r.permutation(3 * 12 * 8)[:K] for _ in range(N * S)]).reshape(N, S, K).astype(np.int32)
        dims = (12, 8, 24, 16)
    return kcase(f"seed-{kind}", xyz, coords, K, base.nseg, base.grid, True, False, seed=seed, seed_dims=dims)


@functools.lru_cache(maxsize=None)
def short_cases():
    """Fewer than K finite points in a frame (frame 0: 7 of them) and in a last segment (frame 1: 2 of its 5)."""
    r = R.rng("short")
    P, K = 133, 16
    xyz = cloud4(lattice(r, 2, P, 3))
    keep = np.array([2, 40, 70, 100, 129, 130, 132])
    dead = np.setdiff1d(np.arange(P), keep)
    xyz[0, dead, :3] = NAN
    xyz[0, 50, 0] = 17  # (one NaN coordinate is enough)
    xyz[1, [128, 130, 131], 1] = NAN
    coords = lattice(r, 3, 2, 3)
    return [kcase(f"short-{'b' if b else 'f'}", xyz, coords, K, 2, boxed=b) for b in (False, True)]


def all_knn_cases():
    out = [c for P in KNN_P for c in shape_cases(P)]
    out += [order_case(o, m) for o in ORDERS for m in MODES] + [seed_case(k) for k in SEEDS] + [seed_case("true", 5)] + short_cases()
    return out


@gpu
@pytest.mark.parametrize("P", KNN_P)
def test_knn_shapes(hip, P):
    for c in shape_cases(P):
        check_case(hip, DEV, c, mock_on=True)


@gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", ORDERS)
def test_knn_orders(hip, kind, mode):
    c = order_case(kind, mode)
    if kind == "same":
        assert np.array_equal(expect_idx(c), np.broadcast_to(np.arange(16, dtype=np.int32), expect_idx(c).shape))
    check_case(hip, DEV, c, mock_on=True)


@gpu
@pytest.mark.parametrize("kind,K", [(k, 16) for k in SEEDS] + [("true", 5)])
def test_knn_seeds(hip, kind, K):
    check_case(hip, DEV, seed_case(kind, K), mock_on=True)


@gpu
def test_knn_fewer_than_k_finite(hip):
    for c in short_cases():
        want = expect_idx(c)
        assert np.all(want[:, 0, 7:] == 132) and np.all(want[:, 0, :7] != 132 - 1) and len(set(want[0, 0, :7])) == 7
        check_case(hip, DEV, c, mock_on=True)


@gpu
def test_knn_refusals(hip):
    r = R.rng("refuse")
    dev = DEV
    xyz, coords = T_(cloud4(lattice(r, 1, 320, 3)), dev), T_(lattice(r, 2, 1, 3), dev)
    keys = torch.full((2 * 64 + 64,), SENT_K, dtype=torch.int64, device=dev)
    idx = torch.full((2 * 16 + 16,), SENT_I, dtype=torch.int32, device=dev)
    box = torch.zeros(1, 5, 8, device=dev)
    hip.tile_aabb(xyz, 320, 1, box)
    seed = torch.arange(8, dtype=torch.int32, device=dev).repeat(2)
    bad = [lambda: hip.knn_scan(xyz, 320, coords, 2, 1, 0, 1, 1, 16, 5, keys),  # nseg * K = 80
           lambda: hip.knn_scan(xyz, 12, coords, 2, 1, 0, 1, 1, 16, 1, keys),  # P < K
           lambda: hip.knn_search(xyz, 12, coords, 2, 1, 0, 1, 1, 16, idx, box),
           lambda: hip.knn_scan(xyz, 320, coords, 2, 1, 0, 1, 1, 4, 4, keys),  # 5 tiles in 4 segments: the last one empty
           lambda: hip.knn_scan_levels([dict(xyz=xyz, P=320, keys=keys, nseg=4)], coords, 2, 1, 0, 1, 1, 4),
           lambda: hip.knn_scan(xyz, 320, coords, 2, 1, 0, 1, 1, 4, 1, keys, box=box, grid=(20, 16)),  # grid no multiple of 8
           lambda: hip.tile_aabb(xyz, 320, 1, box, (20, 16)),
           lambda: hip.knn_search(xyz, 320, coords, 2, 1, 0, 1, 1, 4, idx, box, grid=(20, 16)),
           lambda: hip.knn_scan(xyz, 320, coords, 2, 1, 0, 1, 1, 16, 1, keys, seed_idx=seed, seed_k=8),  # seed_k < K
           lambda: hip.knn_search(xyz, 320, coords, 2, 1, 0, 1, 1, 16, idx, box, seed_idx=seed, seed_k=8),
           lambda: hip.knn_search_levels([dict(xyz=xyz, P=320, seed_idx=seed, box=box, idx_out=idx)], coords, 2, 1, 0, 1, 1, 16, 8)]
    for i, f in enumerate(bad):
        with pytest.raises(hip.HipError, match="arguments rejected"):
            f()
        assert i >= 0
    torch.cuda.synchronize()
    assert bool((keys == SENT_K).all()) and bool((idx == SENT_I).all())


@gpu
def test_linear_frames_refusals(hip):
    """A frame count T is the ring (0, T, 0, T-1): T = 0, frame0 = -1 and frame0 = T are refused by every slot-mapped wrapper
    (and by knn1_gather with frames=T) before anything is launched, on the cloud of test_knn_refusals; with T = 1, frame0 = 0
    the same calls are accepted."""
    r = R.rng("refuse")
    dev, P, N, K, Cc = DEV, 320, 2, 4, 32
    xyz, coords = T_(cloud4(lattice(r, 1, P, 3)), dev), T_(lattice(r, N, 1, 3), dev)
    fvec, tg = T_(small(r, 1, P, Cc), dev), T_(small(r, N, 1, Cc), dev)
    box = torch.zeros(1, 5, 8, device=dev)
    hip.tile_aabb(xyz, P, 1, box)
    nbr = torch.arange(N * K, dtype=torch.int32, device=dev)

    def calls(T, f0, keys, idx, out, feat):
        lv = [dict(xyz=xyz, P=P, keys=keys, nseg=1, box=box, idx_out=idx)]
        return [lambda: hip.knn_scan(xyz, P, coords, N, 1, f0, 1, T, K, 1, keys),
                lambda: hip.knn_search(xyz, P, coords, N, 1, f0, 1, T, K, idx, box),
                lambda: hip.knn_scan_levels(lv, coords, N, 1, f0, 1, T, K),
                lambda: hip.knn_search_levels(lv, coords, N, 1, f0, 1, T, K, 0),
                lambda: hip.corr_gather_dot([xyz], [fvec], [P], [nbr], Cc, tg, coords, N, 1, f0, 1, T, K, out, 4 * K, 0),
                lambda: hip.corr_gather_dot_opts([xyz], [fvec], [P], [nbr], Cc, tg, coords, N, 1, f0, 1, T, K, 1, True, False, out, 4 * K, 0),
                lambda: hip.knn1_gather(fvec, P, Cc, keys, N, 1, f0, feat, idx, frames=T)]

    def bufs():
        return (torch.full((N * K,), SENT_K, dtype=torch.int64, device=dev), torch.full((N * K,), SENT_I, dtype=torch.int32, device=dev),
                torch.full((N, 4 * K), NAN, device=dev), torch.full((N, Cc), NAN, device=dev))

    good = bufs()
    for f in calls(1, 0, *good):
        f()
    torch.cuda.synchronize()
    assert all(not bool(((b == SENT_K) | (b == SENT_I) | torch.isnan(b)).any()) for b in good)
    keys, idx, out, feat = bufs()
    for T, f0 in ((0, 0), (1, -1), (1, 1)):
        for i, f in enumerate(calls(T, f0, keys, idx, out, feat)):
            with pytest.raises(hip.HipError, match="arguments rejected"):
                f()
            assert i >= 0
    torch.cuda.synchronize()
    assert bool((keys == SENT_K).all()) and bool((idx == SENT_I).all()) and bool(torch.isnan(out).all()) and bool(torch.isnan(feat).all())


def test_knn_reference_is_the_oracle():
    """The lattice restatement picks the oracle's neighbours (knn_exact, and corr_sample's own search) on NaN-free cases."""
    for c in [shape_cases(133)[-1], order_case("ties", "boxed"), order_case("same", "patch"), order_case("desc", "free")]:
        want = expect_idx(c)
        for s in range(2):
            ref, q = torch.from_numpy(c.xyz[s, :, :3])[None], torch.from_numpy(c.coords[:, s])[None]
            _, idx = O.knn_exact(c.K, ref, q)
            assert np.array_equal(idx[0].numpy(), want[:, s]), c.name
            fv = torch.from_numpy(small(R.rng("of", c.name, s), 1, c.xyz.shape[1], 8))
            tg = torch.from_numpy(small(R.rng("ot", c.name, s), 1, q.shape[1], 8))
            out, idx2 = O.corr_sample(ref, fv, tg, q, k=c.K, return_idx=True)
            assert np.array_equal(idx2[0].numpy(), want[:, s]), c.name
            mine = R.ref_gather_dot(c.xyz[s:s + 1], fv.numpy(), want[:, s:s + 1], tg[0].numpy()[:, None], c.coords[:, s:s + 1], [0])
            assert np.allclose(out[0].numpy(), mine[:, 0], rtol=1e-6, atol=1e-6)


def test_knn_mock_is_the_rule():
    """The mocks give the restatement's keys and indices on every case of B (the GPU tests compare the kernels with both)."""
    for c in all_knn_cases():
        if c.xyz.shape[1] > 1200 and c.name[0] == "P" and c.K != 16:
            continue  # (the large shape once per nseg is enough on the CPU)
        for e in entries_of(c):
            check_knn(c, run_knn(MOCK, "cpu", c, e), "mock")


def test_probe_threshold_and_ties():
    # ('<' shows where the first threshold IS the K-th distance -- the seeded cases; an unseeded scan of <= 16 neighbours has its
    # ties' winners inside the first two tiles, before any threshold exists, so the tie orders are run for exactness only)
    seen = {"lt-seed": False, "lt-order": False, "tie_high": False}
    for c, tag in [(seed_case("true"), "lt-seed"), (seed_case("true", 5), "lt-seed"), (order_case("same", "patch"), "lt-order"),
                   (order_case("ties", "patch"), "lt-order")]:
        for s in range(2):
            cloud, q = c.xyz[c.slots[s]], c.coords[:, s]
            seed = None if c.seed is None else c.seed[:, s]
            want = R.ref_knn(cloud, q, c.K)
            assert np.array_equal(R.sim_scan(cloud, q, c.K, c.grid, seed), want)  # the restated scan is exact ...
            seen[tag] |= not np.array_equal(R.sim_scan(cloud, q, c.K, c.grid, seed, fault="lt"), want)  # ... and '<' is not
    for o in ORDERS:
        for m in MODES:
            c = order_case(o, m)
            diff = not np.array_equal(expect_idx(c, "tie_high"), expect_idx(c))
            assert diff or o in ("desc", "asc")
            seen["tie_high"] |= diff
    assert seen["lt-seed"] and seen["tie_high"], seen


def test_probe_segment_boundary():
    c = next(c for c in shape_cases(133) if c.K == 16 and c.nseg == 2)
    assert R.segments(133, 2) == [(0, 128), (128, 133)]
    assert not np.array_equal(expect_keys(c, 2, "seg_off"), expect_keys(c, 2))
    for c in (order_case("ties", "free"), short_cases()[0]):
        assert not np.array_equal(expect_keys(c, 2, "seg_off"), expect_keys(c, 2)), c.name


# ================================================================== C: the slot-to-frame map

CT, CS, CP, CN, CK, CC = 5, 8, 133, 3, 5, 64
LINEAR_FR = [(0, 1), (3, 1), (4, -1), (2, -1), (2, 0)]
RINGS = [(0, 4, 5, 8), (3, 4, 6, 8), (2, 4, 2, 2)]  # (base, R, lo, hi)


def frame_content(f):
    r = R.rng("frame", f)
    return cloud4(lattice(r, CP, 3)), small(r, CP, CC)


def ring_fr(ring):
    lo, hi = ring[2], ring[3]
    mid = (lo + hi) // 2
    return [(lo, 1), (hi, -1), (mid, 1), (mid, -1), (hi, 0)]


@functools.lru_cache(maxsize=None)
def map_case(kind, i, j, fault=None):
    """-> (knn case, fvec store (F, P, C)).  Linear: a store of CT frames; ring: R slots, the non-resident ones NaN."""
    r = R.rng("mapq", kind, i, j)
    coords = lattice(r, CN, CS, 3)
    if kind == "linear":
        fr = LINEAR_FR[j]
        xyz, fv = (np.stack(a) for a in zip(*[frame_content(f) for f in range(CT)]))
        slots = [R.frame_linear(fr[0], s, fr[1], CT, fault) for s in range(CS)]
        c = kcase(f"lin{fr}", xyz, coords, CK, 2, fr=fr, slots=slots)
    else:
        ring = RINGS[i]
        base, Rn, lo, hi = ring
        fr = ring_fr(ring)[j]
        xyz, fv = np.full((Rn, CP, 4), NAN, np.float32), np.full((Rn, CP, CC), NAN, np.float32)
        for f in range(lo, hi + 1):
            xyz[(f - base) % Rn], fv[(f - base) % Rn] = frame_content(f)
        slots = [R.slot_ring(fr[0], s, fr[1], ring, fault) for s in range(CS)]
        c = kcase(f"ring{ring}{fr}", xyz, coords, CK, 2, fr=fr, ring=ring, slots=slots)
    return c, fv


def map_cases():
    return [("linear", 0, j) for j in range(len(LINEAR_FR))] + [("ring", i, j) for i in range(len(RINGS)) for j in range(5)]


def run_gather(lib, dev, c, fv, idx, targets, opts=None, K=None, ldo=None, o_off=0, levels=1):
    """corr_gather_dot (opts None) or _opts (groups, add_offset, add_xyz) on ``levels`` copies of the case's store -> (rows, ldo)."""
    N, S = c.coords.shape[:2]
    K = K or idx.shape[2]
    P, Cc = fv.shape[1], fv.shape[2]
    OW = 4 if opts is None else opts[0] + 3 * opts[1] + 3 * opts[2]
    ldo = ldo or o_off + levels * K * OW
    out = torch.full((N * S + 1, ldo), NAN, device=dev)
    where, sfx = (c.ring, "_ring") if c.ring else (c.T, "")
    x, f, ix = T_(c.xyz, dev), (fv if isinstance(fv, torch.Tensor) else torch.from_numpy(fv)).to(dev), T_(idx, dev)
    args = ([x] * levels, [f] * levels, [P] * levels, [ix] * levels, Cc, T_(targets, dev), T_(c.coords, dev), N, S, c.fr[0], c.fr[1], where, K)
    if opts is None:
        getattr(lib, "corr_gather_dot" + sfx)(*args, out, ldo, o_off)
    else:
        getattr(lib, "corr_gather_dot_opts" + sfx)(*args, opts[0], bool(opts[1]), bool(opts[2]), out, ldo, o_off)
    assert bool(torch.isnan(out[N * S:]).all())
    return out[:N * S].cpu()


def map_gather_inputs(c):
    r = R.rng("mapg", c.name)
    return r.integers(0, CP, (CN, CS, CK)).astype(np.int32), small(r, CN, CS, CC)


def check_map_gather(lib, dev, c, fv):
    idx, tg = map_gather_inputs(c)
    res = []
    for opts in (None, (4, 1, 1)):  # (64 and 16 channels per dot: power-of-two divisors)
        got = run_gather(lib, dev, c, fv, idx, tg, opts)
        g, ao, ax = opts or (1, 1, 0)
        ref = R.ref_gather_dot(c.xyz, fv, idx, tg, c.coords, c.slots, g, bool(ao), bool(ax)).reshape(CN * CS, -1)
        assert exact_scale(CC // g)
        assert np.array_equal(got.numpy(), ref.astype(np.float32)), (c.name, opts)
        res.append(got)
    return res


def run_knn1(lib, dev, fv, keys, frame, ring=None, with_idx=True):
    n, nseg = keys.shape
    P, Cc = fv.shape[1], fv.shape[2]
    feat = torch.full((n + 1, Cc), NAN, device=dev)
    idx = torch.full((n + 1,), SENT_I, dtype=torch.int32, device=dev) if with_idx else None
    f = (fv if isinstance(fv, torch.Tensor) else torch.from_numpy(fv)).to(dev)
    io = None if idx is None else idx[:n]
    if ring:
        lib.knn1_gather_ring(f, P, Cc, T_(keys, dev), n, nseg, frame, ring, feat[:n], io)
    else:
        lib.knn1_gather(f, P, Cc, T_(keys, dev), n, nseg, frame, feat[:n], io)
    assert bool(torch.isnan(feat[n:]).all()) and (idx is None or int(idx[n]) == SENT_I)
    return feat[:n].cpu(), None if idx is None else idx[:n].cpu()


def ref_knn1(fv_slot, keys, P):
    idx = R.ref_merge(keys, 1, P)[:, 0]
    return fv_slot[idx].astype(np.float32), idx


def map_knn1_keys(c):
    r = R.rng("map1", c.name)
    return (r.integers(0, 1 << 24, (5, 3)).astype(np.float32).view(np.int32).astype(np.int64) << 32) | r.integers(0, CP, (5, 3))


def check_map_knn1(lib, dev, c, fv):
    keys = map_knn1_keys(c)
    out = []
    frames = range(c.ring[2], c.ring[3] + 1) if c.ring else range(CT)
    for f in frames:
        slot = (f - c.ring[0]) % c.ring[1] if c.ring else f
        feat, idx = run_knn1(lib, dev, fv, keys, f, c.ring)
        rf, ri = ref_knn1(fv[slot], keys, CP)
        assert np.array_equal(feat.numpy(), rf) and np.array_equal(idx.numpy(), ri), (c.name, f)
        out += [feat, idx]
    return out


@gpu
@pytest.mark.parametrize("kind,i,j", map_cases())
def test_slot_to_frame_map(hip, kind, i, j):
    c, fv = map_case(kind, i, j)
    check_case(hip, DEV, c, mock_on=True)
    for a, b in zip(check_map_gather(hip, DEV, c, fv) + check_map_knn1(hip, DEV, c, fv),
                    check_map_gather(MOCK, "cpu", c, fv) + check_map_knn1(MOCK, "cpu", c, fv)):
        assert torch.equal(a, b), c.name


@gpu
def test_ring_refuses_a_frame_that_is_not_resident(hip):
    for i, ring in enumerate(RINGS):
        c, fv = map_case("ring", i, 0)
        for f0 in (ring[2] - 1, ring[3] + 1):
            bad = KCase(**{**vars(c), "fr": (f0, 1)})
            idx, tg = map_gather_inputs(c)
            for e in ENTRIES:
                with pytest.raises(hip.HipError, match="arguments rejected"):
                    run_knn(hip, DEV, bad, e)
            for opts in (None, (1, 1, 0)):
                with pytest.raises(hip.HipError, match="arguments rejected"):
                    run_gather(hip, DEV, bad, fv, idx, tg, opts)
            if f0 >= 0:
                with pytest.raises(hip.HipError, match="arguments rejected"):
                    run_knn1(hip, DEV, fv, map_knn1_keys(c), f0, ring)
    c, fv = map_case("linear", 0, 0)
    for f0 in (-1, CT):
        with pytest.raises(hip.HipError, match="arguments rejected"):
            run_knn(hip, DEV, KCase(**{**vars(c), "fr": (f0, 1)}), "scan")


def test_slot_to_frame_mock_is_the_rule():
    for kind, i, j in map_cases():
        c, fv = map_case(kind, i, j)
        for e in ENTRIES:
            check_knn(c, run_knn(MOCK, "cpu", c, e), "mock")
        check_map_gather(MOCK, "cpu", c, fv)
        check_map_knn1(MOCK, "cpu", c, fv)


def test_probe_frame_map():
    def moved(kind, i, j, fault):
        c, _ = map_case(kind, i, j)
        f, _ = map_case(kind, i, j, fault)
        idx, tg = map_gather_inputs(c)
        fv = map_case(kind, i, j)[1]
        if f.slots == c.slots:
            return False
        a = R.ref_gather_dot(c.xyz, fv, idx, tg, c.coords, c.slots)
        b = R.ref_gather_dot(c.xyz, fv, idx, tg, c.coords, f.slots)
        assert not np.array_equal(expect_idx(f), expect_idx(c)) and not np.array_equal(a, b, equal_nan=True)  # distinct frames: both see it
        return True
    assert [moved("linear", 0, j, "no_lower_clamp") for j in range(5)] == [False, False, True, True, False]
    hit = [[moved("ring", i, j, "ring_no_base") for j in range(5)] for i in range(3)]
    assert not any(hit[0]) and all(hit[1]) and all(hit[2])  # base 0 cannot see it; the two others do in every case


# ================================================================== D: gather-dot with planted indices

DN, DS, DP = 5, 3, (133, 40, 17)


@functools.lru_cache(maxsize=None)
def gather_inputs(Cc, K):
    r = R.rng("gather", Cc, K)
    lv = []
    for l, P in enumerate(DP):
        idx = r.integers(0, P, (DN, DS, K)).astype(np.int32)
        flat = idx.reshape(-1)
        flat[[0, K, 2 * K, 3 * K]] = [0, P - 1, P, -1]  # P and -1 must read row P - 1
        flat[4 * K:4 * K + K] = flat[4 * K]  # a row of repeats
        lv.append((cloud4(lattice(r, 2, P, 3)), small(r, 2, P, Cc), idx))
    return lv, small(r, DN, DS, Cc), lattice(r, DN, DS, 3)


def run_gather_levels(lib, dev, Cc, K, bf, opts, ldo, o_off):
    lv, tg, coords = gather_inputs(Cc, K)
    dt = torch.bfloat16 if bf else torch.float32
    out = torch.full((DN * DS + 1, ldo), NAN, device=dev)
    args = ([T_(x, dev) for x, _, _ in lv], [T_(f, dev, dt) for _, f, _ in lv], list(DP), [T_(i, dev) for _, _, i in lv], Cc, T_(tg, dev),
            T_(coords, dev), DN, DS, 0, 1, 2, K)
    if opts is None:
        lib.corr_gather_dot(*args, out, ldo, o_off)
    else:
        lib.corr_gather_dot_opts(*args, opts[0], bool(opts[1]), bool(opts[2]), out, ldo, o_off)
    assert bool(torch.isnan(out[DN * DS:]).all())
    return out[:DN * DS].cpu()


def check_gather_levels(got, Cc, K, opts, o_off, who):
    lv, tg, coords = gather_inputs(Cc, K)
    g, ao, ax = opts or (1, 1, 0)
    OW = g + 3 * ao + 3 * ax
    used = len(DP) * K * OW
    a = got.numpy()
    assert np.isnan(a[:, :o_off]).all() and np.isnan(a[:, o_off + used:]).all(), who
    a = a[:, o_off:o_off + used].reshape(DN * DS, len(DP), K, OW)
    for l, (x, f, idx) in enumerate(lv):
        ref = R.ref_gather_dot(x, f, idx, tg, coords, [0, 1, 1], g, bool(ao), bool(ax)).reshape(DN * DS, K, OW)
        assert_values(a[:, l, :, :g], ref[..., :g], exact_scale(Cc // g), (who, l, "dots"))
        assert np.array_equal(a[:, l, :, g:], ref[..., g:].astype(np.float32)), (who, l, "offsets")


def close_to_mock(a, b, Cc, g, OW, o_off, K):
    """Kernel and mock outputs: equal where the divisor is a power of two and in every offset column, else both within the bar of the
    reference (checked by the callers), i.e. within two bars of each other."""
    if exact_scale(Cc // g):
        return torch.equal(torch.nan_to_num(a, nan=-77.0), torch.nan_to_num(b, nan=-77.0))
    x, y = a[:, o_off:o_off + len(DP) * K * OW].reshape(-1, OW).double(), b[:, o_off:o_off + len(DP) * K * OW].reshape(-1, OW).double()
    return torch.equal(x[:, g:], y[:, g:]) and bool(((x[:, :g] - y[:, :g]).abs() <= 2 * BAR * y[:, :g].abs()).all())


GATHER_SIZES = [(Cc, bf) for Cc in (32, 64, 128, 256) for bf in (0, 1)]


def gather_sweep(Cc, bf):
    lpr = Cc // (8 if bf else 4)
    for K in (1, 5, 16):
        used = len(DP) * K * 4
        yield K, None, used + 8, 4  # aligned (ldo, o_off): the 16-byte store
        yield K, None, used + 3, 1  # odd pair: the scalar stores
        for n, g in enumerate((1, 2, lpr)):
            for ao in (0, 1):
                for ax in (0, 1):
                    OW = g + 3 * ao + 3 * ax
                    yield K, (g, ao, ax), len(DP) * K * OW + 5, (2, 3)[(n + ao + ax) % 2]


@gpu
@pytest.mark.parametrize("Cc,bf", GATHER_SIZES)
def test_gather_dot_planted_indices(hip, Cc, bf):
    for K, opts, ldo, o_off in gather_sweep(Cc, bf):
        got = run_gather_levels(hip, DEV, Cc, K, bf, opts, ldo, o_off)
        check_gather_levels(got, Cc, K, opts, o_off, ("hip", Cc, bf, K, opts))
        m = run_gather_levels(MOCK, "cpu", Cc, K, bf, opts, ldo, o_off)
        g, ao, ax = opts or (1, 1, 0)
        assert close_to_mock(got, m, Cc, g, g + 3 * ao + 3 * ax, o_off, K), (Cc, bf, K, opts)


@gpu
def test_gather_dot_refuses_bad_groups(hip):
    for Cc, bf in GATHER_SIZES:
        lpr = Cc // (8 if bf else 4)
        for g in (2 * lpr, 3):
            with pytest.raises(hip.HipError, match="arguments rejected"):
                run_gather_levels(hip, DEV, Cc, 5, bf, (g, 1, 0), 3 * 5 * (g + 3) + 4, 0)


@pytest.mark.parametrize("Cc,bf", GATHER_SIZES)
def test_gather_dot_mock_is_the_rule(Cc, bf):
    for K, opts, ldo, o_off in gather_sweep(Cc, bf):
        check_gather_levels(run_gather_levels(MOCK, "cpu", Cc, K, bf, opts, ldo, o_off), Cc, K, opts, o_off, ("mock", Cc, bf, K, opts))


# ================================================================== E: the 1-NN gather

def knn1_inputs(Cc, nseg):
    r = R.rng("knn1", Cc, nseg)
    P, n = 133, 5
    fv = small(r, 3, P, Cc)
    keys = (r.integers(0, 1 << 24, (n, nseg)).astype(np.float32).view(np.int32).astype(np.int64) << 32) | r.integers(0, P, (n, nseg))
    keys[1, :] = keys[1, 0]  # every segment holds the same key
    keys[2, nseg // 2:] = R.KEY_MAX  # short segments
    keys[2, -1] = keys[2].view(np.uint64).min().view(np.int64)  # ... and a tie with the winner behind them
    keys[3, :] = R.KEY_MAX  # nothing finite anywhere: row P - 1
    keys[4, nseg - 1] = 7  # distance 0 in the last segment
    return fv, keys, P


@gpu
@pytest.mark.parametrize("bf", [0, 1])
@pytest.mark.parametrize("Cc", [4, 128, 384])
def test_knn1_gather(hip, Cc, bf):
    for nseg in (1, 3, 64):
        fv, keys, P = knn1_inputs(Cc, nseg)
        f = torch.from_numpy(fv).to(torch.bfloat16 if bf else torch.float32)
        rf, ri = ref_knn1(fv[2], keys, P)
        assert ri[3] == P - 1 and ri[4] == 7
        for with_idx in (True, False):
            feat, idx = run_knn1(hip, DEV, f, keys, 2, with_idx=with_idx)
            assert np.array_equal(feat.numpy(), rf) and (idx is None or np.array_equal(idx.numpy(), ri)), (Cc, bf, nseg, with_idx)
            mf, mi = run_knn1(MOCK, "cpu", f.float(), keys, 2, with_idx=with_idx)
            assert torch.equal(mf, feat) and (idx is None or torch.equal(mi, idx))


def test_knn1_mock_is_the_rule():
    for Cc in (4, 128, 384):
        for nseg in (1, 3, 64):
            fv, keys, P = knn1_inputs(Cc, nseg)
            feat, idx = run_knn1(MOCK, "cpu", fv, keys, 2)
            rf, ri = ref_knn1(fv[2], keys, P)
            assert np.array_equal(feat.numpy(), rf) and np.array_equal(idx.numpy(), ri)


# ================================================================== F: window correlation

WIN_SIZES = [(12, 20), (6, 10), (3, 5), (2, 3)]  # (h, w) per level: independent integer maps


def window_coords(r, h=12, w=20):
    return np.array([[7.25, 5.5], [3, 4], [13.75, 2.25], [-0.25, -0.25], [-(r + 1.25), 2], [5, -(r + 1.25)], [w - 1, h - 1], [w - 0.75, h - 0.75],
                     [w + r + 1, 3], [4.5, h + r + 1], [1e6, 3], [2, -1e6], [-1e6, 1e6]], np.float32)


@functools.lru_cache(maxsize=None)
def window_inputs(Cc, r, BS=2):
    g = R.rng("window", Cc)
    maps = [small(g, BS, h, w, Cc) for h, w in WIN_SIZES]
    c = window_coords(r)
    coords = np.concatenate([c, c[::-1]])[:BS * len(c)] if BS == 2 else np.tile(c, (BS, 1))
    return maps, small(R.rng("wt", Cc, r), coords.shape[0], Cc), coords, len(c)


def run_window(lib, dev, maps, tg, coords, N, r, levels_entry, bf=False, ldo_pad=3, o_off=2):
    """Per-level launches of window_corr, or the one launch of window_corr_levels -> (rows, levels, win^2) cpu."""
    BS, Cc, L = maps[0].shape[0], maps[0].shape[3], len(maps)
    ww = (2 * r + 1) ** 2
    ldo = o_off + L * ww + ldo_pad
    rows = BS * N
    out = torch.full((rows + 1, ldo), NAN, device=dev)
    fm = [T_(m, dev, torch.bfloat16 if bf else torch.float32) for m in maps]
    t, c = T_(tg, dev), T_(coords, dev)
    if levels_entry:
        lib.window_corr_levels(fm, t, c, out, BS, N, Cc, r, ldo, o_off)
    else:
        for l, m in enumerate(fm):
            lib.window_corr(m, t, c, out, BS, N, Cc, m.shape[1], m.shape[2], l, r, ldo, o_off + l * ww)
    o = out.cpu()
    assert bool(torch.isnan(o[rows:]).all() and torch.isnan(o[:rows, :o_off]).all() and torch.isnan(o[:rows, o_off + L * ww:]).all())
    return o[:rows, o_off:o_off + L * ww].reshape(rows, L, ww)


def ref_window_levels(maps, tg, coords, N, r, fault=None):
    return np.stack([R.ref_window(m, tg, coords, N, l, r, fault) for l, m in enumerate(maps)], 1)


@gpu
@pytest.mark.parametrize("r", range(1, 8))
def test_window_corr_radii(hip, r):
    for Cc in (32, 64, 128, 256):
        maps, tg, coords, N = window_inputs(Cc, r)
        ref = ref_window_levels(maps, tg, coords, N, r)
        far = np.abs(coords).max(1) >= 1e6
        assert far.any() and not ref[far].any() and ref[~far].any((1, 2)).sum() >= 6  # +-1e6 is all zeros; so are the windows wholly outside
        per = run_window(hip, DEV, maps, tg, coords, N, r, False)
        assert_values(per.numpy(), ref, exact_scale(Cc), ("window_corr", Cc, r))
        lev = run_window(hip, DEV, maps, tg, coords, N, r, True)
        assert torch.equal(lev, per), (Cc, r)  # the fp32 levels launch is the per-level launches bit for bit
        assert_values(run_window(hip, DEV, maps, tg, coords, N, r, True, bf=True).numpy(), ref, exact_scale(Cc), ("bf16 levels", Cc, r))
        mock = run_window(MOCK, "cpu", maps, tg, coords, N, r, False)
        if exact_scale(Cc):
            assert torch.equal(mock, per)
        else:
            assert_values(mock.numpy(), ref, False, ("mock", Cc, r))


PERM_SHAPES = [(8, 4), (8, 8), (12, 8), (10, 16), (20, 8), (16, 4), (12, 4), (9, 8)]


@functools.lru_cache(maxsize=None)
def perm_inputs(BS, N):
    g = R.rng("perm", BS, N)
    maps = [small(g, BS, h, w, 32) for h, w in WIN_SIZES[1:3]]
    # every row its own window on the 6 x 10 map, within a pixel of it: most hang over the border, none is wholly outside
    coords = (np.stack([g.integers(-4, 41, BS * N), g.integers(-4, 25, BS * N)], 1) * 0.25).astype(np.float32)
    return maps, small(g, BS * N, 32), coords


@gpu
@pytest.mark.parametrize("BS,N", PERM_SHAPES)
def test_window_corr_workgroup_permutation(hip, BS, N):
    maps, tg, coords = perm_inputs(BS, N)
    ref = ref_window_levels(maps, tg, coords, N, 1)
    assert (np.abs(ref).sum((1, 2)) > 0).all() and len({r.tobytes() for r in ref}) == BS * N  # every row is its own, none is zero
    lev = run_window(hip, DEV, maps, tg, coords, N, 1, True)
    assert_values(lev.numpy(), ref, False, ("perm", BS, N))  # every row, no sampling
    assert torch.equal(lev, run_window(hip, DEV, maps, tg, coords, N, 1, False))
    assert_values(run_window(hip, DEV, maps, tg, coords, N, 1, True, bf=True).numpy(), ref, False, ("perm bf16", BS, N))


def test_window_reference_is_the_oracle():
    for Cc, r in [(32, 1), (64, 3), (32, 7)]:
        maps, tg, coords, N = window_inputs(Cc, r)
        near = np.abs(coords).max(1) < 1e6  # (grid_sample's normalised coordinate loses the pixel at 1e6; the zero there is asserted above)
        BS = 2
        # (the oracle in fp64: in fp32 its normalised grid coordinate alone moves a radius-7 sample by more than the 1e-5 asked here)
        pyr = [torch.from_numpy(m).double().permute(0, 3, 1, 2)[None] for m in maps]
        t = torch.from_numpy(tg).double().reshape(1, BS, N, Cc)
        c = torch.from_numpy(coords).double().reshape(1, BS, N, 2)
        want = O.window_corr_sample(pyr, t, c, radius=r).reshape(BS * N, len(maps), -1).numpy()
        mine = ref_window_levels(maps, tg, coords, N, r)
        assert np.abs(want - mine)[near].max() <= 1e-5, (Cc, r)


def test_window_mock_is_the_rule():
    for Cc, r in [(32, 1), (64, 2), (128, 5), (256, 7)]:
        maps, tg, coords, N = window_inputs(Cc, r)
        assert_values(run_window(MOCK, "cpu", maps, tg, coords, N, r, False).numpy(), ref_window_levels(maps, tg, coords, N, r), exact_scale(Cc),
                      ("mock", Cc, r))


def test_probe_window_faults():
    for r in range(1, 8):
        maps, tg, coords, N = window_inputs(32, r)
        ref = ref_window_levels(maps, tg, coords, N, r)
        for fault in ("drop_last_row", "swap_axes"):
            assert not np.array_equal(ref_window_levels(maps, tg, coords, N, r, fault), ref), (r, fault)


def test_probe_workgroup_permutation():
    branches = []
    for BS, N in PERM_SHAPES:
        maps, tg, coords = perm_inputs(BS, N)
        ref = ref_window_levels(maps, tg, coords, N, 1)
        order, branch = R.wg_order(BS, N)
        branches.append(branch)
        assert np.array_equal(np.sort(order), np.arange(len(order)))  # the rule as written visits every workgroup once
        bad, _ = R.wg_order(BS, N, fault="perm_dup")
        out = np.full_like(ref, NAN)
        for wg in bad:
            out[4 * wg:4 * wg + 4] = ref[4 * wg:4 * wg + 4]
        assert np.array_equal(out, ref, equal_nan=True) == (branch == "row"), (BS, N)  # a folded permutation leaves rows unwritten
    assert branches == ["whole", "whole", "leftover", "leftover", "leftover", "whole", "row", "row"]
