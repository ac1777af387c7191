"""Cloud preparation on the device against the fp64 restatement tests/cloud_prep_ref.py (numpy + cKDTree; brute force for the exact
cases).  Open3D is installed neither here nor with the reference's tests, so the restatement of its rules is the yardstick
(tests/test_cloud_prep_host.py shows that it meets the end-to-end condition on its own).

1. Neighbour lists on dyadic clouds (coordinates in multiples of 1/4: every fp32 d2 exact, ties everywhere): nbr_idx and nbr_cnt equal
   to the brute-force search with the (d2, index) rule, on point lists and organised clouds, max_nn 3 / 30 / 64, the radius at a
   lattice distance (strict), one float above it, and +inf; fewer points than max_nn, NaN rows, a cloud of NaNs, a shuffled copy.
2. Covariance: bit-equal on the dyadic clouds, within 1e-12 trace on rendered ones.
3. Normals: integer-slope planes within 1e-6; the eigen-residual within 4e-7 lambda_max (rounding a unit vector to fp32 moves it by
   at most sqrt(3) 2^-24 = 1.03e-7; the bar is four times that) and lambda = n^T C n / n^T n within 1e-9 lambda_max of eigh's smallest
   (the quotient, since the fp32 normal is a unit vector only to 1.2e-7: see check_normal_rows), where the gap
   lambda_mid - lambda_min is at least 1e-2 lambda_max; NaN rows exactly where n < 3 or the neighbours are collinear; the viewpoint.
4. Rendered clouds: every point's neighbour set equals the restatement's up to members tied (1e-6 relative) with its last kept d2 or r^2.
5. Voxels: exact on dyadic clouds (faces, duplicates, NaN rows, one point), membership and means on rendered ones, the range bit.
6. Determinism.  7. End to end.  Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_align_cases as Cs  # noqa: E402
import camera_align_ref as A  # noqa: E402
import cloud_prep_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
INF = float("inf")
LATTICE = 0.5  # a distance between lattice points of the dyadic clouds: r^2 = 1/4 is a d2 many pairs have exactly
RADII = (LATTICE, float(np.nextafter(np.float32(LATTICE), np.float32(1))), INF)
NNS = (3, 30, 64)
# name -> (H, W, organised): point lists of 40, 448 (7 tiles: beyond the +-2 ring) and 8 320 points (130 tiles, 3 groups), shuffled so
# that neighbours lie in far tiles; organised 24 x 40 (beyond the 3 x 3 ring) and 72 x 80 (90 tiles, 2 groups)
CLOUDS = {"list40": (5, 8, False), "list448": (16, 28, False), "list8320": (80, 104, False), "grid24x40": (24, 40, True), "grid72x80": (72, 80, True)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sync_np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def device_estimate(cloud, grid, radius, max_nn, viewpoint=None):
    """One cloud (P, 4) float32 through mvt_tile_aabb -> mvt_tile_group_aabb -> mvt_normals_estimate with every diagnostic output."""
    from mvtracker_amd import cloud as C
    vp = None if viewpoint is None else dev(np.asarray([viewpoint], np.float32))
    nrm, idx, cnt, cov = C.normals_of_clouds(dev(cloud)[None].contiguous(), 1, len(cloud), grid, radius, max_nn, viewpoint=vp, details=True)
    return dict(nrm=sync_np(nrm)[0], idx=sync_np(idx)[0], cnt=sync_np(cnt)[0], cov=sync_np(cov)[0])


_cache = {}


def dyadic(name):
    """(cloud (P, 4) float32, grid, the brute-force lists at max_nn 64 without a radius), computed once."""
    if name not in _cache:
        H, W, organised = CLOUDS[name]
        pts, _ = Cs.dyadic_target(H, W, seed=3)
        if not organised:
            pts = pts[np.random.default_rng(H * W).permutation(len(pts))]
        cloud = Cs.linear(pts)
        _cache[name] = (cloud, (W, H) if organised else (0, 0), R.neighbours_brute(cloud, INF, R.MAX_NN))
    return _cache[name]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def check_normal_rows(tag, cloud, got, cov_ref, cnt_ref, nan_exact=True):
    """Section 3's general checks of the normals of one run against C from the restatement."""
    n = got["nrm"][:, :3].astype(np.float64)
    ref, eig = R.normals_of(cloud, cov_ref, cnt_ref)
    nan_g, nan_r = np.isnan(n[:, 0]), np.isnan(ref[:, 0])
    assert (got["nrm"][:, 3] == 0).all() and np.isnan(n[nan_g]).all()
    both = ~nan_g & ~nan_r
    gap = both & (eig[:, 1] - eig[:, 0] >= 1e-2 * eig[:, 2])
    unit = np.abs(np.linalg.norm(n[~nan_g], axis=1) - 1).max() if (~nan_g).any() else 0.0
    res = lam_over = lam_plain = sign = 0.0
    if gap.any():
        # lambda is the Rayleigh quotient n^T C n / n^T n.  The plain product n^T C n carries the fp32 rounding of the LENGTH of n
        # (1 +- 1.2e-7) times lambda_min: the exact eigenvector rounded to fp32 already measures 2.9e-9 lambda_max that way on
        # list40, where lambda_min is 3 % of lambda_max, and 1.4e-15 as the quotient.  The length has its own bar (1e-6).
        Cm = R.sym(cov_ref[gap])
        Cn = np.einsum("pij,pj->pi", Cm, n[gap])
        lam = (n[gap] * Cn).sum(1) / (n[gap] * n[gap]).sum(1)
        res = (np.linalg.norm(Cn - lam[:, None] * n[gap], axis=1) / eig[gap, 2]).max()
        lam_over = ((lam - eig[gap, 0]) / eig[gap, 2]).max()
        lam_plain = (((n[gap] * Cn).sum(1) - eig[gap, 0]) / eig[gap, 2]).max()
        sign = (1 - np.abs((n[gap] * ref[gap]).sum(1))).max()
    print(f"{tag}: {int((~nan_g).sum())} normals (ref {int((~nan_r).sum())}), NaN mask differs at {int((nan_g != nan_r).sum())}, {int(gap.sum())} with a "
          f"gap >= 1e-2: max |Cn - lambda n| / lambda_max {res:.2e}, max (lambda - lambda_min) / lambda_max {lam_over:.2e} "
          f"(n^T C n without the division by n^T n: {lam_plain:.2e}), max 1 - |n . n_ref| {sign:.2e}, max | |n| - 1 | {unit:.2e}")
    assert res <= 4e-7 and lam_over <= 1e-9 and unit <= 1e-6 and sign <= 1e-6
    if nan_exact:
        assert np.array_equal(nan_g, nan_r)
    return ref


# ------------------------------------------------------------------------------------------------------------------ 1 / 2 / 3. dyadic clouds
@pytest.mark.parametrize("name", list(CLOUDS))
def test_neighbour_lists_covariance_and_normals_are_exact_on_dyadic_clouds(name):
    cloud, grid, (idx64, cnt64, d264) = dyadic(name)
    valid = R.valid_rows(cloud)
    assert (~valid).any() and (name != "list40" or valid.sum() < 64)  # planted NaN rows; a cloud with fewer points than max_nn
    for max_nn in NNS:
        for radius in RADII:
            got = device_estimate(cloud, grid, radius, max_nn)
            idx, cnt = R.cut(idx64, cnt64, d264, max_nn, radius)
            cov = R.covariance(cloud, idx, cnt)
            bad_i, bad_c = int((got["idx"] != idx).any(1).sum()), int((got["cnt"] != cnt).sum())
            cov_ok = same_bits(got["cov"], cov) or np.array_equal(got["cov"][valid], cov[valid])  # (NaN rows: any NaN)
            print(f"{name} max_nn {max_nn} radius {radius!r}: {int(valid.sum())} of {len(cloud)} points, counts {cnt[valid].min()}..{cnt.max()}, "
                  f"lists differ at {bad_i}, counts at {bad_c}, covariance bit-equal {cov_ok}")
            assert bad_i == 0 and bad_c == 0 and cov_ok and np.isnan(got["cov"][~valid]).all() and (got["cnt"][~valid] == -1).all()
            check_normal_rows(f"{name} max_nn {max_nn} radius {radius!r}", cloud, got, cov, cnt)
    # the strict test: the shell at exactly r^2 = 1/4 is excluded at r = 1/2 and included one float above
    at, above = R.cut(idx64, cnt64, d264, 64, RADII[0])[1], R.cut(idx64, cnt64, d264, 64, RADII[1])[1]
    assert (above > at).any()


def test_a_cloud_of_nans_and_a_shuffled_copy():
    cloud = np.full((200, 4), np.nan, np.float32)
    cloud[:, 3] = 0
    got = device_estimate(cloud, (0, 0), 1.0, 30)
    assert (got["cnt"] == -1).all() and (got["idx"] == -1).all() and np.isnan(got["nrm"][:, :3]).all() and np.isnan(got["cov"]).all()
    # a shuffled copy: the same neighbour SETS after unshuffling, where the radius alone cuts the lists (no tie at a max_nn-th place)
    base, _, _ = dyadic("list448")
    perm = np.random.default_rng(9).permutation(len(base))
    a, b = device_estimate(base, (0, 0), 0.75, 64), device_estimate(base[perm], (0, 0), 0.75, 64)
    print(f"shuffled copy: counts {a['cnt'].max()} at most of 64")
    assert a["cnt"].max() < 64 and np.array_equal(b["cnt"], a["cnt"][perm])
    for i in range(len(base)):
        mine = b["idx"][i][b["idx"][i] >= 0]
        assert set(perm[mine].tolist()) == set(a["idx"][perm[i]][a["idx"][perm[i]] >= 0].tolist())


def test_planes_of_integer_slope():
    ys, xs = np.meshgrid(np.arange(24) / 4.0, np.arange(40) / 4.0, indexing="ij")
    for (sa, sb) in ((0, 0), (1, 0), (-2, 3), (5, -4)):
        pts = np.stack([xs, ys, sa * xs + sb * ys], -1).reshape(-1, 3).astype(np.float32)
        true = np.array([-sa, -sb, 1.0]) / np.sqrt(sa * sa + sb * sb + 1.0)
        got = device_estimate(Cs.linear(pts), (40, 24), INF, 30)
        n = got["nrm"][:, :3].astype(np.float64)
        err, unit = np.abs(np.abs(n @ true) - 1).max(), np.abs(np.linalg.norm(n, axis=1) - 1).max()
        print(f"plane z = {sa} x + {sb} y: max | |n . n_true| - 1 | {err:.2e}, max | |n| - 1 | {unit:.2e}")
        assert err <= 1e-6 and unit <= 1e-6


def test_nan_rows_where_there_are_too_few_or_collinear_neighbours_and_the_viewpoint():
    base, _ = Cs.dyadic_target(8, 16, seed=1)
    extra = np.array([[100, 0, 0], [100.25, 0, 0], [100.5, 0, 0],      # an exactly collinear triple
                      [0, 200, 0], [0.25, 200.25, 0.5], [0.5, 200.5, 1],  # another, along a diagonal
                      [0, 0, 300],                                       # an isolated point: n = 1
                      [300, 300, 0], [300.25, 300, 0]], np.float32)       # a pair: n = 2
    cloud = Cs.linear(np.concatenate([base, extra]))
    P0 = len(base)
    r = R.estimate(cloud, 2.0, 30, brute=True)
    vp = (1.0, -2.0, 50.0)
    got, got_vp = device_estimate(cloud, (0, 0), 2.0, 30), device_estimate(cloud, (0, 0), 2.0, 30, viewpoint=vp)
    print(f"planted rows: counts {got['cnt'][P0:].tolist()}, NaN {np.isnan(got['nrm'][P0:, 0]).tolist()}")
    assert np.array_equal(got["idx"], r["idx"]) and got["cnt"][P0:].tolist() == [3, 3, 3, 3, 3, 3, 1, 2, 2]
    assert np.isnan(got["nrm"][P0:, 0]).all() and np.array_equal(np.isnan(got["nrm"][:, 0]), np.isnan(r["nrm"][:, 0]))
    check_normal_rows("planted", cloud, got, r["cov"], r["cnt"])
    ok = ~np.isnan(got["nrm"][:, 0])
    n, nv = got["nrm"][ok, :3].astype(np.float64), got_vp["nrm"][ok, :3].astype(np.float64)
    dots = (nv * (np.asarray(vp, np.float32).astype(np.float64) - cloud[ok, :3].astype(np.float64))).sum(1)
    flipped = (nv != n).any(1).sum()
    print(f"viewpoint: min n . (vp - p) {dots.min():.3e}, {int(flipped)} of {int(ok.sum())} normals flipped")
    assert (dots >= 0).all() and np.array_equal(np.abs(nv), np.abs(n)) and np.array_equal(np.isnan(got_vp["nrm"]), np.isnan(got["nrm"]))
    # towards a viewpoint on the other side every normal is the opposite one
    other = device_estimate(cloud, (0, 0), 2.0, 30, viewpoint=(1.0, -2.0, -50.0))["nrm"][ok, :3]
    assert np.array_equal(other, -got_vp["nrm"][ok, :3])


# ------------------------------------------------------------------------------------------------------------------ 4. rendered clouds
@pytest.fixture(scope="module")
def planted():
    sc = Cs.scene(4, 48, 64)
    G = Cs.rigid(**Cs.PLANTED)
    ex = Cs.perturbed(sc["extrs"], 1, G)
    true = Cs.unproject(sc["depths"], sc["intrs"], sc["extrs"])
    moved = Cs.unproject(sc["depths"], sc["intrs"], ex)
    return dict(sc, extrs_bad=ex, G=G, true=true, moved=moved, d={k: dev(v) for k, v in dict(sc, extrs=ex).items()})


@pytest.fixture(scope="module")
def rendered(planted):
    """The four organised 48 x 64 clouds of frame 0, float32."""
    clouds, grid = Cs.organised_clouds(planted["moved"][:, [0]])
    return [c[0] for c in clouds], grid


@pytest.mark.parametrize("radius,max_nn", [(0.3, 30), (0.1, 64)])
def test_rendered_neighbour_sets_covariance_and_normals(rendered, radius, max_nn):
    clouds, grid = rendered
    r2 = R.radius_sq(radius)
    for v, cloud in enumerate(clouds):
        got = device_estimate(cloud, grid, radius, max_nn)
        idx, cnt, d2 = R.neighbours_tree(cloud, radius, max_nn)
        p = cloud[:, :3].astype(np.float64)
        differ = np.flatnonzero((np.sort(got["idx"], 1) != np.sort(idx, 1)).any(1))
        outside = 0
        for i in differ:
            a, b = set(got["idx"][i][got["idx"][i] >= 0].tolist()), set(idx[i][idx[i] >= 0].tolist())
            last = d2[i, cnt[i] - 1] if cnt[i] > 0 else r2
            for j in a ^ b:
                dj = ((p[j] - p[i]) ** 2).sum()
                if not (abs(dj - last) <= 1e-6 * last or abs(dj - r2) <= 1e-6 * r2):
                    outside += 1
        valid = R.valid_rows(cloud)
        cov = R.covariance(cloud, got["idx"], got["cnt"])  # the device's own lists
        tr = cov[valid][:, [0, 3, 5]].sum(1)
        ecov = (np.abs(got["cov"][valid] - cov[valid]).max(1) / np.where(tr > 0, tr, 1)).max()
        print(f"view {v} radius {radius} max_nn {max_nn}: {int(valid.sum())} points, sets differ at {len(differ)} ({100 * len(differ) / valid.sum():.2f} %), "
              f"{outside} members outside the ties, counts differ at {int((got['cnt'] != cnt).sum())} beyond them, max |cov - fp64| / trace {ecov:.2e}")
        assert outside == 0 and (got["cnt"][~valid] == -1).all() and ecov <= 1e-12
        assert np.array_equal(got["cnt"][np.setdiff1d(np.arange(len(cloud)), differ)], cnt[np.setdiff1d(np.arange(len(cloud)), differ)])
        # (a NaN row may differ where lambda_mid sits at the threshold; none does on these surfaces)
        check_normal_rows(f"view {v}", cloud, got, cov, got["cnt"])


# ------------------------------------------------------------------------------------------------------------------ 5. voxels
def device_voxel(pts, voxel_size):
    from mvtracker_amd import voxel_downsample
    p, c, f, lab = voxel_downsample(dev(np.asarray(pts, np.float32)), voxel_size, return_labels=True)
    return dict(points=sync_np(p), counts=sync_np(c), first=sync_np(f), labels=sync_np(lab))


@pytest.mark.parametrize("name", ["one", "list40", "list448", "list8320"])
def test_voxels_are_exact_on_dyadic_clouds(name):
    if name == "one":
        pts = np.array([[0.25, -1.5, 3.0]], np.float32)
    else:
        base = dyadic(name)[0][:, :3]
        pts = np.concatenate([base, base[::7], base[5:6].repeat(4, 0)])  # duplicates, NaN rows among them
    for voxel_size in (0.5, 2.0):
        r = R.voxel(pts, voxel_size)
        got = device_voxel(pts, voxel_size)
        u = (pts[R.valid_rows(pts)].astype(np.float64) - r["origin"]) / voxel_size
        on_face = int((u == np.floor(u)).any(1).sum())
        print(f"{name} voxel {voxel_size}: {len(pts)} points ({int(R.valid_rows(pts).sum())} taking part, {on_face} on a cell face) -> "
              f"{len(got['counts'])} voxels (ref {len(r['counts'])}), largest {int(got['counts'].max())}")
        assert got["points"].dtype == np.float32 and got["points"].shape == (len(r["counts"]), 3)
        assert np.array_equal(got["counts"], r["counts"]) and np.array_equal(got["first"], r["first"]) and np.array_equal(got["labels"], r["labels"])
        assert np.array_equal(got["points"].view(np.uint32), r["points"].view(np.uint32)) and (np.diff(got["first"]) > 0).all()
        assert np.abs(got["points"] - r["mean64"]).max() <= 2.0 ** -20  # (and the mean of the members it is)
        assert name == "one" or (on_face > 0 and got["counts"].max() > 1)


@pytest.mark.parametrize("P,nb", [(65700, 257), (179000, 700)])
def test_voxels_of_more_than_256_workgroups(P, nb):
    """More than 65 536 points: every thread of mvt_voxel_emit's one-workgroup scan owns a chunk of 2 (257 workgroups) or 3 (700: the
    last chunk partial) counts.  A dyadic cloud (multiples of 1/8) in a box that grows in steps with the index, so that cells are
    repeated many times and first points of new voxels still appear in late workgroups, with whole workgroups between them that emit
    nothing."""
    assert (P + 255) // 256 == nb
    rng = np.random.default_rng(P)
    limit = 16 + 4 * ((np.arange(P) * 8) // P)  # coordinates below 2, 2.5, .. 5.5 (in eighths): the box grows by a cell eight times
    pts = (np.floor(rng.random((P, 3)) * limit[:, None]) / 8.0).astype(np.float32)
    pts[::1001] = np.nan  # rows that take no part
    r, got = R.voxel(pts, 0.5), device_voxel(pts, 0.5)
    per = np.bincount(r["first"] // 256, minlength=nb)
    print(f"{P} points, {nb} workgroups -> {len(got['counts'])} voxels (ref {len(r['counts'])}), largest {int(r['counts'].max())}, "
          f"{int((per == 0).sum())} workgroups emit nothing, the last one that emits: {int(np.flatnonzero(per)[-1])}")
    assert got["points"].shape == (len(r["counts"]), 3) and len(r["counts"]) > 1000  # n_out
    assert np.array_equal(got["counts"], r["counts"]) and np.array_equal(got["first"], r["first"]) and np.array_equal(got["labels"], r["labels"])
    assert np.array_equal(got["points"].view(np.uint32), r["points"].view(np.uint32))
    assert r["counts"].max() > 20 and (per == 0).sum() > 10 and np.flatnonzero(per)[-1] > nb // 2 and (np.diff(per.nonzero()[0]) > 1).any()


@pytest.mark.parametrize("voxel_size", [0.05, 0.2])
def test_voxels_on_a_rendered_cloud(planted, voxel_size):
    pts = planted["moved"][:, 0].reshape(-1, 3).astype(np.float32)
    r, got = R.voxel(pts, voxel_size), device_voxel(pts, voxel_size)
    assert np.array_equal(got["labels"], r["labels"]) and np.array_equal(got["counts"], r["counts"]) and np.array_equal(got["first"], r["first"])
    bar = 0.5 * np.spacing(np.abs(r["mean64"]).astype(np.float32)).astype(np.float64) + 2.0 ** -30 * voxel_size
    err = np.abs(got["points"].astype(np.float64) - r["mean64"])
    print(f"voxel {voxel_size}: {len(r['counts'])} voxels, membership equal, max |mean - fp64 mean| / bar {(err / bar).max():.3f}, "
          f"bits equal to the restatement's fixed-point mean: {np.array_equal(got['points'].view(np.uint32), r['points'].view(np.uint32))}")
    assert (err <= bar).all()


def test_a_cloud_spanning_more_than_2_to_the_21_cells_sets_the_range_bit():
    from mvtracker_amd import hip, voxel_downsample
    pts = np.zeros((70, 4), np.float32)
    pts[:, 0] = np.arange(70)
    pts[69, 0] = 2.0 ** 21 + 5  # cell 2^21 + 5 at voxel 1
    xyz = dev(pts)
    cap = hip.voxel_capacity(70)
    state = torch.zeros(hip.VOXEL_STATE_WORDS, dtype=torch.int64, device=DEV)
    partial = torch.empty(hip.VOXEL_BOUND_BLOCKS * 4, dtype=torch.float64, device=DEV)
    table = torch.empty(cap * hip.VOXEL_SLOT_WORDS, dtype=torch.int64, device=DEV)
    out, counts, first, labels = (torch.full((70, 4), -7.0, device=DEV), torch.full((70,), -7, dtype=torch.int32, device=DEV),
                                  torch.full((70,), -7, dtype=torch.int32, device=DEV), torch.full((70,), -7, dtype=torch.int32, device=DEV))
    n_out = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    hip.voxel_bounds(xyz, 70, 1.0, partial, state)
    hip.voxel_insert(xyz, 70, state, table, cap)
    hip.voxel_emit(xyz, 70, state, table, cap, torch.empty(1, dtype=torch.int32, device=DEV), out, counts, first, n_out, labels)
    st = sync_np(state)
    print(f"status {st[hip.VOXEL_STATUS]}, points {st[hip.VOXEL_POINTS]}, n_out {int(n_out[0])}")
    assert st[hip.VOXEL_STATUS] == hip.VOXEL_RANGE and st[hip.VOXEL_POINTS] == 70 and int(n_out[0]) == 0
    assert (sync_np(out) == -7).all() and (sync_np(counts) == -7).all() and (sync_np(labels) == -1).all()
    assert st.view(np.float64)[:4].tolist() == [-0.5, -0.5, -0.5, 1.0]
    with pytest.raises(ValueError, match="too small"):
        voxel_downsample(xyz[:, :3].contiguous(), 1.0)
    p, c, f = voxel_downsample(xyz[:69, :3].contiguous(), 1.0)  # without the far point: one voxel per point
    assert p.shape == (69, 3) and sync_np(c).tolist() == [1] * 69 and sync_np(f).tolist() == list(range(69))


# ------------------------------------------------------------------------------------------------------------------ 6. determinism
def test_two_runs_give_equal_bits(rendered):
    clouds, grid = rendered
    a, b = device_estimate(clouds[1], grid, 0.3, 30), device_estimate(clouds[1], grid, 0.3, 30)
    assert all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)
    pts = np.concatenate([c[:, :3] for c in clouds])
    a, b = device_voxel(pts, 0.2), device_voxel(pts, 0.2)
    assert all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a) and a["counts"].max() > 20


# ------------------------------------------------------------------------------------------------------------------ 7. end to end
@pytest.mark.parametrize("frames", [(0,), (0, 1)])
def test_end_to_end_with_pca_normals(planted, frames):
    from mvtracker_amd import PcaCameraAlignment, align, align_cameras
    d = planted["d"]
    a = PcaCameraAlignment(max_distance=0.05, normal_radius=0.3, frames=frames)
    c = align_cameras(d["depths"], d["intrs"], d["extrs"], a)
    D = sync_np(c.transforms)
    xyz0 = sync_np(align.ClipAlignment(d["depths"][0], d["intrs"][0], d["extrs"][0], a).xyz0)
    ref = R.align_views_pca([[xyz0[v, f] for f in range(xyz0.shape[1])] for v in range(4)], 64, 48, 0.05, 0.3, 30, 30, 2)
    before = Cs.displacement(np.eye(4), planted["moved"][1], planted["true"][1])
    left = Cs.displacement(D[1], planted["moved"][1], planted["true"][1])
    left_ref = Cs.displacement(ref["D"][1], planted["moved"][1], planted["true"][1])
    print(f"frames {frames}: planted {1e3 * before:.2f} mm, left by the device {1e3 * left:.3f} mm, by the restatement {1e3 * left_ref:.3f} mm "
          f"(ratio {left / left_ref:.3f}); max |D_device - D_restatement| {np.abs(D - ref['D']).max():.2e}; iterations {c.iterations.tolist()} "
          f"(ref {ref['iterations'].tolist()}), status {c.status.tolist()}")
    assert left <= before / 10 and left <= 1.5 * left_ref
    assert np.array_equal(D[0], np.eye(4)) and c.status.tolist() == [0, 0, 0, 0] and (D[:, 3] == [0, 0, 0, 1]).all()


def bowl(step):
    """The analytic bowl of the existing list test, sampled every ``step``: points (n, 3) float32."""
    xs, ys = np.arange(-5, 5, step), np.arange(-3, 3, step)
    xy = np.stack(np.meshgrid(xs, ys, indexing="xy"), -1).reshape(-1, 2)
    return np.concatenate([xy, (0.05 * (xy ** 2).sum(1) + 0.3 * np.sin(xy[:, 0]))[:, None]], 1).astype(np.float32)


def test_align_point_clouds_estimates_the_normals_and_takes_a_downsampled_target():
    from mvtracker_amd import align_point_clouds, estimate_normals, voxel_downsample
    # the dense target: four points around every point of the list test's target, (+-1/32, +-1/32) aside at its height, so that a
    # voxel of 1/4 holds exactly those four and their mean is that point.  (A bowl resampled on another lattice is no such test: it
    # constrains sliding so weakly that the restatement itself ends 1e-2 from the planted motion on it.)
    pts = bowl(0.25)
    dense = (pts[:, None, :] + np.array([[-1, -1, 0], [1, -1, 0], [-1, 1, 0], [1, 1, 0]], np.float32) / 32).reshape(-1, 3)
    G = Cs.rigid(0.4, (0.2, 1.0, -0.3), (0.01, -0.015, 0.02))
    src = dev(((pts.astype(np.float64) - G[:3, 3]) @ G[:3, :3]).astype(np.float32))
    t = dev(pts)
    T1, f1, r1 = align_point_clouds(src, t, None, 0.2, 20, normal_radius=0.6, normal_max_nn=30)
    T2, f2, r2 = align_point_clouds(src, t, estimate_normals(t, 0.6, 30), 0.2, 20)
    print(f"normals estimated on the way: max |T - planted| {np.abs(sync_np(T1) - G).max():.2e}, fitness {f1:.4f}, rmse {r1:.3e}")
    assert torch.equal(T1, T2) and (f1, r1) == (f2, r2) and np.abs(sync_np(T1) - G).max() < 2e-3
    small, counts, _ = voxel_downsample(dev(dense), 0.25)
    T3, f3, r3 = align_point_clouds(src, small, None, 0.2, 20, normal_radius=0.6, normal_max_nn=30)
    print(f"target of {len(dense)} points downsampled to {small.shape[0]} voxels (up to {int(counts.max())} points each): "
          f"max |T - planted| {np.abs(sync_np(T3) - G).max():.2e}, fitness {f3:.4f}, rmse {r3:.3e}")
    assert small.shape[0] == len(pts) and sync_np(counts).tolist() == [4] * len(pts) and np.abs(sync_np(small) - pts).max() <= 2.0 ** -20
    assert np.abs(sync_np(T3) - G).max() < 2e-3 and f3 > 0.9
