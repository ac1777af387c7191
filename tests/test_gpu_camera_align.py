"""Camera alignment on the device against the fp64 restatement tests/camera_align_ref.py (numpy + cKDTree; brute force for the exact
cases).  No recorded output of the reference exists for this feature: its ICP calls Open3D, which is installed neither here nor with
the reference's tests, so the restatement of Open3D's rules is the yardstick (tests/test_camera_align_host.py shows that it meets the
end-to-end condition on its own and that near ties are rare on the teacher-forced scene).

1. Normals: valid mask equal, normals within 1e-6 of fp64; max_edge at and just below a neighbour distance.
2. Correspondences on dyadic clouds (every fp32 d2 exact): indices equal to a brute-force fp64 search, planted ties across patches and
   clouds, the strict cap, no match; mvt_align_transform's bits.
3. Normal equations: all 30 sums equal on the dyadic clouds (every product and sum exact); on rendered clouds within
   1e-9 sqrt(A_ii A_jj) (fp64 sums of fewer than 1e5 terms).
4. Solve: x within 1e-10 of numpy.linalg.solve; T(x) = Rz Ry Rx | t on planted single-axis cases.
5. One iteration at a time, each from the device's own D.  6. End to end, one perturbed view (two at once: the restatement itself
   does not meet the condition with sweeps=2, see tests/test_camera_align_host.py).  7. Determinism and the done flag.  8. Wiring.
Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_align_cases as Cs  # noqa: E402
import camera_align_ref as R  # noqa: E402
from mvtracker_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N_TOL, A_TOL, X_TOL, NEAR_FRAC = 1e-6, 1e-9, 1e-10, 0.005


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sync_np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ 1. normals
def device_normals(cloud, grid, max_edge):
    from mvtracker_amd import hip
    xyz = dev(cloud)[None].contiguous()
    nrm = torch.empty_like(xyz)
    hip.align_normals(xyz, 1, grid, max_edge, nrm)
    return sync_np(nrm)[0]


def check_normals(tag, cloud, grid, max_edge, expect_valid=None):
    got = device_normals(cloud, grid, max_edge)
    ref = R.normals(cloud, grid[0], grid[1], max_edge)
    ok_g, ok_r = ~np.isnan(got[:, 0]), ~np.isnan(ref[:, 0])
    err = np.abs(got[ok_r & ok_g, :3].astype(np.float64) - ref[ok_r & ok_g]).max() if (ok_r & ok_g).any() else 0.0
    unit = np.abs(np.linalg.norm(got[ok_g, :3].astype(np.float64), axis=1) - 1).max() if ok_g.any() else 0.0
    print(f"{tag}: {int(ok_g.sum())} valid (ref {int(ok_r.sum())}) of {len(cloud)}, mask differs at {int((ok_g != ok_r).sum())}, "
          f"max |n - ref| {err:.2e}, max | |n| - 1 | {unit:.2e}")
    assert np.array_equal(ok_g, ok_r) and err <= N_TOL and unit <= N_TOL
    assert np.isnan(got[~ok_g, :3]).all() and (got[:, 3] == 0).all()
    assert expect_valid is None or int(ok_g.sum()) == expect_valid
    return got


@pytest.mark.parametrize("hw", [(8, 8), (9, 17), (24, 40)])
def test_normals_on_lattices(hw):
    H, W = hw
    row, col = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for sx, sy in ((0, 0), (2, -1), (-3, 1)):  # integer-slope planes z = sx x + sy y: every interior pixel has the same normal
        pts = np.stack([col / 4.0, row / 4.0, sx * col / 4.0 + sy * row / 4.0], -1).reshape(-1, 3).astype(np.float32)
        cloud, grid, _ = organised(pts, H, W)
        got = check_normals(f"{H}x{W} plane {sx},{sy}", cloud, grid, 4.0, expect_valid=(H - 2) * (W - 2))
        n = np.array([-sx, -sy, 1.0]) / np.sqrt(sx * sx + sy * sy + 1.0)
        ok = ~np.isnan(got[:, 0])
        assert np.abs(np.abs(got[ok, :3] @ n) - 1).max() <= N_TOL  # (the orientation is left as it falls)
    pts, _ = Cs.dyadic_target(H, W)  # a bumpy raster with planted NaN rows
    cloud, grid, _ = organised(pts, H, W)
    for me in (4.0, 0.75, 0.5):  # (dyadic coordinates: every d2 is exact, so the fp32 and the fp64 edge tests agree)
        check_normals(f"{H}x{W} bumpy max_edge {me}", cloud, grid, me)


def organised(pts, H, W):
    Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
    out = np.full((Hp, Wp, 4), np.nan, np.float32)
    out[..., 3] = 0
    out[:H, :W, :3] = pts.reshape(H, W, 3)
    idx = (np.arange(H)[:, None] * Wp + np.arange(W)[None, :]).reshape(-1)
    return out.reshape(-1, 4), (Wp, Hp), idx


def test_normals_max_edge_at_and_just_below_a_neighbour_distance():
    H, W = 16, 24
    row, col = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    pts = np.stack([col / 4.0, row / 4.0, np.zeros_like(col, dtype=np.float64)], -1).reshape(-1, 3).astype(np.float32)
    cloud, grid, _ = organised(pts, H, W)
    check_normals("max_edge = the neighbour distance", cloud, grid, 0.25, expect_valid=(H - 2) * (W - 2))
    below = float(np.nextafter(np.float32(0.25), np.float32(0)))
    check_normals("max_edge one float below it", cloud, grid, below, expect_valid=0)
    pts[5 * W + 7, 2] = 0.25  # one raised point: its four neighbours lose their normal at max_edge 0.25, and so does it
    cloud, grid, _ = organised(pts, H, W)
    check_normals("one raised point", cloud, grid, 0.25, expect_valid=(H - 2) * (W - 2) - 5)
    from mvtracker_amd import hip
    x = dev(cloud)[None].contiguous()
    for kw in (dict(grid=(20, 16)), dict(me=0.0), dict(me=float("inf"))):
        with pytest.raises(hip.HipError, match="arguments rejected"):
            hip.align_normals(x, 1, kw.get("grid", grid), kw.get("me", 1.0), torch.empty_like(x))


# ------------------------------------------------------------------------------------------------------------------ 2 / 3. dyadic clouds
TH, TW = 24, 40


def dyadic_targets(n):
    """n target clouds on the same x, y lattice with different heights: (points (P,3), normals (P,3)) float32, axis-aligned normals."""
    return [Cs.dyadic_target(TH, TW, seed=k, axis_normals=True) for k in range(n)]


def device_targets(tg, organised_layout, organised_grid=(TW, TH)):
    from mvtracker_amd import align
    out = []
    for pts, nrm in tg:
        P = len(pts)
        grid = organised_grid if organised_layout else (0, 0)
        xyz, nn = dev(Cs.linear(pts))[None].contiguous(), dev(Cs.linear(nrm))[None].contiguous()
        nt = (P + 63) // 64
        box, gbox = torch.empty(1, nt, 8, device=DEV), torch.empty(1, (nt + 63) // 64, 8, device=DEV)
        align.build_search(xyz, 1, P, grid, box, gbox)
        out.append(dict(xyz=xyz, nrm=nn, box=box, gbox=gbox, P=P, grid=grid))
    return out


def run_once(src, src_grid, stride, targets, cap, D=None, max_iterations=3):
    from mvtracker_amd import align
    D = align._eye_rows(1, DEV)[0] if D is None else D
    run = align.IcpRun(dev(Cs.linear(src))[None].contiguous(), len(src), src_grid, 1, targets, cap, stride, D, max_iterations, keep_queries=True)
    run.step()
    torch.cuda.synchronize()
    return run


def check_exact(tag, src, src_grid, stride, tg, organised_layout, cap=0.5):
    from mvtracker_amd import align
    run = run_once(src, src_grid, stride, device_targets(tg, organised_layout), cap)
    slots = align.query_slots(len(src), src_grid, stride).numpy()
    q = np.full((len(slots), 3), np.nan, np.float32)
    q[slots >= 0] = src[slots[slots >= 0]]
    union = R.target_union(tg)
    ref = R.correspond(q, union, R.cap_squared(cap), brute=True)
    idx, d2 = run.q_idx.cpu().numpy()[0], run.q_d2.cpu().numpy()[0]
    hit = ref["idx"] >= 0
    sums_ref = R.normal_equations(q, ref, union)
    sums = run.sums.cpu().numpy()
    rows = run.partial.cpu().numpy()[0]
    print(f"{tag}: {int((slots >= 0).sum())} queries in {len(slots) // 64} tiles, {int(hit.sum())} matched (device {int((idx >= 0).sum())}), "
          f"indices differ at {int((idx != ref['idx']).sum())}, d2 differs at {int((d2[hit] != ref['d2'][hit]).sum())}, "
          f"sums differ at {int((sums != sums_ref).sum())} of 30")
    assert np.array_equal(idx, ref["idx"]) and np.array_equal(d2[hit].astype(np.float64), ref["d2"][hit]) and np.isnan(d2[~hit]).all()
    assert np.array_equal(sums, sums_ref) and np.array_equal(rows.sum(0), sums_ref) and sums[27] == hit.sum() > 0
    for t in range(len(rows)):  # every tile's row on its own
        sl = slice(64 * t, 64 * t + 64)
        assert np.array_equal(rows[t], R.normal_equations(q[sl], {k: v[sl] for k, v in ref.items()}, union))
    return run, ref


@pytest.mark.parametrize("n_targets,organised_layout", [(1, False), (3, True), (3, False)])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 4097])
def test_correspondences_and_sums_are_exact_on_point_lists(count, n_targets, organised_layout):
    tg = dyadic_targets(n_targets)
    src = Cs.dyadic_source(tg[0][0], count)
    for k in range(1, n_targets):  # every n-th query sits next to a point of cloud k
        src[k::n_targets] = Cs.dyadic_source(tg[k][0], count, seed=k)[k::n_targets]
    if count >= 64:
        src[5] = np.nan  # a query that takes no part
    _, ref = check_exact(f"list of {count} vs {n_targets} {'organised' if organised_layout else 'list'} target(s)", src, (0, 0), 1, tg, organised_layout)
    if n_targets == 3 and count == 4097:  # the three clouds all serve, and some queries fall to a neighbour of their own point
        P = TH * TW
        assert all(((ref["idx"] >= k * P) & (ref["idx"] < (k + 1) * P)).sum() > 50 for k in range(3))


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("n_targets", [1, 3])
def test_correspondences_and_sums_are_exact_on_an_organised_source(n_targets, stride):
    tg = dyadic_targets(n_targets)
    src = (tg[-1][0] + np.asarray(Cs.SHIFT, np.float32)).astype(np.float32)  # the last target's raster, shifted
    check_exact(f"organised {TH}x{TW} stride {stride} vs {n_targets} target(s)", src, (TW, TH), stride, tg, True)


def test_ties_go_to_the_lower_cloud_and_index_across_patches():
    """Planted exact ties.  Tiles of an organised cloud are 8x8 patches, so the patch visited second holds lower raster indices than
    some of the first: a candidate there at exactly the query's best d2 sits ON the face of its tile's box (box distance == d2) and
    must still be seen.  Target: 8 x 16 pixels at (col / 4, row / 4, 0); pixels (0, 6) and (0, 7) are missing.  The query
    (1.75, 0, 0) is 1/4 from pixel (1, 7) = index 23 in patch 0 and from pixel (0, 8) = index 8 in patch 1: the answer is 8.
    Further queries tie between two rows of one patch, between patches with the lower index in the first one, and three ways."""
    gw, gh = 16, 8
    row, col = np.meshgrid(np.arange(gh), np.arange(gw), indexing="ij")
    pts = np.stack([col / 4.0, row / 4.0, np.zeros_like(col, dtype=np.float64)], -1).reshape(-1, 3).astype(np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (gw * gh, 1))
    pts[[6, 7]] = np.nan
    pts[3 * gw + 8] = np.nan  # pixel (3, 8): its four neighbours tie, two in each patch
    src = np.array([[1.75, 0.0, 0.0], [2.0, 0.75, 0.0], [0.625, 0.5, 0.0], [1.875, 1.0, 0.0], [1.875, 1.125, 0.0]], np.float32)
    want_first = [8, 2 * gw + 8, 2 * gw + 2, 4 * gw + 7, 4 * gw + 7]
    for n_clouds, layout in ((1, True), (1, False), (2, True), (2, False)):  # two identical clouds: every tie also ties across clouds
        tg = [(pts, nrm)] * n_clouds
        run = run_once(src, (0, 0), 1, device_targets(tg, layout, (gw, gh)), 0.5)
        union = R.target_union(tg)
        ref = R.correspond(src, union, R.cap_squared(0.5), brute=True)  # (stable sort: the lowest global index of the nearest)
        idx, d2 = run.q_idx.cpu().numpy()[0, :len(src)], run.q_d2.cpu().numpy()[0, :len(src)]
        print(f"{n_clouds} cloud(s), {'organised' if layout else 'list'}: indices {idx.tolist()} (brute force {ref['idx'].tolist()}), d2 {d2.tolist()}")
        assert ref["idx"].tolist() == want_first and idx.tolist() == want_first and np.array_equal(d2.astype(np.float64), ref["d2"])
        assert np.array_equal(run.sums.cpu().numpy(), R.normal_equations(src, ref, union))
    # the tie at pixel (3, 8) really has members in both patches, and the reviewer's case really is a tie
    d = ((pts[None, :, :].astype(np.float64) - src[:, None, :]) ** 2).sum(-1)
    ties = [np.flatnonzero(d[i] == np.nanmin(d[i])).tolist() for i in range(len(src))]
    assert ties[0] == [8, 23] and ties[1] == [2 * gw + 8, 3 * gw + 7, 3 * gw + 9, 4 * gw + 8] and len(ties[3]) == 2


def test_transform_rounds_once_and_keeps_nan_rows():
    from mvtracker_amd import hip
    rng = np.random.default_rng(8)
    n = 1000
    for tag, D, pts, exact in (
            ("dyadic", np.array([[0.5, -0.25, 1.0, 3 / 16], [2.0, 0.125, -0.5, -1 / 16], [-1.0, 0.75, 0.25, 5.0]]),
             rng.integers(-200, 200, (n, 3)) / 32.0, True),
            ("rigid", Cs.rigid(17.0, (0.3, -0.5, 0.8), (0.03, -0.02, 0.025))[:3], rng.uniform(-6, 6, (n, 3)), False)):
        x0 = np.zeros((n, 4), np.float32)
        x0[:, :3] = pts
        x0[:, 3] = 7.0  # (.w of the input is ignored, the output's is 0)
        x0[5, 1] = np.nan
        x0[9, :3] = np.nan
        x0[11, 0] = np.inf
        out = torch.full((n + 1, 4), 3.0, device=DEV)
        hip.align_transform(dev(x0), dev(D.reshape(-1)), n, out)
        got = sync_np(out)
        want = R.transform(D, x0)
        ok = np.isfinite(want[:, 0])
        ulp = np.abs(got[:n, :3][ok].view(np.int32).astype(np.int64) - want[ok].view(np.int32).astype(np.int64)).max()
        print(f"{tag}: {int(ok.sum())} finite rows, max difference from the fp64 product rounded once {ulp} ulp, NaN rows {int((~ok).sum())}")
        assert ulp <= (0 if exact else 1) and (~ok).sum() == 3 and np.isnan(got[:n, :3][~ok]).all()  # (a row with one NaN is NaN throughout)
        assert (got[:n, 3] == 0).all() and (got[n] == 3.0).all()  # (nothing past n rows is written)
    assert (np.abs(got[:n, :3][ok].astype(np.float64) - (x0[ok, :3].astype(np.float64) @ D[:, :3].T + D[:, 3])) <= 2.4e-7 * 8).all()


def test_the_cap_is_strict_and_no_match_sets_the_status_bit():
    from mvtracker_amd import hip
    pts = np.full((64, 3), np.nan, np.float32)
    nrm = np.full((64, 3), np.nan, np.float32)
    pts[9], nrm[9] = (0, 0, 0), (0, 0, 1)
    pts[10], nrm[10] = (0, 0.25, 0), (np.nan, np.nan, np.nan)  # nearer, but without a normal: takes no part
    src = np.array([[0.5, 0.0, 0.0], [0.0, 0.375, 0.0]], np.float32)  # d2 = 0.25 and 0.140625 to point 9
    at = run_once(src, (0, 0), 1, device_targets([(pts, nrm)], False), 0.5)  # cap2 = 0.25 exactly
    above = float(np.nextafter(np.float32(0.5), np.float32(1)))
    over = run_once(src, (0, 0), 1, device_targets([(pts, nrm)], False), above)
    i_at, i_over = at.q_idx.cpu().numpy()[0, :2], over.q_idx.cpu().numpy()[0, :2]
    print(f"d2 == cap2: index {i_at[0]}; cap one float above: index {i_over[0]} (d2 {over.q_d2.cpu().numpy()[0, 0]}); the other query: {i_at[1]}")
    assert i_at.tolist() == [-1, 9] and i_over.tolist() == [9, 9] and float(over.q_d2[0, 0]) == 0.25
    # nothing within the cap: count 0, the status bit, D as it was, and the run is over
    far = run_once(src + 100, (0, 0), 1, device_targets([(pts, nrm)], False), 0.5)
    D0 = far.D.clone()
    ist, hist = far.istate.cpu().numpy(), far.hist.cpu().numpy()
    print(f"no match: istate {ist.tolist()}, count {hist[0, 0]}, result {far.result.cpu().tolist()}")
    assert ist.tolist() == [1, 0, hip.ALIGN_FEW, 1] and hist[0, 0] == 0 and (far.q_idx.cpu().numpy()[0] == -1).all()
    assert far.result.cpu().tolist() == [0.0, 0.0, 0.0, float(hip.ALIGN_FEW)]
    far.step()
    torch.cuda.synchronize()
    assert torch.equal(far.D, D0) and far.istate.cpu().numpy().tolist() == [1, 0, hip.ALIGN_FEW, 1]
    tg = device_targets([(pts, nrm)], False)
    for kw in (dict(cap2=0.0), dict(stride=2), dict(targets=[])):
        with pytest.raises(hip.HipError):
            hip.align_correspond(at.src0, 2, (0, 0), kw.get("stride", 1), 1, at.D, kw.get("cap2", 0.25), kw.get("targets", tg), at.istate, at.partial)


# ------------------------------------------------------------------------------------------------------------------ 4. solve
def solve_rows(rows, D0, n_queries=100.0, final=False):
    from mvtracker_amd import align, hip
    partial = dev(np.asarray(rows, np.float64))
    D = align._rows12(dev(D0))
    ist = torch.zeros(4, dtype=torch.int32, device=DEV)
    hist = torch.zeros(2, hip.ALIGN_HIST, dtype=torch.float64, device=DEV)
    res, sums = torch.zeros(4, dtype=torch.float64, device=DEV), torch.zeros(30, dtype=torch.float64, device=DEV)
    hip.align_solve(partial, len(rows), dev(np.array([n_queries])), final, D, ist, hist, res, sums)
    torch.cuda.synchronize()
    return D.cpu().numpy().reshape(3, 4), ist.cpu().numpy(), hist.cpu().numpy(), res.cpu().numpy(), sums.cpu().numpy()


def test_solve_transform_convention_and_pivots():
    from mvtracker_amd import hip
    eye_row = np.zeros(30)
    eye_row[[0, 6, 11, 15, 18, 20]] = 1.0  # J^T J = I
    eye_row[27], eye_row[29] = 10.0, 10 * 0.01 ** 2
    D0 = Cs.rigid(25.0, (0.2, -0.4, 1.0), (0.3, 0.1, -0.2))
    for x in ([0.3, 0, 0, 0, 0, 0], [0, 0.3, 0, 0, 0, 0], [0, 0, 0.3, 0, 0, 0], [0.2, -0.5, 0.7, 0.1, -0.2, 0.3]):
        row = eye_row.copy()
        row[21:27] = -np.asarray(x)
        D, ist, hist, res, _ = solve_rows([row], D0)
        want = R.transform_of(np.asarray(x, np.float64)) @ D0
        print(f"x {x}: max |D - T(x) D0| {np.abs(D - want[:3]).max():.2e}, x error {np.abs(hist[0, 4:] - x).max():.2e}")
        assert np.abs(D - want[:3]).max() <= 1e-14 and np.abs(hist[0, 4:] - x).max() <= 1e-15
        assert ist.tolist() == [0, 1, 0, 1] and res[0] == 0.1 and abs(res[1] - np.sqrt(eye_row[29] / 10.0)) <= 1e-15 and res[2:].tolist() == [1.0, 0.0]
        assert hist[0, 0] == 10.0 and np.array_equal(hist[0, 1:3], res[:2]) and hist[0, 3] == 0.0
        # Rx alone turns y towards z, Ry z towards x, Rz x towards y (right-handed): the convention, not only the restatement's copy of it
    for axis, (a, b) in enumerate(((1, 2), (2, 0), (0, 1))):
        row = eye_row.copy()
        row[21 + axis] = -0.3
        D = solve_rows([row], np.eye(4))[0]
        assert abs(D[b, a] - np.sin(0.3)) <= 1e-15 and abs(D[a, b] + np.sin(0.3)) <= 1e-15 and abs(D[axis, axis] - 1) <= 1e-15
    # a dense system, cut over many rows: the sums and x
    rng = np.random.default_rng(2)
    J = rng.standard_normal((500, 6)) * np.array([2.0, 3.0, 1.0, 1.0, 1.0, 0.5])
    r = rng.standard_normal(500) * 0.01
    A, b = J.T @ J, J.T @ r
    full = np.concatenate([A[np.triu_indices(6)], b, [500.0, (r * r).sum(), 0.3]])
    w = rng.uniform(size=(37, 1))
    rows = (w / w.sum()) * full
    D, ist, hist, res, sums = solve_rows(rows, np.eye(4), n_queries=1000.0)
    A_dev, b_dev = R.unpack(sums)
    x_np = np.linalg.solve(A_dev, -b_dev)
    rel = np.linalg.norm(hist[0, 4:] - x_np) / np.linalg.norm(x_np)
    print(f"dense: sums rel error {np.abs(sums / full - 1).max():.2e}, x rel error against numpy.linalg.solve {rel:.2e}")
    assert np.abs(sums / full - 1).max() <= 1e-13 and rel <= X_TOL and ist.tolist() == [0, 1, 0, 1]
    # final call: the figures, no update; fewer than 6 correspondences; a singular system
    D, ist, hist, res, _ = solve_rows(rows, D0, final=True)
    assert np.array_equal(D, D0[:3]) and ist.tolist() == [0, 0, 0, 1] and abs(res[0] - sums[27] / 100.0) <= 1e-12
    few = eye_row.copy()
    few[27] = 5.0
    D, ist, _, _, _ = solve_rows([few], D0)
    assert np.array_equal(D, D0[:3]) and ist.tolist() == [1, 0, hip.ALIGN_FEW, 1]
    sing = eye_row.copy()
    sing[20] = 1e-13  # the last pivot <= 1e-12 x the largest diagonal
    D, ist, _, _, _ = solve_rows([sing], D0)
    assert np.array_equal(D, D0[:3]) and ist.tolist() == [1, 0, hip.ALIGN_SINGULAR, 1]


# ------------------------------------------------------------------------------------------------------------------ 5 / 6. the rendered scene
@pytest.fixture(scope="module")
def planted():
    sc = Cs.scene(4, 48, 64)
    G = Cs.rigid(**Cs.PLANTED)
    ex = Cs.perturbed(sc["extrs"], 1, G)
    true = Cs.unproject(sc["depths"], sc["intrs"], sc["extrs"])
    moved = Cs.unproject(sc["depths"], sc["intrs"], ex)
    return dict(sc, extrs_bad=ex, G=G, true=true, moved=moved, d={k: dev(v) for k, v in dict(sc, extrs=ex).items()})


def alignment(**kw):
    from mvtracker_amd import CameraAlignment
    return CameraAlignment(**dict(dict(max_distance=0.05, normal_max_edge=Cs.NORMAL_MAX_EDGE), **kw))


def test_rendered_points_and_normals(planted):
    from mvtracker_amd import align
    d = planted["d"]
    st = align.ClipAlignment(d["depths"][0], d["intrs"][0], d["extrs"][0], alignment(frames=(0, 1)))
    xyz, nrm = sync_np(st.xyz), sync_np(st.nrm)
    assert xyz.shape == (4, 2, 48 * 64, 4) and np.array_equal(xyz[:, 0].view(np.uint32), xyz[:, 1].view(np.uint32))  # (the scene is static)
    valid = np.isfinite(xyz[..., 0])
    want = planted["moved"].reshape(4, 2, -1, 3)
    err = np.abs(xyz[..., :3][valid] - want[valid]).max()
    print(f"{int(valid.sum())} valid points, max |device point - fp64 unprojection| {err:.2e}")
    assert np.array_equal(valid, np.isfinite(want[..., 0])) and err < 5e-6
    for v in range(4):
        ref = R.normals(xyz[v, 0], 64, 48, Cs.NORMAL_MAX_EDGE)
        ok_g, ok_r = ~np.isnan(nrm[v, 0, :, 0]), ~np.isnan(ref[:, 0])
        both = ok_g & ok_r
        e = np.abs(nrm[v, 0][both, :3] - ref[both]).max()
        print(f"view {v}: {int(ok_g.sum())} normals (ref {int(ok_r.sum())}), max |n - ref| {e:.2e}")
        # (rendered distances are not dyadic: a neighbour within one fp32 rounding of max_edge may fall either way; none does here)
        assert np.array_equal(ok_g, ok_r) and e <= N_TOL and ok_g.sum() > 1500


def test_normal_max_edge_defaults_to_max_distance(planted):
    from mvtracker_amd import CameraAlignment, align
    d = planted["d"]
    a, b = (align.ClipAlignment(d["depths"][0], d["intrs"][0], d["extrs"][0], x)
            for x in (CameraAlignment(max_distance=0.3), CameraAlignment(max_distance=0.3, normal_max_edge=0.3)))
    na, nb, none = sync_np(a.nrm), sync_np(b.nrm), sync_np(align.ClipAlignment(d["depths"][0], d["intrs"][0], d["extrs"][0], CameraAlignment()).nrm)
    print(f"normals with max_distance 0.3 and the default edge: {int(np.isfinite(na[..., 0]).sum())}; with the defaults (5 cm) at this size: "
          f"{int(np.isfinite(none[..., 0]).sum())}")
    assert np.array_equal(na.view(np.uint32), nb.view(np.uint32)) and np.isfinite(na[..., 0]).sum() > 6000
    # the 5 cm defaults at 48 x 64: most pixels' neighbours are farther apart than that, which is why the rendered tests set the edge.
    # A smaller edge only removes normals, and a normal that stays keeps its bits.
    small, large = np.isfinite(none[..., 0]), np.isfinite(na[..., 0])
    assert not (small & ~large).any() and small.sum() < large.sum() and np.array_equal(none[small].view(np.uint32), na[small].view(np.uint32))


def test_confidence_removes_pixels_before_anything_else(planted):
    from mvtracker_amd import align
    d = planted["d"]
    conf = np.random.default_rng(3).uniform(0, 10, planted["depths"].shape).astype(np.float32)
    plain = align.ClipAlignment(d["depths"][0], d["intrs"][0], d["extrs"][0], alignment(frames=(1,)), depths_conf=dev(conf)[0])
    st = align.ClipAlignment(d["depths"][0], d["intrs"][0], d["extrs"][0], alignment(frames=(1,), conf_thresh=3.0), depths_conf=dev(conf)[0])
    a, b = sync_np(plain.xyz0), sync_np(st.xyz0)
    want = (planted["depths"][0, :, 1, 0] > 0) & (conf[0, :, 1, 0] > np.float32(3.0))
    got = np.isfinite(b[:, 0, :, 0]).reshape(4, 48, 64)
    print(f"{int(np.isfinite(a[..., 0]).sum())} points without a threshold (the map is ignored), {int(got.sum())} with conf > 3")
    assert np.array_equal(np.isfinite(a[:, 0, :, 0]).reshape(4, 48, 64), planted["depths"][0, :, 1, 0] > 0) and np.array_equal(got, want)
    assert np.array_equal(b[:, 0][got.reshape(4, -1)].view(np.uint32), a[:, 0][got.reshape(4, -1)].view(np.uint32))
    assert np.isnan(sync_np(st.nrm)[:, 0, :, 0][~got.reshape(4, -1)]).all()  # (no normal on a point that is not there)


def test_align_point_clouds_against_the_restatement():
    """The registration_icp call on point lists: an analytic bowl with exact normals, the source moved by a planted rigid motion."""
    from mvtracker_amd import align_point_clouds
    tgt, _ = Cs.dyadic_target(24, 40)
    xy = tgt[R.valid_rows(tgt), :2].astype(np.float64)
    pts = np.concatenate([xy, (0.05 * (xy ** 2).sum(1) + 0.3 * np.sin(xy[:, 0]))[:, None]], 1).astype(np.float32)
    n = np.stack([-(0.1 * xy[:, 0] + 0.3 * np.cos(xy[:, 0])), -0.1 * xy[:, 1], np.ones(len(xy))], 1)
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    n[::17] = np.nan  # targets without a normal take no part
    G = Cs.rigid(0.4, (0.2, 1.0, -0.3), (0.01, -0.015, 0.02))
    src = ((pts.astype(np.float64) - G[:3, 3]) @ G[:3, :3]).astype(np.float32)
    src[3] = np.inf  # a source row that is not finite takes no part
    ref = R.icp([np.where(np.isfinite(src).all(1, keepdims=True), src, np.nan).astype(np.float32)], [[(pts, n)]], 0.2, 20)
    T, fit, rmse = align_point_clouds(dev(src), dev(pts), dev(n), 0.2, 20)
    T = sync_np(T)
    print(f"max |T - restatement| {np.abs(T - ref['D']).max():.2e}, max |T - planted| {np.abs(T - G).max():.2e}, fitness {fit:.6f} "
          f"(ref {ref['fitness']:.6f}), rmse {rmse:.3e} (ref {ref['rmse']:.3e}), restatement iterations {ref['iterations']}")
    # the same correspondences (no near tie decides anything here): the transforms differ by fp64 rounding through <= 20 solves
    assert np.abs(T - ref["D"]).max() <= 1e-9 and abs(fit - ref["fitness"]) <= 1e-12 and abs(rmse - ref["rmse"]) <= 1e-9
    assert np.abs(T - G).max() < 2e-3 and fit > 0.9 and T.shape == (4, 4) and (T[3] == [0, 0, 0, 1]).all()
    T2, _, _ = align_point_clouds(dev(src), dev(pts), dev(n), 0.2, 20, init=dev(G))
    assert np.abs(sync_np(T2) - G).max() < 1e-4


def test_one_iteration_at_a_time_from_the_devices_own_transform(planted):
    """Teacher-forced: every device iteration starts from the device's own D and is compared with the restatement's step from that D,
    fed the device's points and normals."""
    from mvtracker_amd import align
    d = planted["d"]
    st = align.ClipAlignment(d["depths"][0], d["intrs"][0], d["extrs"][0], alignment())
    run = st.icp(1, keep_queries=True)
    xyz0, xyz, nrm = sync_np(st.xyz0), sync_np(st.xyz), sync_np(st.nrm)
    union = R.target_union([(xyz[u, 0], nrm[u, 0, :, :3]) for u in (0, 2, 3)])
    slots = align.query_slots(st.P, st.grid, 1).numpy()
    cap2 = R.cap_squared(0.05)
    assert float(run.n_queries[0]) == np.isfinite(xyz0[1, 0, :, 0]).sum()
    worst_near = worst_D = 0.0
    steps = 0
    for it in range(6):
        D_before = np.vstack([sync_np(run.D).reshape(3, 4), [0, 0, 0, 1]])
        run.step()
        torch.cuda.synchronize()
        if int(run.istate[0]):  # converged: this evaluation made no update (the restatement takes 4 updates from the planted error)
            break
        steps += 1
        q = np.full((len(slots), 3), np.nan, np.float32)
        q[slots >= 0] = R.transform(D_before, xyz0[1, 0][slots[slots >= 0]])
        ref = R.correspond(q, union, cap2)
        idx = run.q_idx.cpu().numpy()[0]
        valid = np.isfinite(q[:, 0])
        near = ref["near"] & valid
        differ = (idx != ref["idx"]) & valid
        worst_near = max(worst_near, near.sum() / valid.sum())
        # the sums against fp64 numpy on the DEVICE's correspondences
        gid = union[2]
        pos = np.full(len(idx), -1, np.int64)
        pos[idx >= 0] = np.searchsorted(gid, idx[idx >= 0])
        assert np.array_equal(gid[pos[idx >= 0]], idx[idx >= 0])  # (every index names a candidate: a point with a valid normal)
        d2_dev = run.q_d2.cpu().numpy()[0].astype(np.float64)
        sums_dev_corr = R.normal_equations(q, dict(pos=pos, d2=d2_dev), union)
        sums = run.sums.cpu().numpy()
        A, b = R.unpack(sums)
        Ar, br = R.unpack(sums_dev_corr)
        scale = np.sqrt(np.outer(A.diagonal(), A.diagonal()))
        eA = (np.abs(A - Ar) / scale).max()
        eb = (np.abs(b - br) / np.sqrt(A.diagonal() * sums[28])).max()
        hist = run.hist.cpu().numpy()[it]
        x_np = np.linalg.solve(A, -b)
        ex = np.linalg.norm(hist[4:] - x_np) / np.linalg.norm(x_np)
        # the restatement's own step from D_before
        x_ref, status = R.solve(R.normal_equations(q, ref, union))
        D_ref = R.transform_of(x_ref) @ D_before
        D_after = sync_np(run.D).reshape(3, 4)
        eD = np.abs(D_after - D_ref[:3]).max()
        worst_D = max(worst_D, eD)
        dsc = 1 / np.sqrt(A.diagonal())
        cond = np.linalg.cond(A * np.outer(dsc, dsc))
        print(f"iteration {it}: {int(valid.sum())} queries, {int((idx >= 0).sum())} matched (ref {int((ref['idx'] >= 0).sum())}), near ties "
              f"{int(near.sum())}, indices differ at {int(differ.sum())} ({int((differ & ~near).sum())} outside the near ties), "
              f"A err {eA:.2e}, b err {eb:.2e}, x rel err vs numpy {ex:.2e}, |D - restatement's step| {eD:.2e}, cond {cond:.1f}, "
              f"count/fitness/rmse {hist[0]:.0f} {hist[1]:.4f} {hist[2]:.5f}")
        assert not (differ & ~near).any() and near.sum() <= NEAR_FRAC * valid.sum()
        assert sums[27] == (idx >= 0).sum() and eA <= A_TOL and eb <= A_TOL and ex <= X_TOL and status == 0
        assert abs(sums[29] - d2_dev[idx >= 0].sum()) <= 1e-12 * sums[29] and abs(sums[28] - sums_dev_corr[28]) <= A_TOL * sums[28]
        assert hist[0] == sums[27] and abs(hist[1] - sums[27] / valid.sum()) <= 1e-15 and abs(hist[2] - np.sqrt(sums[29] / sums[27])) <= 1e-15
        if not differ.any():  # the same correspondences: x differs by the sums' rounding only, amplified by the conditioning
            assert eD <= 10 * A_TOL * cond * max(np.abs(x_ref).max(), 1e-6)
    print(f"{steps} updates compared, worst near-tie share {100 * worst_near:.3f} %, worst |D - restatement's step| {worst_D:.2e}")
    assert steps >= 3


@pytest.fixture(scope="module")
def end_to_end_reference(planted):
    """The restatement on the device's own unprojected points, once per frame set."""
    cache = {}

    def get(frames, xyz0):
        if frames not in cache:
            clouds = [[xyz0[v, f] for f in range(xyz0.shape[1])] for v in range(4)]
            cache[frames] = R.align_views(clouds, 64, 48, 0.05, Cs.NORMAL_MAX_EDGE, 30, 2)
        return cache[frames]
    return get


@pytest.mark.parametrize("frames", [(0,), (0, 1)])
def test_end_to_end_one_perturbed_view(planted, end_to_end_reference, frames):
    from mvtracker_amd import align, align_cameras
    d = planted["d"]
    a = alignment(frames=frames)
    c = align_cameras(d["depths"], d["intrs"], d["extrs"], a)
    D = sync_np(c.transforms)
    st = align.ClipAlignment(d["depths"][0], d["intrs"][0], d["extrs"][0], a)
    ref = end_to_end_reference(frames, sync_np(st.xyz0))
    before = Cs.displacement(np.eye(4), planted["moved"][1], planted["true"][1])
    left = Cs.displacement(D[1], planted["moved"][1], planted["true"][1])
    left_ref = Cs.displacement(ref["D"][1], planted["moved"][1], planted["true"][1])
    print(f"frames {frames}: planted {1e3 * before:.2f} mm, left by the device {1e3 * left:.3f} mm, by the restatement {1e3 * left_ref:.3f} mm "
          f"(ratio {left / left_ref:.3f}); max |D_device - D_restatement| {np.abs(D - ref['D']).max():.2e}; "
          f"iterations {c.iterations.tolist()} (ref {ref['iterations'].tolist()}), fitness {np.round(sync_np(c.fitness), 4).tolist()}, "
          f"rmse {np.round(sync_np(c.rmse), 5).tolist()}, status {c.status.tolist()}")
    assert left <= before / 10 and left <= 1.5 * left_ref
    assert np.array_equal(D[0], np.eye(4)) and c.status.tolist() == [0, 0, 0, 0] and (D[:, 3] == [0, 0, 0, 1]).all()
    assert c.transforms.dtype == torch.float64 and c.transforms.shape == (4, 4, 4) and c.iterations.tolist()[0] == 0


# ------------------------------------------------------------------------------------------------------------------ 7. determinism, done
def test_two_runs_give_equal_bits_and_done_stops_the_updates(planted):
    from mvtracker_amd import align, align_cameras
    d = planted["d"]
    a = alignment(frames=(0, 1), sample_stride=2)
    one, two = align_cameras(d["depths"], d["intrs"], d["extrs"], a), align_cameras(d["depths"], d["intrs"], d["extrs"], a)
    same = [torch.equal(getattr(one, k), getattr(two, k)) for k in ("transforms", "fitness", "rmse", "iterations", "status")]
    print(f"transforms, fitness, rmse, iterations, status identical: {same}; iterations {one.iterations.tolist()}")
    assert all(same) and float((one.transforms[1] - torch.eye(4, dtype=torch.float64, device=DEV)).abs().max()) > 1e-3
    st = align.ClipAlignment(d["depths"][0], d["intrs"][0], d["extrs"][0], alignment())
    run = st.icp(1)
    run.run()
    torch.cuda.synchronize()
    ist, D1, hist = run.istate.cpu().numpy(), run.D.clone(), run.hist.cpu().numpy()
    print(f"istate after the run {ist.tolist()}, evaluations with a count {int((hist[:, 0] > 0).sum())}")
    assert ist[0] == 1 and 1 <= ist[1] < 30 and ist[3] == ist[1] + 1 and ist[2] == 0  # converged early: iterations < max_iterations
    assert (hist[ist[3]:] == 0).all() and abs(hist[ist[3] - 1, 1] - hist[ist[3] - 2, 1]) < 1e-6 and abs(hist[ist[3] - 1, 2] - hist[ist[3] - 2, 2]) < 1e-6
    run.partial.fill_(1.0)  # anything a further evaluation would turn into an update
    for _ in range(3):
        run.step()
    torch.cuda.synchronize()
    assert torch.equal(run.D, D1) and run.istate.cpu().numpy().tolist() == ist.tolist() and bool((run.partial == 1.0).all())


# ------------------------------------------------------------------------------------------------------------------ 8. wiring
@pytest.fixture(scope="module")
def predictor():
    from mvtracker_amd import EvaluationPredictor
    from mvtracker_amd.tracker import MVTracker
    m = MVTracker(hidden_size=256).eval()
    sd = synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return EvaluationPredictor(m.to(DEV), interp_shape=None, grid_size=2, n_iters=2)


def test_wiring_predictor(predictor):
    from mvtracker_amd import align_cameras
    sc = Cs.scene(2, 128, 128, T=8)
    sc["extrs"] = Cs.perturbed(sc["extrs"], 1, Cs.rigid(0.5, (0.3, -0.5, 0.8), (0.01, -0.008, 0.01)))
    pts = Cs.unproject(sc["depths"], sc["intrs"], sc["extrs"])[0, 0].reshape(-1, 3)
    pick = pts[np.isfinite(pts[:, 0])][::701][:12]
    rng = np.random.default_rng(4)
    c = {k: dev(v) for k, v in sc.items()}
    c["rgbs"] = dev(rng.integers(0, 256, (1, 2, 8, 3, 128, 128)).astype(np.float32))
    c["query_points"] = dev(np.concatenate([np.zeros((len(pick), 1)), pick], 1).astype(np.float32)[None])
    a = alignment(normal_max_edge=0.15, max_iterations=10, sweeps=1)
    fwd = lambda **kw: predictor(rgbs=c["rgbs"], depths=c["depths"], query_points_3d=c["query_points"], intrs=c["intrs"],
                                 extrs=kw.pop("extrs", c["extrs"]), **kw)
    before = c["extrs"].clone()
    corr = align_cameras(c["depths"], c["intrs"], c["extrs"], a)
    fixed = corr.apply(c["extrs"])
    moved = float((corr.transforms[1] - torch.eye(4, dtype=torch.float64, device=DEV)).abs().max())
    print(f"correction of view 1: max |D - I| {moved:.2e}, iterations {corr.iterations.tolist()}, fitness {corr.fitness.tolist()}")
    assert torch.equal(c["extrs"], before) and moved > 1e-4 and torch.equal(fixed[0, 0], c["extrs"][0, 0]) and fixed.dtype == torch.float32
    seen = {}
    hook = predictor.model.register_forward_pre_hook(lambda m, args, kw: seen.update(extrs=kw["extrs"]), with_kwargs=True)
    try:
        plain = fwd()
        assert torch.equal(seen["extrs"], c["extrs"]) and predictor.last_camera_correction is None
        none = fwd(camera_alignment=None)
        out = fwd(camera_alignment=a)
        assert torch.equal(seen["extrs"], fixed) and torch.equal(predictor.last_camera_correction.transforms, corr.transforms)
        by_hand = fwd(extrs=fixed)
        ready = fwd(camera_alignment=corr)
        assert torch.equal(seen["extrs"], fixed) and predictor.last_camera_correction is corr
    finally:
        hook.remove()
    assert torch.equal(plain["traj_e"], none["traj_e"]) and torch.equal(plain["vis_e_as_prob"], none["vis_e_as_prob"])
    for o in (by_hand, ready):
        assert torch.equal(out["traj_e"], o["traj_e"]) and torch.equal(out["vis_e_as_prob"], o["vis_e_as_prob"])
    assert bool(torch.isfinite(out["traj_e"]).all()) and not torch.equal(out["traj_e"], plain["traj_e"])
