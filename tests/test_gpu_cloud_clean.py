"""Depth cleaning on the device against the fp64 restatement tests/cloud_clean_ref.py (numpy + cKDTree; brute force without scipy).

No recorded output of the reference exists for this feature: its cleaning calls Open3D, which is installed neither here nor with the
reference's tests, so the restatement of Open3D's rules (searches include the query, deviation over valid - 1, strict radius) is
the yardstick.  tests/test_cloud_clean_host.py shows on the restatement alone that these bars see a left-out self, k - 1 neighbours
and the wrong divisor.

1. Lattice clouds (coordinates integers / 4: every fp32 d2 is exact): a_i = the fp32 rounding of the restatement's mean or its
   neighbour (1 ulp for the double rounding), counts, M and keep equal on every point; organised and linear feed, raster and a seeded
   random order, K in {1, 2, 16, 17, 20, 64}.
2. Rendered clouds with 20 flying pixels each: point bits = mvt_unproject's; the restatement is fed the device's points; a_i within
   1e-6 relative (fp32 d2 carries <= 5 * 2^-24 = 3e-7, the distance 1.5e-7; plus a swapped near-tie at the K-th place and one fp32
   rounding); keep equal outside |a - thr| <= 1e-5 thr, at most 0.1 % of the valid points inside it; radius mode equal wherever the
   restatement decides the same at r (1 -+ 1e-5), at most 0.1 % undecided.
3. Two runs give the same bits.  4. The predictor / streaming wiring, bit for bit.
Every figure is printed before it is asserted."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_clean_cases as Cs  # noqa: E402
import cloud_clean_ref as R  # noqa: E402
from mvtracker_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
A_TOL, BAND, BAND_FRAC = 1e-6, 1e-5, 1e-3


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)


def cleaning(method="statistical", **kw):
    from mvtracker_amd import DepthCleaning
    return DepthCleaning(method, **kw)


def search(clouds, grid, c):
    """clouds: list of (P, 4) float32 of one size -> (values (C,P), state (C,4), keep (C,P)) as numpy."""
    from mvtracker_amd import clean
    xyz = dev(np.stack(clouds))
    v, s, k = clean.search_clouds(xyz, len(clouds), clouds[0].shape[0], grid, c)
    torch.cuda.synchronize()
    return v.cpu().numpy(), s.cpu().numpy(), k.cpu().numpy() != 0


def check_statistical(tag, x, a, state, keep, k, std_ratio=2.0):
    """One cloud x (P,4) on lattice coordinates against the restatement: a to 1 ulp, M equal, thr to 1e-5, keep equal everywhere."""
    ref = R.clean_cloud(x, "statistical", k, std_ratio)
    ok = R.valid_rows(x)
    ulp = np.abs(bits(a[ok]) - bits(ref["a32"][ok])).max() if ok.any() else 0
    thr_rel = abs(state[3] - ref["thr"]) / ref["thr"] if ref["thr"] > 0 else abs(state[3])
    a64 = ref["a32"][ok].astype(np.float64)
    closest = (np.abs(a64 - ref["thr"]) / ref["thr"]).min() if ref["thr"] > 0 and ok.any() else np.inf
    nd = int((keep != ref["keep"]).sum())
    print(f"{tag}: K {k} M {int(state[0])} (ref {ref['M']}) a max ulp {ulp} thr rel {thr_rel:.2e} closest |a-thr|/thr {closest:.2e} "
          f"kept {int(keep.sum())} (ref {int(ref['keep'].sum())}) keep differs at {nd}")
    assert np.isnan(a[~ok]).all() and not keep[~ok].any()
    assert int(state[0]) == ref["M"] and ulp <= 1 and thr_rel <= BAND and closest > BAND and nd == 0


# ------------------------------------------------------------------------------------------------------------------ 1. lattice, exact
@pytest.mark.parametrize("order", ["raster", "permuted"])
@pytest.mark.parametrize("hw", Cs.LATTICE_SHAPES)
def test_lattice_statistical_is_exact(hw, order):
    H, W = hw
    p = Cs.lattice_cloud(H, W)
    if order == "permuted":
        p = Cs.permuted(p)
    org, grid, idx = Cs.organised(p, H, W)
    lin = Cs.linear(p)
    for k in Cs.KS:
        c = cleaning(nb_neighbors=k)
        a, st, keep = search([org], grid, c)
        check_statistical(f"{H}x{W} {order} organised", org, a[0], st[0], keep[0], k)
        a2, st2, keep2 = search([lin], (0, 0), c)
        check_statistical(f"{H}x{W} {order} linear", lin, a2[0], st2[0], keep2[0], k)
        # the two feeds hold the same points: the same a bits and mask on them
        assert np.array_equal(bits(a[0][idx]), bits(a2[0])) and np.array_equal(keep[0][idx], keep2[0])


@pytest.mark.parametrize("order", ["raster", "permuted"])
@pytest.mark.parametrize("hw", Cs.LATTICE_SHAPES)
def test_lattice_radius_counts_are_equal(hw, order):
    H, W = hw
    p = Cs.lattice_cloud(H, W)
    if order == "permuted":
        p = Cs.permuted(p)
    org, grid, idx = Cs.organised(p, H, W)
    lin = Cs.linear(p)
    for rad2, mp in ((2.5, 5), (2.5, 1000), (20.5, 1000), (20.5, 0)):  # r^2 in lattice units: never a lattice distance
        radius = float(np.sqrt(rad2) / 4)
        c = cleaning("radius", radius=radius, min_points=mp)
        for tag, x, g in (("organised", org, grid), ("linear", lin, (0, 0))):
            ref = R.clean_cloud(x, "radius", radius=radius, min_points=mp)
            cnt, st, keep = search([x], g, c)
            want = np.where(ref["c"] >= 0, np.minimum(ref["c"], mp + 1), -1)
            nd = int((cnt[0] != want).sum())
            print(f"{H}x{W} {order} {tag}: r2 {rad2} min_points {mp} M {int(st[0, 0])} (ref {ref['M']}) max count {cnt[0].max()} "
                  f"(ref {want.max()}) counts differ at {nd}, kept {int(keep[0].sum())} (ref {int(ref['keep'].sum())})")
            assert nd == 0 and int(st[0, 0]) == ref["M"] and np.array_equal(keep[0], ref["keep"])


def test_lattice_special_clouds_and_cloud_strides():
    """5 valid points at K = 20 (k' = M = 5), an all-NaN cloud, and three clouds of different content and valid counts in one call."""
    H, W = 24, 40
    full = Cs.lattice_cloud(H, W)
    five = np.full_like(full, np.nan)
    pick = np.flatnonzero(R.valid_rows(full))[[3, 200, 401, 650, 900]]
    five[pick] = full[pick]
    empty = np.full_like(full, np.nan)
    other = Cs.lattice_cloud(H, W, seed=9)
    other[::3] = np.nan
    one = np.full_like(full, np.nan)
    one[17] = full[pick[0]]
    clouds = [full, five, other, empty, one]
    for tag, feed, grid in (("organised", [Cs.organised(x, H, W)[0] for x in clouds], Cs.organised(full, H, W)[1]),
                            ("linear", [Cs.linear(x) for x in clouds], (0, 0))):
        for k in (20, 2):
            a, st, keep = search(feed, grid, cleaning(nb_neighbors=k))
            for i, x in enumerate(feed):
                if i in (3, 4):  # no valid point / a single one: nothing kept, M as counted
                    print(f"{tag} cloud {i}: M {st[i, 0]} kept {keep[i].sum()}")
                    assert st[i, 0] == (0 if i == 3 else 1) and not keep[i].any()
                    assert np.isnan(a[i]).sum() == len(x) - (0 if i == 3 else 1)
                    continue
                check_statistical(f"{tag} cloud {i}", x, a[i], st[i], keep[i], k)
        ref5 = R.clean_cloud(feed[1], "statistical", 20, 2.0)
        assert ref5["M"] == 5  # (the divisor of a_i is k' = 5: checked by check_statistical's 1 ulp)
        radius = float(np.sqrt(2.5) / 4)
        cnt, st, keep = search(feed, grid, cleaning("radius", radius=radius, min_points=5))
        for i, x in enumerate(feed):
            ref = R.clean_cloud(x, "radius", radius=radius, min_points=5)
            assert np.array_equal(cnt[i], np.where(ref["c"] >= 0, np.minimum(ref["c"], 6), -1)) and np.array_equal(keep[i], ref["keep"])
            assert int(st[i, 0]) == ref["M"]


def test_argument_errors_come_before_any_launch():
    from mvtracker_amd import hip
    x = dev(Cs.linear(Cs.lattice_cloud(8, 8)))[None].contiguous()
    box, gbox = torch.empty(1, 1, 8, device=DEV), torch.empty(1, 1, 8, device=DEV)
    a = torch.empty(1, 64, device=DEV)
    for kw in (dict(K=0), dict(K=65), dict(grid=(8, 4)), dict(grid=(12, 8))):
        with pytest.raises(hip.HipError, match="arguments rejected"):
            hip.clean_search(x, 1, 64, kw.get("grid", (0, 0)), hip.CLEAN_STATISTICAL, kw.get("K", 4), 0.0, 0, box, gbox, a_out=a)
    cnt = torch.empty(1, 64, device=DEV, dtype=torch.int32)
    with pytest.raises(hip.HipError, match="arguments rejected"):
        hip.clean_search(x, 1, 64, (0, 0), hip.CLEAN_RADIUS, 0, 0.0, 5, box, gbox, c_out=cnt)


# ------------------------------------------------------------------------------------------------------------------ 2. rendered clouds
@pytest.fixture(scope="module")
def flying():
    clip = Cs.flying_clip()
    return clip, {k: dev(clip[k]) for k in ("depths", "intrs", "extrs")}


def run_clip(d, c, conf=None):
    from mvtracker_amd import clean
    out = clean.clean_clip(d["depths"][0], d["intrs"][0], d["extrs"][0], c, depths_conf=conf, details=True)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]  # keep (V,T,1,H,W), values (V,T,H,W), states (V,T,4), points (V,T,H,W,4)


def test_rendered_points_are_unproject_bits(flying):
    from mvtracker_amd import hip
    clip, d = flying
    keep, a, st, pts = run_clip(d, cleaning(nb_neighbors=8))
    V, T, _, H, W = clip["depths"][0].shape
    kinv, einv = torch.empty(V * T, 9, device=DEV), torch.empty(V * T, 12, device=DEV)
    hip.invert_cameras(d["intrs"][0].reshape(-1, 9).contiguous(), d["extrs"][0].reshape(-1, 12).contiguous(), kinv, einv, V * T)
    ds = d["depths"][0, :, :, 0].permute(1, 0, 2, 3).contiguous()  # level-0 depth [T][V][H][W], stride 1
    xyz = torch.empty(T, V, H, W, 4, device=DEV)
    hip.unproject(ds, kinv, einv, xyz, V, T, H, W, 1, 0)
    want = xyz.permute(1, 0, 2, 3, 4).cpu().numpy()
    valid = clip["depths"][0, :, :, 0] > 0
    same = np.array_equal(pts[valid].view(np.uint32), want[valid].view(np.uint32))
    print(f"{int(valid.sum())} valid pixels, point bits equal: {same}; NaN on the others: {bool(np.isnan(pts[~valid][:, :3]).all())}")
    assert same and np.isnan(pts[~valid][:, :3]).all() and valid.sum() > 11000


@pytest.mark.parametrize("k", [20, 8])
def test_rendered_statistical(flying, k):
    clip, d = flying
    keep, a, st, pts = run_clip(d, cleaning(nb_neighbors=k, std_ratio=2.0))
    V, T = pts.shape[:2]
    for v in range(V):
        for t in range(T):
            x = pts[v, t].reshape(-1, 4)
            ok = R.valid_rows(x)
            ref = R.clean_cloud(x, "statistical", k, 2.0)
            av, kv = a[v, t].reshape(-1), keep[v, t, 0].reshape(-1)
            rel = np.abs(av[ok].astype(np.float64) - ref["a"][ok]) / ref["a"][ok]
            band = np.zeros(len(x), bool)
            band[ok] = np.abs(ref["a32"][ok].astype(np.float64) - ref["thr"]) <= BAND * ref["thr"]
            differ = kv != ref["keep"]
            removed = int((ok & ~kv).sum())
            print(f"view {v} frame {t} K {k}: M {int(st[v, t, 0])} (ref {ref['M']}) a rel max {rel.max():.2e} thr {st[v, t, 3]:.6f} "
                  f"(ref {ref['thr']:.6f}) removed {removed} in band {int(band.sum())} keep differs outside {int((differ & ~band).sum())} "
                  f"inside {int((differ & band).sum())}")
            assert int(st[v, t, 0]) == ref["M"] == int(ok.sum()) and rel.max() <= A_TOL
            assert abs(st[v, t, 3] - ref["thr"]) <= BAND * ref["thr"]
            assert not (differ & ~band).any() and (differ & band).sum() <= BAND_FRAC * ok.sum()
            assert np.isnan(av[~ok]).all() and not kv[~ok].any() and 20 <= removed <= 100


@pytest.mark.parametrize("radius", [0.25, 0.4])
def test_rendered_radius(flying, radius):
    clip, d = flying
    keep, cnt, st, pts = run_clip(d, cleaning("radius", radius=radius, min_points=5))
    V, T = pts.shape[:2]
    r2 = R.radius_sq(radius)
    for v in range(V):
        for t in range(T):
            x = pts[v, t].reshape(-1, 4)
            ok = R.valid_rows(x)
            lo = R.clean_cloud(x, "radius", radius=radius, min_points=5, r2=r2 * (1 - 1e-5) ** 2)["keep"]
            hi = R.clean_cloud(x, "radius", radius=radius, min_points=5, r2=r2 * (1 + 1e-5) ** 2)["keep"]
            decided = lo == hi
            kv = keep[v, t, 0].reshape(-1)
            nd = int(((kv != lo) & decided).sum())
            print(f"view {v} frame {t} r {radius}: M {int(st[v, t, 0])} removed {int((ok & ~kv).sum())} undecided {int((~decided).sum())} "
                  f"keep differs where decided {nd}")
            assert nd == 0 and (~decided).sum() <= BAND_FRAC * ok.sum() and int(st[v, t, 0]) == int(ok.sum())
            assert not kv[~ok].any() and cnt[v, t].reshape(-1)[~ok].max(initial=-1) == -1 and (ok & ~kv).sum() >= 10


def test_confidence_and_sphere_remove_pixels_before_the_search(flying):
    clip, d = flying
    base = run_clip(d, cleaning(nb_neighbors=8))
    conf = np.random.default_rng(3).uniform(0, 10, clip["depths"].shape).astype(np.float32)
    keep, a, st, pts = run_clip(d, cleaning(nb_neighbors=8, conf_thresh=3.0), conf=dev(conf)[0])
    valid = (clip["depths"][0, :, :, 0] > 0) & (conf[0, :, :, 0] > np.float32(3.0))
    print(f"confidence: {int(valid.sum())} pixels enter, M sums to {int(st[..., 0].sum())}")
    assert np.array_equal(np.isfinite(pts[..., 0]), valid) and int(st[..., 0].sum()) == int(valid.sum())
    assert np.array_equal(pts[valid].view(np.uint32), base[3][valid].view(np.uint32)) and not keep[:, :, 0][~valid].any()
    x = pts[1, 1].reshape(-1, 4)  # the search runs on what is left
    assert np.array_equal(keep[1, 1, 0].reshape(-1), R.clean_cloud(x, "statistical", 8, 2.0)["keep"])
    centre = np.nanmean(base[3][..., :3].reshape(-1, 3), 0).astype(np.float32)
    keep, a, st, pts = run_clip(d, cleaning(nb_neighbors=8, sphere_radius=1.5, sphere_center=centre))
    inside, near = R.sphere_inside(base[3], centre, 1.5, margin=1e-6)  # (fp32 d2 carries 3e-7: the surface shell may go either way)
    inside &= clip["depths"][0, :, :, 0] > 0
    got = np.isfinite(pts[..., 0])
    print(f"sphere: {int(inside.sum())} of {int((clip['depths'] > 0).sum())} pixels inside, {int(near.sum())} in the surface shell, "
          f"differing outside the shell {int(((got != inside) & ~near).sum())}, M sums to {int(st[..., 0].sum())}")
    assert 0.1 < inside.mean() < 0.9 and not ((got != inside) & ~near).any() and near.sum() <= 2 and int(st[..., 0].sum()) == int(got.sum())
    assert np.array_equal(pts[got].view(np.uint32), base[3][got].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ 3. determinism
@pytest.mark.parametrize("method", ["statistical", "radius"])
def test_two_runs_give_the_same_bits(flying, method):
    clip, d = flying
    c = cleaning(method, nb_neighbors=20, radius=0.25)
    one, two = run_clip(d, c), run_clip(d, c)
    same = [np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(one, two)]
    print(f"{method}: keep, values, state, points identical: {same}")
    assert all(same)


# ------------------------------------------------------------------------------------------------------------------ 4. wiring
@pytest.fixture(scope="module")
def predictor():
    from mvtracker_amd import EvaluationPredictor
    from mvtracker_amd.tracker import MVTracker
    m = MVTracker(hidden_size=256).eval()
    sd = synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return EvaluationPredictor(m.to(DEV), interp_shape=None, grid_size=2, n_iters=2)


@pytest.fixture(scope="module")
def e2e_clip():
    c = synth.make_clip(5, V=2, T=8, H=128, W=128, N=12, late_queries=True, query_frames=(2,))
    d = c["depths"]
    rng = np.random.default_rng(11)
    d[(rng.uniform(size=d.shape) < 0.01) & (d > 0)] *= 0.6  # flying pixels
    return {k: dev(v) for k, v in c.items()}


def _fwd(pred, c, **kw):
    d = kw.pop("depths", c["depths"])
    return pred(rgbs=c["rgbs"], depths=d, query_points_3d=c["query_points"], intrs=c["intrs"], extrs=c["extrs"], **kw)


def test_wiring_predictor_and_stream(predictor, e2e_clip):
    from mvtracker_amd import SceneTransform, clean_depths
    c = e2e_clip
    cl = cleaning(nb_neighbors=20, std_ratio=2.0)
    before = c["depths"].clone()
    dc, keep = clean_depths(c["depths"], c["intrs"], c["extrs"], cl)
    removed = int((~keep & (c["depths"] > 0)).sum())
    print(f"{removed} of {int((c['depths'] > 0).sum())} valid pixels removed")
    assert torch.equal(c["depths"], before) and keep.dtype == torch.bool and keep.shape == c["depths"].shape
    assert torch.equal(dc, torch.where(keep, c["depths"], torch.zeros((), device=DEV))) and removed > 500
    plain = _fwd(predictor, c)
    none = _fwd(predictor, c, depth_cleaning=None)
    assert torch.equal(plain["traj_e"], none["traj_e"]) and torch.equal(plain["vis_e_as_prob"], none["vis_e_as_prob"])
    out = _fwd(predictor, c, depth_cleaning=cl)
    by_hand = _fwd(predictor, c, depths=dc)
    assert torch.equal(out["traj_e"], by_hand["traj_e"]) and torch.equal(out["vis_e_as_prob"], by_hand["vis_e_as_prob"])
    assert bool(torch.isfinite(out["traj_e"]).all()) and not torch.equal(out["traj_e"], plain["traj_e"])
    for xf in (None, SceneTransform(1.25, None, (0.1, -0.2, 0.05))):
        off = _fwd(predictor, c, depth_cleaning=cl, scene_transform=xf)
        st = predictor.open_stream(c["query_points"], scene_transform=xf, depth_cleaning=cl)
        outs = [st.push(*(c[k][:, :, a:a + 3] for k in ("rgbs", "depths", "intrs", "extrs"))) for a in range(0, 8, 3)]
        outs.append(st.finish())
        assert torch.equal(torch.cat([o["traj_e"] for o in outs], 1), off["traj_e"])
        assert torch.equal(torch.cat([o["vis_e_as_prob"] for o in outs], 1), off["vis_e_as_prob"])


# ------------------------------------------------------------------------------------------- 5. more than 64 groups of tiles
# The searches' shared walk takes the groups of tiles 64 at a time, so a cloud needs more than 4096 tiles to reach the second round.
# 65 * 64 * 64 lattice points, coordinates integers / 64 (every fp32 d2 is exact), stored as a point list of 4x4x4 blocks, one block
# per tile (tight boxes), the BLOCKS in a seeded random order: 4160 tiles in 65 groups, neighbours on both sides of group 64.
BIG_BLOCKS, BIG_SEED = (13, 20, 16), 11
BIG_R2 = 6.5  # in lattice steps: no lattice distance (6 and 8 are); 81 offsets lie within it


@functools.lru_cache(maxsize=None)
def big_lattice():
    """(xyz (P, 4) float32, slot (X, Y, Z): the list index of every lattice point)."""
    bx, by, bz = BIG_BLOCKS
    nb = bx * by * bz
    tile_of_block = np.random.default_rng(BIG_SEED).permutation(nb).reshape(bx, by, bz)
    i, j, k = np.meshgrid(np.arange(4 * bx), np.arange(4 * by), np.arange(4 * bz), indexing="ij")
    slot = tile_of_block[i // 4, j // 4, k // 4] * 64 + (i % 4) * 16 + (j % 4) * 4 + k % 4
    xyz = np.zeros((nb * 64, 4), np.float32)
    xyz[slot.ravel(), 0], xyz[slot.ravel(), 1], xyz[slot.ravel(), 2] = i.ravel() / 64, j.ravel() / 64, k.ravel() / 64
    return xyz, slot


def lattice_offsets(r2):
    m = int(np.sqrt(r2))
    return [(a, b, c) for a in range(-m, m + 1) for b in range(-m, m + 1) for c in range(-m, m + 1) if a * a + b * b + c * c < r2]


def shifted(a, o, fill):
    """b[p] = a[p + o] where p + o lies in the lattice, else fill."""
    b = np.full_like(a, fill)
    src = tuple(slice(max(d, 0), a.shape[e] + min(d, 0)) for e, d in enumerate(o))
    dst = tuple(slice(max(-d, 0), a.shape[e] + min(-d, 0)) for e, d in enumerate(o))
    b[dst] = a[src]
    return b


def test_radius_counts_beyond_64_groups():
    from mvtracker_amd import hip
    xyz, slot = big_lattice()
    P = xyz.shape[0]
    offs = lattice_offsets(BIG_R2)
    assert P == 65 * 64 * 64 and (P // 64 + 63) // 64 == 65 and len(offs) == 81
    # the closed form: the lattice points within the radius, by shifted sums; and the pairs that only the second round of groups finds
    want = np.zeros(slot.shape, np.int64)
    across = np.zeros(slot.shape, bool)
    for o in offs:
        nb_slot = shifted(slot, o, -1)
        want += nb_slot >= 0
        across |= (slot // 64 < 4096) & (nb_slot // 64 >= 4096)
    ref = np.empty(P, np.int64)
    ref[slot.ravel()] = want.ravel()
    x = dev(xyz[None])
    box, gbox = hip.cloud_boxes(x, 1, P, (0, 0))
    cnt = torch.empty(1, P, dtype=torch.int32, device=DEV)
    # min_points = the largest possible count: no counter stops early, every lane keeps its bound to the end
    hip.clean_search(x, 1, P, (0, 0), hip.CLEAN_RADIUS, 0, float(np.sqrt(BIG_R2) / 64), len(offs), box, gbox, c_out=cnt)
    torch.cuda.synchronize()
    got = cnt[0].cpu().numpy()
    nd = int((got != ref).sum())
    print(f"{P} points, {P // 64} tiles: counts {ref.min()}..{ref.max()}, {int(across.sum())} points below group 64 with a neighbour in it, "
          f"counts differ at {nd}")
    assert across.any() and nd == 0


def test_nearest_indices_beyond_64_groups():
    """The same cloud through the normals' search, max_nn = 8: on a lattice the 8 smallest (d2, index) pairs are full of equal d2, so
    the indices check the tie rule across the round of groups as well."""
    from mvtracker_amd import cloud
    xyz, slot = big_lattice()
    P = xyz.shape[0]
    offs = lattice_offsets(3.5)  # 27 offsets: every point, a corner included, has at least 8 of them inside the lattice
    d2 = np.array([a * a + b * b + c * c for a, b, c in offs], np.int64)
    nb = np.stack([shifted(slot, o, -1).ravel() for o in offs], 1)  # (P, 27) in lattice order
    key = np.where(nb >= 0, d2[None] * (1 << 32) + nb, np.int64(1) << 62)
    ref = np.empty((P, 8), np.int64)
    ref[slot.ravel()] = np.sort(key, 1)[:, :8] & 0xFFFFFFFF
    assert (np.sort(key, 1)[:, 7] < (np.int64(1) << 62)).all()
    _, idx, cnt, _ = cloud.normals_of_clouds(dev(xyz[None]), 1, P, (0, 0), float(np.sqrt(3.5) / 64), 8, details=True)
    torch.cuda.synchronize()
    nd = int((idx[0].cpu().numpy() != ref).any(1).sum())
    print(f"{P} points: neighbour lists differ at {nd}, counts {int(cnt.min())}..{int(cnt.max())}")
    assert nd == 0 and int(cnt.min()) == 8 and int(cnt.max()) == 8
