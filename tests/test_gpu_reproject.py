"""Reprojection check on the device against the restatement tests/reproject_ref.py (bit for bit for the render, exact for the integer
scores) and the recorded reference (tests/golden/reproject_render.npz).

1. Planted list: a 7 x 9 image, fx = fy = 4, dyadic cx, cy, identity extrinsics, depths that are powers of two: every uf, vf is exact.
2. Contention: 4096 points on one pixel.
3. Clip form: scene(3, 24, 40, T=2), "others" / "all", uint8 / fp32 frames; the restatement is fed the device's own point bits
   (mvt_clean_points), as the depth cleaning tests do, and every pixel of index, depth and colour is equal.  The fixture holds fp32
   POINTS (the reference function takes a list), which the clip form cannot be handed: it derives its points from the depth maps with
   mvt_unproject's fp32 arithmetic, whose last bits differ from the fixture's fp64 unprojection rounded once.  The fixture is met in
   every pixel of index, depth and colour through the list entries on its own points, and by the clip form on the same scene in
   every pixel of index (the fixture's winner as a clip index) and colour, with no excluded share; only the depth word, whose bits
   cannot agree, has a bar, 1e-5: about 7 fp32 roundings per coordinate at magnitudes below 8 (half an ulp, 2.4e-7, each), three
   coordinates through a unit row of E, the fp32 rounding of the inverse cameras (6e-8 x 8 x 3) and the final rounding come to 5e-6.
4. Splat 3 and 5 on a 13 x 11 image.  5. Scores: integer words exact, SSIM sums within 1e-10 N, depth sums within 1e-12 relative.
6. Calibration signal: scene(4, 48, 64), view 1 perturbed by PLANTED: the close-depth share drops, and align_cameras brings it up."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_align_cases as Cs  # noqa: E402
import reproject_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reproject_render.npz")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sync_np(*ts):
    torch.cuda.synchronize()
    out = [t.cpu().numpy() for t in ts]
    return out[0] if len(out) == 1 else out


def same_render(tag, got, want):
    color, depth, index = got
    dc, dd, di = (int((color != want[0]).any(0).sum()), int((depth.view(np.uint32) != want[1].view(np.uint32)).sum()), int((index != want[2]).sum()))
    print(f"{tag}: {int((want[2] >= 0).sum())} of {want[2].size} pixels covered; differing pixels: colour {dc}, depth {dd}, index {di}")
    assert dc == 0 and dd == 0 and di == 0


def device_list_render(points, colors, intr, extr, H, W, min_depth=0.01, splat=1):
    from mvtracker_amd import render_point_cloud
    return sync_np(*render_point_cloud(dev(points), dev(colors), dev(intr), dev(extr), H, W, min_depth, splat))


# ------------------------------------------------------------------------------------------------------------------ 1. planted list
PLANT_K = np.array([[4, 0, 3.5], [0, 4, 2.25], [0, 0, 1]], np.float32)
PLANT_E = np.eye(4, dtype=np.float32)[:3]


def at(uf, vf, z):
    """The point that projects to exactly (uf, vf) at depth z (a power of two; uf - cx and vf - cy are multiples of 1/4)."""
    return [(uf - 3.5) * z / 4, (vf - 2.25) * z / 4, z]


def test_planted_list():
    H, W = 7, 9
    rows = [at(2.5, 1.25, 2.0), at(2.75, 1.5, 1.0),      # 0, 1: one pixel (2, 1), different depth: 1 wins
            at(5.0, 3.0, 4.0), at(5.5, 3.75, 4.0),       # 2, 3: pixel (5, 3), equal fp32 depth: 2 wins
            at(1.0, 5.0, 0.25),                          # 4: c_2 == min_depth: dropped (strict)
            [np.nan, 0.0, 1.0], at(4.0, 4.0, -2.0),      # 5: a NaN row; 6: behind the camera
            at(-0.5, 2.0, 2.0),                          # 7: uf = -0.5 truncates to column 0: drawn
            at(-1.0, 3.0, 2.0),                          # 8: uf = -1.0: dropped
            at(9.0, 4.0, 2.0),                           # 9: uf = W: dropped
            at(8.75, 6.0, 2.0),                          # 10: uf = W - 0.25: drawn in column 8
            at(3.0, -0.25, 1.0), at(3.0, 7.0, 1.0),      # 11: vf = -0.25: row 0; 12: vf = H: dropped
            at(1.0, 5.0, 0.5), [0.0, np.inf, 1.0]]       # 13: just beyond min_depth, drawn where 4 was not; 14: an infinite row
    pts = np.array(rows, np.float32)
    cols = (np.arange(len(pts) * 3).reshape(-1, 3) * 7 % 255 + 1).astype(np.uint8)
    got = device_list_render(pts, cols, PLANT_K, PLANT_E, H, W, min_depth=0.25)
    want_index = np.full((H, W), -1, np.int32)
    for (y, x), i in {(1, 2): 1, (3, 5): 2, (2, 0): 7, (6, 8): 10, (0, 3): 11, (5, 1): 13}.items():
        want_index[y, x] = i
    assert np.array_equal(got[2], want_index), got[2]  # the winners, written down by hand
    assert got[1][1, 2] == 1.0 and got[1][3, 5] == 4.0 and got[1][5, 1] == 0.5 and got[1][0, 0] == 0.0
    assert np.array_equal(got[0][:, 3, 5], cols[2]) and not got[0][:, 0, 0].any()
    same_render("planted list", got, R.render_points(pts, cols, PLANT_K, PLANT_E, H, W, 0.25))


# ------------------------------------------------------------------------------------------------------------------ 2. contention
def test_contention_on_one_pixel_is_order_independent():
    H, W, n = 7, 9, 4096
    rng = np.random.default_rng(4)
    z = (1.0 + rng.permutation(n).astype(np.float32) / 8192).astype(np.float32)  # distinct fp32 depths in [1, 1.5), shuffled
    z[rng.choice(n, 64, replace=False)] = z[rng.choice(n, 64, replace=False)]    # some equal pairs
    near = np.flatnonzero(z == z.min())
    z[near[0] + 1 if near[0] + 1 < n else 0] = z.min()                           # the nearest depth twice: the lower index wins
    pts = np.stack([np.zeros(n, np.float32), np.zeros(n, np.float32), z], 1)     # all on the optical axis: pixel (3, 2)
    cols = rng.integers(1, 256, size=(n, 3), dtype=np.uint8)
    want = R.render_points(pts, cols, PLANT_K, PLANT_E, H, W)
    assert (want[2] >= 0).sum() == 1 and want[2][2, 3] == np.flatnonzero(z == z.min())[0] and (z == z.min()).sum() >= 2
    a = device_list_render(pts, cols, PLANT_K, PLANT_E, H, W)
    b = device_list_render(pts, cols, PLANT_K, PLANT_E, H, W)
    same_render("contention", a, want)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------ 3. clip form
@pytest.fixture(scope="module")
def clip():
    V, H, W, T = 3, 24, 40, 2
    sc = Cs.scene(V, H, W, T)
    sc["depths"][0, 1, 1, 0, 6:14, 8:30] = 0  # frame 1: a block of view 1's depths zeroed
    rng = np.random.default_rng(9)
    g = np.load(GOLDEN)
    rgbs = rng.integers(1, 256, size=(1, V, T, 3, H, W), dtype=np.uint8)
    rgbs[0, :, 0] = g["colors"]  # frame 0 carries the fixture's colours
    conf = rng.uniform(size=sc["depths"].shape).astype(np.float32)
    return dict(sc, rgbs=rgbs, conf=conf, golden=g, V=V, H=H, W=W, T=T)


def device_points(c, t, conf_thresh=None):
    """Frame t's source points with the device's bits: mvt_clean_points, cut to (V,H,W,3), and their validity."""
    from mvtracker_amd import hip
    V, H, W, T = c["V"], c["H"], c["W"], c["T"]
    kinv, einv = torch.empty(V * T, 9, device=DEV), torch.empty(V * T, 12, device=DEV)
    hip.invert_cameras(dev(c["intrs"][0].reshape(-1, 9)), dev(c["extrs"][0].reshape(-1, 12)), kinv, einv, V * T)
    Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
    xyz = torch.empty(V, Hp * Wp, 4, device=DEV)
    hip.clean_points(dev(c["depths"][0]), None if conf_thresh is None else dev(c["conf"][0]), kinv, einv, V, T, t, 1, H, W, conf_thresh, None, xyz)
    p = sync_np(xyz).reshape(V, Hp, Wp, 4)[:, :H, :W, :3]
    return p, np.isfinite(p).all(-1)


@pytest.mark.parametrize("float_rgb", [False, True])
@pytest.mark.parametrize("sources", ["others", "all"])
def test_clip_form_equals_the_restatement_in_every_pixel(clip, sources, float_rgb):
    from mvtracker_amd import reproject_views
    c = clip
    rgbs = c["rgbs"].astype(np.float32) + np.float32(0.25) if float_rgb else c["rgbs"]  # (+0.25 rounds back: rintf is in the path)
    color, depth, index = sync_np(*reproject_views(dev(rgbs), dev(c["depths"]), dev(c["intrs"]), dev(c["extrs"]), sources=sources,
                                                   depths_conf=dev(c["conf"]), conf_thresh=0.2))
    assert color.shape == (1, 3, 2, 3, 24, 40) and depth.shape == (1, 3, 2, 1, 24, 40) and index.shape == (1, 3, 2, 24, 40)
    for t in range(c["T"]):
        pts, valid = device_points(c, t, 0.2)
        want = R.render_views(pts, valid, c["rgbs"][0, :, t], c["intrs"][0, :, t], c["extrs"][0, :, t], sources)
        for v in range(c["V"]):
            same_render(f"{sources} fp32={float_rgb} frame {t} view {v}", (color[0, v, t], depth[0, v, t, 0], index[0, v, t]), [w[v] for w in want])
    assert not np.array_equal(index[0, :, 0], index[0, :, 1])  # the zeroed block shows


def test_golden_fixture_in_every_pixel(clip):
    """The list entries on the fixture's own fp32 points: the reference's image in every pixel; then the clip form on the same scene:
    the fixture's winner and colour in every pixel, the depth within the bar of the module docstring."""
    from mvtracker_amd import reproject_views
    c, g = clip, clip["golden"]
    V, H, W = c["V"], c["H"], c["W"]
    sc = Cs.scene(V, H, W)
    assert all(np.array_equal(g[k], sc[k]) for k in ("depths", "intrs", "extrs"))
    got_list = []
    for tv in range(V):
        got = device_list_render(g[f"points_{tv}"], g[f"point_colors_{tv}"], g["intrs"][0, tv, 0], g["extrs"][0, tv, 0], H, W, float(g["min_depth"][0]))
        differ = int((got[0] != g[f"color_{tv}"]).any(0).sum())
        print(f"view {tv}: coverage {(got[2] >= 0).mean():.3f}; pixels differing from the reference's image: {differ} of {H * W}")
        assert differ == 0 and 0.4 < (got[2] >= 0).mean() < 0.5
        same_render(f"golden view {tv}", got, R.render_points(g[f"points_{tv}"], g[f"point_colors_{tv}"], g["intrs"][0, tv, 0], g["extrs"][0, tv, 0],
                                                              H, W, float(g["min_depth"][0])))
        got_list.append(got)
    color, depth, index = sync_np(*reproject_views(dev(c["rgbs"]), dev(sc["depths"]), dev(sc["intrs"]), dev(sc["extrs"]), frames=(0,)))
    for tv in range(V):
        src = np.where(got_list[tv][2] >= 0, g[f"point_source_{tv}"][np.maximum(got_list[tv][2], 0)], -1)  # the fixture's winners as clip indices
        agree = index[0, tv, 0] == src
        gap = float(np.abs(depth[0, tv, 0, 0] - got_list[tv][1]).max())
        print(f"view {tv}: clip form's winners equal the fixture's in {int(agree.sum())} of {H * W} pixels; largest depth gap {gap:.2e}")
        assert np.array_equal(index[0, tv, 0], src) and np.array_equal(color[0, tv, 0], g[f"color_{tv}"])  # every pixel, no excluded share
        assert gap < 1e-5  # (only the depth word: the unprojections differ in the last fp32 bits)


# ------------------------------------------------------------------------------------------------------------------ 4. splat
@pytest.mark.parametrize("splat", [1, 3, 5])
def test_splat_sprites_are_clipped_and_depth_tested(splat):
    H, W = 13, 11
    K = np.array([[4, 0, 0.5], [0, 4, 0.5], [0, 0, 1]], np.float32)

    def px(x, y, z):
        return [(x + 0.25 - 0.5) * z / 4, (y + 0.25 - 0.5) * z / 4, z]

    rows = [px(0, 0, 2.0), px(10, 0, 2.0), px(0, 12, 2.0), px(10, 12, 2.0),  # the corners
            px(5, 0, 1.0), px(0, 6, 1.0), px(10, 7, 4.0), px(4, 12, 4.0),    # the borders
            px(5, 6, 2.0), px(6, 6, 1.0), px(7, 7, 1.0), px(4, 5, 1.0)]      # overlapping sprites: equal depths, the lower index wins
    pts = np.array(rows, np.float32)
    cols = (np.arange(len(pts) * 3).reshape(-1, 3) * 11 % 255 + 1).astype(np.uint8)
    got = device_list_render(pts, cols, K, PLANT_E, H, W, splat=splat)
    want = R.render_points(pts, cols, K, PLANT_E, H, W, splat=splat)
    r = splat // 2
    assert got[2][0, 0] == 0 and got[2][12, 10] == 3 and got[2][6, 6] == 9  # (7, 7)'s sprite reaches (6, 6) at the same depth: 9 < 10 stays
    assert got[2][r, r] == 0 and got[2][12 - r, 10 - r] == 3  # a corner's sprite reaches r pixels into the image and no further out
    assert got[2][6, 5] == (8 if splat == 1 else 9)  # the nearer point's sprite covers the centre of the farther one
    assert (got[2] >= 0).sum() == (len(pts) if splat == 1 else (want[2] >= 0).sum()) and (want[2] >= 0).sum() > len(pts) * (splat > 1)
    same_render(f"splat {splat}", got, want)


# ------------------------------------------------------------------------------------------------------------------ 5. scores
def device_scores(a, b, index, depth, zt, tol):
    from mvtracker_amd import hip
    n, _, H, W = a.shape
    s = torch.empty(n, hip.SCORE_WORDS, dtype=torch.int64, device=DEV)
    hip.photometric_score(dev(a), dev(b), dev(index), dev(depth), dev(zt), n, H, W, tol, s)
    return sync_np(s)


def check_scores(tag, got, a, b, index, depth, zt, tol):
    ints = (R.N, R.COVERED, R.SSE, R.SAE, R.SSE_COV, R.SAE_COV, R.N_DEPTH, R.N_CLOSE)
    for j in range(len(a)):
        want = R.score(a[j], b[j], index[j], depth[j], zt[j], tol)
        gd = got[j].view(np.float64)
        n = want[R.N]
        print(f"{tag}[{j}]: N {n} covered {want[R.COVERED]} depth pixels {want[R.N_DEPTH]} close {want[R.N_CLOSE]}; "
              + " ".join(f"{name} {gd[w]:.15g} (want {want[w]:.15g}, diff {abs(gd[w] - want[w]):.2e})"
                         for name, w in (("ssim", R.SSIM), ("ssim_cov", R.SSIM_COV), ("dsae", R.DEPTH_SAE), ("dsae_close", R.DEPTH_SAE_CLOSE))))
        assert [int(got[j][w]) for w in ints] == [want[w] for w in ints] and not got[j][12:].any()
        assert abs(gd[R.SSIM] - want[R.SSIM]) <= 1e-10 * n and abs(gd[R.SSIM_COV] - want[R.SSIM_COV]) <= 1e-10 * n
        assert abs(gd[R.DEPTH_SAE] - want[R.DEPTH_SAE]) <= 1e-12 * want[R.DEPTH_SAE]
        assert abs(gd[R.DEPTH_SAE_CLOSE] - want[R.DEPTH_SAE_CLOSE]) <= 1e-12 * want[R.DEPTH_SAE_CLOSE]


@pytest.mark.parametrize("float_rgb", [False, True])
def test_scores_on_the_clip_renders(clip, float_rgb):
    from mvtracker_amd import ReprojectionCheck, reproject_views, reprojection_report
    c = clip
    V, T, H, W = c["V"], c["T"], c["H"], c["W"]
    rgbs = c["rgbs"].astype(np.float32) if float_rgb else c["rgbs"]
    color, depth, index = sync_np(*reproject_views(dev(rgbs), dev(c["depths"]), dev(c["intrs"]), dev(c["extrs"])))
    a, ix, z = color[0].reshape(V * T, 3, H, W), index[0].reshape(V * T, H, W), depth[0].reshape(V * T, H, W)
    b, zt = rgbs[0].reshape(V * T, 3, H, W), c["depths"][0].reshape(V * T, H, W).copy()
    zt[0, 3, 5], zt[0, 4, 6] = np.nan, np.inf  # a target depth that is not finite takes no part
    got = device_scores(a, b, ix, z, zt, 0.05)
    check_scores(f"clip fp32={float_rgb}", got, a, b, ix, z, zt, 0.05)
    assert np.array_equal(got, device_scores(a, b, ix, z, zt, 0.05))  # two runs: the same bits
    # the host layer's report is these records (with the clip's own depth maps)
    rep = reprojection_report(dev(rgbs), dev(c["depths"]), dev(c["intrs"]), dev(c["extrs"]), ReprojectionCheck(frames=(0, 1)))
    want = device_scores(a, b, ix, z, c["depths"][0].reshape(V * T, H, W), 0.05)
    assert np.array_equal(rep.records.numpy().reshape(V * T, -1), want)
    assert rep.depth_close_fraction.shape == (V, T) and float(rep.coverage.min()) > 0.3


@pytest.mark.parametrize("hw", [(13, 11), (6, 6), (17, 33)])
def test_scores_on_small_pairs(hw):
    H, W = hw
    rng = np.random.default_rng(H * 100 + W)
    a = rng.integers(0, 256, size=(2, 3, H, W), dtype=np.uint8)
    b = np.clip(a.astype(np.int64) + rng.integers(-40, 41, size=a.shape), 0, 255).astype(np.uint8)
    index = np.where(rng.uniform(size=(2, H, W)) < 0.6, rng.integers(0, 1000, size=(2, H, W)), -1).astype(np.int32)
    depth = np.where(index >= 0, rng.uniform(0.5, 3.0, size=(2, H, W)), 0).astype(np.float32)
    zt = (depth + rng.choice([0.0, 0.01, 0.05, 0.2], size=depth.shape) * rng.choice([-1, 1], size=depth.shape)).astype(np.float32)
    zt[rng.uniform(size=zt.shape) < 0.1] = 0
    index[0, 0, 0], depth[0, 0, 0], zt[0, 0, 0] = 5, 1.0, 1.0625  # exactly at the (dyadic) tolerance: close (<=)
    index[1, 0, 0], depth[1, 0, 0], zt[1, 0, 0] = 5, 1.0, 1.0625 + 2.0 ** -20  # just beyond it: not close
    got = device_scores(a, b, index, depth, zt, 0.0625)
    check_scores(f"{H}x{W}", got, a, b, index, depth, zt, 0.0625)
    bf = b.astype(np.float32) + np.float32(0.4)  # fp32 frames against uint8 renders: the same 8-bit values
    assert np.array_equal(device_scores(a, bf, index, depth, zt, 0.0625), got)


def test_identical_pair_and_the_size_limit():
    from mvtracker_amd import hip
    H, W = 13, 11
    a = np.random.default_rng(1).integers(0, 256, size=(1, 3, H, W), dtype=np.uint8)
    index = np.zeros((1, H, W), np.int32)
    z = np.ones((1, H, W), np.float32)
    got = device_scores(a, a, index, z, z, 0.0)
    gd = got[0].view(np.float64)
    assert got[0][R.SSE] == 0 and got[0][R.SAE] == 0 and gd[R.SSIM] == float(H * W) and gd[R.SSIM_COV] == float(H * W)
    assert got[0][R.N_CLOSE] == H * W and gd[R.DEPTH_SAE] == 0.0
    small = np.zeros((1, 3, 5, 8), np.uint8)
    with pytest.raises(hip.HipError, match="code 1 "):
        hip.photometric_score(dev(small), dev(small), dev(np.zeros((1, 5, 8), np.int32)), dev(np.zeros((1, 5, 8), np.float32)),
                              dev(np.zeros((1, 5, 8), np.float32)), 1, 5, 8, 0.05, torch.empty(1, 16, dtype=torch.int64, device=DEV),
                              partial=torch.empty(64, dtype=torch.int64, device=DEV))


def test_entries_refuse_bad_arguments_before_any_launch():
    from mvtracker_amd import hip
    keys = torch.empty(2, 63, dtype=torch.int64, device=DEV)
    K, E, pts = dev(PLANT_K.reshape(1, 9)), dev(PLANT_E.reshape(1, 12)), dev(np.zeros((4, 3), np.float32))
    for kw in (dict(splat=2), dict(min_depth=float("nan")), dict(min_depth=-1.0), dict(M=0), dict(H=0), dict(n_targets=0),
               dict(n_targets=hip.REPROJECT_MAX_TARGETS + 1)):
        args = dict(points=pts, M=4, n_targets=1, intrs=K, extrs=E, H=7, W=9, min_depth=0.01, splat=1, keys=keys)
        args.update(kw)
        if args["n_targets"] > 1:
            args["intrs"], args["extrs"] = K.repeat(17, 1), E.repeat(17, 1)
            args["keys"] = torch.empty(17 * 63, dtype=torch.int64, device=DEV)
        with pytest.raises(hip.HipError, match="code 1 "):
            hip.reproject_splat_points(**args)
    d = dev(np.ones((2, 1, 1, 7, 9), np.float32))
    kinv, einv = torch.zeros(2, 9, device=DEV), torch.zeros(2, 12, device=DEV)
    for kw in (dict(t=1), dict(target_views=[0, 2]), dict(splat=4), dict(target_views=[])):
        args = dict(depths=d, conf=None, kinv=kinv, einv=einv, V=2, T=1, t=0, H=7, W=9, conf_thresh=None, target_views=[0, 1],
                    intrs=K.repeat(2, 1), extrs=E.repeat(2, 1), exclude_self=True, min_depth=0.01, splat=1, keys=keys)
        args.update(kw)
        with pytest.raises(hip.HipError, match="code 1 "):
            hip.reproject_splat_depths(**args)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ 6. the signal
def test_calibration_signal_follows_the_cameras():
    """The close-depth share of the perturbed view: below that of the true cameras (0.117 against 0.356 with the restatement on the
    CPU), and above the perturbed value once align_cameras has corrected them.  The order only; the three numbers are printed."""
    from mvtracker_amd import CameraAlignment, ReprojectionCheck, align_cameras, reprojection_report
    sc = Cs.scene(4, 48, 64)
    ex_bad = Cs.perturbed(sc["extrs"], 1, Cs.rigid(**Cs.PLANTED))
    rgbs = dev(np.random.default_rng(6).integers(0, 256, size=(1, 4, 2, 3, 48, 64), dtype=np.uint8))
    d, K = dev(sc["depths"]), dev(sc["intrs"])
    ck = ReprojectionCheck(frames=(0,), sources="others", depth_tol=0.05, splat=1)
    true = reprojection_report(rgbs, d, K, dev(sc["extrs"]), ck)
    bad = reprojection_report(rgbs, d, K, dev(ex_bad), ck)
    corr = align_cameras(d, K, dev(ex_bad), CameraAlignment(max_distance=0.05, normal_max_edge=Cs.NORMAL_MAX_EDGE))
    fixed = reprojection_report(rgbs, d, K, corr.apply(dev(ex_bad)), ck)
    f_true, f_bad, f_fixed = (float(r.depth_close_fraction[1, 0]) for r in (true, bad, fixed))
    print(f"depth_close_fraction of view 1: true cameras {f_true:.4f}, perturbed {f_bad:.4f}, corrected {f_fixed:.4f}; "
          f"depth_mae {float(true.depth_mae[1, 0]):.3f} / {float(bad.depth_mae[1, 0]):.3f} / {float(fixed.depth_mae[1, 0]):.3f}")
    assert f_bad < f_true and f_fixed > f_bad
