"""Depth cleaning, host side (no GPU): DepthCleaning's validation, the per-(view, frame) cloud split, the predictor / streaming / demo
wiring on mocked kernels (tests/hip_mock_clean.py, whose fake entries call the restatement tests/cloud_clean_ref.py), and checks that
the bars of tests/test_gpu_cloud_clean.py can see a defect, run on the restatement alone.

No recorded output of the reference exists for this feature: its cleaning calls Open3D, which is not a dependency of either project's
tests; the restatement of Open3D's documented rules is the yardstick."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_clean_cases as Cs  # noqa: E402
import cloud_clean_ref as R  # noqa: E402
import hip_mock_clean  # noqa: E402
import hip_mock_scene  # noqa: E402
from mvtracker_amd import synth  # noqa: E402

A_TOL, BAND, BAND_FRAC = 1e-6, 1e-5, 1e-3  # the GPU test's bars: relative a_i, |a - thr| <= BAND thr may differ, for at most 0.1 %


# ------------------------------------------------------------------------------------------------------------------ validation
def test_depth_cleaning_validation_and_defaults():
    import inspect
    from mvtracker_amd import DepthCleaning, clean
    assert DepthCleaning is clean.DepthCleaning
    p = inspect.signature(DepthCleaning.__init__).parameters
    assert list(p)[1:] == ["method", "nb_neighbors", "std_ratio", "radius", "min_points", "conf_thresh", "sphere_radius", "sphere_center"]
    c = DepthCleaning()  # the reference's pc_clean_cfg defaults
    assert (c.method, c.nb_neighbors, c.std_ratio, c.radius, c.min_points, c.conf_thresh, c.sphere_radius, c.sphere_center) == \
        ("statistical", 20, 2.0, 0.05, 5, None, None, (0.0, 0.0, 0.0))
    for kw in (dict(method="median"), dict(nb_neighbors=0), dict(nb_neighbors=65), dict(nb_neighbors=2.5), dict(std_ratio=float("nan")),
               dict(std_ratio=float("inf")), dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(min_points=-1),
               dict(sphere_radius=0.0), dict(sphere_center=(0.0, 1.0)), dict(conf_thresh=float("nan"))):
        with pytest.raises(ValueError):
            DepthCleaning(**kw)
    DepthCleaning("radius", nb_neighbors=64, min_points=0, std_ratio=-1.0)
    DepthCleaning(nb_neighbors=1)


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    from mvtracker_amd import DepthCleaning, clean_depths, clean_point_cloud
    hip_mock_clean.install(monkeypatch)
    clip = {k: torch.from_numpy(v) for k, v in synth.make_clip(3, V=2, T=2, H=8, W=8, N=2).items()}
    d, i, e = clip["depths"], clip["intrs"], clip["extrs"]
    with pytest.raises(ValueError):
        clean_depths(d, i, e, "statistical")
    with pytest.raises(ValueError):
        clean_depths(d[0, :, :, 0], i[0], e[0], DepthCleaning())
    with pytest.raises(ValueError):
        clean_depths(d, i[0], e[0], DepthCleaning())
    with pytest.raises(ValueError):
        clean_depths(d, i, e, DepthCleaning(), depths_conf=d[:, :, :1])
    with pytest.raises(ValueError):
        clean_point_cloud(torch.zeros(5, 4), DepthCleaning())
    assert hip_mock_clean.calls == []
    assert clean_point_cloud(torch.zeros(0, 3), DepthCleaning()).shape == (0,) and hip_mock_clean.calls == []


# ------------------------------------------------------------------------------------------------------------------ cloud split
@pytest.fixture(scope="module")
def flying():
    return Cs.flying_clip()


def _points_of(clip):
    """The clouds' points (V,T,H,W,4) as the mocked clean_points leaves them (fp32 unprojection, NaN where not valid)."""
    import hip_mock
    d = torch.from_numpy(clip["depths"][0])
    V, T, _, H, W = d.shape
    kinv, einv = torch.empty(V * T, 9), torch.empty(V * T, 12)
    hip_mock.invert_cameras(torch.from_numpy(clip["intrs"][0]).reshape(-1, 9), torch.from_numpy(clip["extrs"][0]).reshape(-1, 12), kinv, einv, V * T)
    Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
    xyz = torch.empty(V * T, Hp * Wp, 4)
    hip_mock_clean.clean_points(d.contiguous(), None, kinv, einv, V, T, 0, T, H, W, None, None, xyz)
    return xyz.reshape(V, T, Hp, Wp, 4)[:, :, :H, :W].numpy()


@pytest.mark.parametrize("method", ["statistical", "radius"])
def test_every_view_and_frame_is_its_own_cloud_for_both_ranks(flying, monkeypatch, method):
    from mvtracker_amd import DepthCleaning, clean_depths
    hip_mock_clean.install(monkeypatch)
    c = DepthCleaning(method, nb_neighbors=8, radius=0.25)
    d, i, e = (torch.from_numpy(flying[k]) for k in ("depths", "intrs", "extrs"))
    before = d.clone()
    dc6, k6 = clean_depths(d, i, e, c)
    assert hip_mock_clean.calls == ["clean_points", "clean_search", "clean_mask"]
    dc5, k5 = clean_depths(d[0], i[0], e[0], c)
    assert k6.shape == d.shape and k6.dtype == torch.bool and dc6.shape == d.shape and dc6.dtype == d.dtype
    assert k5.shape == d.shape[1:] and torch.equal(k5, k6[0]) and torch.equal(dc5, dc6[0])
    assert torch.equal(d, before)  # the inputs are not written
    assert torch.equal(dc6, torch.where(k6, d, torch.zeros(())))
    pts = _points_of(flying)
    V, T = pts.shape[:2]
    removed = 0
    for v in range(V):
        for t in range(T):  # one cloud per depth map: the restatement on that map alone gives the mask
            want = R.clean_cloud(pts[v, t].reshape(-1, 4), method, 8, 2.0, 0.25, 5)["keep"].reshape(pts.shape[2:4])
            assert np.array_equal(k6[0, v, t, 0].numpy(), want)
            removed += int((~want & (flying["depths"][0, v, t, 0] > 0)).sum())
    assert removed > 100 and not k6[~(d > 0)].any()
    # most of the planted flying pixels go (statistical: those that did not land next to each other)
    if method == "statistical":
        assert (~k6.numpy())[flying["planted"]].mean() > 0.5


def test_clip_is_cut_into_runs_of_frames_with_the_same_mask(flying, monkeypatch):
    from mvtracker_amd import DepthCleaning, clean, clean_depths
    hip_mock_clean.install(monkeypatch)
    d, i, e = (torch.from_numpy(flying[k]) for k in ("depths", "intrs", "extrs"))
    c = DepthCleaning(nb_neighbors=8)
    whole = clean_depths(d, i, e, c)[1]
    monkeypatch.setattr(clean, "MAX_CHUNK_POINTS", 3 * 40 * 56)  # room for one frame of the three views
    del hip_mock_clean.calls[:]
    assert torch.equal(clean_depths(d, i, e, c)[1], whole)
    assert hip_mock_clean.calls == ["clean_points", "clean_search", "clean_mask"] * 2


def test_confidence_and_sphere_remove_pixels_before_the_search(flying, monkeypatch):
    from mvtracker_amd import DepthCleaning, clean_depths
    hip_mock_clean.install(monkeypatch)
    d, i, e = (torch.from_numpy(flying[k]) for k in ("depths", "intrs", "extrs"))
    conf = torch.rand(d.shape, generator=torch.Generator().manual_seed(1)) * 10
    k_plain = clean_depths(d, i, e, DepthCleaning(nb_neighbors=8))[1]
    assert torch.equal(clean_depths(d, i, e, DepthCleaning(nb_neighbors=8), depths_conf=conf)[1], k_plain)  # no threshold: the map is ignored
    k_conf = clean_depths(d, i, e, DepthCleaning(nb_neighbors=8, conf_thresh=3.0), depths_conf=conf)[1]
    assert not k_conf[conf <= 3.0].any() and k_conf.sum() < 0.8 * k_plain.sum()
    pts = _points_of(flying)
    centre = np.nanmean(pts[..., :3].reshape(-1, 3), 0)
    k_sph = clean_depths(d, i, e, DepthCleaning(nb_neighbors=8, sphere_radius=1.5, sphere_center=centre))[1]
    inside = R.sphere_inside(pts, centre, 1.5)
    assert 0.1 < inside.mean() < 0.9 and not k_sph[0, :, :, 0].numpy()[~inside].any() and k_sph.any()


def test_clean_point_cloud_on_an_unorganised_list(monkeypatch):
    from mvtracker_amd import DepthCleaning, clean_point_cloud
    hip_mock_clean.install(monkeypatch)
    p = Cs.permuted(Cs.lattice_cloud(24, 40))
    p[3, 1] = np.inf
    keep = clean_point_cloud(torch.from_numpy(p), DepthCleaning(nb_neighbors=16))
    want = R.clean_cloud(np.where(np.isfinite(p).all(1, keepdims=True), p, np.nan), "statistical", 16, 2.0)["keep"]
    assert keep.dtype == torch.bool and np.array_equal(keep.numpy(), want) and not keep[3] and 0 < (~keep).sum() < 100


# ------------------------------------------------------------------------------------------------------------------ wiring
class FakeSession:
    def __init__(self, queries):
        self.queries, self.pushed = [queries], []
        self.nan_flag = torch.zeros(1, dtype=torch.int32)

    def add_queries(self, q):
        self.queries.append(q)

    def _res(self, a, b):
        n = sum(q.shape[1] for q in self.queries)
        return {"frames": (a, b), "traj_e": torch.zeros(1, b - a, n, 3), "vis_e": torch.zeros(1, b - a, n)}

    def push(self, rgbs, depths, intrs, extrs):
        self.pushed.append((depths, extrs))
        n = sum(d.shape[2] for d, _ in self.pushed)
        return self._res(n - depths.shape[2], n - 1)

    def finish(self):
        n = sum(d.shape[2] for d, _ in self.pushed)
        return self._res(n - 1, n)


class FakeModel(torch.nn.Module):
    S = 4

    def forward(self, rgbs, depths=None, query_points=None, intrs=None, extrs=None, **kw):
        self.seen = dict(depths=depths, query_points=query_points, extrs=extrs, kw=kw)
        return {"traj_e": torch.zeros(1, rgbs.shape[2], query_points.shape[1], 3), "vis_e": torch.zeros(1, rgbs.shape[2], query_points.shape[1])}

    def open_stream(self, query_points, iters=4, ring_blocks=3):
        self.session = FakeSession(query_points)
        return self.session


@pytest.fixture()
def wired(monkeypatch):
    from mvtracker_amd import DepthCleaning, EvaluationPredictor
    hip_mock_clean.install(monkeypatch)
    clip = synth.make_clip(3, V=2, T=6, H=16, W=24, N=5, invalid_frac=0.02)
    d = clip["depths"]
    rng = np.random.default_rng(5)
    d[rng.uniform(size=d.shape) < 0.02] *= 0.6  # flying pixels
    c = {k: torch.from_numpy(v) for k, v in clip.items()}
    pred = EvaluationPredictor(FakeModel(), interp_shape=None, grid_size=2)
    return pred, c, DepthCleaning(nb_neighbors=8, std_ratio=1.0)


def _call(pred, c, **kw):
    return pred(rgbs=c["rgbs"], depths=c["depths"], query_points_3d=c["query_points"], intrs=c["intrs"], extrs=c["extrs"], **kw)


def _all_calls():
    return hip_mock_scene.calls + hip_mock_clean.calls


def test_none_makes_no_call_and_changes_nothing(wired):
    pred, c, cleaning = wired
    _call(pred, c)
    plain = pred.model.seen
    del hip_mock_clean.calls[:]
    _call(pred, c, depth_cleaning=None)
    assert hip_mock_clean.calls == [] and hip_mock_scene.calls == []
    assert all(torch.equal(pred.model.seen[k], plain[k]) for k in ("depths", "query_points", "extrs"))
    assert torch.equal(pred.model.seen["depths"], c["depths"]) and "depth_cleaning" not in pred.model.seen["kw"]
    st = pred.open_stream(c["query_points"])
    st.push(*(c[k][:, :, :3] for k in ("rgbs", "depths", "intrs", "extrs")))
    st.finish()
    assert hip_mock_clean.calls == []
    _call(pred, c, depth_cleaning=cleaning)
    assert hip_mock_clean.calls == ["clean_points", "clean_search", "clean_mask"]
    with pytest.raises(ValueError, match="DepthCleaning"):
        _call(pred, c, depth_cleaning="statistical")
    with pytest.raises(ValueError, match="DepthCleaning"):
        pred.open_stream(c["query_points"], depth_cleaning="radius")


def test_predictor_cleans_then_normalises_then_resizes(wired, monkeypatch):
    from mvtracker_amd import SceneTransform, auto_scene_normalization, clean_depths, hip
    pred, c, cleaning = wired
    dc, keep = clean_depths(c["depths"], c["intrs"], c["extrs"], cleaning)
    assert 0 < int((~keep & (c["depths"] > 0)).sum())
    _call(pred, c, depth_cleaning=cleaning)
    assert torch.equal(pred.model.seen["depths"], dc)
    # with a transform and a resize: the model sees resize(scale(clean(depths))), and the entries run in that order
    order = []
    for name in ("clean_points", "scene_apply", "resize_nearest"):
        real = getattr(hip, name)
        monkeypatch.setattr(hip, name, (lambda n, f: lambda *a, **k: (order.append(n), f(*a, **k))[1])(name, real))
    xf = SceneTransform(2.0, None, (0.5, -1.0, 0.25))
    pred.interp_shape = (8, 12)
    _call(pred, c, depth_cleaning=cleaning, scene_transform=xf)
    assert order.index("clean_points") < order.index("scene_apply") < order.index("resize_nearest")
    want = torch.empty(1, 2, 6, 1, 8, 12)
    hip.resize_nearest(xf.apply(depths=dc)[0].contiguous(), want, 12, 16, 24, 8, 12)
    assert torch.equal(pred.model.seen["depths"], want)
    # "auto" sees the cleaned depths (and the confidence map)
    pred.interp_shape = None
    monkeypatch.setattr("mvtracker_amd.scene.MIN_POINTS", 10)
    _call(pred, c, depth_cleaning=cleaning, scene_transform="auto")
    assert pred.last_scene_transform == auto_scene_normalization(dc, c["intrs"], c["extrs"])
    assert pred.last_scene_transform != auto_scene_normalization(c["depths"], c["intrs"], c["extrs"])


def test_streamed_blocks_are_cleaned_to_the_offline_mask(wired):
    from mvtracker_amd import SceneTransform, clean_depths
    pred, c, cleaning = wired
    dc = clean_depths(c["depths"], c["intrs"], c["extrs"], cleaning)[0]
    for xf in (None, SceneTransform(2.0, None, (0.5, -1.0, 0.25))):
        st = pred.open_stream(c["query_points"], scene_transform=xf, depth_cleaning=cleaning)
        for t0 in (0, 2, 3):  # uneven blocks
            t1 = {0: 2, 2: 3, 3: 6}[t0]
            st.push(*(c[k][:, :, t0:t1] for k in ("rgbs", "depths", "intrs", "extrs")))
        st.finish()
        got = torch.cat([p[0] for p in pred.model.session.pushed], 2)
        assert torch.equal(got, dc if xf is None else xf.apply(depths=dc)[0])


def test_demo_flags_parse():
    import demo_amd
    ap = demo_amd.build_parser()
    a = ap.parse_args(["--synthetic"])
    assert a.clean_depths is None and demo_amd.depth_cleaning_from_args(a) is None
    assert (a.pc_clean_nb_neighbors, a.pc_clean_std_ratio, a.pc_clean_radius, a.pc_clean_min_points) == (20, 2.0, 0.05, 5)
    a = ap.parse_args("--synthetic --clean-depths radius --pc-clean-radius 0.1 --pc-clean-min-points 7 --pc-clean-nb-neighbors 12 "
                      "--pc-clean-std-ratio 1.5".split())
    c = demo_amd.depth_cleaning_from_args(a)
    assert (c.method, c.radius, c.min_points, c.nb_neighbors, c.std_ratio) == ("radius", 0.1, 7, 12, 1.5)
    assert demo_amd.depth_cleaning_from_args(ap.parse_args(["--synthetic", "--clean-depths", "statistical"])).method == "statistical"
    with pytest.raises(SystemExit):
        ap.parse_args(["--synthetic", "--clean-depths", "median"])
    with pytest.raises(ValueError):
        demo_amd.depth_cleaning_from_args(ap.parse_args(["--synthetic", "--clean-depths", "statistical", "--pc-clean-nb-neighbors", "100"]))


def test_save_result_keeps_the_mask(tmp_path):
    from mvtracker_amd import sample_io
    s = {"query_points_3d": torch.zeros(1, 2, 4), "keep": np.ones((2, 3, 1, 4, 4), bool)}
    sample_io.save_result(str(tmp_path / "r.npz"), torch.zeros(1, 3, 2, 3), torch.ones(1, 3, 2, dtype=torch.bool), s, include_clip=False)
    assert np.load(tmp_path / "r.npz")["keep"].shape == (2, 3, 1, 4, 4)


# ------------------------------------------------------------------------------------------------------------------ the bars see a defect
def _clouds(flying):
    pts = _points_of(flying)
    return [pts[v, t].reshape(-1, 4) for v in range(pts.shape[0]) for t in range(pts.shape[1])]


@pytest.mark.parametrize("defect", [dict(include_self=False), dict(drop_last=True)])
@pytest.mark.parametrize("k", [20, 8])
def test_bars_see_a_wrong_neighbourhood(flying, defect, k):
    """Self left out, or k - 1 neighbours: every a_i moves by far more than the 1e-6 bar, and the mask differs outside the band."""
    out_of_band = 0
    for x in _clouds(flying):
        ok = R.valid_rows(x)
        good, bad = R.clean_cloud(x, "statistical", k, 2.0), R.clean_cloud(x, "statistical", k, 2.0, **defect)
        rel = np.abs(bad["a"][ok] - good["a"][ok]) / good["a"][ok]
        assert rel.min() > 1000 * A_TOL
        a = good["a32"][ok].astype(np.float64)
        band = np.abs(a - good["thr"]) <= BAND * good["thr"]
        assert not band.any()  # (checked for this seed and planting: the GPU test compares every point)
        n = int((bad["keep"] != good["keep"])[ok][~band].sum())
        assert k != 20 or n >= 1  # at k = 20 in every cloud
        out_of_band += n
    assert out_of_band >= 6
    # the lattice clouds, where a_i must match to 1 ulp
    p = Cs.lattice_cloud(24, 40)
    ok = R.valid_rows(p)
    good, bad = R.clean_cloud(p, "statistical", k, 2.0), R.clean_cloud(p, "statistical", k, 2.0, **defect)
    assert (np.abs(bad["a"][ok] - good["a"][ok]) > 1e-3 * good["a"][ok]).mean() > 0.9  # (1 ulp is 6e-8)


def test_bars_see_the_wrong_divisor():
    """Divisor 'number of a > 0' where M is required: a_i is untouched, so only the duplicate pairs at K = 2 (a = 0) can show it --
    mu, sigma and thr move by percents (the GPU test holds thr to 1e-5) and the mask differs at points far outside the band."""
    p = Cs.lattice_cloud(24, 40)
    ok = R.valid_rows(p)
    good, bad = R.clean_cloud(p, "statistical", 2, 2.0), R.clean_cloud(p, "statistical", 2, 2.0, divisor="positive")
    a = good["a32"][ok].astype(np.float64)
    assert (a == 0).sum() >= 100 and np.array_equal(good["a"][ok], bad["a"][ok])
    assert abs(bad["thr"] - good["thr"]) > 1000 * BAND * good["thr"] and abs(bad["mu"] - good["mu"]) > 0.05 * good["mu"]
    diff = (bad["keep"] != good["keep"])[ok]
    assert diff.sum() >= 1 and (np.abs(a[diff] - good["thr"]) > BAND * good["thr"]).all()
    # on a cloud with no a = 0 the two divisors agree: the rendered clouds alone could not see this defect
    q = R.clean_cloud(p, "statistical", 16, 2.0)
    assert np.array_equal(q["keep"], R.clean_cloud(p, "statistical", 16, 2.0, divisor="positive")["keep"])


@pytest.mark.parametrize("hw", Cs.LATTICE_SHAPES)
def test_lattice_fixtures_are_decided(hw):
    """What the GPU test relies on: no a_i within 1e-5 thr of thr on any lattice cloud, duplicates give a = 0 at K = 2, the off-surface
    points go, and the permuted cloud is the same set."""
    p = Cs.lattice_cloud(*hw)
    ok = R.valid_rows(p)
    assert 0 < (~ok).sum() < len(p) // 16
    q = Cs.permuted(p)
    assert np.array_equal(np.sort(p[ok].view("f4,f4,f4"), axis=0), np.sort(q[R.valid_rows(q)].view("f4,f4,f4"), axis=0)) and not np.array_equal(p, q)
    far = p[:, 2] > 40
    for k in Cs.KS:
        r = R.clean_cloud(p, "statistical", k, 2.0)
        a = r["a32"][ok].astype(np.float64)
        if k == 1:
            assert (a == 0).all() and not r["keep"].any()
            continue
        assert (np.abs(a - r["thr"]) > 100 * BAND * r["thr"]).all()
        assert ((a == 0).sum() >= 2) == (k == 2) and r["keep"][ok & ~far].mean() > 0.8
        assert k == 2 or not r["keep"][far].any()  # (at K = 2 two planted points that landed side by side keep each other)
    for rad2 in (2.5, 20.5):  # r^2 in lattice units: not a lattice distance
        c = R.clean_cloud(p, "radius", radius=np.sqrt(rad2) / 4, min_points=5)
        d2 = 16 * ((p[ok][:, None, :].astype(np.float64) - p[ok][None, :, :]) ** 2).sum(-1) if len(p) < 2000 else None
        if d2 is not None:
            assert np.abs(d2 - 16 * R.radius_sq(np.sqrt(rad2) / 4)).min() > 0.4 and np.array_equal(c["c"][ok], (d2 < rad2).sum(1))
        assert not c["keep"][far].any() and c["keep"].any()
