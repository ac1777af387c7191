"""Reprojection check, host side (no GPU): ReprojectionCheck's validation, the shapes, argument errors and frame runs of
mvtracker_amd/reproject.py on mocked kernels (tests/hip_mock_reproject.py, whose fake entries call the restatement
tests/reproject_ref.py), "others" against "all", the report arithmetic, the predictor / demo wiring, and the restatement itself
against the recorded results of the reference (tests/golden/reproject_render.npz: render_dense_pointcloud, compute_mse / _psnr / _mae)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_align_cases as Cs  # noqa: E402
import hip_mock_align  # noqa: E402
import hip_mock_clean  # noqa: E402
import hip_mock_reproject as M  # noqa: E402
import hip_mock_scene  # noqa: E402
import reproject_ref as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reproject_render.npz")


def test_check_validation_and_defaults():
    import inspect
    from mvtracker_amd import ReprojectionCheck, reproject
    assert ReprojectionCheck is reproject.ReprojectionCheck
    assert list(inspect.signature(ReprojectionCheck.__init__).parameters)[1:] == ["frames", "sources", "min_depth", "splat", "depth_tol", "conf_thresh"]
    c = ReprojectionCheck()
    assert (c.frames, c.sources, c.min_depth, c.splat, c.depth_tol, c.conf_thresh) == ((0,), "others", 0.01, 1, 0.05, None)
    for kw in (dict(frames=()), dict(frames=(0, 0)), dict(frames=(-1,)), dict(frames=3), dict(frames=(0.5,)), dict(sources="self"),
               dict(min_depth=-1.0), dict(min_depth=float("nan")), dict(splat=2), dict(splat=7), dict(depth_tol=-0.1), dict(depth_tol=float("inf")),
               dict(conf_thresh=float("nan"))):
        with pytest.raises(ValueError):
            ReprojectionCheck(**kw)
    ReprojectionCheck(frames=[3, 1], sources="all", splat=5, conf_thresh=-1.0)
    assert list(inspect.signature(reproject.render_point_cloud).parameters) == ["points", "colors", "intr", "extr", "height", "width", "min_depth",
                                                                                "splat"]
    assert list(inspect.signature(reproject.reproject_views).parameters) == ["rgbs", "depths", "intrs", "extrs", "frames", "sources", "min_depth",
                                                                             "splat", "depths_conf", "conf_thresh"]


def _clip(V=3, H=24, W=40, T=2, seed=3, float_rgb=False):
    sc = {k: torch.from_numpy(v) for k, v in Cs.scene(V, H, W, T).items()}
    rgb = np.random.default_rng(seed).integers(1, 256, size=(1, V, T, 3, H, W), dtype=np.uint8)
    sc["rgbs"] = torch.from_numpy(rgb.astype(np.float32) if float_rgb else rgb)
    return sc


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    from mvtracker_amd import ReprojectionCheck, render_point_cloud, reproject_views, reprojection_report
    M.install(monkeypatch)
    s = _clip()
    r, d, i, e = s["rgbs"], s["depths"], s["intrs"], s["extrs"]
    for kw in (dict(depths=d[0, :, :, 0]), dict(intrs=i[0]), dict(rgbs=r[0]), dict(rgbs=r[:, :, :, :2]), dict(frames=(0, 2)), dict(frames=()),
               dict(sources="none"), dict(splat=2), dict(min_depth=float("nan")), dict(depths_conf=d[:, :, :1]),
               dict(rgbs=r[:, :1], depths=d[:, :1], intrs=i[:, :1], extrs=e[:, :1])):  # (one view has no others)
        args = dict(rgbs=r, depths=d, intrs=i, extrs=e)
        args.update(kw)
        with pytest.raises(ValueError):
            reproject_views(**args)
    with pytest.raises(ValueError):
        reprojection_report(r, d, i, e, "check")
    with pytest.raises(ValueError):  # the SSIM window: refused before the render
        reprojection_report(r[..., :5, :8], d[..., :5, :8], i, e, ReprojectionCheck())
    pts, col = torch.zeros(5, 3), torch.ones(5, 3, dtype=torch.uint8)
    for bad in (dict(points=torch.zeros(5, 4)), dict(colors=torch.ones(4, 3, dtype=torch.uint8)), dict(colors=torch.ones(5, 3)),
                dict(intr=torch.eye(4)), dict(extr=torch.eye(4)), dict(height=0), dict(splat=4), dict(min_depth=-1.0)):
        kw = dict(points=pts, colors=col, intr=torch.eye(3), extr=torch.eye(4)[:3], height=7, width=9)
        kw.update(bad)
        with pytest.raises(ValueError):
            render_point_cloud(**kw)
    assert M.calls == [] and hip_mock_clean.calls == []
    c, z, ix = render_point_cloud(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.uint8), torch.eye(3), torch.eye(4)[:3], 7, 9)
    assert M.calls == [] and c.shape == (3, 7, 9) and not c.any() and not z.any() and (ix == -1).all()


def _device_points(s, t, conf=None, conf_thresh=None):
    """The points the mocked entries see for frame t: (V,H,W,3) fp32 and their validity."""
    from mvtracker_amd import hip
    d = s["depths"][0].float().contiguous()
    V, T, _, H, W = d.shape
    kinv, einv = torch.empty(V * T, 9), torch.empty(V * T, 12)
    hip.invert_cameras(s["intrs"][0].reshape(-1, 9).contiguous(), s["extrs"][0].reshape(-1, 12).contiguous(), kinv, einv, V * T)
    Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
    xyz = torch.empty(V, Hp * Wp, 4)
    n = len(hip_mock_clean.calls)
    hip_mock_clean.clean_points(d, conf, kinv, einv, V, T, t, 1, H, W, conf_thresh, None, xyz)
    del hip_mock_clean.calls[n:]  # (the helper's own call, not the host layer's)
    p = xyz.reshape(V, Hp, Wp, 4)[:, :H, :W, :3].numpy()
    return p, np.isfinite(p).all(-1)


@pytest.mark.parametrize("float_rgb", [False, True])
def test_shapes_frame_runs_and_others_against_all(monkeypatch, float_rgb):
    from mvtracker_amd import reproject, reproject_views
    M.install(monkeypatch)
    s = _clip(T=3, float_rgb=float_rgb)
    V, T, H, W = 3, 3, 24, 40
    s["depths"][0, 1, 2, 0, 4:12, 10:30] = 0  # frame 2 differs from the others
    monkeypatch.setattr(reproject, "MAX_RUN_PIXELS", 2 * V * H * W)  # two frames per run
    out = {}
    for sources in ("others", "all"):
        del M.calls[:], M.splats[:]
        color, depth, index = reproject_views(s["rgbs"], s["depths"], s["intrs"], s["extrs"], frames=(2, 0, 1), sources=sources)
        assert color.shape == (1, V, 3, 3, H, W) and color.dtype == torch.uint8 and depth.shape == (1, V, 3, 1, H, W) and depth.dtype == torch.float32
        assert index.shape == (1, V, 3, H, W) and index.dtype == torch.int32
        assert M.calls == ["reproject_clear"] + ["reproject_splat_depths", "reproject_resolve"] * 2 + ["reproject_clear", "reproject_splat_depths",
                                                                                                    "reproject_resolve"]
        assert M.splats == [(2, sources == "others", 1), (0, sources == "others", 1), (1, sources == "others", 1)] and hip_mock_clean.calls == []
        for fi, t in enumerate((2, 0, 1)):
            pts, valid = _device_points(s, t)
            want = R.render_views(pts, valid, s["rgbs"][0, :, t].numpy(), s["intrs"][0, :, t].numpy(), s["extrs"][0, :, t].numpy(), sources)
            assert np.array_equal(color[0, :, fi].numpy(), want[0]) and np.array_equal(index[0, :, fi].numpy(), want[2])
            assert np.array_equal(depth[0, :, fi, 0].numpy().view(np.uint32), want[1].view(np.uint32))
        out[sources] = (color, depth, index)
    ix_o, ix_a = out["others"][2][0].numpy(), out["all"][2][0].numpy()
    own = np.arange(V)[:, None, None, None]
    assert ((ix_o < 0) | (ix_o // (H * W) != own)).all() and 0.3 < (ix_o >= 0).mean() < 0.6  # leave-one-out, and not vacuous
    assert ((ix_a >= 0) | (ix_o < 0)).all() and (ix_a >= 0).mean() > (ix_o >= 0).mean() and (ix_a // (H * W) == own).any()
    assert not np.array_equal(ix_o[:, 0], ix_o[:, 1]) and np.array_equal(ix_o[:, 1], ix_o[:, 2])  # frame 2 first, then the two equal ones
    # without the batch dimension: the same, without it
    c5 = reproject_views(s["rgbs"][0], s["depths"][0], s["intrs"][0], s["extrs"][0], frames=(2, 0, 1), sources="all")
    assert all(torch.equal(a, b[0]) for a, b in zip(c5, out["all"]))
    allf = reproject_views(s["rgbs"][0], s["depths"][0], s["intrs"][0], s["extrs"][0])
    assert allf[2].shape == (V, T, H, W) and torch.equal(allf[2][:, 2], out["others"][2][0, :, 0])


def test_confidence_and_splat_reach_the_entries(monkeypatch):
    from mvtracker_amd import reproject_views
    M.install(monkeypatch)
    s = _clip()
    conf = torch.rand(s["depths"].shape, generator=torch.Generator().manual_seed(1))
    plain = reproject_views(s["rgbs"], s["depths"], s["intrs"], s["extrs"], frames=(0,))
    same = reproject_views(s["rgbs"], s["depths"], s["intrs"], s["extrs"], frames=(0,), depths_conf=conf)  # no threshold: the map is unused
    cut = reproject_views(s["rgbs"], s["depths"], s["intrs"], s["extrs"], frames=(0,), depths_conf=conf, conf_thresh=0.5)
    assert torch.equal(plain[2], same[2]) and int((cut[2] >= 0).sum()) < int((plain[2] >= 0).sum())
    won = cut[2][cut[2] >= 0].long()
    assert bool((conf[0, :, 0, 0].reshape(-1)[won] > 0.5).all())
    fat = reproject_views(s["rgbs"], s["depths"], s["intrs"], s["extrs"], frames=(0,), splat=3)
    assert M.splats[-1] == (0, True, 3) and int((fat[2] >= 0).sum()) > int((plain[2] >= 0).sum())


def _records(rows):
    rec = np.zeros((len(rows), len(rows[0]), R.WORDS), np.int64)
    for v, row in enumerate(rows):
        for f, d in enumerate(row):
            rec[v, f] = R.record_words(d)
    return torch.from_numpy(rec)


def test_report_arithmetic_and_the_summary_rules():
    from mvtracker_amd import ReprojectionReport
    base = {R.N: 100, R.COVERED: 40, R.SSE: 30000, R.SAE: 1500, R.SSE_COV: 12000, R.SAE_COV: 600, R.SSIM: 25.0, R.SSIM_COV: 20.0, R.N_DEPTH: 32,
            R.N_CLOSE: 8, R.DEPTH_SAE: 6.4, R.DEPTH_SAE_CLOSE: 0.2}
    exact = {**base, R.SSE: 0, R.SAE: 0, R.SSE_COV: 0, R.SAE_COV: 0, R.SSIM: 100.0, R.SSIM_COV: 40.0}
    empty = {**base, R.COVERED: 0, R.SSE_COV: 0, R.SAE_COV: 0, R.SSIM_COV: 0.0, R.N_DEPTH: 0, R.N_CLOSE: 0, R.DEPTH_SAE: 0.0, R.DEPTH_SAE_CLOSE: 0.0}
    worse = {**base, R.SSE: 60000}
    rep = ReprojectionReport(_records([[base, exact, worse], [exact, exact, exact], [empty, base, base]]), frames=(0, 1, 2))
    assert rep.mse.dtype == torch.float64 and rep.mse.shape == (3, 3)
    assert rep.mse[0].tolist() == [100.0, 0.0, 200.0] and rep.mae[0, 0] == 5.0 and rep.coverage[0, 0] == 0.4 and rep.ssim[0, 0] == 0.25
    assert rep.psnr[0, 0] == 10 * np.log10(255.0 ** 2 / 100.0) and rep.psnr[0, 1] == float("inf")
    assert rep.mse_covered[0, 0] == 100.0 and rep.mae_covered[0, 0] == 5.0 and rep.ssim_covered[0, 0] == 0.5
    assert rep.depth_pixels[0, 0] == 32 and rep.depth_close_fraction[0, 0] == 0.25 and rep.depth_mae[0, 0] == 0.2 and rep.depth_mae_close[0, 0] == 0.025
    assert torch.isnan(rep.mse_covered[2, 0]) and torch.isnan(rep.depth_close_fraction[2, 0]) and rep.coverage[2, 0] == 0
    s = rep.summary()
    assert s["frame_count"] == 3 and set(s) == set(rep.FIGURES) | {"frame_count"}
    assert s["mse"][0].tolist() == [100.0, 0.0, 100.0] and s["mse"][1][0] == np.std([100.0, 0.0, 200.0])
    finite = [10 * np.log10(255.0 ** 2 / 100.0), 10 * np.log10(255.0 ** 2 / 200.0)]  # compare_videos: infinite PSNRs are left out ...
    assert abs(float(s["psnr"][0][0]) - np.mean(finite)) < 1e-12 and abs(float(s["psnr"][1][0]) - np.std(finite)) < 1e-12
    assert s["psnr"][0][1] == 0 and s["psnr"][1][1] == 0  # ... and with none left the mean is 0
    table = rep.table("icp")
    assert len(table.split("\n")) == 2 + 3 and "PSNR" in table and "icp" in table
    with pytest.raises(ValueError):
        ReprojectionReport(torch.zeros(3, 2, R.WORDS, dtype=torch.int64), frames=(0, 1, 2))


def test_report_on_the_mock_is_the_restatement(monkeypatch):
    from mvtracker_amd import ReprojectionCheck, reproject_views, reprojection_report
    M.install(monkeypatch)
    s = _clip()
    ck = ReprojectionCheck(frames=(1, 0), sources="all", depth_tol=0.1)
    rep = reprojection_report(s["rgbs"], s["depths"], s["intrs"], s["extrs"], ck)
    assert M.calls == ["reproject_clear"] + ["reproject_splat_depths", "reproject_resolve"] * 2 + ["photometric_score"]
    color, depth, index = reproject_views(s["rgbs"], s["depths"], s["intrs"], s["extrs"], frames=(1, 0), sources="all")
    assert rep.records.shape == (3, 2, R.WORDS) and rep.frames == (1, 0)
    for v in range(3):
        for fi, t in enumerate((1, 0)):
            want = R.score(color[0, v, fi].numpy(), s["rgbs"][0, v, t].numpy(), index[0, v, fi].numpy(), depth[0, v, fi, 0].numpy(),
                           s["depths"][0, v, t, 0].numpy(), 0.1)
            assert np.array_equal(rep.records[v, fi].numpy(), R.record_words(want))
    assert bool((rep.depth_close_fraction > 0.5).all())  # "all": a view's own points land on their own pixels


# ------------------------------------------------------------------------------------------------------------------ wiring
class FakeModel(torch.nn.Module):
    S = 4

    def forward(self, rgbs, depths=None, query_points=None, intrs=None, extrs=None, **kw):
        self.seen = dict(depths=depths, query_points=query_points, extrs=extrs, kw=kw)
        return {"traj_e": torch.zeros(1, rgbs.shape[2], query_points.shape[1], 3), "vis_e": torch.zeros(1, rgbs.shape[2], query_points.shape[1])}


@pytest.fixture()
def wired(monkeypatch):
    from mvtracker_amd import CameraAlignment, EvaluationPredictor, hip
    M.install(monkeypatch)
    sc = Cs.scene(3, 16, 24)
    sc["extrs"] = Cs.perturbed(sc["extrs"], 1, Cs.rigid(0.8, (0.3, -0.5, 0.8), (0.02, -0.01, 0.015)))
    c = {k: torch.from_numpy(v) for k, v in sc.items()}
    c["rgbs"] = torch.from_numpy(np.random.default_rng(2).integers(0, 256, size=(1, 3, 2, 3, 16, 24), dtype=np.uint8))
    c["query_points"] = torch.tensor([[[0.0, 0.1, 0.2, 0.0], [1.0, -0.3, 0.4, 0.0]]])
    pred = EvaluationPredictor(FakeModel(), interp_shape=None, grid_size=2)
    order = []
    import types
    for name in [n for n in dir(hip) if n[0] != "_" and isinstance(getattr(hip, n), types.FunctionType)]:  # every entry, real or mocked
        if name in ("require_device", "device_guard", "guarded"):
            continue
        real = getattr(hip, name)
        monkeypatch.setattr(hip, name, (lambda n, f: lambda *a_, **k: (order.append(n), f(*a_, **k))[1])(name, real))
    return pred, c, CameraAlignment(max_distance=0.3, max_iterations=3, sweeps=1, normal_max_edge=1.0), order


def _call(pred, c, **kw):
    return pred(rgbs=c["rgbs"], depths=c["depths"], query_points_3d=c["query_points"], intrs=c["intrs"], extrs=c["extrs"], **kw)


def test_none_keeps_the_launch_sequence(wired):
    from mvtracker_amd import ReprojectionCheck
    pred, c, a, order = wired
    _call(pred, c)
    plain, plain_seen = list(order), pred.model.seen
    assert plain and not any(n.startswith("reproject") or n.startswith("photometric") for n in plain)
    del order[:]
    _call(pred, c, reprojection_check=None)
    assert order == plain and M.calls == [] and "reprojection_check" not in pred.model.seen["kw"]
    assert pred.last_reprojection_report is None and pred.last_reprojection_report_before is None
    with pytest.raises(ValueError, match="ReprojectionCheck"):
        _call(pred, c, reprojection_check="yes")
    # with a check: its entries come first, the rest of the sequence and everything the model sees are what they were
    del order[:]
    _call(pred, c, reprojection_check=ReprojectionCheck())
    own = ["invert_cameras", "reproject_clear", "reproject_splat_depths", "reproject_resolve", "photometric_score"]
    assert order[:len(own)] == own and order[len(own):] == plain
    assert all(torch.equal(pred.model.seen[k], plain_seen[k]) for k in ("depths", "query_points", "extrs"))
    assert pred.last_reprojection_report.records.shape == (3, 1, R.WORDS) and pred.last_reprojection_report_before is None
    _call(pred, c)
    assert pred.last_reprojection_report is None


def test_before_and_after_reports_with_camera_alignment(wired):
    from mvtracker_amd import ReprojectionCheck, align_cameras, compare_reports, reprojection_report
    pred, c, a, order = wired
    ck = ReprojectionCheck(frames=(0, 1), depth_tol=0.1)
    corr = align_cameras(c["depths"], c["intrs"], c["extrs"], a)
    want_before = reprojection_report(c["rgbs"], c["depths"], c["intrs"], c["extrs"], ck)
    want_after = reprojection_report(c["rgbs"], c["depths"], c["intrs"], corr.apply(c["extrs"]), ck)
    del order[:]
    _call(pred, c, camera_alignment=a, reprojection_check=ck)
    before, after = pred.last_reprojection_report_before, pred.last_reprojection_report
    assert torch.equal(before.records, want_before.records) and torch.equal(after.records, want_after.records)
    assert not torch.equal(before.records, after.records)
    assert order.index("align_solve") < order.index("reproject_clear") and order.count("photometric_score") == 2
    assert torch.equal(pred.model.seen["extrs"], corr.apply(c["extrs"])) and torch.equal(pred.model.seen["depths"], c["depths"])
    text = compare_reports(before, after)
    assert len(text.split("\n")) == 2 + 3 and "dPSNR" in text
    _call(pred, c, camera_alignment=corr, reprojection_check=ck)  # a ready correction: both reports too
    assert torch.equal(pred.last_reprojection_report_before.records, want_before.records)
    assert torch.equal(pred.last_reprojection_report.records, want_after.records)


def test_demo_flags_parse():
    import demo_amd
    ap = demo_amd.build_parser()
    a = ap.parse_args(["--synthetic"])
    assert not a.reprojection_check and demo_amd.reprojection_check_from_args(a) is None
    assert (a.reproject_frames, a.reproject_sources, a.reproject_splat, a.reproject_depth_tol) == ([0], "others", 1, 0.05)
    a = ap.parse_args("--synthetic --reprojection-check --reproject-frames 0 3 --reproject-sources all --reproject-splat 3 "
                      "--reproject-depth-tol 0.1".split())
    c = demo_amd.reprojection_check_from_args(a)
    assert (c.frames, c.sources, c.splat, c.depth_tol) == ((0, 3), "all", 3, 0.1)


# ------------------------------------------------------------------------------------------------------------------ the yardstick
def test_the_restatement_equals_the_recorded_reference():
    """Every pixel of every view: the restatement's render of the recorded fp32 points is the reference's image, and the report's
    mse / psnr / mae from the restatement's integer sums are the reference's compute_mse / compute_psnr / compute_mae."""
    from mvtracker_amd import ReprojectionReport
    g = np.load(GOLDEN)
    V, H, W = 3, 24, 40
    sc = Cs.scene(V, H, W)
    assert all(np.array_equal(g[k], sc[k]) for k in ("depths", "intrs", "extrs"))  # the fixture is the case the tests build
    for tv in range(V):
        color, depth, index = R.render_points(g[f"points_{tv}"], g[f"point_colors_{tv}"], g["intrs"][0, tv, 0], g["extrs"][0, tv, 0], H, W,
                                              float(g["min_depth"][0]))
        assert np.array_equal(color, g[f"color_{tv}"]) and 0.4 < (index >= 0).mean() < 0.5
        assert ((color != 0).all(0) == (index >= 0)).all() and ((depth > 0) == (index >= 0)).all()
        rec = R.score(color, g["colors"][tv], index, depth, g["depths"][0, tv, 0, 0], 0.05)
        rep = ReprojectionReport(_records([[rec]]), frames=(0,))
        mse, psnr, mae = g[f"scores_{tv}"]
        assert abs(float(rep.mse[0, 0]) - mse) <= 1e-12 * mse and abs(float(rep.psnr[0, 0]) - psnr) <= 1e-12 * psnr
        assert abs(float(rep.mae[0, 0]) - mae) <= 1e-12 * mae


def test_the_ssim_restatement_is_stable_under_its_own_summation_order():
    """A check of the yardstick alone (it says nothing about the kernels): the GPU bar on the SSIM sums is 1e-10 N, and two
    summation orders of the restatement differ by far less; an identical pair gives a map of exactly 1."""
    rng = np.random.default_rng(0)
    a, b = rng.integers(0, 256, size=(2, 3, 24, 40), dtype=np.uint8)
    assert abs(R.gaussian_taps().sum() - 1) < 1e-15 and abs(R.gaussian_taps()[0] - 1.0e-3) < 1e-4  # the smallest tap weight
    full = R.ssim_map(a, b)
    assert abs(full.sum() - full[::-1, ::-1].sum()) < 1e-12 * full.size
    same = R.ssim_map(a, a)
    assert same.sum() == same.size and (same == 1.0).all()
