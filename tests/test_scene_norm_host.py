"""Scene normalisation, host side (no GPU): the numpy restatement (tests/scene_norm_ref.py) against the reference's recorded values
(tests/golden/scene_norm.npz), SceneTransform's rules, and the predictor / streaming wiring on mocked kernels
(tests/hip_mock_scene.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hip_mock_scene  # noqa: E402
import scene_norm_ref as R  # noqa: E402
from mvtracker_amd import synth  # noqa: E402

V, T, H, W = 3, 2, 37, 53
CASES = [(c, r) for c in (1, 2, 3) for r in ("cam", "rad")]


@pytest.fixture(scope="module")
def fx(golden):
    g = golden("scene_norm")
    clip = synth.make_clip(int(g["clip_seed"][0]), V=V, T=T, H=H, W=W, N=4, invalid_frac=0.02)
    return g, clip


def conf_of(g, case):
    return {1: g["conf"], 2: g["conf_case2"], 3: None, 4: g["conf_case4"]}[case]


def restated(g, clip, case, rule):
    return R.auto_scene_normalization(clip["depths"][0], clip["intrs"][0], clip["extrs"][0], conf_of(g, case), float(g["conf_thresh"][0]),
                                      float(g["target_radius"][0]), rule == "cam")


def test_fixture_is_what_the_issue_asks(fx):
    g, clip = fx
    assert g["conf"].shape == (V, T, 1, H, W) and clip["depths"].shape == (1, V, T, 1, H, W)
    thr = np.float32(g["conf_thresh"][0])
    per_view = lambda c: ((c[:, 0, 0] > thr) & (clip["depths"][0][:, 0, 0] > 0)).reshape(V, -1).sum(1)
    assert all(1100 < n < 1500 for n in per_view(g["conf"]))
    assert per_view(g["conf_case2"])[1] == 99 and per_view(g["conf_case4"]).sum() == 0
    assert int(g["c2_cam_M"][0]) < int(g["c1_cam_M"][0]) < int(g["c3_cam_M"][0]) and int(g["c4_raises"][0]) == 1
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "scene_norm.npz")) < 512 * 1024


@pytest.mark.parametrize("case,rule", CASES)
def test_restatement_reproduces_the_reference(fx, case, rule):
    g, clip = fx
    m, k = restated(g, clip, case, rule), f"c{case}_{rule}_"
    ext = float(g[k + "extent"][0])
    assert m["M"] == int(g[k + "M"][0]) and m["z_rank"] == int(g[k + "z_rank"][0])  # integers: equal
    d = {"scale": abs(m["scale"] - float(g[k + "scale"][0])) / float(g[k + "scale"][0]),
         "centroid": R.rel_inf(m["centroid"], g[k + "centroid"], ext),
         "floor_z": R.rel_inf(m["floor_z"], g[k + "floor_z"], ext),
         "translate": R.rel_inf(m["translate"], g[k + "translate"], ext),
         "zc_order": R.rel_inf(np.array([m["z_lo"], m["z_hi"]]) - m["centroid"][2], g[k + "zc_order"], ext)}
    if rule == "rad":
        assert m["r_rank"] == int(g[k + "r_rank"][0])
        d["r_order"] = R.rel_inf(np.array([m["r_lo"], m["r_hi"]]), g[k + "r_order"], ext)
    for name, v in d.items():
        assert v <= float(g[k + "dref_" + name][0]) < 1e-6, (name, v)  # d_ref is this distance (and it is rounding-sized)


def test_restatement_case_4_raises_and_case_2_skips_a_view(fx):
    g, clip = fx
    with pytest.raises(RuntimeError, match="Too few valid points"):
        restated(g, clip, 4, "cam")
    a, b = restated(g, clip, 1, "cam"), restated(g, clip, 2, "cam")
    assert a["M"] - b["M"] > 1000 and abs(a["scale"] - b["scale"]) > 1e-4  # the 99 pixels are not in the pool either


@pytest.mark.parametrize("name", ["auto", "manual", "identity"])
def test_restated_transform_reproduces_the_reference(fx, name):
    g, clip = fx
    k = f"xf_{name}_"
    out = R.transform_scene(float(g[k + "scale"][0]), g[k + "rotation"], g[k + "translation"], clip["depths"][0], clip["extrs"][0], g["queries"],
                            g["tracks"])
    for part, got in zip(("depths", "extrs", "queries", "tracks"), out):
        assert got.shape == g[k + part].shape
        assert R.rel_inf(got, g[k + part]) <= float(g[k + "dref_" + part][0]) <= 1.2e-7, part
    if name == "identity":
        for part, src in (("depths", clip["depths"][0]), ("extrs", clip["extrs"][0]), ("queries", g["queries"]), ("tracks", g["tracks"])):
            assert np.array_equal(g[k + part], src)


# ------------------------------------------------------------------------------------------------------------------ SceneTransform
def test_scene_transform_validation():
    from mvtracker_amd import SceneTransform, scene
    assert SceneTransform is scene.SceneTransform
    t = SceneTransform(2.0)
    assert np.array_equal(t.rotation, np.eye(3)) and np.array_equal(t.translation, np.zeros(3)) and t.scale == 2.0
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="scale"):
            SceneTransform(bad)
    with pytest.raises(ValueError, match="orthonormal"):
        SceneTransform(1.0, np.eye(3) * 1.01)
    SceneTransform(1.0, np.eye(3) * 1.0004)  # inside the reference's 1e-3
    with pytest.raises(ValueError):
        SceneTransform(1.0, np.eye(4))
    with pytest.raises(ValueError):
        SceneTransform(1.0, None, (0.0, float("nan"), 0.0))
    assert SceneTransform(1.5, torch.eye(3), torch.tensor([1.0, 2.0, 3.0])) == SceneTransform(1.5, None, (1.0, 2.0, 3.0))


def test_inverse_composes_to_identity(fx):
    from mvtracker_amd import SceneTransform
    g, _ = fx
    t = SceneTransform(float(g["xf_manual_scale"][0]), g["xf_manual_rotation"], g["xf_manual_translation"])
    i = t.inverse()
    x = np.random.default_rng(0).uniform(-5, 5, size=(100, 3))
    fwd = lambda tr, p: tr.translation + (tr.scale * p) @ tr.rotation.T
    # (the fixture's rotation is an fp32 rounding of an orthonormal matrix: R^T R is the identity to 1e-7, and so is the round trip)
    assert np.abs(fwd(i, fwd(t, x)) - x).max() < 1e-6 and np.abs(fwd(t, fwd(i, x)) - x).max() < 1e-6
    e = SceneTransform(3.0, None, (1.0, -2.0, 0.5))
    assert np.abs(fwd(e.inverse(), fwd(e, x)) - x).max() < 1e-14  # exact rotation: fp64 rounding only
    ii = e.inverse().inverse()
    assert abs(ii.scale - e.scale) < 1e-15 and np.abs(ii.translation - e.translation).max() < 1e-15


def test_apply_on_mocked_kernels_equals_the_restatement(fx, monkeypatch):
    from mvtracker_amd import SceneTransform
    hip_mock_scene.install(monkeypatch)
    g, clip = fx
    t = SceneTransform(float(g["xf_manual_scale"][0]), g["xf_manual_rotation"], g["xf_manual_translation"])
    d, e, q, tr = (torch.from_numpy(a) for a in (clip["depths"], clip["extrs"], g["queries"][None], g["tracks"][None]))
    out = t.apply(depths=d, extrs=e, query_points=q, tracks=tr)
    assert [tuple(o.shape) for o in out] == [tuple(a.shape) for a in (d, e, q, tr)]  # the leading 1 is kept
    for part, o in zip(("depths", "extrs", "queries", "tracks"), out):
        assert R.rel_inf(o[0].numpy(), g["xf_manual_" + part]) <= 4 * float(g["xf_manual_dref_" + part][0])
    assert t.apply() == (None, None, None, None) and t.apply(tracks=tr)[:3] == (None, None, None)
    back = t.restore_tracks(out[3])
    assert (back - tr).abs().max() < 1e-5
    with pytest.raises(ValueError):
        t.apply(tracks=q)
    with pytest.raises(ValueError):
        t.apply(query_points=tr)


@pytest.mark.parametrize("case,rule", CASES)
def test_auto_on_mocked_kernels(fx, case, rule, monkeypatch):
    from mvtracker_amd import auto_scene_normalization
    hip_mock_scene.install(monkeypatch)
    g, clip = fx
    conf = conf_of(g, case)
    m = restated(g, clip, case, rule)
    t = auto_scene_normalization(*(torch.from_numpy(clip[k]) for k in ("depths", "intrs", "extrs")),
                                 depths_conf=None if conf is None else torch.from_numpy(conf)[None], conf_thresh=float(g["conf_thresh"][0]),
                                 target_radius=float(g["target_radius"][0]), rescale_by_camera_radius=rule == "cam")
    # (the mock unprojects in fp32 like the kernel: the host arithmetic is what this checks, to a bound far above both)
    assert abs(t.scale - m["scale"]) / m["scale"] < 1e-5 and np.abs(t.translation - m["translate"]).max() < 1e-4
    assert np.array_equal(t.rotation, np.eye(3))


def test_auto_errors_and_signature(fx, monkeypatch):
    import inspect
    from mvtracker_amd import auto_scene_normalization
    hip_mock_scene.install(monkeypatch)
    g, clip = fx
    d, i, e = (torch.from_numpy(clip[k]) for k in ("depths", "intrs", "extrs"))
    with pytest.raises(RuntimeError, match="Too few valid points for normalization."):
        auto_scene_normalization(d, i, e, depths_conf=torch.from_numpy(g["conf_case4"])[None])
    bad = d.clone()
    bad[0, 0, 0, 0, 5, 5] = float("inf")
    with pytest.raises(ValueError, match="not finite"):
        auto_scene_normalization(bad, i, e)
    with pytest.raises(ValueError):
        auto_scene_normalization(d[0], i, e)
    with pytest.raises(ValueError, match="frame"):
        auto_scene_normalization(d, i, e, frame=T)
    p = inspect.signature(auto_scene_normalization).parameters
    assert list(p) == ["depths", "intrs", "extrs", "depths_conf", "conf_thresh", "target_radius", "rescale_by_camera_radius", "frame"]
    assert (p["conf_thresh"].default, p["target_radius"].default, p["rescale_by_camera_radius"].default, p["frame"].default) == (4.8, 6.3, True, 0)


# ------------------------------------------------------------------------------------------------------------------ wiring
class FakeSession:
    def __init__(self, queries):
        self.queries, self.pushed = [queries], []
        self.nan_flag = torch.zeros(1, dtype=torch.int32)

    def add_queries(self, q):
        self.queries.append(q)

    def _res(self, a, b):
        n = sum(q.shape[1] for q in self.queries)
        g = torch.Generator().manual_seed(100 + a)
        return {"frames": (a, b), "traj_e": torch.randn(1, b - a, n, 3, generator=g), "vis_e": torch.rand(1, b - a, n, generator=g)}

    def push(self, rgbs, depths, intrs, extrs):
        self.pushed.append((depths, extrs))
        n = sum(d.shape[2] for d, _ in self.pushed)
        return self._res(n - depths.shape[2], n - 1)

    def finish(self):
        n = sum(d.shape[2] for d, _ in self.pushed)
        return self._res(n - 1, n)


class FakeModel(torch.nn.Module):
    """Records what the predictor hands to the model; its tracks are a seeded draw."""
    S = 4

    def forward(self, rgbs, depths=None, query_points=None, intrs=None, extrs=None, **kw):
        self.seen = dict(depths=depths, query_points=query_points, extrs=extrs)
        g = torch.Generator().manual_seed(7)
        n, t = query_points.shape[1], rgbs.shape[2]
        return {"traj_e": torch.randn(1, t, n, 3, generator=g) * 3, "vis_e": torch.rand(1, t, n, generator=g)}

    def open_stream(self, query_points, iters=4, ring_blocks=3):
        self.session = FakeSession(query_points)
        return self.session


@pytest.fixture()
def wired(fx, monkeypatch):
    from mvtracker_amd import EvaluationPredictor, SceneTransform
    hip_mock_scene.install(monkeypatch)
    g, _ = fx
    clip = synth.make_clip(3, V=2, T=6, H=16, W=24, N=5)
    c = {k: torch.from_numpy(v) for k, v in clip.items()}
    pred = EvaluationPredictor(FakeModel(), interp_shape=None, grid_size=2)
    xf = SceneTransform(float(g["xf_manual_scale"][0]), g["xf_manual_rotation"], g["xf_manual_translation"])
    return pred, c, xf


def _call(pred, c, **kw):
    return pred(rgbs=c["rgbs"], depths=c["depths"], query_points_3d=c["query_points"], intrs=c["intrs"], extrs=c["extrs"], **kw)


def test_forward_hands_the_model_the_applied_inputs(wired):
    pred, c, xf = wired
    out = _call(pred, c, scene_transform=xf)
    d, e, q, _ = xf.apply(depths=c["depths"], extrs=c["extrs"], query_points=c["query_points"])
    seen = pred.model.seen
    n = c["query_points"].shape[1]
    assert torch.equal(seen["depths"], d) and torch.equal(seen["extrs"], e) and torch.equal(seen["query_points"][:, :n], q)
    assert seen["query_points"].shape[1] == n + 2 * 2 * 2  # + the support grid, built from the transformed depths and cameras
    plain = FakeModel()(c["rgbs"], query_points=seen["query_points"])
    assert torch.equal(out["traj_e"], xf.restore_tracks(plain["traj_e"][:, :, :n]))
    assert torch.equal(out["vis_e_as_prob"], plain["vis_e"][:, :, :n]) and pred.last_scene_transform is xf


def test_forward_without_a_transform_calls_no_scene_entry(wired):
    pred, c, xf = wired
    del hip_mock_scene.calls[:]
    out = _call(pred, c)
    assert hip_mock_scene.calls == [] and pred.last_scene_transform is None
    assert torch.equal(pred.model.seen["depths"], c["depths"]) and torch.equal(pred.model.seen["extrs"], c["extrs"])
    n = c["query_points"].shape[1]
    assert torch.equal(out["traj_e"], FakeModel()(c["rgbs"], query_points=pred.model.seen["query_points"])["traj_e"][:, :, :n])
    _call(pred, c, scene_transform=xf)
    assert hip_mock_scene.calls == ["scene_apply", "scene_tracks"]
    with pytest.raises(ValueError, match="scene_transform"):
        _call(pred, c, scene_transform="manual")


def test_forward_auto_uses_the_raw_inputs_and_the_confidence(wired):
    from mvtracker_amd import auto_scene_normalization
    pred, c, _ = wired
    pred.interp_shape = (8, 12)  # the transform must come from the frames as given, not the resized ones
    conf = (c["depths"] > c["depths"].median()).float() * 10
    _call(pred, c, scene_transform="auto", depths_conf=conf)
    want = auto_scene_normalization(c["depths"], c["intrs"], c["extrs"], depths_conf=conf)
    assert pred.last_scene_transform == want
    assert want != auto_scene_normalization(c["depths"], c["intrs"], c["extrs"])
    assert pred.model.seen["depths"].shape[-2:] == (8, 12)


def test_stream_transforms_blocks_and_restores_chunks(wired):
    pred, c, xf = wired
    st = pred.open_stream(c["query_points"], scene_transform=xf)
    assert pred.last_scene_transform is xf
    sess = pred.model.session
    assert torch.equal(sess.queries[0], xf.apply(query_points=c["query_points"])[2])
    outs = []
    for t0 in (0, 3):
        outs.append(st.push(*(c[k][:, :, t0:t0 + 3] for k in ("rgbs", "depths", "intrs", "extrs"))))
    outs.append(st.finish())
    d, e, _, _ = xf.apply(depths=c["depths"], extrs=c["extrs"])
    assert torch.equal(torch.cat([p[0] for p in sess.pushed], 2), d) and torch.equal(torch.cat([p[1] for p in sess.pushed], 2), e)
    assert len(sess.queries) == 2  # the support grid, from the first (transformed) frame
    n = c["query_points"].shape[1]
    for o, (a, b) in zip(outs, ((0, 2), (3, 5), (5, 6))):
        assert o["frames"] == (a, b)
        raw = sess._res(a, b)
        assert torch.equal(o["traj_e"], xf.restore_tracks(raw["traj_e"][:, :, :n])) and torch.equal(o["vis_e_as_prob"], raw["vis_e"][:, :, :n])


def test_stream_refuses_auto_and_none_calls_nothing(wired):
    pred, c, _ = wired
    with pytest.raises(ValueError, match="auto_scene_normalization"):
        pred.open_stream(c["query_points"], scene_transform="auto")
    del hip_mock_scene.calls[:]
    st = pred.open_stream(c["query_points"])
    st.push(*(c[k][:, :, :3] for k in ("rgbs", "depths", "intrs", "extrs")))
    st.finish()
    assert hip_mock_scene.calls == [] and pred.last_scene_transform is None
