"""The predictor's stages, host side (no GPU), on mocked kernels and a spy model: the order of the stages of ``forward`` and what each
is handed, the same stages in a streaming session's ``push``, the batched lift of the support points on inputs where fp32 is exact,
and the one NaN guard."""
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_align_cases as Cs  # noqa: E402
import hip_mock_overlay  # noqa: E402
import hip_mock_reproject  # noqa: E402
from mvtracker_amd import synth  # noqa: E402

V, T, H, W = 2, 6, 16, 24


class SpySession:
    def __init__(self, queries, nan):
        self.queries, self.pushed = [queries], []
        self.nan_flag = torch.full((1,), nan, dtype=torch.int32)

    def add_queries(self, q):
        self.queries.append(q)

    def _res(self, a, b):
        n = sum(q.shape[1] for q in self.queries)
        return {"frames": (a, b), "traj_e": torch.zeros(1, b - a, n, 3), "vis_e": torch.zeros(1, b - a, n)}

    def push(self, rgbs, depths, intrs, extrs):
        self.pushed.append(dict(rgbs=rgbs, depths=depths, intrs=intrs, extrs=extrs))
        n = sum(p["depths"].shape[2] for p in self.pushed)
        return self._res(n - depths.shape[2], n - 1)

    def finish(self):
        n = sum(p["depths"].shape[2] for p in self.pushed)
        return self._res(n - 1, n)


class SpyModel(torch.nn.Module):
    """Records what the predictor hands to the model; every track stays at its query's own point, in the world the model is given."""
    S = 4

    def __init__(self, events=None, nan=()):
        super().__init__()
        self.events, self.nan, self.calls = [] if events is None else events, list(nan), 0

    def forward(self, rgbs, depths=None, query_points=None, intrs=None, extrs=None, **kw):
        self.events.append("model")
        self.seen = dict(rgbs=rgbs, depths=depths, query_points=query_points, intrs=intrs, extrs=extrs, kw=kw)
        self.last_nan_flag = torch.full((1,), self.nan[self.calls] if self.calls < len(self.nan) else 0, dtype=torch.int32)
        self.calls += 1
        n_frames, n = rgbs.shape[2], query_points.shape[1]
        return {"traj_e": query_points[:, None, :, 1:].repeat(1, n_frames, 1, 1), "vis_e": torch.ones(1, n_frames, n)}

    def open_stream(self, query_points, iters=4, ring_blocks=3):
        self.session = SpySession(query_points, self.nan[0] if self.nan else 0)
        return self.session


def _call(pred, c, **kw):
    return pred(rgbs=c["rgbs"], depths=c["depths"], query_points_3d=c["query_points"], intrs=c["intrs"], extrs=c["extrs"], **kw)


# ------------------------------------------------------------------------------------------------------------------ 1. stage order
@pytest.fixture()
def rendered(monkeypatch):
    """The camera-alignment tests' rendered scene (its views agree, so an alignment converges) with one view's cameras off and some
    flying pixels for the cleaning to remove."""
    hip_mock_reproject.install(monkeypatch)
    hip_mock_overlay.install(monkeypatch)
    monkeypatch.setattr("mvtracker_amd.scene.MIN_POINTS", 10)
    sc = Cs.scene(V, H, W, T=T)
    sc["extrs"] = Cs.perturbed(sc["extrs"], 1, Cs.rigid(0.8, (0.3, -0.5, 0.8), (0.02, -0.01, 0.015)))
    d = sc["depths"]
    rng = np.random.default_rng(5)
    d[(rng.uniform(size=d.shape) < 0.03) & (d > 0)] *= 0.6
    c = {k: torch.from_numpy(v) for k, v in sc.items()}
    c["rgbs"] = torch.from_numpy(rng.integers(0, 256, size=(1, V, T, 3, H, W), dtype=np.uint8))
    c["query_points"] = torch.tensor([[[0.0, 0.1, 0.2, 0.0], [1.0, -0.3, 0.4, 0.0], [3.0, 0.4, 0.3, 0.6]]])
    return c


def _recorders(monkeypatch, events):
    """name -> list of (args, kwargs, result) of every call of the six stage entries, which still run (on the mocked kernels)."""
    from mvtracker_amd import align, clean, hip, overlay, reproject, scene
    seen = {}
    for name, mod, attr in (("clean", clean, "clean_depths"), ("align", align, "align_cameras"), ("report", reproject, "reprojection_report"),
                            ("auto", scene, "auto_scene_normalization"), ("resize", hip, "resize_nearest"),
                            ("overlay", overlay, "render_track_overlays")):
        def wrap(name=name, real=getattr(mod, attr)):
            def w(*a, **k):
                events.append(name)
                out = real(*a, **k)
                seen.setdefault(name, []).append((a, k, out))
                return out
            return w
        monkeypatch.setattr(mod, attr, wrap())
    return seen


def test_stage_order_and_what_each_stage_is_handed(rendered, monkeypatch):
    from mvtracker_amd import CameraAlignment, DepthCleaning, EvaluationPredictor, ReprojectionCheck, TrackOverlay
    c, events = rendered, []
    seen = _recorders(monkeypatch, events)
    pred = EvaluationPredictor(SpyModel(events), interp_shape=(8, 12), grid_size=2)
    out = _call(pred, c, depth_cleaning=DepthCleaning(nb_neighbors=8, std_ratio=1.0), reprojection_check=ReprojectionCheck(frames=(0, 1), depth_tol=0.1),
                camera_alignment=CameraAlignment(max_distance=0.3, max_iterations=3, sweeps=1, normal_max_edge=1.0), scene_transform="auto",
                track_overlay=TrackOverlay(pad=2))
    assert events == ["clean", "align", "report", "report", "auto", "resize", "resize", "model", "overlay"]
    raw = tuple(c["depths"].shape)
    cleaned = seen["clean"][0][2][0]
    assert tuple(cleaned.shape) == raw and int((cleaned != c["depths"]).sum()) > 0  # (the cleaning removed something)
    corrected = pred.last_camera_correction.apply(c["extrs"])
    assert pred.last_camera_correction is seen["align"][0][2] and not torch.equal(corrected, c["extrs"])
    # the alignment sees the cleaned depths with the caller's cameras
    a = seen["align"][0][0]
    assert torch.equal(a[0], cleaned) and torch.equal(a[1], c["intrs"]) and torch.equal(a[2], c["extrs"])
    # "before": the uncorrected cameras; "after": the corrected ones; both the cleaned depths at raw resolution
    (before, _, rep_before), (after, _, rep_after) = seen["report"]
    assert torch.equal(before[3], c["extrs"]) and torch.equal(after[3], corrected)
    assert all(torch.equal(r[1], cleaned) and torch.equal(r[2], c["intrs"]) and tuple(r[0].shape[-2:]) == (H, W) for r in (before, after))
    assert pred.last_reprojection_report_before is rep_before and pred.last_reprojection_report is rep_after
    # the normalisation is computed from the cleaned depths and the corrected cameras, at raw resolution
    auto, auto_kw, xf = seen["auto"][0]
    assert torch.equal(auto[0], cleaned) and torch.equal(auto[1], c["intrs"]) and torch.equal(auto[2], corrected) and auto_kw == {"depths_conf": None}
    assert pred.last_scene_transform is xf and xf.scale != 1.0
    # frames first, then depths, from the raw resolution; the model gets the resized clip with rescaled intrinsics
    (r0, _, _), (r1, _, _) = seen["resize"]
    assert r0[2:] == (V * T * 3, H, W, 8, 12) and r1[2:] == (V * T, H, W, 8, 12) and r0[0].dtype == torch.float32
    assert torch.equal(r1[0], xf.apply(depths=cleaned)[0])
    m = pred.model.seen
    assert tuple(m["rgbs"].shape[-2:]) == tuple(m["depths"].shape[-2:]) == (8, 12) and torch.equal(m["extrs"], xf.apply(extrs=corrected)[1])
    assert torch.equal(m["intrs"][0, 0, 0, 0], c["intrs"][0, 0, 0, 0] * 0.5) and m["query_points"].shape[1] == 3 + V * 4
    # the overlay: the caller's own frames and cameras, the tracks as returned (in the caller's world), the thresholded visibility
    o = seen["overlay"][0][0]
    assert o[0].data_ptr() == c["rgbs"].data_ptr() and o[0].dtype == torch.uint8 and tuple(o[0].shape) == (V, T, 3, H, W)
    assert torch.equal(o[1], out["traj_e"][0]) and torch.equal(o[2], out["vis_e"][0]) and torch.equal(o[3], c["query_points"][0, :, 0])
    assert torch.equal(o[4], c["intrs"][0]) and torch.equal(o[5], corrected[0])
    world = c["query_points"][0, :, 1:]
    assert (o[1] - world).abs().max() < 1e-5 < (m["query_points"][0, :3, 1:] - world).abs().max()  # (the model's world is another)
    assert pred.last_track_overlay is seen["overlay"][0][2]


def test_every_option_off_runs_no_stage_entry(rendered, monkeypatch):
    from mvtracker_amd import EvaluationPredictor
    c, events = rendered, []
    _recorders(monkeypatch, events)
    pred = EvaluationPredictor(SpyModel(events), interp_shape=None, grid_size=2)
    _call(pred, c)
    assert events == ["model"]  # no clean, align, report, auto-normalise, overlay -- and no resize at interp_shape=None
    assert pred.model.seen["rgbs"].dtype == torch.uint8 and torch.equal(pred.model.seen["depths"], c["depths"])
    assert (pred.last_scene_transform, pred.last_camera_correction, pred.last_reprojection_report, pred.last_reprojection_report_before,
            pred.last_track_overlay) == (None,) * 5
    del events[:]
    pred.interp_shape = (8, 12)
    _call(pred, c)
    assert events == ["resize", "resize", "model"]


# ------------------------------------------------------------------------------------------------------------------ 2. the stream's stages
@pytest.mark.parametrize("interp_shape", [None, (8, 12)])
@pytest.mark.parametrize("uint8", [True, False])
def test_stream_blocks_go_through_the_stages_of_forward(monkeypatch, uint8, interp_shape):
    from mvtracker_amd import DepthCleaning, EvaluationPredictor, SceneTransform
    hip_mock_reproject.install(monkeypatch)
    clip = synth.make_clip(3, V=V, T=T, H=H, W=W, N=5, invalid_frac=0.02)
    d = clip["depths"]
    d[np.random.default_rng(5).uniform(size=d.shape) < 0.02] *= 0.6  # flying pixels
    c = {k: torch.from_numpy(v) for k, v in clip.items()}
    c["rgbs"] = c["rgbs"].to(torch.uint8) if uint8 else c["rgbs"].float()
    cleaning, xf, g = DepthCleaning(nb_neighbors=8, std_ratio=1.0), SceneTransform(2.0, None, (0.5, -1.0, 0.25)), 2
    pred = EvaluationPredictor(SpyModel(), interp_shape=interp_shape, grid_size=g)
    _call(pred, c, depth_cleaning=cleaning, scene_transform=xf)
    want = pred.model.seen
    assert want["rgbs"].dtype == (torch.uint8 if uint8 and interp_shape is None else torch.float32)
    assert not torch.equal(want["depths"], c["depths"]) and tuple(want["depths"].shape[-2:]) == ((H, W) if interp_shape is None else interp_shape)
    st = pred.open_stream(c["query_points"], scene_transform=xf, depth_cleaning=cleaning)
    for a, b in ((0, 2), (2, 5), (5, 6)):
        st.push(*(c[k][:, :, a:b] for k in ("rgbs", "depths", "intrs", "extrs")))
    st.finish()
    sess = pred.model.session
    for k in ("rgbs", "depths", "intrs", "extrs"):
        got = torch.cat([p[k] for p in sess.pushed], 2)
        assert got.dtype == want[k].dtype and torch.equal(got, want[k]), k
    n = c["query_points"].shape[1]
    assert len(sess.queries) == 2 and torch.equal(sess.queries[0], want["query_points"][:, :n])
    assert sess.queries[1].shape[1] == V * g * g and torch.equal(sess.queries[1], want["query_points"][:, n:n + V * g * g])


# ------------------------------------------------------------------------------------------------------------------ 3. the batched lift
LH, LW = 32, 48


@pytest.fixture()
def dyadic(monkeypatch):
    """A clip on which every product and sum of the lift is exact in fp32: depths in multiples of 1/4 below 4, focal lengths 8 and 4,
    principal points in whole pixels, rotations by quarter turns about the optical axis, translations in multiples of 1/2."""
    hip_mock_reproject.install(monkeypatch)
    rng = np.random.default_rng(7)
    depths = torch.from_numpy(rng.integers(4, 16, size=(1, V, 3, 1, LH, LW)).astype(np.float32) / 4)
    K = torch.tensor([[[8.0, 0, 24], [0, 8, 16], [0, 0, 1]], [[4.0, 0, 20], [0, 4, 12], [0, 0, 1]]])
    E = torch.tensor([[[1.0, 0, 0, 0.5], [0, 1, 0, -1.0], [0, 0, 1, 0]], [[0.0, -1, 0, 1.5], [1, 0, 0, 0.5], [0, 0, 1, 0]]])
    intrs, extrs = K[None, :, None].repeat(1, 1, 3, 1, 1), E[None, :, None].repeat(1, 1, 3, 1, 1)
    kinv = torch.linalg.inv(K.double()).float()[:, None].repeat(1, 3, 1, 1)
    Rt = E[:, :, :3].transpose(1, 2)
    einv = torch.cat([Rt, -(Rt @ E[:, :, 3:])], 2)[:, None].repeat(1, 3, 1, 1)
    assert torch.equal(kinv[0, 0], torch.tensor([[0.125, 0, -3], [0, 0.125, -2], [0, 0, 1]]))
    return depths, intrs, extrs, kinv, einv


def _restated_rows(pred, depths, vid, fid, x, y, kinv, einv):
    """Row by row through the per-camera form: ``_bilinear_sample_depth``, then ``_unproject``."""
    from mvtracker_amd.predictor import _bilinear_sample_depth
    rows = []
    for v, t, px, py in zip(vid, fid, x, y):
        pix = torch.tensor([[px, py]], dtype=torch.float32)
        z = _bilinear_sample_depth(depths[0, v, t, 0], pix[:, 0], pix[:, 1])
        rows.append(torch.cat([torch.tensor([[float(t)]]), pred._unproject(pix, z, kinv[v, t], einv[v, t])], 1))
    return torch.cat(rows, 0) if rows else torch.zeros(0, 4)


def test_uniform_rows_are_the_per_camera_lift_exactly(dyadic, monkeypatch):
    from mvtracker_amd import EvaluationPredictor, predictor
    depths, intrs, extrs, kinv, einv = dyadic
    # planted draws (t, the column scaled by the width, the one scaled by the height): whole pixels, one of them outside the map
    planted = torch.tensor([[0.0, 3, 5], [2.0, 47, 31], [1.0, 20, 0], [2.0, 9, 40], [0.0, 0, 17]])
    monkeypatch.setattr(predictor, "get_uniformly_sampled_pts", lambda size, num_frames, extent, device="cpu": planted[None])
    pred = EvaluationPredictor(SpyModel(), interp_shape=None, num_uniformly_sampled_pts=len(planted))
    rows = pred._uniform_rows(depths, kinv, einv)
    # sample-major, then view; the reference's order of the two columns: (t, y, x)
    vid = [v for _ in planted for v in range(V)]
    fid = [int(p[0]) for p in planted for _ in range(V)]
    x = [float(p[2]) for p in planted for _ in range(V)]
    y = [float(p[1]) for p in planted for _ in range(V)]
    want = _restated_rows(pred, depths, vid, fid, x, y, kinv, einv)
    assert rows.shape == (len(planted) * V, 4) and rows.dtype == torch.float32 and torch.equal(rows, want)
    assert torch.equal(rows[0], torch.tensor([0.0, float(depths[0, 0, 0, 0, 3, 5]) * (5 - 24) / 8 - 0.5, float(depths[0, 0, 0, 0, 3, 5]) * (3 - 16) / 8 + 1.0,
                                              float(depths[0, 0, 0, 0, 3, 5])]))  # (the restatement is not wrong in the same way)


def test_local_grid_rows_are_the_per_camera_lift_exactly(dyadic):
    from mvtracker_amd import EvaluationPredictor
    from mvtracker_amd.predictor import points_on_a_grid
    depths, intrs, extrs, kinv, einv = dyadic
    pred = EvaluationPredictor(SpyModel(), interp_shape=None, local_grid_size=3, local_extent=32)  # grid: the centre and +-15.5 pixels
    # queries at depth 2 (divisions by a power of two are exact) behind whole pixels of view 0: mid-image, near a corner, far outside
    lift0 = lambda px, py: (torch.tensor([(px - 24) / 8, (py - 16) / 8, 1.0]) * 2 - torch.tensor([0.5, -1.0, 0.0])).tolist()
    queries = torch.tensor([[0.0] + lift0(24, 16), [2.0] + lift0(4, 30), [1.0] + lift0(-400, -300)])
    qt = [0, 2, 1]
    local = pred._local_grid_rows(queries, torch.tensor(qt), qt, depths, intrs, extrs, kinv, einv)
    want, counts = [], []
    for i, q in enumerate(queries):
        want.append([])
        for v in range(V):
            cam = extrs[0, v, qt[i], :, :3].double() @ q[1:].double() + extrs[0, v, qt[i], :, 3].double()
            ph = intrs[0, v, qt[i]].double() @ cam
            px, py = float(ph[0] / ph[2]), float(ph[1] / ph[2])
            assert px == int(px) and py == int(py)  # (whole pixels in every view: the grids are in half pixels)
            pix = points_on_a_grid(3, (32, 32), (py, px))
            pix = pix[(pix[:, 0] >= 0) & (pix[:, 0] < LW) & (pix[:, 1] >= 0) & (pix[:, 1] < LH)]
            counts.append(len(pix))
            if len(pix):
                want[i].append(_restated_rows(pred, depths, [v] * len(pix), [qt[i]] * len(pix), pix[:, 0].tolist(), pix[:, 1].tolist(), kinv, einv))
    assert counts[0] == 9 and counts[2] == 4 and counts[4:] == [0, 0] and 0 < counts[1] and 0 < counts[3]  # whole, partly, wholly outside
    assert [len(rows) for rows in local] == [len(rows) for rows in want] and local[2] == []
    for got_q, want_q in zip(local, want):
        for got, w in zip(got_q, want_q):
            assert got.dtype == torch.float32 and torch.equal(got, w)
    assert [sum(len(r) for r in rows) for rows in local] == [counts[0] + counts[1], counts[2] + counts[3], 0]
    pred.local_grid_size = 0
    assert pred._local_grid_rows(queries, torch.tensor(qt), qt, depths, intrs, extrs, kinv, einv) == [[], [], []]


# ------------------------------------------------------------------------------------------------------------------ 4. one NaN guard
def _errors(caplog):
    return [r for r in caplog.records if r.levelno == logging.ERROR and "NaN" in r.getMessage()]


@pytest.mark.parametrize("single_point", [False, True])
def test_forward_reads_the_models_flag_once(monkeypatch, caplog, single_point):
    from mvtracker_amd import EvaluationPredictor
    hip_mock_reproject.install(monkeypatch)
    c = {k: torch.from_numpy(v) for k, v in synth.make_clip(3, V=V, T=T, H=H, W=W, N=3).items()}
    kw = dict(interp_shape=None, grid_size=2, single_point=single_point, local_grid_size=0)
    caplog.set_level(logging.ERROR, logger="mvtracker_amd.predictor")
    pred = EvaluationPredictor(SpyModel(nan=(0, 1, 0)), **kw)  # (single_point: the second of three forwards; joint: no NaN)
    _call(pred, c)
    assert pred.last_nan is single_point and len(_errors(caplog)) == int(single_point) and pred.model.calls == (3 if single_point else 1)
    caplog.clear()
    pred.model.nan, pred.model.calls = [1, 1, 1], 0
    _call(pred, c)
    assert pred.last_nan is True and len(_errors(caplog)) == 1  # one message per call, whatever the number of flags
    caplog.clear()
    pred.model.nan = []
    _call(pred, c)
    assert pred.last_nan is False and _errors(caplog) == []


def test_finish_reads_the_sessions_flag_once(monkeypatch, caplog):
    from mvtracker_amd import EvaluationPredictor
    hip_mock_reproject.install(monkeypatch)
    c = {k: torch.from_numpy(v) for k, v in synth.make_clip(3, V=V, T=T, H=H, W=W, N=3).items()}
    caplog.set_level(logging.ERROR, logger="mvtracker_amd.predictor")
    for nan in (1, 0, 3):
        pred = EvaluationPredictor(SpyModel(nan=(nan,)), interp_shape=None, grid_size=2)
        pred.last_nan = not nan
        st = pred.open_stream(c["query_points"])
        st.push(*(c[k] for k in ("rgbs", "depths", "intrs", "extrs")))
        assert pred.last_nan is (not nan) and _errors(caplog) == []  # (deferred: nothing is read before ``finish``)
        st.finish()
        assert pred.last_nan is bool(nan) and len(_errors(caplog)) == int(bool(nan))
        caplog.clear()
