"""Camera alignment, host side (no GPU): CameraAlignment's validation, the sweep and target order, CameraCorrection.apply, the
predictor / demo wiring on mocked kernels (tests/hip_mock_align.py, whose fake entries call the restatement
tests/camera_align_ref.py), and what tests/test_gpu_camera_align.py relies on, checked on the restatement alone: the end-to-end
condition, and the share of near-tie queries on the teacher-forced scene.

No recorded output of the reference exists for this feature: its ICP calls Open3D, which is not a dependency of either project's
tests; the restatement of Open3D's documented rules is the yardstick.  Two perturbed views at once are NOT covered by the GPU tests: with sweeps=2 the
restatement itself leaves 36 mm of 50 mm on this scene (test_two_perturbed_views_are_out_of_reach_of_two_sweeps reproduces the
figures), so the end-to-end cases keep one perturbed view."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_align_cases as Cs  # noqa: E402
import camera_align_ref as R  # noqa: E402
import hip_mock_align  # noqa: E402
import hip_mock_clean  # noqa: E402
import hip_mock_scene  # noqa: E402


# ------------------------------------------------------------------------------------------------------------------ validation
def test_camera_alignment_validation_and_defaults():
    import inspect
    from mvtracker_amd import CameraAlignment, align
    assert CameraAlignment is align.CameraAlignment
    p = inspect.signature(CameraAlignment.__init__).parameters
    assert list(p)[1:] == ["max_distance", "max_iterations", "sweeps", "frames", "anchor", "sample_stride", "normal_max_edge", "conf_thresh"]
    a = CameraAlignment()
    assert (a.max_distance, a.max_iterations, a.sweeps, a.frames, a.anchor, a.sample_stride, a.normal_max_edge, a.conf_thresh) == \
        (0.05, 30, 2, (0,), 0, 1, 0.05, None)
    assert CameraAlignment(max_distance=0.1).normal_max_edge == 0.1 and CameraAlignment(normal_max_edge=0.3).normal_max_edge == 0.3
    for kw in (dict(max_distance=0.0), dict(max_distance=-1.0), dict(max_distance=float("nan")), dict(max_distance=float("inf")),
               dict(max_iterations=0), dict(max_iterations=2.5), dict(sweeps=0), dict(frames=()), dict(frames=(0, 0)), dict(frames=(-1,)),
               dict(frames=3), dict(frames=(0.5,)), dict(anchor=-1), dict(anchor=0.5), dict(sample_stride=0), dict(sample_stride=1.5),
               dict(normal_max_edge=0.0), dict(normal_max_edge=float("nan")), dict(conf_thresh=float("nan"))):
        with pytest.raises(ValueError):
            CameraAlignment(**kw)
    CameraAlignment(frames=[3, 1], anchor=2, sample_stride=4, conf_thresh=-1.0)


def _scene(V=3, H=16, W=24, T=2):
    return {k: torch.from_numpy(v) for k, v in Cs.scene(V, H, W, T).items()}


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    from mvtracker_amd import CameraAlignment, align_cameras, align_point_clouds
    hip_mock_align.install(monkeypatch)
    s = _scene()
    d, i, e = s["depths"], s["intrs"], s["extrs"]
    a = CameraAlignment()
    with pytest.raises(ValueError):
        align_cameras(d, i, e, "icp")
    with pytest.raises(ValueError):
        align_cameras(d[0, :, :, 0], i[0], e[0], a)
    with pytest.raises(ValueError):
        align_cameras(d, i[0], e[0], a)
    with pytest.raises(ValueError):
        align_cameras(d, i, e, a, depths_conf=d[:, :, :1])
    with pytest.raises(ValueError):
        align_cameras(d, i, e, CameraAlignment(anchor=3))
    with pytest.raises(ValueError):
        align_cameras(d, i, e, CameraAlignment(frames=(0, 2)))
    with pytest.raises(ValueError):
        align_cameras(d[:, :1], i[:, :1], e[:, :1], a)  # one view: nothing to align against
    pts = torch.zeros(5, 3)
    for bad in (dict(source=torch.zeros(5, 4)), dict(target_normals=torch.zeros(4, 3)), dict(max_distance=0.0), dict(max_iterations=0),
                dict(init=torch.eye(3)), dict(source=torch.zeros(0, 3))):
        kw = dict(source=pts, target=pts, target_normals=pts, max_distance=0.1, max_iterations=3)
        kw.update(bad)
        with pytest.raises(ValueError):
            align_point_clouds(**kw)
    assert hip_mock_align.calls == [] and hip_mock_clean.calls == []


# ------------------------------------------------------------------------------------------------------------------ the sweep
@pytest.fixture(scope="module")
def planted():
    """4 views at 48 x 64, two frames, view 1 perturbed: the scene of the GPU tests."""
    sc = Cs.scene(4, 48, 64)
    G = Cs.rigid(**Cs.PLANTED)
    ex = Cs.perturbed(sc["extrs"], 1, G)
    true = Cs.unproject(sc["depths"], sc["intrs"], sc["extrs"])
    moved = Cs.unproject(sc["depths"], sc["intrs"], ex)
    return dict(sc, extrs_bad=ex, G=G, true=true, moved=moved)


def test_sweep_and_target_order_and_the_result_of_the_restatement(monkeypatch):
    """On the mock the launch sequence is fixed (max_iterations + 1 pairs per view and sweep), every view but the anchor is the source
    in view order in every sweep with all other views, in view order, as its targets, and the transforms are the restatement's."""
    from mvtracker_amd import CameraAlignment, align_cameras
    hip_mock_align.install(monkeypatch)
    sc = Cs.scene(3, 16, 24)
    ex = Cs.perturbed(sc["extrs"], 2, Cs.rigid(0.8, (0.3, -0.5, 0.8), (0.02, -0.01, 0.015)))
    a = CameraAlignment(max_distance=0.3, max_iterations=4, sweeps=2, frames=(1, 0), anchor=1, normal_max_edge=1.0)
    c = align_cameras(torch.from_numpy(sc["depths"]), torch.from_numpy(sc["intrs"]), torch.from_numpy(ex), a)
    per_run = ["align_correspond", "align_solve"] * 5 + ["align_transform", "align_normals"]
    assert hip_mock_clean.calls == ["clean_points"] * 2
    assert hip_mock_align.calls == ["align_normals"] + per_run * 4
    srcs = sorted({s for s, _ in hip_mock_align.searches})
    tgts = sorted({t for _, ts in hip_mock_align.searches for t in ts})
    assert len(srcs) == 2 and len(tgts) == 3
    order = []
    for s, ts in hip_mock_align.searches:
        run = ((0, 2)[srcs.index(s)], tuple(tgts.index(t) for t in ts))
        if not order or order[-1] != run:
            order.append(run)
    assert order == [(0, (1, 2)), (2, (0, 1)), (0, (1, 2)), (2, (0, 1))]
    moved = Cs.unproject(sc["depths"], sc["intrs"], ex)
    clouds, (gw, gh) = Cs.organised_clouds(moved[:, [1, 0]])
    ref = R.align_views(clouds, gw, gh, 0.3, 1.0, 4, 2, anchor=1)
    assert ref["order"] == order
    got = c.transforms.numpy()
    assert got.shape == (3, 4, 4) and c.transforms.dtype == torch.float64 and np.array_equal(got[1], np.eye(4))
    # the mock unprojects in fp32 through the library's inverse cameras, the restatement's clouds come from fp64: equal to rounding
    assert np.abs(got - ref["D"]).max() < 1e-4 and np.abs(got[2] - np.eye(4)).max() > 1e-3
    assert c.iterations.tolist()[1] == 0 and all(1 <= n <= 4 for n in (c.iterations[0], c.iterations[2]))
    assert c.status.tolist() == [0, 0, 0] and c.fitness.dtype == torch.float64 and float(c.fitness[2]) > 0.2 and float(c.rmse[2]) > 0


def test_apply_is_extrs_times_the_fp64_inverse():
    from mvtracker_amd import CameraCorrection
    rng = np.random.default_rng(0)
    D = np.stack([np.eye(4), Cs.rigid(3.0, (1, 2, 3), (0.1, -0.2, 0.3)), Cs.rigid(-40.0, (0, 1, 0.2), (1.0, 2.0, -0.5))])
    ex = rng.standard_normal((1, 3, 5, 3, 4)).astype(np.float32)
    c = CameraCorrection(torch.from_numpy(D))
    got = c.apply(torch.from_numpy(ex))
    want = np.zeros_like(ex, dtype=np.float64)
    for v in range(3):
        E4 = np.concatenate([ex[0, v].astype(np.float64), np.broadcast_to([0, 0, 0, 1.0], (5, 1, 4))], 1)
        want[0, v] = (E4 @ np.linalg.inv(D[v]))[:, :3]
    assert got.dtype == torch.float32 and got.shape == ex.shape and torch.equal(got[0, 0], torch.from_numpy(ex[0, 0]))
    assert np.array_equal(got.numpy(), want.astype(np.float32))  # fp64, rounded once
    assert torch.equal(c.apply(torch.from_numpy(ex[0])), got[0])  # without the batch dimension
    got64 = c.apply(torch.from_numpy(ex).double()).numpy()
    assert np.abs(got64 - want).max() < 1e-12
    # a corrected camera sees the corrected world point where the old camera saw the old one
    X = rng.standard_normal(3)
    for v in range(3):
        old = ex[0, v, 0].astype(np.float64) @ np.append(X, 1)
        new = got64[0, v, 0] @ np.append(D[v, :3, :3] @ X + D[v, :3, 3], 1)
        assert np.abs(old - new).max() < 1e-12
    with pytest.raises(ValueError):
        c.apply(torch.zeros(1, 2, 5, 3, 4))
    with pytest.raises(ValueError):
        CameraCorrection(torch.zeros(3, 3, 4))


def test_align_point_clouds_on_the_mock_recovers_a_planted_motion(monkeypatch):
    from mvtracker_amd import align_point_clouds
    hip_mock_align.install(monkeypatch)
    tgt, _ = Cs.dyadic_target(24, 40)
    ok = R.valid_rows(tgt)
    # an analytic bowl: points and exact normals
    xy = tgt[ok, :2].astype(np.float64)
    z = 0.05 * (xy ** 2).sum(1) + 0.3 * np.sin(xy[:, 0])
    pts = np.concatenate([xy, z[:, None]], 1)
    n = np.stack([-(0.1 * xy[:, 0] + 0.3 * np.cos(xy[:, 0])), -0.1 * xy[:, 1], np.ones(len(xy))], 1)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    G = Cs.rigid(0.4, (0.2, 1.0, -0.3), (0.01, -0.015, 0.02))
    src = (pts - G[:3, 3]) @ G[:3, :3]  # inv(G) of the target's own points
    T, fit, rmse = align_point_clouds(torch.from_numpy(src.astype(np.float32)), torch.from_numpy(pts.astype(np.float32)),
                                      torch.from_numpy(n.astype(np.float32)), 0.2, 20)
    assert T.shape == (4, 4) and T.dtype == torch.float64 and fit > 0.99 and rmse < 2e-3
    assert np.abs(T.numpy() - G).max() < 2e-3
    ref = R.icp([src.astype(np.float32)], [[(pts.astype(np.float32), n.astype(np.float32))]], 0.2, 20)
    assert np.abs(T.numpy() - ref["D"]).max() < 1e-9 and abs(fit - ref["fitness"]) < 1e-12 and abs(rmse - ref["rmse"]) < 1e-9
    T2, _, _ = align_point_clouds(torch.from_numpy(src.astype(np.float32)), torch.from_numpy(pts.astype(np.float32)),
                                  torch.from_numpy(n.astype(np.float32)), 0.2, 20, init=torch.from_numpy(G))
    assert np.abs(T2.numpy() - G).max() < 1e-4


def test_query_slots_cover_the_sampled_pixels_once():
    from mvtracker_amd import align
    for grid, s in (((64, 48), 1), ((64, 48), 2), ((24, 16), 3), ((40, 24), 5)):
        slots = align.query_slots(grid[0] * grid[1], grid, s).numpy()
        want = (np.arange(0, grid[1], s)[:, None] * grid[0] + np.arange(0, grid[0], s)[None]).reshape(-1)
        assert len(slots) % 64 == 0 and np.array_equal(np.sort(slots[slots >= 0]), want)
    slots = align.query_slots(4097).numpy()
    assert len(slots) == 65 * 64 and np.array_equal(slots[:4097], np.arange(4097)) and (slots[4097:] == -1).all()


# ------------------------------------------------------------------------------------------------------------------ wiring
class FakeModel(torch.nn.Module):
    S = 4

    def forward(self, rgbs, depths=None, query_points=None, intrs=None, extrs=None, **kw):
        self.seen = dict(depths=depths, query_points=query_points, extrs=extrs, kw=kw)
        return {"traj_e": torch.zeros(1, rgbs.shape[2], query_points.shape[1], 3), "vis_e": torch.zeros(1, rgbs.shape[2], query_points.shape[1])}


@pytest.fixture()
def wired(monkeypatch):
    from mvtracker_amd import CameraAlignment, EvaluationPredictor
    hip_mock_align.install(monkeypatch)
    sc = Cs.scene(3, 16, 24)
    sc["extrs"] = Cs.perturbed(sc["extrs"], 1, Cs.rigid(0.8, (0.3, -0.5, 0.8), (0.02, -0.01, 0.015)))
    d = sc["depths"]
    rng = np.random.default_rng(5)
    d[(rng.uniform(size=d.shape) < 0.03) & (d > 0)] *= 0.6  # flying pixels, for the cleaning to remove
    c = {k: torch.from_numpy(v) for k, v in sc.items()}
    c["rgbs"] = torch.zeros(1, 3, 2, 3, 16, 24)
    c["query_points"] = torch.tensor([[[0.0, 0.1, 0.2, 0.0], [1.0, -0.3, 0.4, 0.0]]])
    pred = EvaluationPredictor(FakeModel(), interp_shape=None, grid_size=2)
    return pred, c, CameraAlignment(max_distance=0.3, max_iterations=3, sweeps=1, normal_max_edge=1.0)


def _call(pred, c, **kw):
    return pred(rgbs=c["rgbs"], depths=c["depths"], query_points_3d=c["query_points"], intrs=c["intrs"], extrs=c["extrs"], **kw)


def test_none_makes_no_call_and_changes_nothing(wired):
    pred, c, a = wired
    _call(pred, c)
    plain = pred.model.seen
    _call(pred, c, camera_alignment=None)
    assert hip_mock_align.calls == [] and hip_mock_clean.calls == [] and hip_mock_scene.calls == []
    assert all(torch.equal(pred.model.seen[k], plain[k]) for k in ("depths", "query_points", "extrs"))
    assert torch.equal(pred.model.seen["extrs"], c["extrs"]) and "camera_alignment" not in pred.model.seen["kw"]
    assert pred.last_camera_correction is None
    with pytest.raises(ValueError, match="CameraAlignment"):
        _call(pred, c, camera_alignment="icp")
    assert hip_mock_align.calls == []


def test_predictor_cleans_then_aligns_then_normalises(wired, monkeypatch):
    from mvtracker_amd import DepthCleaning, SceneTransform, align_cameras, clean_depths, hip
    pred, c, a = wired
    want = align_cameras(c["depths"], c["intrs"], c["extrs"], a)
    assert float((want.transforms[1] - torch.eye(4, dtype=torch.float64)).abs().max()) > 1e-3
    del hip_mock_align.calls[:]
    _call(pred, c, camera_alignment=a)
    got = pred.last_camera_correction
    assert torch.equal(got.transforms, want.transforms) and torch.equal(pred.model.seen["extrs"], want.apply(c["extrs"]))
    assert torch.equal(pred.model.seen["depths"], c["depths"]) and hip_mock_align.calls.count("align_correspond") == 2 * 4
    # with cleaning and a transform: the alignment sees the cleaned depths, the normalisation the corrected cameras
    cl = DepthCleaning(nb_neighbors=8, std_ratio=1.0)
    dc = clean_depths(c["depths"], c["intrs"], c["extrs"], cl)[0]
    assert int((dc != c["depths"]).sum()) > 0
    want_c = align_cameras(dc, c["intrs"], c["extrs"], a)
    assert not torch.equal(want_c.transforms, want.transforms)
    order = []
    for name in ("clean_mask", "align_normals", "align_solve", "scene_apply"):
        real = getattr(hip, name)
        monkeypatch.setattr(hip, name, (lambda n, f: lambda *a_, **k: (order.append(n), f(*a_, **k))[1])(name, real))
    xf = SceneTransform(2.0, None, (0.5, -1.0, 0.25))
    _call(pred, c, depth_cleaning=cl, camera_alignment=a, scene_transform=xf)
    assert order[0] == "clean_mask" and order[1] == "align_normals" and order[-1] == "scene_apply" and "align_solve" in order
    assert torch.equal(pred.last_camera_correction.transforms, want_c.transforms)
    assert torch.equal(pred.model.seen["extrs"], xf.apply(extrs=want_c.apply(c["extrs"]))[1])
    assert torch.equal(pred.model.seen["depths"], xf.apply(depths=dc)[0])


def test_a_ready_correction_is_passed_through(wired):
    from mvtracker_amd import CameraCorrection
    pred, c, a = wired
    D = torch.from_numpy(np.stack([np.eye(4), Cs.rigid(2.0, (0, 0, 1), (0.1, 0.0, -0.1)), np.eye(4)]))
    corr = CameraCorrection(D)
    _call(pred, c, camera_alignment=corr)
    assert hip_mock_align.calls == [] and hip_mock_clean.calls == []
    assert pred.last_camera_correction is corr and torch.equal(pred.model.seen["extrs"], corr.apply(c["extrs"]))
    assert not torch.equal(pred.model.seen["extrs"][0, 1], c["extrs"][0, 1]) and torch.equal(pred.model.seen["extrs"][0, 0], c["extrs"][0, 0])


def test_demo_flags_parse():
    import demo_amd
    ap = demo_amd.build_parser()
    a = ap.parse_args(["--synthetic"])
    assert not a.align_cameras and demo_amd.camera_alignment_from_args(a) is None
    assert (a.align_max_distance, a.align_iterations, a.align_sweeps, a.align_frames, a.align_anchor, a.align_sample_stride) == (0.05, 30, 2, [0], 0, 1)
    a = ap.parse_args("--synthetic --align-cameras --align-max-distance 0.1 --align-iterations 12 --align-frames 0 3 --align-sweeps 3 "
                      "--align-anchor 1 --align-sample-stride 2 --align-normal-max-edge 0.2".split())
    c = demo_amd.camera_alignment_from_args(a)
    assert (c.max_distance, c.max_iterations, c.frames, c.sweeps, c.anchor, c.sample_stride, c.normal_max_edge) == (0.1, 12, (0, 3), 3, 1, 2, 0.2)
    with pytest.raises(ValueError):
        demo_amd.camera_alignment_from_args(ap.parse_args(["--synthetic", "--align-cameras", "--align-iterations", "0"]))


def test_save_result_keeps_the_corrections(tmp_path):
    from mvtracker_amd import sample_io
    s = {"query_points_3d": torch.zeros(1, 2, 4), "camera_corrections": np.zeros((3, 4, 4))}
    sample_io.save_result(str(tmp_path / "r.npz"), torch.zeros(1, 3, 2, 3), torch.ones(1, 3, 2, dtype=torch.bool), s, include_clip=False)
    assert np.load(tmp_path / "r.npz")["camera_corrections"].shape == (3, 4, 4)


# ------------------------------------------------------------------------------------------------------------------ what the GPU bars rely on
@pytest.mark.parametrize("frames", [(0,), (0, 1)])
def test_the_restatement_meets_the_end_to_end_condition(planted, frames):
    """(a) of the GPU test on the restatement alone: at most a tenth of the planted displacement is left."""
    clouds, (gw, gh) = Cs.organised_clouds(planted["moved"][:, list(frames)])
    info = R.align_views(clouds, gw, gh, 0.05, Cs.NORMAL_MAX_EDGE, 30, 2)
    before = Cs.displacement(np.eye(4), planted["moved"][1], planted["true"][1])
    after = Cs.displacement(info["D"][1], planted["moved"][1], planted["true"][1])
    print(f"frames {frames}: planted {1e3 * before:.2f} mm, left {1e3 * after:.3f} mm, D - G max {np.abs(info['D'][1] - planted['G']).max():.2e}")
    assert 0.045 < before < 0.055 and after <= before / 10
    assert np.array_equal(info["D"][0], np.eye(4)) and info["status"].tolist() == [0, 0, 0, 0]
    for v in (2, 3):  # the views that were right are pulled by the wrong one, by no more than the same tenth
        assert Cs.displacement(info["D"][v], planted["moved"][v], planted["true"][v]) <= before / 10


def test_two_perturbed_views_are_out_of_reach_of_two_sweeps(planted):
    """Why the end-to-end GPU cases keep ONE perturbed view: with view 2 also off (Cs.PLANTED_2, 43 mm) the restatement itself, at
    the issue's settings (cap 0.05, 30 iterations, sweeps=2), misses condition (a) by far on both views -- each view is pulled onto
    targets of which one is as wrong as itself, and a 5 cm cap leaves few right correspondences.  The figures are printed; should the
    restatement ever meet (a) here, this test fails and the two-view case belongs in the GPU tests."""
    ex = Cs.perturbed(planted["extrs_bad"], 2, Cs.rigid(**Cs.PLANTED_2))
    moved = Cs.unproject(planted["depths"], planted["intrs"], ex)
    clouds, (gw, gh) = Cs.organised_clouds(moved[:, [0]])
    info = R.align_views(clouds, gw, gh, 0.05, Cs.NORMAL_MAX_EDGE, 30, 2)
    for v in (1, 2):
        before = Cs.displacement(np.eye(4), moved[v], planted["true"][v])
        after = Cs.displacement(info["D"][v], moved[v], planted["true"][v])
        print(f"two views perturbed, view {v}: planted {1e3 * before:.2f} mm, left by the restatement {1e3 * after:.2f} mm")
        assert before > 0.04 and after > before / 10


def test_near_ties_stay_below_half_a_percent_on_the_teacher_forced_scene(planted):
    """The GPU test leaves queries whose best two fp64 candidates (the cap counting as one) differ by less than 1e-6 relative out of
    the index comparison, and asserts that they are at most 0.5 % of the queries: here, along the restatement's own path."""
    clouds, (gw, gh) = Cs.organised_clouds(planted["moved"][:, [0]])
    nrm = [R.normals(clouds[u][0], gw, gh, Cs.NORMAL_MAX_EDGE) for u in range(4)]
    union = R.target_union([(clouds[u][0], nrm[u]) for u in (0, 2, 3)])
    D, cap2 = np.eye(4), R.cap_squared(0.05)
    worst = 0.0
    for it in range(6):
        sums, qs, corrs = R.evaluate([clouds[1][0]], D, [union], cap2)
        valid = R.valid_rows(qs[0])
        worst = max(worst, corrs[0]["near"][valid].mean())
        x, st = R.solve(sums)
        assert st == 0
        D = R.transform_of(x) @ D
    print(f"near-tie share over 6 iterations: at most {100 * worst:.3f} %")
    assert worst <= 0.005


def test_align_cloud_struct_matches_the_header(tmp_path):
    """hip.AlignCloud against the C compiler's layout of mvt_align_cloud (as tests/test_abi.py does for the older structs)."""
    import ctypes
    import shutil
    import subprocess
    from mvtracker_amd import hip
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mvtracker_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(mvt_align_cloud));']
    lines += [f'  printf("{f} %zu\\n", offsetof(mvt_align_cloud, {f}));' for f, _ in hip.AlignCloud._fields_]
    lines += [f'  printf("{n} %d\\n", {n});' for n in ("MVT_ALIGN_MAX_TARGETS", "MVT_ALIGN_ROW", "MVT_ALIGN_HIST", "MVT_ALIGN_FEW", "MVT_ALIGN_SINGULAR")]
    lines += ['  return 0;', '}']
    (tmp_path / "probe.c").write_text("\n".join(lines))
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True).stdout.strip().split("\n"))
    assert int(got["size"]) == ctypes.sizeof(hip.AlignCloud)
    for f, _ in hip.AlignCloud._fields_:
        assert int(got[f]) == getattr(hip.AlignCloud, f).offset, f
    assert [int(got[n]) for n in ("MVT_ALIGN_MAX_TARGETS", "MVT_ALIGN_ROW", "MVT_ALIGN_HIST", "MVT_ALIGN_FEW", "MVT_ALIGN_SINGULAR")] == \
        [hip.ALIGN_MAX_TARGETS, hip.ALIGN_ROW, hip.ALIGN_HIST, hip.ALIGN_FEW, hip.ALIGN_SINGULAR]
