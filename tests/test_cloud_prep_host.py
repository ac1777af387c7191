"""Cloud preparation, host side (no GPU): the exports, the validation of estimate_normals / voxel_downsample / PcaCameraAlignment /
align_point_clouds(target_normals=None), the launch order on mocked kernels (tests/hip_mock_prep.py, whose fake entries call the
restatement tests/cloud_prep_ref.py), the demo flags, and what tests/test_gpu_cloud_prep.py relies on, checked on the restatement
alone: the end-to-end condition with PCA normals, and the fixed-point mean.  Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_align_cases as Cs  # noqa: E402
import cloud_prep_ref as R  # noqa: E402
import hip_mock_align  # noqa: E402
import hip_mock_clean  # noqa: E402
import hip_mock_prep  # noqa: E402

PCA_RADIUS, PCA_MAX_NN = 0.3, 30


def test_exports():
    import mvtracker_amd
    from mvtracker_amd import PcaCameraAlignment, CameraAlignment, cloud, estimate_normals, hip, voxel_downsample
    assert estimate_normals is cloud.estimate_normals and voxel_downsample is cloud.voxel_downsample
    assert issubclass(PcaCameraAlignment, CameraAlignment)
    assert {"cloud", "estimate_normals", "voxel_downsample", "PcaCameraAlignment"} <= set(mvtracker_amd.__all__)
    assert all(n in hip.SIGNATURES for n in ("mvt_normals_estimate", "mvt_voxel_bounds", "mvt_voxel_insert", "mvt_voxel_emit"))
    assert (hip.NORMALS_MAX_NN, hip.VOXEL_RANGE, hip.VOXEL_FULL) == (64, 1, 2)


def test_header_constants_match_the_binding(tmp_path):
    import shutil
    import subprocess
    from mvtracker_amd import hip
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = {"MVT_NORMALS_MAX_NN": hip.NORMALS_MAX_NN, "MVT_VOXEL_RANGE": hip.VOXEL_RANGE, "MVT_VOXEL_FULL": hip.VOXEL_FULL,
             "MVT_VOXEL_ORIGIN": hip.VOXEL_ORIGIN, "MVT_VOXEL_SIZE": hip.VOXEL_SIZE, "MVT_VOXEL_STATUS": hip.VOXEL_STATUS,
             "MVT_VOXEL_POINTS": hip.VOXEL_POINTS, "MVT_VOXEL_STATE_WORDS": hip.VOXEL_STATE_WORDS,
             "MVT_VOXEL_BOUND_BLOCKS": hip.VOXEL_BOUND_BLOCKS, "MVT_VOXEL_SLOT_WORDS": hip.VOXEL_SLOT_WORDS}
    lines = ['#include <stdio.h>', '#include "mvtracker_hip.h"', 'int main(void) {'] + [f'  printf("{n} %d\\n", {n});' for n in names] + ['  return 0;', '}']
    (tmp_path / "probe.c").write_text("\n".join(lines))
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True).stdout.strip().split("\n"))
    assert {k: int(v) for k, v in got.items()} == names


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    from mvtracker_amd import PcaCameraAlignment, align_point_clouds, estimate_normals, voxel_downsample
    hip_mock_prep.install(monkeypatch)
    pts = torch.zeros(5, 3)
    for kw in (dict(points=torch.zeros(5, 4)), dict(points=torch.zeros(0, 3)), dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")),
               dict(max_nn=2), dict(max_nn=65), dict(max_nn=7.5), dict(viewpoint=(0.0, 1.0)), dict(viewpoint=(0.0, float("inf"), 0.0))):
        with pytest.raises(ValueError):
            estimate_normals(**dict(dict(points=pts), **kw))
    for kw in (dict(points=torch.zeros(5, 2)), dict(points=torch.zeros(0, 3)), dict(voxel_size=0.0), dict(voxel_size=-0.1),
               dict(voxel_size=float("inf")), dict(voxel_size=float("nan"))):
        with pytest.raises(ValueError):
            voxel_downsample(**dict(dict(points=pts, voxel_size=0.1), **kw))
    for kw in (dict(normal_radius=0.0), dict(normal_radius=float("nan")), dict(normal_max_nn=2), dict(normal_max_nn=65), dict(max_distance=0.0)):
        with pytest.raises(ValueError):
            PcaCameraAlignment(**kw)
    for kw in (dict(normal_radius=0.0), dict(normal_max_nn=100), dict(max_distance=0.0), dict(source=torch.zeros(5, 4))):
        with pytest.raises(ValueError):
            align_point_clouds(**dict(dict(source=pts, target=pts, target_normals=None, max_distance=0.1, max_iterations=3), **kw))
    with pytest.raises(TypeError):
        align_point_clouds(pts, pts, None, 0.1, 3, None, 0.05)  # normal_radius / normal_max_nn are keyword-only
    assert hip_mock_prep.calls == [] and hip_mock_prep.order == [] and hip_mock_align.calls == [] and hip_mock_clean.calls == []
    a = PcaCameraAlignment(max_distance=0.1)
    assert (a.normal_radius, a.normal_max_nn) == (0.1, 30) and PcaCameraAlignment(normal_radius=float("inf")).normal_radius == float("inf")
    assert (PcaCameraAlignment(normal_radius=0.3, normal_max_nn=12).normal_radius, "normal_max_nn=12" in repr(PcaCameraAlignment(normal_max_nn=12))) == (0.3, True)


def test_launch_order_plain_and_pca(monkeypatch):
    """A plain CameraAlignment makes exactly the parent's call list (grid normals, then the boxes); a PcaCameraAlignment builds the
    boxes first and then calls the PCA entry, at construction and after every commit, and never the grid normals."""
    from mvtracker_amd import CameraAlignment, PcaCameraAlignment, align_cameras
    sc = Cs.scene(3, 16, 24)
    ex = Cs.perturbed(sc["extrs"], 2, Cs.rigid(0.8, (0.3, -0.5, 0.8), (0.02, -0.01, 0.015)))
    args = (torch.from_numpy(sc["depths"]), torch.from_numpy(sc["intrs"]), torch.from_numpy(ex))
    kw = dict(max_distance=0.3, max_iterations=2, sweeps=1, frames=(0,))
    hip_mock_prep.install(monkeypatch)
    align_cameras(*args, CameraAlignment(normal_max_edge=1.0, **kw))
    per_run = ["align_correspond", "align_solve"] * 3 + ["align_transform", "align_normals"]
    assert hip_mock_clean.calls == ["clean_points"] and hip_mock_align.calls == ["align_normals"] + per_run * 2 and hip_mock_prep.calls == []
    assert hip_mock_prep.order == ["align_normals", "tile_aabb", "tile_group_aabb"] * 3
    hip_mock_prep.install(monkeypatch)
    c = align_cameras(*args, PcaCameraAlignment(normal_radius=1.0, **kw))
    assert hip_mock_align.calls == (["align_correspond", "align_solve"] * 3 + ["align_transform"]) * 2
    assert hip_mock_prep.order == ["tile_aabb", "tile_group_aabb", "normals_estimate"] * 3 and hip_mock_prep.calls == ["normals_estimate"] * 3
    got = c.transforms.numpy()
    moved = Cs.unproject(sc["depths"], sc["intrs"], ex)
    clouds, (gw, gh) = Cs.organised_clouds(moved[:, [0]])
    ref = R.align_views_pca(clouds, gw, gh, 0.3, 1.0, 30, 2, 1)
    print(f"max |D_mock - D_restatement| {np.abs(got - ref['D']).max():.2e}")
    assert np.array_equal(got[0], np.eye(4)) and np.abs(got - ref["D"]).max() < 1e-4 and c.status.tolist() == [0, 0, 0]


def test_align_point_clouds_without_normals_is_the_call_with_estimated_ones(monkeypatch):
    from mvtracker_amd import align_point_clouds, estimate_normals
    hip_mock_prep.install(monkeypatch)
    tgt, _ = Cs.dyadic_target(16, 24)
    xy = tgt[R.valid_rows(tgt), :2].astype(np.float64)
    pts = np.concatenate([xy, (0.05 * (xy ** 2).sum(1) + 0.3 * np.sin(xy[:, 0]))[:, None]], 1).astype(np.float32)
    G = Cs.rigid(0.4, (0.2, 1.0, -0.3), (0.01, -0.015, 0.02))
    src = torch.from_numpy(((pts.astype(np.float64) - G[:3, 3]) @ G[:3, :3]).astype(np.float32))
    t = torch.from_numpy(pts)
    a = align_point_clouds(src, t, None, 0.2, 10, normal_radius=0.6, normal_max_nn=12)
    assert hip_mock_prep.calls == ["normals_estimate"]
    n = estimate_normals(t, 0.6, 12)
    b = align_point_clouds(src, t, n, 0.2, 10)
    print(f"max |T - planted| {np.abs(a[0].numpy() - G).max():.2e}, fitness {a[1]:.4f}, rmse {a[2]:.2e}")
    assert torch.equal(a[0], b[0]) and a[1:] == b[1:] and np.abs(a[0].numpy() - G).max() < 5e-3


def test_wrappers_on_the_mock():
    """estimate_normals / voxel_downsample shapes, dtypes and the single read-back, on the mock."""
    mp = pytest.MonkeyPatch()
    try:
        from mvtracker_amd import estimate_normals, voxel_downsample
        hip_mock_prep.install(mp)
        rng = np.random.default_rng(0)
        xy = rng.uniform(-1, 1, (200, 2))
        pts = np.concatenate([xy, (0.5 * xy[:, :1] - 0.25 * xy[:, 1:])], 1).astype(np.float32)
        pts[7] = np.nan
        n, idx, cnt = estimate_normals(torch.from_numpy(pts), radius=0.5, max_nn=10, viewpoint=(0.0, 0.0, 5.0), return_neighbors=True)
        true = np.array([-0.5, 0.25, 1.0]) / np.linalg.norm([-0.5, 0.25, 1.0])
        ok = ~torch.isnan(n[:, 0]).numpy()
        print(f"{int(ok.sum())} normals of 200, max |n - true| {np.abs(n.numpy()[ok] - true).max():.2e}")
        assert n.shape == (200, 3) and idx.shape == (200, 10) and idx.dtype == cnt.dtype == torch.int32 and int(cnt[7]) == -1 and not ok[7]
        assert ok.sum() > 150 and np.abs(n.numpy()[ok] - true).max() < 1e-5
        p, c, f, lab = voxel_downsample(torch.from_numpy(pts), 0.25, return_labels=True)
        r = R.voxel(pts, 0.25)
        assert p.shape == (len(r["counts"]), 3) and np.array_equal(p.numpy(), r["points"]) and np.array_equal(c.numpy(), r["counts"])
        assert np.array_equal(f.numpy(), r["first"]) and np.array_equal(lab.numpy(), r["labels"]) and int(lab[7]) == -1 and int(c.sum()) == 199
        assert (np.diff(f.numpy()) > 0).all() and hip_mock_prep.calls == ["normals_estimate", "voxel_bounds", "voxel_insert", "voxel_emit"]
        with pytest.raises(ValueError, match="too small"):
            voxel_downsample(torch.from_numpy(pts), 1e-7)
    finally:
        mp.undo()


def test_demo_flags_parse():
    import demo_amd
    from mvtracker_amd import PcaCameraAlignment
    ap = demo_amd.build_parser()
    a = ap.parse_args(["--synthetic", "--align-cameras"])
    assert (a.align_normals, a.align_normal_radius, a.align_normal_max_nn) == ("grid", None, 30)
    assert not isinstance(demo_amd.camera_alignment_from_args(a), PcaCameraAlignment)
    a = ap.parse_args("--synthetic --align-cameras --align-max-distance 0.1 --align-normals pca --align-normal-radius 0.25 --align-normal-max-nn 20".split())
    c = demo_amd.camera_alignment_from_args(a)
    assert isinstance(c, PcaCameraAlignment) and (c.max_distance, c.normal_radius, c.normal_max_nn) == (0.1, 0.25, 20)
    c = demo_amd.camera_alignment_from_args(ap.parse_args("--synthetic --align-cameras --align-max-distance 0.1 --align-normals pca".split()))
    assert c.normal_radius == 0.1
    with pytest.raises(SystemExit):
        ap.parse_args(["--synthetic", "--align-normals", "open3d"])


# ------------------------------------------------------------------------------------------------------------------ what the GPU bars rely on
@pytest.fixture(scope="module")
def planted():
    """4 views at 48 x 64, two frames, view 1 perturbed: the scene of tests/test_camera_align_host.py and of the GPU tests."""
    sc = Cs.scene(4, 48, 64)
    G = Cs.rigid(**Cs.PLANTED)
    ex = Cs.perturbed(sc["extrs"], 1, G)
    true = Cs.unproject(sc["depths"], sc["intrs"], sc["extrs"])
    moved = Cs.unproject(sc["depths"], sc["intrs"], ex)
    return dict(sc, extrs_bad=ex, G=G, true=true, moved=moved)


@pytest.mark.parametrize("frames", [(0,), (0, 1)])
def test_the_restatement_meets_the_end_to_end_condition_with_pca_normals(planted, frames):
    """The condition of the GPU test on the restatement alone, view 1 only: at most a tenth of the planted displacement is left.
    (The untouched views 2 and 3 drift to about 4.9 mm, too close to before / 10 to be a condition.)"""
    clouds, (gw, gh) = Cs.organised_clouds(planted["moved"][:, list(frames)])
    info = R.align_views_pca(clouds, gw, gh, 0.05, PCA_RADIUS, PCA_MAX_NN, 30, 2)
    before = Cs.displacement(np.eye(4), planted["moved"][1], planted["true"][1])
    after = Cs.displacement(info["D"][1], planted["moved"][1], planted["true"][1])
    drift = [Cs.displacement(info["D"][v], planted["moved"][v], planted["true"][v]) for v in (2, 3)]
    n_pca = sum(int(np.isfinite(R.pca_normals(clouds[v][0], PCA_RADIUS, PCA_MAX_NN)[:, 0]).sum()) for v in range(4))
    print(f"frames {frames}: planted {1e3 * before:.2f} mm, left {1e3 * after:.3f} mm, views 2 / 3 drift {1e3 * drift[0]:.2f} / {1e3 * drift[1]:.2f} mm, "
          f"{n_pca} PCA normals in frame {frames[0]}")
    assert 0.045 < before < 0.055 and after <= before / 10
    assert np.array_equal(info["D"][0], np.eye(4)) and info["status"].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("voxel_size", [0.05, 0.2, 1.0])
def test_the_fixed_point_mean_stays_within_2_to_the_minus_32_voxel(planted, voxel_size):
    """Each member's offset is rounded to a multiple of 2^-32 voxel (an error of at most 2^-33 voxel), so their mean is within 2^-33
    voxel of the mean of the exact offsets; the bar of 2^-32 leaves the fp64 rounding of both sides (1e-15 of the coordinate) room."""
    pts = planted["moved"][:, 0].reshape(-1, 3).astype(np.float32)
    r = R.voxel(pts, voxel_size)
    err = np.abs(r["fixed64"] - r["mean64"]).max() / voxel_size
    print(f"voxel {voxel_size}: {int(R.valid_rows(pts).sum())} points -> {len(r['counts'])} voxels, largest {int(r['counts'].max())}, "
          f"max |fixed-point mean - fp64 mean| {err:.3e} voxel (2^-32 = {2.0 ** -32:.3e})")
    assert r["status"] == 0 and err <= 2.0 ** -32 and int(r["counts"].sum()) == int(R.valid_rows(pts).sum())
    assert (np.diff(r["first"]) > 0).all() and np.array_equal(r["first"], [np.flatnonzero(r["labels"] == k)[0] for k in range(len(r["counts"]))])
    # every member lies in its voxel's cell
    m = r["labels"] >= 0
    u = (pts[m].astype(np.float64) - r["origin"]) / voxel_size
    assert np.array_equal(np.floor(u).astype(np.int64), r["cells"][r["labels"][m]])
