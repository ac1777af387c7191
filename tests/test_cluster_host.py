"""Region clustering, host side (no GPU): the restatement tests/cluster_ref.py against sklearn's recorded labels
(tests/golden/cluster_dbscan.npz) and the fixture's margin condition; then the host code of mvtracker_amd/cluster.py and the region
path of sample_queries on mocked kernels (tests/hip_mock_cluster.py): exports, validation before any launch, the pose inverse,
chunking, report fields, the pool restriction, and that region=None calls nothing.  Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_align_cases as Cs  # noqa: E402
import cluster_ref as R  # noqa: E402
import hip_mock_cluster  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cluster_dbscan.npz")
MARGIN = 1e-5
BOX, EPS, MS = ((-0.45, 0.45), (-0.45, 0.45), (-0.45, 0.45)), 0.12, 6


def fixture_cases():
    g = np.load(GOLDEN)
    for name in sorted(k[:-len("_points")] for k in g.files if k.endswith("_points")):
        for eps, ms, lab in zip(g[name + "_eps"], g[name + "_min_samples"], g[name + "_labels"]):
            yield name, g[name + "_points"], float(eps), int(ms), lab


def test_restatement_reproduces_sklearn_labels():
    n = 0
    for name, pts, eps, ms, lab in fixture_cases():
        assert pts.dtype == np.float32 and lab.dtype == np.int32 and lab.shape == (len(pts),)
        got = R.dbscan(pts, eps, ms)
        print(f"{name} eps {eps} min_samples {ms}: {len(pts)} points, clusters {lab.max() + 1}, noise {int((lab < 0).sum())}, "
              f"mismatches {int((got['labels'] != lab).sum())}")
        assert np.array_equal(got["labels"], lab)
        n += 1
    assert n >= 6 and os.path.getsize(GOLDEN) < 100 * 1024


def test_restatement_paths_agree_with_each_other_and_with_cluster_points(monkeypatch):
    """Brute force and the cKDTree path of the restatement give the same labels, pairs exactly at eps included (a lattice cloud), and
    ``cluster_points`` on the mocked entries, which build the labels stage by stage (count, link, border, finish), gives them too."""
    from mvtracker_amd import cluster_points
    hip_mock_cluster.install(monkeypatch)
    rng = np.random.default_rng(3)
    pts = (rng.integers(0, 48, (1500, 3)) / 64.0).astype(np.float32)
    pts[::17] = np.nan
    a = R.dbscan(pts, 3 / 64, 4)
    monkeypatch.setattr(R, "BRUTE", 10)
    b = R.dbscan(pts, 3 / 64, 4)
    d2 = ((pts[:200, None].astype(np.float64) - pts[None, :200]) ** 2).sum(-1)
    print("clusters", a["labels"].max() + 1, "pairs exactly at eps among the first 200", int((d2 == 9 / 4096).sum()))
    assert (d2 == 9 / 4096).any() and a["labels"].max() >= 1
    assert np.array_equal(a["labels"], b["labels"]) and np.array_equal(a["core"], b["core"])
    got, info = cluster_points(torch.from_numpy(pts), 3 / 64, 4, return_info=True)
    assert np.array_equal(got.numpy(), a["labels"]) and np.array_equal(info["core"].numpy(), a["core"])


def test_fixture_margin_condition():
    for name, pts, eps, ms, lab in fixture_cases():
        gap = R.min_pair_gap(pts, eps)
        print(f"{name} eps {eps}: smallest |d2 - eps^2| / eps^2 = {gap:.3g}")
        assert gap > MARGIN


def test_exports_and_constants(tmp_path):
    import shutil
    import subprocess
    import mvtracker_amd
    from mvtracker_amd import RegionCluster, RegionReport, cluster, cluster_points, hip, region_masks, select_region_points
    assert cluster_points is cluster.cluster_points and region_masks is cluster.region_masks and select_region_points is cluster.select_region_points
    assert RegionCluster is cluster.RegionCluster and RegionReport is cluster.RegionReport
    assert {"cluster", "RegionCluster", "RegionReport", "cluster_points", "select_region_points", "region_masks"} <= set(mvtracker_amd.__all__)
    assert all(n in hip.SIGNATURES for n in ("mvt_cluster_crop", "mvt_cluster_count", "mvt_cluster_link", "mvt_cluster_border", "mvt_cluster_finish"))
    assert hip.abi_version() == 9
    r = RegionCluster()
    assert (r.box, r.eps, r.min_samples, r.conf_thresh) == (((-0.08, 0.08), (-0.07, 0.07), (-0.04, 0.18)), 0.03, 12, None)  # the reference's
    assert r.bounds == (-0.08, 0.08, -0.07, 0.07, -0.04, 0.18) and RegionCluster(box=None).bounds is None
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    names = {"MVT_CLUSTER_" + k.upper(): i for i, k in enumerate(cluster.STATE_FIELDS)}
    assert [getattr(hip, "CLUSTER_" + k.upper()) for k in cluster.STATE_FIELDS] == list(range(8)) and R.STATE_FIELDS == cluster.STATE_FIELDS
    names.update(MVT_CLUSTER_STATE_WORDS=hip.CLUSTER_STATE_WORDS, MVT_CLUSTER_FEW=hip.CLUSTER_FEW, MVT_CLUSTER_NONE=hip.CLUSTER_NONE,
                 MVT_CLUSTER_EMPTY=hip.CLUSTER_EMPTY)
    assert (R.FEW, R.NONE, R.EMPTY) == (hip.CLUSTER_FEW, hip.CLUSTER_NONE, hip.CLUSTER_EMPTY)
    lines = ['#include <stdio.h>', '#include "mvtracker_hip.h"', 'int main(void) {'] + [f'  printf("{n} %d\\n", {n});' for n in names] + ['  return 0;', '}']
    (tmp_path / "probe.c").write_text("\n".join(lines))
    p = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True).stdout.strip().split("\n"))
    assert {k: int(v) for k, v in got.items()} == names


def test_entries_refuse_bad_arguments_without_a_launch():
    """Every mvt_cluster_* entry returns MVT_ERR_ARG (1) for null or misaligned pointers and shapes it refuses, before any HIP call
    (so this runs without a device)."""
    import ctypes
    from mvtracker_amd import hip
    lib = hip._lib
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.addressof(buf) + 15) // 16 * 16  # host memory: only looked at for alignment, never launched on
    b6 = (ctypes.c_float * 6)(-1, 1, -1, 1, -1, 1)
    rc = {
        "crop null": lib.mvt_cluster_crop(None, 1, 64, a, b6, None),
        "crop misaligned": lib.mvt_cluster_crop(a + 4, 1, 64, a, b6, None),
        "crop empty box": lib.mvt_cluster_crop(a, 1, 64, a, (ctypes.c_float * 6)(-1, 1, 1, 1, -1, 1), None),
        "crop infinite box": lib.mvt_cluster_crop(a, 1, 64, a, (ctypes.c_float * 6)(-1, float("inf"), -1, 1, -1, 1), None),
        "crop no clouds": lib.mvt_cluster_crop(a, 0, 64, a, b6, None),
        "count null": lib.mvt_cluster_count(None, 1, 64, 0, 0, 0.01, 3, a, a, a, None),
        "count r2": lib.mvt_cluster_count(a, 1, 64, 0, 0, 0.0, 3, a, a, a, None),
        "count r2 nan": lib.mvt_cluster_count(a, 1, 64, 0, 0, float("nan"), 3, a, a, a, None),
        "count min_samples": lib.mvt_cluster_count(a, 1, 64, 0, 0, 0.01, 0, a, a, a, None),
        "count grid": lib.mvt_cluster_count(a, 1, 64, 12, 8, 0.01, 3, a, a, a, None),
        "count grid size": lib.mvt_cluster_count(a, 1, 64, 16, 8, 0.01, 3, a, a, a, None),
        "count too many clouds": lib.mvt_cluster_count(a, 70000, 64, 0, 0, 0.01, 3, a, a, a, None),
        "count too many points": lib.mvt_cluster_count(a, 1, 1 << 31, 0, 0, 0.01, 3, a, a, a, None),
        "link null parent": lib.mvt_cluster_link(a, 1, 64, 0, 0, 0.01, a, a, a, None, a, None),
        "link misaligned state": lib.mvt_cluster_link(a, 1, 64, 0, 0, 0.01, a, a, a, a, a + 4, None),
        "link no points": lib.mvt_cluster_link(a, 1, 0, 0, 0, 0.01, a, a, a, a, a, None),
        "border null root": lib.mvt_cluster_border(a, 1, 64, 0, 0, 0.01, a, a, a, a, None, None),
        "border boxes": lib.mvt_cluster_border(a, 1, 64, 0, 0, 0.01, a + 4, a, a, a, a, None),
        "finish null labels": lib.mvt_cluster_finish(a, 1, 64, 3, a, a, a, None, a, a, None),
        "finish min_samples": lib.mvt_cluster_finish(a, 1, 64, 0, a, a, a, a, a, a, None),
        "finish null select": lib.mvt_cluster_finish(a, 1, 64, 3, a, a, a, a, None, a, None),
    }
    print(rc)
    assert all(v == 1 for v in rc.values()), rc


def small_clip(V=2, T=3, H=16, W=24):
    s = Cs.scene(V, H, W, T)
    return {k: torch.from_numpy(v) for k, v in s.items()}


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    from mvtracker_amd import RegionCluster, cluster, cluster_points, queries, region_masks, select_region_points
    hip_mock_cluster.install(monkeypatch)
    for kw in (dict(box=((0, 1), (0, 1))), dict(box=((0, 1), (0, 1), (1, 0))), dict(box=((0, 1), (0, 1), (0, float("inf")))), dict(box=5),
               dict(box=((0, 1), (0, 1), (0.5, 0.5))), dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(eps=float("inf")),
               dict(min_samples=0), dict(min_samples=2.5), dict(min_samples=-3), dict(conf_thresh=float("nan"))):
        with pytest.raises(ValueError):
            RegionCluster(**kw)
    pts = torch.zeros(5, 3)
    for kw in (dict(points=torch.zeros(5, 4)), dict(points=torch.zeros(5)), dict(eps=0.0), dict(eps=float("nan")), dict(min_samples=0), dict(min_samples=1.5)):
        with pytest.raises(ValueError):
            cluster_points(**dict(dict(points=pts), **kw))
    eye = torch.eye(4, dtype=torch.float64)
    for kw in (dict(points=torch.zeros(5, 2)), dict(pose=torch.eye(3)), dict(pose=torch.zeros(4, 4)), dict(pose=eye * float("nan")), dict(region="box")):
        with pytest.raises(ValueError):
            select_region_points(**dict(dict(points=pts, pose=eye, region=RegionCluster()), **kw))
    c = small_clip()
    d, K, E = c["depths"], c["intrs"], c["extrs"]
    region = RegionCluster(BOX, EPS, MS)
    for args, kw in (((d[0, :, :, 0], K[0], E[0], eye, region), {}), ((d, K[0], E[0], eye, region), {}), ((d[0], K[0, :1], E[0], eye, region), {}),
                     ((d[0], K[0], E[0], torch.eye(4)[None].expand(2, 4, 4), region), {}), ((d[0], K[0], E[0], None, region), {}),
                     ((d[0], K[0], E[0], eye, None), {}), ((d[0], K[0], E[0], eye, region), dict(depths_conf=d[0, :, :1])),
                     ((torch.cat([d, d]), torch.cat([K, K]), torch.cat([E, E]), eye, region), {})):
        with pytest.raises(ValueError):
            region_masks(*args, **kw)
    spec = [(0, -10.0, 10.0, 100.0, 5, "")]
    for kw in (dict(region="box"), dict(region=region), dict(region=region, region_poses=torch.eye(4)[None].expand(2, 4, 4)), dict(region_poses=eye)):
        with pytest.raises(ValueError):
            queries.sample_queries(d, K, E, spec, **kw)
    print("entries called", hip_mock_cluster.calls)
    assert hip_mock_cluster.calls == []
    assert cluster_points(torch.zeros(0, 3)).shape == (0,) and select_region_points(torch.zeros(0, 3), eye).shape == (0,)
    assert hip_mock_cluster.calls == []
    assert cluster.check_dbscan(0.5, 3) == (0.5, 3)


def test_pose_inverse():
    from mvtracker_amd import cluster
    poses = np.stack([Cs.rigid(25.0, (0.3, -0.5, 0.8), (0.4, -1.2, 2.5)), Cs.rigid(-140.0, (1.0, 0.2, 0.1), (-3.0, 0.5, 0.25))])
    got = cluster.invert_poses(torch.from_numpy(poses), 2)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3, 4)
    for i in range(2):
        exp = R.region_T_world(poses[i])
        err = float(np.abs(got[i].numpy().astype(np.float64) - np.linalg.inv(poses[i])[:3]).max())
        print("pose", i, "largest difference from the fp64 inverse", err)
        assert np.array_equal(got[i].numpy(), exp) and err <= 2.0 ** -24 * 4  # rounded once: half an ulp of entries below 4
    one = cluster.invert_poses(poses[0], 3)  # one pose for every frame
    assert tuple(one.shape) == (3, 3, 4) and all(np.array_equal(one[i].numpy(), R.region_T_world(poses[0])) for i in range(3))
    assert np.array_equal(cluster.invert_poses(poses[0].astype(np.float32).tolist()).numpy()[0], R.region_T_world(poses[0].astype(np.float32)))
    assert cluster.radius_sq(0.03) == float(np.float32(0.03 ** 2)) == R.r2_of(0.03)


def clip_case(monkeypatch, V=2, T=3):
    from mvtracker_amd import RegionCluster
    hip_mock_cluster.install(monkeypatch)
    c = small_clip(V, T)
    poses = np.stack([Cs.rigid(10.0 * t, (0.2, 0.4, 1.0), np.add(Cs.SPHERES[1][0], (0.1 * t, 0.0, 0.0))) for t in range(T)])
    return c, poses, RegionCluster(BOX, EPS, MS)


def expected_masks(c, poses, region, monkeypatch):
    """Per (view, frame): the restatement on the mock's own clouds."""
    import hip_mock_clean
    from mvtracker_amd import clean
    pts = clean.clean_clip(c["depths"][0], c["intrs"][0], c["extrs"][0], clean.DepthCleaning(), details=True)[3].numpy()
    V, T = pts.shape[:2]
    return pts, [[R.select(pts[v, t].reshape(-1, 4), poses[t], region.box, region.eps, region.min_samples) for t in range(T)] for v in range(V)]


def test_region_masks_report_and_chunking(monkeypatch):
    from mvtracker_amd import cluster, region_masks
    c, poses, region = clip_case(monkeypatch)
    pts, exp = expected_masks(c, poses, region, monkeypatch)
    V, T, H, W = pts.shape[:4]
    del hip_mock_cluster.calls[:], hip_mock_cluster.shapes[:]
    mask, report = region_masks(c["depths"], c["intrs"], c["extrs"], poses, region)
    assert hip_mock_cluster.calls == ["cluster_crop", "cluster_count", "cluster_link", "cluster_border", "cluster_finish"]
    assert hip_mock_cluster.shapes == [(V * T, H * W)] and mask.shape == c["depths"].shape and mask.dtype == torch.bool
    for v in range(V):
        for t in range(T):
            assert np.array_equal(mask[0, v, t, 0].numpy().reshape(-1), exp[v][t]["select"]), (v, t)
            for k in R.STATE_FIELDS:
                assert int(getattr(report, k)[v, t]) == exp[v][t]["state"][k], (v, t, k)
            assert int(report.selected[v, t]) == int(exp[v][t]["select"].sum())
    print(report.table())
    print(report.summary())
    assert report.candidates.shape == (V, T) and report.candidates.sum() > 0 and len(report.table().split("\n")) == 1 + V * T
    assert report.summary().startswith(f"{V * T} clouds: {int(mask.sum())} points selected of {int(report.candidates.sum())} in the box")
    # chunked: one frame per launch sequence, the same result
    del hip_mock_cluster.calls[:], hip_mock_cluster.shapes[:]
    monkeypatch.setattr(cluster, "MAX_CHUNK_POINTS", V * H * W)
    mask2, report2 = region_masks(c["depths"][0], c["intrs"][0], c["extrs"][0], torch.from_numpy(poses), region)
    assert hip_mock_cluster.shapes == [(V, H * W)] * T and len(hip_mock_cluster.calls) == 5 * T
    assert torch.equal(mask2, mask[0]) and all(np.array_equal(getattr(report, k), getattr(report2, k)) for k in R.STATE_FIELDS + ("selected",))
    # no box: no crop, no poses needed
    del hip_mock_cluster.calls[:]
    m3 = region_masks(c["depths"], c["intrs"], c["extrs"], None, cluster.RegionCluster(None, EPS, MS))[0]
    assert "cluster_crop" not in hip_mock_cluster.calls and m3.any()
    # the status word raises
    from mvtracker_amd import hip
    st = torch.zeros(2, 8, dtype=torch.int64)
    cluster.check_status(st)
    st[1, hip.CLUSTER_STATUS] = 1
    with pytest.raises(hip.HipError):
        cluster.check_status(st)


def test_point_list_entries_on_the_mock(monkeypatch):
    from mvtracker_amd import RegionCluster, cluster_points, select_region_points
    hip_mock_cluster.install(monkeypatch)
    name, pts, eps, ms, lab = next(fixture_cases())
    bad = np.concatenate([pts, [[np.nan, 0, 0], [0, np.inf, 0]]]).astype(np.float32)
    got, info = cluster_points(torch.from_numpy(bad), eps, ms, return_info=True)
    assert got.dtype == torch.int32 and np.array_equal(got.numpy()[:-2], lab) and got.numpy()[-2:].tolist() == [-1, -1]
    assert info["candidates"] == len(pts) and info["clusters"] == lab.max() + 1 and info["noise"] == int((lab < 0).sum()) and info["status"] == 0
    assert info["core"].dtype == torch.bool and np.array_equal(info["core"].numpy()[:-2], R.dbscan(pts, eps, ms)["core"])
    pose = Cs.rigid(30.0, (0.1, 0.9, 0.2), (0.05, -0.02, 0.01))
    box = ((-0.2, 0.1), (-0.1, 0.2), (-0.15, 0.15))
    sel = select_region_points(torch.from_numpy(bad), torch.from_numpy(pose), RegionCluster(box, eps, ms))
    exp = R.select(bad, pose, box, eps, ms)
    print("selected", int(sel.sum()), "state", exp["state"])
    assert sel.dtype == torch.bool and np.array_equal(sel.numpy(), exp["select"]) and 0 < exp["select"].sum() < exp["state"]["candidates"]
    assert not torch.isnan(torch.from_numpy(pts)).any()  # (the crop worked on a copy)


def test_sample_queries_region(monkeypatch):
    from mvtracker_amd import EvaluationPredictor, queries, region_masks
    c, poses, region = clip_case(monkeypatch)
    d, K, E = c["depths"], c["intrs"], c["extrs"]
    pts, exp = expected_masks(c, poses, region, monkeypatch)
    V = pts.shape[0]
    spec = [(1, -10.0, 10.0, 100.0, 7, ""), (2, -10.0, 10.0, 100.0, 10 ** 6, ""), (0, -10.0, 10.0, 100.0, 4, "kmeans")]
    # region=None: not one cluster entry, and the bits of a call that does not name the arguments at all
    del hip_mock_cluster.calls[:]
    plain = queries.sample_queries(d, K, E, spec, seed=5)
    assert hip_mock_cluster.calls == [] and torch.equal(plain, queries.sample_queries(d, K, E, spec, seed=5, region=None, region_poses=None))
    assert hip_mock_cluster.calls == []
    q = queries.sample_queries(d, K, E, spec, seed=5, region=region, region_poses=poses)
    assert hip_mock_cluster.calls.count("cluster_finish") == 3  # one frame per spec row
    pools = [np.concatenate([pts[v, t].reshape(-1, 4)[exp[v][t]["select"]][:, :3] for v in range(V)]) for t in range(3)]
    print("pool sizes", [len(p) for p in pools], "queries", tuple(q.shape))
    n2 = len(pools[2])
    assert min(len(p) for p in pools) > 7 and tuple(q.shape) == (1, 7 + n2 + 4, 4)
    rows = q[0].numpy()
    assert (rows[:7, 0] == 1).all() and (rows[7:7 + n2, 0] == 2).all() and (rows[7 + n2:, 0] == 0).all()
    for t, r in ((1, rows[:7]), (2, rows[7:7 + n2])):
        pool = {tuple(p) for p in pools[t].tolist()}
        assert all(tuple(x) in pool for x in r[:, 1:].tolist()), t
    assert {tuple(x) for x in rows[7:7 + n2, 1:].tolist()} == {tuple(p) for p in pools[2].tolist()}  # a count above the pool: the pool whole
    assert ((rows[7 + n2:, 1:] >= pools[0].min(0)) & (rows[7 + n2:, 1:] <= pools[0].max(0))).all()  # centres inside the pool's box
    assert torch.equal(q, queries.sample_queries(d, K, E, spec, seed=5, region=region, region_poses=torch.from_numpy(poses)))
    assert torch.equal(q, EvaluationPredictor.sample_queries(d, K, E, spec, seed=5, region=region, region_poses=poses))
    # rows that share a frame share its mask: one launch sequence, and the reports come back per frame
    del hip_mock_cluster.calls[:]
    reports = {}
    two = queries.sample_queries(d, K, E, [spec[0], (1, -10.0, 10.0, 100.0, 3, "kmeans"), spec[1]], seed=5, region=region, region_poses=poses,
                                 region_reports=reports)
    assert hip_mock_cluster.calls.count("cluster_finish") == 2 and sorted(reports) == [1, 2] and tuple(two.shape) == (1, 7 + 3 + n2, 4)
    assert torch.equal(two[:, :7], q[:, :7])
    for t in (1, 2):
        assert reports[t].candidates.shape == (V, 1) and [int(x) for x in reports[t].selected[:, 0]] == [int(exp[v][t]["select"].sum()) for v in range(V)]
    # with a confidence map the masked pixels leave the pool too
    conf = torch.ones_like(d)
    qc = queries.sample_queries(d, K, E, spec[:2], depths_conf=conf, seed=5, region=region, region_poses=poses)
    assert torch.equal(qc, q[:, :7 + n2])
    # a single pose for all frames
    one = queries.sample_queries(d, K, E, spec[:1], seed=5, region=region, region_poses=poses[1])
    assert torch.equal(one, q[:, :7])
    # an empty region pool is an empty pool
    far = np.eye(4)
    far[:3, 3] = 50.0
    with pytest.raises(ValueError):
        queries.sample_queries(d, K, E, spec[:1], region=region, region_poses=far)


def test_demo_flags():
    import demo_amd
    ap = demo_amd.build_parser()
    a = ap.parse_args(["--synthetic"])
    assert demo_amd.query_region_from_args(a) == (None, None)
    a = ap.parse_args(["--synthetic", "--sample-queries", "kmeans", "--query-region-box", "-0.08", "0.08", "-0.07", "0.07", "-0.04", "0.18",
                       "--query-region-pose", *[str(v) for v in Cs.rigid(10.0, (0, 0, 1), (0.5, 0.25, 1.0)).reshape(-1)],
                       "--query-region-eps", "0.05", "--query-region-min-samples", "8"])
    region, poses = demo_amd.query_region_from_args(a)
    assert region.box == ((-0.08, 0.08), (-0.07, 0.07), (-0.04, 0.18)) and (region.eps, region.min_samples) == (0.05, 8)
    assert poses.shape == (4, 4) and np.allclose(poses, Cs.rigid(10.0, (0, 0, 1), (0.5, 0.25, 1.0)))
    region, poses = demo_amd.query_region_from_args(ap.parse_args(["--synthetic", "--sample-queries", "random", "--query-region-box", "0", "1", "0", "1", "0", "1"]))
    assert np.array_equal(poses, np.eye(4)) and (region.eps, region.min_samples) == (0.03, 12)
    for bad in (["--synthetic", "--query-region-box", "0", "1", "0", "1", "0", "1"],
                ["--synthetic", "--sample-queries", "random", "--query-region-pose", *["1"] * 16],
                ["--synthetic", "--sample-queries", "random", "--query-region-box", "0", "1", "0", "1", "0", "1", "--query-region-pose-key", "ee"]):
        with pytest.raises(SystemExit):
            demo_amd.query_region_from_args(ap.parse_args(bad))


def test_demo_pose_key(tmp_path):
    import demo_amd
    poses = np.stack([Cs.rigid(5.0 * t, (0, 1, 0), (t, 0, 0)) for t in range(6)])
    path = tmp_path / "sample.npz"
    np.savez(path, ee_pose=poses)
    ap = demo_amd.build_parser()
    base = ["--sample-path", str(path), "--sample-queries", "random", "--query-region-box", "0", "1", "0", "1", "0", "1", "--query-region-pose-key"]
    got = demo_amd.query_region_from_args(ap.parse_args(base + ["ee_pose"]), temporal_stride=2)[1]
    assert np.array_equal(got, poses[::2])
    with pytest.raises(SystemExit):
        demo_amd.query_region_from_args(ap.parse_args(base + ["missing"]))
