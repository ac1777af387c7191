"""Motion masks, host side (no GPU): the restatement tests/motion_ref.py against the reference's recorded masks and static prefixes
(tests/golden/motion_mask.npz), bit for bit; then the host code of mvtracker_amd/motion.py and the motion path of sample_queries on
mocked kernels (tests/hip_mock_motion.py): exports, validation before any launch, T == 1, the collapsed window, the report, the
static-prefix rule at its edges, the pool restriction, the AND with a region, and that motion=None calls nothing.  Every figure is
printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_align_cases as Cs  # noqa: E402
import hip_mock_cluster  # noqa: E402
import hip_mock_motion  # noqa: E402
import motion_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "motion_mask.npz")


def fixture_clips():
    g = np.load(GOLDEN)
    for name in ("moving", "prefix", "unit"):
        frames = g[name + "_frames"] if name != "unit" else g["moving_frames"].astype(np.float32) / np.float32(255.0)
        masks = [np.unpackbits(g[f"{name}_static_{i}"])[:frames[:, :, 0].size].reshape(frames[:, :, 0].shape).astype(bool) for i in range(len(g["configs"]))]
        yield name, frames, float(g[name + "_thresh"][0]), [tuple(int(x) for x in c) for c in g["configs"]], masks, g


def test_restatement_reproduces_the_reference():
    n = 0
    for name, frames, thresh, configs, masks, g in fixture_clips():
        assert frames.shape == (2, 6, 3, 40, 70) and configs == [(-1, 7), (2, 3), (1, 0)]
        for (win, r), exp in zip(configs, masks):
            got = R.static_mask(frames, win, r, thresh)
            print(f"{name} window {win} r {r} thresh {thresh:.6g}: static {exp.mean():.3f}, mismatches {int((got != exp).sum())}")
            assert 0.5 < exp.mean() < 1.0 and np.array_equal(got, exp)
            n += 1
        if name != "unit":
            diffs = R.boundary_mean_diff(frames)
            for j, (thr, mx) in enumerate(g["prefix_rules"]):
                exp = g[f"{name}_prefix_{j}"].tolist()
                print(f"{name} prefix rule ({thr}, {int(mx)}): {exp}")
                assert R.static_prefix(diffs, frames.shape[1], thr, int(mx)) == exp
    assert n == 9 and np.load(GOLDEN)["prefix_prefix_0"].tolist() == [0, 1, 2, 3] and os.path.getsize(GOLDEN) < 256 * 1024


def test_exports_and_constants(tmp_path):
    import shutil
    import subprocess
    import mvtracker_amd
    from mvtracker_amd import MotionMask, MotionReport, hip, motion, motion_masks
    assert MotionMask is motion.MotionMask and MotionReport is motion.MotionReport and motion_masks is motion.motion_masks
    assert {"motion", "MotionMask", "MotionReport", "motion_masks"} <= set(mvtracker_amd.__all__)
    assert all(n in hip.SIGNATURES for n in ("mvt_motion_blocks", "mvt_motion_tiles", "mvt_motion_temporal", "mvt_motion_mask", "mvt_motion_report"))
    assert hip.abi_version() == 9
    m = MotionMask()
    assert (m.window, m.patch_radius, m.diff_thresh) == (-1, 7, 10.0)  # the reference's
    with pytest.raises(Exception):
        m.window = 3  # frozen
    assert hip.motion_blocks(40, 70) == 3 and hip.motion_blocks(32, 32) == 1 and hip.motion_blocks(512, 512) == 256
    assert hip.motion_tiles(40, 70) == 4 and hip.motion_tiles(32, 64) == 1 and hip.motion_tiles(33, 65) == 4
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    names = dict(MVT_MOTION_BLOCK_PIXELS=1024, MVT_MOTION_TILE_W=64, MVT_MOTION_TILE_H=32, MVT_MOTION_MAX_RADIUS=hip.MOTION_MAX_RADIUS)
    lines = ['#include <stdio.h>', '#include "mvtracker_hip.h"', 'int main(void) {'] + [f'  printf("{n} %d\\n", {n});' for n in names] + ['  return 0;', '}']
    (tmp_path / "probe.c").write_text("\n".join(lines))
    p = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True).stdout.strip().split("\n"))
    assert {k: int(v) for k, v in got.items()} == names


def test_entries_refuse_bad_arguments_without_a_launch():
    """Every mvt_motion_* entry returns MVT_ERR_ARG (1) for null or misaligned pointers and shapes it refuses, before any HIP call
    (so this runs without a device)."""
    import ctypes
    from mvtracker_amd import hip
    lib = hip._lib
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.addressof(buf) + 15) // 16 * 16  # host memory: only looked at for alignment, never launched on
    rc = {
        "temporal null": lib.mvt_motion_temporal(None, 1, 1, 2, 8, 8, 1, a, a, None),
        "temporal null out": lib.mvt_motion_temporal(a, 1, 1, 2, 8, 8, 1, None, a, None),
        "temporal one frame": lib.mvt_motion_temporal(a, 1, 1, 1, 8, 8, 1, a, a, None),
        "temporal no view": lib.mvt_motion_temporal(a, 1, 0, 2, 8, 8, 1, a, a, None),
        "temporal no pixel": lib.mvt_motion_temporal(a, 1, 1, 2, 0, 8, 1, a, a, None),
        "temporal too many images": lib.mvt_motion_temporal(a, 1, 300, 300, 8, 8, 1, a, a, None),
        "temporal too many pixels": lib.mvt_motion_temporal(a, 1, 1, 2, 1 << 16, 1 << 15, 1, a, a, None),
        "temporal misaligned floats": lib.mvt_motion_temporal(a + 2, 0, 1, 2, 8, 8, 1, a, a, None),
        "temporal misaligned partial": lib.mvt_motion_temporal(a, 1, 1, 2, 8, 8, 1, a, a + 4, None),
        "mask null": lib.mvt_motion_mask(None, 1, 2, 8, 8, 1, 1, 10.0, a, a, None),
        "mask radius": lib.mvt_motion_mask(a, 1, 2, 8, 8, 1, 16, 10.0, a, a, None),
        "mask negative radius": lib.mvt_motion_mask(a, 1, 2, 8, 8, 1, -1, 10.0, a, a, None),
        "mask negative window": lib.mvt_motion_mask(a, 1, 2, 8, 8, -1, 1, 10.0, a, a, None),
        "mask nan": lib.mvt_motion_mask(a, 1, 2, 8, 8, 1, 1, float("nan"), a, a, None),
        "mask inf": lib.mvt_motion_mask(a, 1, 2, 8, 8, 1, 1, float("inf"), a, a, None),
        "mask one frame": lib.mvt_motion_mask(a, 1, 1, 8, 8, 1, 1, 10.0, a, a, None),
        "report null": lib.mvt_motion_report(a, None, 1, 2, 8, 8, 1, a, None),
        "report misaligned": lib.mvt_motion_report(a, a, 1, 2, 8, 8, 1, a + 4, None),
        "report one frame": lib.mvt_motion_report(a, a, 1, 1, 8, 8, 1, a, None),
    }
    print(rc)
    assert all(v == 1 for v in rc.values()), rc
    assert lib.mvt_motion_blocks(0, 8) == -1 and lib.mvt_motion_blocks(1 << 16, 1 << 15) == -1 and lib.mvt_motion_tiles(8, 0) == -1


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    from mvtracker_amd import MotionMask, motion_masks, queries
    hip_mock_motion.install(monkeypatch)
    for kw in (dict(window=0), dict(window=-2), dict(window=1.5), dict(window=True), dict(patch_radius=-1), dict(patch_radius=16), dict(patch_radius=2.5),
               dict(diff_thresh=float("nan")), dict(diff_thresh=float("inf"))):
        with pytest.raises(ValueError):
            MotionMask(**kw)
    assert MotionMask(window=2.0, patch_radius=0, diff_thresh=1) == MotionMask(2, 0, 1.0)
    rgb = torch.zeros(2, 3, 3, 16, 24, dtype=torch.uint8)
    for args in ((rgb[0],), (rgb[:, :, :2],), (torch.stack([rgb, rgb]),), (rgb.to(torch.int32),), (rgb, "moving"), (rgb, None), (rgb[:, :, :, :0],)):
        with pytest.raises(ValueError):
            motion_masks(*args)
    c = {k: torch.from_numpy(v) for k, v in Cs.scene(2, 16, 24, 3).items()}
    d, K, E = c["depths"], c["intrs"], c["extrs"]
    spec = [(0, -10.0, 10.0, 100.0, 5, "")]
    for kw in (dict(motion=MotionMask()), dict(motion="moving", rgbs=rgb), dict(motion=MotionMask(), rgbs=rgb, motion_keep="both"), dict(rgbs=rgb),
               dict(motion=MotionMask(), rgbs=rgb[:1]), dict(motion=MotionMask(), rgbs=rgb[:, :2]), dict(motion=MotionMask(), rgbs=rgb[..., :20]),
               dict(motion=MotionMask(), rgbs=rgb[:, :, :, :8]), dict(motion=MotionMask(), rgbs=torch.stack([rgb, rgb]))):
        with pytest.raises(ValueError):
            queries.sample_queries(d, K, E, spec, **kw)
    with pytest.raises(NotImplementedError):  # (the method check comes first, as before)
        queries.sample_queries(d, K, E, [(0, -10.0, 10.0, 100.0, 5, "fps")], motion=MotionMask(), rgbs=rgb)
    print("entries called", hip_mock_motion.calls)
    assert hip_mock_motion.calls == [] and hip_mock_cluster.calls == []


def planted_clip(V=2, T=5, H=16, W=24, seed=0):
    """uint8 frames: a fixed image per view and a 4 x 6 block that jumps by 3 pixels per frame in view 0 and rests in view 1."""
    rng = np.random.default_rng(seed)
    rgb = np.repeat(rng.integers(30, 120, (V, 1, 3, H, W)), T, 1)
    for t in range(T):
        rgb[0, t, :, 2:6, 3 * t:3 * t + 6] += 100
        rgb[1, t, :, 8:12, 4:10] += 100
    return rgb.astype(np.uint8)


def test_motion_masks_on_the_mock(monkeypatch):
    from mvtracker_amd import MotionMask, motion_masks
    hip_mock_motion.install(monkeypatch)
    rgb = planted_clip()
    V, T, _, H, W = rgb.shape
    for cfg in (MotionMask(), MotionMask(1, 0), MotionMask(2, 3, 40.0)):
        del hip_mock_motion.calls[:], hip_mock_motion.args[:]
        static, report = motion_masks(torch.from_numpy(rgb), cfg)
        exp = R.static_mask(rgb, cfg.window, cfg.patch_radius, cfg.diff_thresh)
        print(cfg, "static", float(exp.mean()), hip_mock_motion.args)
        assert hip_mock_motion.calls == ["motion_temporal", "motion_mask", "motion_report"]
        assert hip_mock_motion.args[0] == dict(dtype=torch.uint8, shape=(V, T, H, W), all_mode=cfg.window == -1)  # uint8 stays uint8
        assert hip_mock_motion.args[1] == dict(win=max(cfg.window, 0), r=cfg.patch_radius, thresh=cfg.diff_thresh)
        assert static.dtype == torch.bool and tuple(static.shape) == (V, T, H, W) and np.array_equal(static.numpy(), exp)
        assert exp[1].all() and not exp[0].all()
        assert np.array_equal(report.static_fraction, exp.mean((2, 3))) and np.array_equal(report.boundary_mean_diff, R.boundary_mean_diff(rgb))
        batched = motion_masks(torch.from_numpy(rgb)[None].double(), cfg)[0]  # any float type goes in as fp32, the batch axis is dropped
        assert hip_mock_motion.args[-2]["dtype"] == torch.float32 and torch.equal(batched, static)
    # a window that holds every boundary is the whole-clip form: one map
    for w in (T - 1, T, T + 5):
        del hip_mock_motion.args[:]
        s = motion_masks(torch.from_numpy(rgb), MotionMask(w, 2))[0]
        assert hip_mock_motion.args[0]["all_mode"] and hip_mock_motion.args[1]["win"] == 0
        assert np.array_equal(s.numpy(), R.static_mask(rgb, -1, 2)) and np.array_equal(s.numpy(), R.static_mask(rgb, w, 2))
    del hip_mock_motion.args[:]
    motion_masks(torch.from_numpy(rgb), MotionMask(T - 2, 2))
    assert not hip_mock_motion.args[0]["all_mode"] and hip_mock_motion.args[1]["win"] == T - 2
    print(report.summary())
    print(report.table())
    assert report.summary().startswith(f"{V} views x {T} frames: ") and len(report.table().split("\n")) == 1 + T


def test_single_frame_launches_nothing(monkeypatch):
    from mvtracker_amd import MotionMask, motion_masks
    hip_mock_motion.install(monkeypatch)
    static, report = motion_masks(torch.zeros(2, 1, 3, 8, 9, dtype=torch.uint8), MotionMask(2, 3))
    assert hip_mock_motion.calls == [] and static.dtype == torch.bool and tuple(static.shape) == (2, 1, 8, 9) and bool(static.all())
    assert report.static_fraction.tolist() == [[1.0], [1.0]] and report.boundary_mean_diff.shape == (0,)
    assert report.static_prefix_frames() == [0] and "a single frame" in report.summary() and len(report.table().split("\n")) == 2


def test_static_prefix_rule_at_its_edges():
    from mvtracker_amd import MotionReport
    rep = MotionReport(np.ones((1, 6)), [0.25, 0.5, 0.5000001, 0.0, 0.0])
    assert rep.static_prefix_frames() == [0, 1, 2]  # a delta equal to the threshold is included, the first failure stops
    assert rep.static_prefix_frames(diff_threshold=0.25) == [0, 1] and rep.static_prefix_frames(diff_threshold=0.2) == [0]
    assert rep.static_prefix_frames(diff_threshold=1.0) == [0, 1, 2, 3, 4, 5]
    assert rep.static_prefix_frames(diff_threshold=1.0, max_frames=3) == [0, 1, 2] and rep.static_prefix_frames(1.0, 1) == [0]
    assert MotionReport(np.ones((2, 1)), []).static_prefix_frames() == [0]
    for thr, mx in ((0.5, 10), (0.3, 10), (1.0, 2), (1.0, 6), (1.0, 7)):
        assert rep.static_prefix_frames(thr, mx) == R.static_prefix(rep.boundary_mean_diff, 6, thr, mx)


def query_case(monkeypatch, T=4):
    from mvtracker_amd import clean
    hip_mock_motion.install(monkeypatch)
    c = {k: torch.from_numpy(v) for k, v in Cs.scene(2, 16, 24, T).items()}
    rgb = planted_clip(2, T, 16, 24, seed=4)
    pts = clean.clean_clip(c["depths"][0], c["intrs"][0], c["extrs"][0], clean.DepthCleaning(), details=True)[3].numpy()  # (V,T,H,W,4)
    return c, rgb, pts


def test_sample_queries_motion(monkeypatch):
    from mvtracker_amd import EvaluationPredictor, MotionMask, queries
    c, rgb, pts = query_case(monkeypatch)
    d, K, E = c["depths"], c["intrs"], c["extrs"]
    V, T = rgb.shape[:2]
    cfg = MotionMask(1, 1)
    static = R.static_mask(rgb, 1, 1)
    big = 10 ** 6
    spec = [(1, -10.0, 10.0, 100.0, big, ""), (2, -10.0, 10.0, 100.0, 5, ""), (1, -10.0, 10.0, 100.0, 3, "kmeans"), (0, -10.0, 10.0, 100.0, big, "")]
    # motion=None: not one motion entry, and the bits of a call that does not name the arguments at all
    plain = queries.sample_queries(d, K, E, spec, seed=5)
    assert hip_mock_motion.calls == [] and torch.equal(plain, queries.sample_queries(d, K, E, spec, seed=5, motion=None, rgbs=None))
    assert hip_mock_motion.calls == []
    reports = {}
    q = queries.sample_queries(d, K, E, spec, seed=5, motion=cfg, rgbs=torch.from_numpy(rgb)[None], motion_reports=reports)
    assert hip_mock_motion.calls == ["motion_temporal", "motion_mask", "motion_report"]  # once, for four rows over three frames
    assert hip_mock_cluster.calls == [] and sorted(reports) == ["clip"] and np.array_equal(reports["clip"].static_fraction, static.mean((2, 3)))
    ok = c["depths"][0, :, :, 0].numpy() > 0
    pools = {(t, keep): np.concatenate([pts[v, t][ok[v, t] & (static[v, t] if keep == "static" else ~static[v, t])][:, :3] for v in range(V)])
             for t in range(T) for keep in ("moving", "static")}
    print("moving pool sizes", [len(pools[(t, "moving")]) for t in range(T)], "queries", tuple(q.shape))
    n1, n0 = len(pools[(1, "moving")]), len(pools[(0, "moving")])
    assert n1 > 5 and n0 > 0 and tuple(q.shape) == (1, n1 + 5 + 3 + n0, 4)
    rows = q[0].numpy()
    # method "": the pool is the unrestricted pool filtered by the mask, in its order, behind the seeded permutation of its length
    g = torch.Generator(device="cpu").manual_seed(5)
    for (t, count), block in (((1, big), rows[:n1]), ((2, 5), rows[n1:n1 + 5])):
        pool = pools[(t, "moving")]
        perm = torch.randperm(len(pool), generator=g)[:count].numpy()
        assert (block[:, 0] == t).all() and np.array_equal(block[:, 1:], pool[perm])
    km = rows[n1 + 5:n1 + 8, 1:]
    assert ((km >= pools[(1, "moving")].min(0)) & (km <= pools[(1, "moving")].max(0))).all()  # centres inside the moving pool's box
    full = {tuple(x) for x in pts[:, 1][ok[:, 1]][:, :3].tolist()}
    assert {tuple(x) for x in rows[:n1, 1:].tolist()} < full
    # the static side is the complement within the unrestricted pool
    qs = queries.sample_queries(d, K, E, spec[:1], seed=5, motion=cfg, rgbs=torch.from_numpy(rgb), motion_keep="static")
    assert {tuple(x) for x in qs[0, :, 1:].tolist()} | {tuple(x) for x in rows[:n1, 1:].tolist()} == full
    assert qs.shape[1] + n1 == len(full) == int(ok[:, 1].sum())
    # float frames, the predictor's pass-through
    assert torch.equal(q, EvaluationPredictor.sample_queries(d, K, E, spec, seed=5, motion=cfg, rgbs=torch.from_numpy(rgb).float()))
    # nothing moves in view 1: with a threshold nothing reaches, the moving pool is empty
    with pytest.raises(ValueError):
        queries.sample_queries(d, K, E, spec, motion=MotionMask(1, 1, 1e6), rgbs=torch.from_numpy(rgb))
    # rows beyond the clip alone: no mask is computed
    del hip_mock_motion.calls[:]
    with pytest.raises(ValueError):
        queries.sample_queries(d, K, E, [(T, -10.0, 10.0, 100.0, 5, "")], motion=cfg, rgbs=torch.from_numpy(rgb))
    assert hip_mock_motion.calls == []


def test_sample_queries_motion_and_region(monkeypatch):
    from mvtracker_amd import MotionMask, RegionCluster, queries, region_masks
    c, rgb, pts = query_case(monkeypatch)
    d, K, E = c["depths"], c["intrs"], c["extrs"]
    V = rgb.shape[0]
    region = RegionCluster(((-0.45, 0.45), (-0.45, 0.45), (-0.45, 0.45)), 0.12, 6)
    pose = Cs.rigid(10.0, (0.2, 0.4, 1.0), Cs.SPHERES[1][0])
    rmask = region_masks(d, K, E, pose, region)[0][0, :, :, 0].numpy()  # (V,T,H,W)
    t = 1
    v0 = int(rmask[:, t].sum((1, 2)).argmax())
    xm = int(np.median(np.nonzero(rmask[v0, t])[1]))
    rgb = np.full_like(rgb, 90)
    rgb[v0, 2:, :, :, :xm] += 60  # the columns left of the region's middle change once, in the view that sees the region best
    cfg = MotionMask(-1, 0, 5.0)
    static = R.static_mask(rgb, -1, 0, 5.0)
    both = rmask[:, t] & static[:, t]
    print("region", int(rmask[:, t].sum()), "static", int(static[:, t].sum()), "both", int(both.sum()))
    assert 0 < both.sum() < min(rmask[:, t].sum(), static[:, t].sum())
    del hip_mock_motion.calls[:], hip_mock_cluster.calls[:]
    q = queries.sample_queries(d, K, E, [(t, -10.0, 10.0, 100.0, 10 ** 6, "")], seed=2, region=region, region_poses=pose, motion=cfg,
                               rgbs=torch.from_numpy(rgb), motion_keep="static")
    assert hip_mock_motion.calls.count("motion_mask") == 1 and hip_mock_cluster.calls.count("cluster_finish") == 1
    pool = np.concatenate([pts[v, t][both[v]][:, :3] for v in range(V)])
    perm = torch.randperm(len(pool), generator=torch.Generator(device="cpu").manual_seed(2)).numpy()
    assert np.array_equal(q[0, :, 1:].numpy(), pool[perm])


def test_demo_flags():
    import demo_amd
    ap = demo_amd.build_parser()
    a = ap.parse_args(["--synthetic"])
    assert demo_amd.query_motion_from_args(a) == (None, "moving") and not a.print_motion
    a = ap.parse_args(["--synthetic", "--sample-queries", "kmeans", "--query-motion", "moving"])
    m, keep = demo_amd.query_motion_from_args(a)
    assert (m.window, m.patch_radius, m.diff_thresh, keep) == (-1, 7, 10.0, "moving")  # the reference's defaults
    a = ap.parse_args(["--synthetic", "--sample-queries", "random", "--query-motion", "static", "--query-motion-window", "2", "--query-motion-radius", "3",
                       "--query-motion-thresh", "0.04", "--print-motion"])
    m, keep = demo_amd.query_motion_from_args(a)
    assert (m.window, m.patch_radius, m.diff_thresh, keep) == (2, 3, 0.04, "static") and a.print_motion
    for bad in (["--synthetic", "--query-motion", "moving"], ["--synthetic", "--sample-queries", "random", "--query-motion-window", "2"],
                ["--synthetic", "--sample-queries", "random", "--query-motion-radius", "3"],
                ["--synthetic", "--sample-queries", "random", "--query-motion-thresh", "3"],
                ["--synthetic", "--sample-queries", "random", "--query-motion", "moving", "--query-motion-window", "0"],
                ["--synthetic", "--sample-queries", "random", "--query-motion", "moving", "--query-motion-radius", "16"]):
        with pytest.raises(SystemExit):
            demo_amd.query_motion_from_args(ap.parse_args(bad))
    with pytest.raises(SystemExit):
        ap.parse_args(["--synthetic", "--query-motion", "both"])
