"""Rigid object motion, host side (no GPU): the host code of mvtracker_amd/rigid.py and the ``rigid_motion`` hook of the predictor on
mocked kernels (tests/hip_mock_rigid.py) against the restatement tests/rigid_ref.py: option checks, the entries called and their
order, no launch without ``rigid_motion``, at most the one documented host read, the predictor's wiring (caller rows only,
``last_rigid_motion`` reset), ``fill_tracks`` keeping untouched bits, ``move_points`` returning its input at t = f, the demo's flags,
the entries' refusals, and the restatement pinned to the reference's ``align_umeyama`` (tests/golden/rigid_umeyama.npz)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hip_mock_rigid  # noqa: E402
import rigid_ref as R  # noqa: E402
from test_mask_queries_host import _GroupedModel, _predictor_inputs  # noqa: E402

from mvtracker_amd import synth  # noqa: E402

EPS = 2.0 ** -23


@pytest.fixture(scope="module")
def clip():
    c = R.planted_clip(4)
    c["ref"] = R.rigid_motion(c["tracks"], c["visibility"], c["query_frames"], c["object_ids"])
    return c


def tensors(c):
    return [torch.from_numpy(c[k]) for k in ("tracks", "visibility", "query_frames", "object_ids")]


def test_exports_and_option_checks():
    import mvtracker_amd
    from mvtracker_amd import RigidMotion, hip, rigid
    names = {"rigid", "RigidMotion", "RigidMotionResult", "rigid_motion", "move_points", "fill_tracks"}
    assert names <= set(mvtracker_amd.__all__) and all(getattr(mvtracker_amd, n) is getattr(rigid, n) for n in names - {"rigid"})
    assert all(n in hip.SIGNATURES for n in ("mvt_rigid_members", "mvt_rigid_fit", "mvt_rigid_compose", "mvt_rigid_move", "mvt_rigid_fill"))
    assert hip.abi_version() == 9
    o = RigidMotion()
    assert (o.inlier_threshold, o.iterations, o.min_points, o.use_visibility, o.min_spread, o.live_before_query) == tuple(R.options().values())
    with pytest.raises(Exception):
        o.iterations = 2  # frozen
    for kw in (dict(inlier_threshold=-1e-3), dict(inlier_threshold=float("nan")), dict(inlier_threshold=True), dict(inlier_threshold="0.1"),
               dict(iterations=0), dict(iterations=1.5), dict(iterations=65), dict(iterations=True), dict(min_points=2), dict(min_points=4.5),
               dict(use_visibility=1), dict(live_before_query=0), dict(min_spread=-1.0), dict(min_spread=float("inf"))):
        with pytest.raises(ValueError):
            RigidMotion(**kw)
    assert RigidMotion(iterations=2.0, min_points=np.int64(3), inlier_threshold=1).iterations == 2


def test_entries_order_reads_and_result(monkeypatch, clip):
    from mvtracker_amd import RigidMotion, rigid_motion
    hip_mock_rigid.install(monkeypatch)
    tr, vis, qf, ids = tensors(clip)
    res = rigid_motion(tr, vis, qf.long(), ids.long())
    assert hip_mock_rigid.calls == ["rigid_members", "rigid_fit"] and hip_mock_rigid.reads == [()]  # the one read: the largest id
    ref = clip["ref"]
    for k in ("poses", "reference_frames", "inliers", "residual", "used", "inlier_count", "rmse", "status"):
        got = getattr(res, k)
        assert got.dtype == torch.from_numpy(ref[k]).dtype and np.array_equal(got.numpy(), ref[k], equal_nan=True), k
    assert res.poses.shape == (9, 5, 4, 4) and res.inliers.shape == (5, 1100) and res.num_objects == 9
    assert "9 objects x 5 frames" in res.summary() and len(res.table().split("\n")) == 10
    # num_objects given: nothing is read back, and the objects beyond the ids are empty
    del hip_mock_rigid.calls[:], hip_mock_rigid.reads[:]
    res = rigid_motion(tr, vis, qf, ids, RigidMotion(iterations=1), num_objects=12)
    assert hip_mock_rigid.calls == ["rigid_members", "rigid_fit"] and hip_mock_rigid.reads == []
    assert res.poses.shape[0] == 12 and bool((res.status[9:] == R.TOO_FEW).all()) and bool((res.reference_frames[9:] == -1).all())
    # fewer objects than ids: the ids beyond take no part
    res = rigid_motion(tr, vis, qf, ids, num_objects=7)
    assert bool(torch.isnan(res.residual[:, ids >= 7]).all()) and not bool(res.inliers[:, ids >= 7].any())
    # no object at all: not one launch
    del hip_mock_rigid.calls[:], hip_mock_rigid.reads[:]
    res = rigid_motion(tr, vis, qf, torch.full_like(ids, -1))
    assert hip_mock_rigid.calls == [] and res.poses.shape == (0, 5, 4, 4) and bool(torch.isnan(res.residual).all()) and not bool(res.inliers.any())


def test_refusals_before_any_launch(monkeypatch, clip):
    from mvtracker_amd import RigidMotion, fill_tracks, move_points, rigid_motion
    hip_mock_rigid.install(monkeypatch)
    tr, vis, qf, ids = tensors(clip)
    for bad in ((tr.double(), vis, qf, ids), (tr[None], vis, qf, ids), (tr[..., :2], vis, qf, ids), (tr, vis.float(), qf, ids), (tr, vis[:, :-1], qf, ids),
                (tr, vis, qf.float(), ids), (tr, vis, qf[:-1], ids), (tr, vis, qf, ids > 0), (tr, vis, qf, ids[None])):
        with pytest.raises(ValueError):
            rigid_motion(*bad)
    with pytest.raises(ValueError):
        rigid_motion(tr, vis, qf, ids, dict(iterations=3))
    with pytest.raises(ValueError):
        rigid_motion(tr, vis, qf, ids, num_objects=-1)
    assert hip_mock_rigid.calls == []
    res = rigid_motion(tr, vis, qf, ids, RigidMotion(), num_objects=9)
    del hip_mock_rigid.calls[:]
    pts, oid = torch.zeros(6, 3), torch.zeros(6, dtype=torch.int32)
    for bad in ((pts.double(), oid), (pts[:, :2], oid), (pts, oid[:-1]), (pts, oid.float())):
        with pytest.raises(ValueError):
            move_points(*bad, res)
    for f in (-1, 5, 1.5):
        with pytest.raises(ValueError):
            move_points(pts, oid, res, frame=f)
    with pytest.raises(ValueError):
        move_points(pts, oid, clip["ref"])
    for rep in ((), ("hidden",), "visible"):
        with pytest.raises(ValueError):
            fill_tracks(tr, vis, res, rep)
    with pytest.raises(ValueError):
        fill_tracks(tr[:, :-1], vis[:, :-1], res)
    assert hip_mock_rigid.calls == []


def test_fill_tracks_keeps_untouched_bits(monkeypatch, clip):
    from mvtracker_amd import fill_tracks, rigid_motion
    hip_mock_rigid.install(monkeypatch)
    tr, vis, qf, ids = tensors(clip)
    res = rigid_motion(tr, vis, qf, ids, num_objects=9)
    del hip_mock_rigid.calls[:]
    out, filled = fill_tracks(tr, vis, res)
    assert hip_mock_rigid.calls == ["rigid_fill"] and hip_mock_rigid.reads == []
    f = filled.numpy()
    assert filled.dtype == torch.bool and 0 < f.sum() < f.size and not (f & clip["visibility"]).any()
    assert np.array_equal(out.numpy()[~f].view(np.uint32), clip["tracks"][~f].view(np.uint32))
    # a filled point is its object's pose applied to the member's reference point
    t, i = np.argwhere(f)[0]
    g = clip["object_ids"][i]
    P = clip["tracks"][clip["ref"]["reference_frames"][g], i].astype(np.float64)
    A = clip["ref"]["poses"][g, t].astype(np.float64)
    assert np.array_equal(out.numpy()[t, i], (A[:3, :3] @ P + A[:3, 3]).astype(np.float32))
    both, f_both = fill_tracks(tr, vis, res, ("occluded", "outliers"))
    only, f_only = fill_tracks(tr, vis, res, "outliers")
    assert bool((f_both >= filled).all()) and torch.equal(f_both, f_only | filled) and int(f_only.sum()) > 0
    live = torch.from_numpy(np.arange(5)[:, None] >= clip["query_frames"][None])
    assert not bool((f_both & ~live).any())  # before its query frame a track is not live: never filled


def test_move_points_round_trip_and_nan(monkeypatch, clip):
    """frame=f at t = f: the composed transform is R R^T ~ I, so out - p = (R R^T - I)(p - t), every entry of R R^T - I within
    4 * 2^-23 (the bar of the GPU test on the poses), plus the output's own rounding."""
    from mvtracker_amd import move_points, rigid_motion
    hip_mock_rigid.install(monkeypatch)
    tr, vis, qf, ids = tensors(clip)
    res = rigid_motion(tr, vis, qf, ids, num_objects=9)
    del hip_mock_rigid.calls[:]
    rng = np.random.default_rng(0)
    pts = rng.uniform(-1, 1, size=(400, 3)).astype(np.float32)
    oid = rng.integers(-1, 10, size=400).astype(np.int32)
    f = 3
    out = move_points(torch.from_numpy(pts), torch.from_numpy(oid).long(), res, frame=f).numpy()
    assert hip_mock_rigid.calls == ["rigid_compose", "rigid_move"] and hip_mock_rigid.reads == [] and out.shape == (5, 400, 3)
    st = clip["ref"]["status"]
    valid = (oid >= 0) & (oid < 9)
    ok = valid[None] & (st[np.clip(oid, 0, 8)].T == 0) & (st[np.clip(oid, 0, 8), f] == 0)[None]
    assert np.array_equal(np.isfinite(out).all(-1), ok) and np.isnan(out[~ok]).all() and ok[f].sum() > 100
    t_norm = np.abs(clip["ref"]["poses"][np.clip(oid, 0, 8), f, :3, 3]).max(-1)
    bar = 3 * 4 * EPS * (np.abs(pts).max(-1) + t_norm) + np.spacing(np.abs(pts).max(-1))
    err = np.abs(out[f] - pts).max(-1)
    print("round trip: worst", (err[ok[f]] / bar[ok[f]]).max(), "bars")
    assert (err[ok[f]] <= bar[ok[f]]).all()
    # frame=None: pose[g, t] p, the restatement's bits
    out = move_points(torch.from_numpy(pts), torch.from_numpy(oid), res).numpy()
    assert np.array_equal(out, R.move_points(pts, oid, clip["ref"]["poses"], st), equal_nan=True)
    assert move_points(torch.zeros(0, 3), torch.zeros(0, dtype=torch.int32), res).shape == (5, 0, 3)


def test_predictor_wiring(monkeypatch):
    """Caller rows only (no support point), the ids of query_groups or object 0, the thresholded visibility, the query frames of the
    queries; None: not one launch; every forward resets ``last_rigid_motion``."""
    from mvtracker_amd import EvaluationPredictor, RigidMotion
    hip_mock_rigid.install(monkeypatch)
    c = synth.make_clip(5, 2, 5, 12, 16, 1)
    model = _GroupedModel()
    p = EvaluationPredictor(model, interp_shape=None, grid_size=2, visibility_threshold=0.5)
    rgbs, d, q, k, e = _predictor_inputs(c, 9)
    q[0, :, 0] = torch.tensor([0, 1, 0, 2, 0, 0, 1, 0, 0], dtype=torch.float32)
    ids = torch.tensor([1, 0, 1, 1, 0, 0, 0, 1, 1], dtype=torch.int32)
    assert p.last_rigid_motion is None
    res = p(rgbs, d, q, k, e, query_groups=ids, rigid_motion=RigidMotion(min_points=3))
    rm = p.last_rigid_motion
    assert hip_mock_rigid.calls == ["rigid_members", "rigid_fit"] and hip_mock_rigid.reads == []
    assert rm.poses.shape == (2, 5, 4, 4) and rm.residual.shape == (5, 9) and rm.reference_frames.tolist() == [1, 2]
    ref = R.rigid_motion(res["traj_e"][0].numpy(), res["vis_e"][0].numpy(), q[0, :, 0].numpy().astype(np.int32), ids.numpy(), R.options(min_points=3))
    assert np.array_equal(rm.poses.numpy(), ref["poses"], equal_nan=True) and np.array_equal(rm.status.numpy(), ref["status"])
    assert (ref["status"] == R.OK).any()  # (the mock model translates every track by the frame number: a rigid motion)
    # without query_groups: one object of all queries
    del hip_mock_rigid.calls[:]
    p(rgbs, d, q, k, e, rigid_motion=RigidMotion())
    assert p.last_rigid_motion.poses.shape == (1, 5, 4, 4) and p.last_rigid_motion.reference_frames.tolist() == [2] and hip_mock_rigid.reads == []
    # None: not one launch, and the last result is gone
    del hip_mock_rigid.calls[:]
    p(rgbs, d, q, k, e, query_groups=ids)
    assert hip_mock_rigid.calls == [] and p.last_rigid_motion is None
    with pytest.raises(ValueError):
        p(rgbs, d, q, k, e, rigid_motion=dict())
    assert hip_mock_rigid.calls == []


def test_demo_flags(tmp_path):
    import demo_amd
    from mvtracker_amd import RigidMotion, sample_io
    parse = lambda *a: demo_amd.build_parser().parse_args(["--synthetic", *a])
    assert demo_amd.rigid_motion_from_args(parse()) is None
    assert demo_amd.rigid_motion_from_args(parse("--rigid-motion")) == RigidMotion()
    got = demo_amd.rigid_motion_from_args(parse("--rigid-motion", "--rigid-threshold", "0.05", "--rigid-iterations", "2", "--rigid-min-points", "6",
                                                "--rigid-fill", "--print-rigid", "--backward-tracking"))
    assert got == RigidMotion(inlier_threshold=0.05, iterations=2, min_points=6, live_before_query=True)
    for bad in (("--rigid-threshold", "0.1"), ("--rigid-iterations", "2"), ("--rigid-min-points", "5"), ("--rigid-fill",), ("--print-rigid",),
                ("--rigid-motion", "--rigid-iterations", "0"), ("--rigid-motion", "--rigid-min-points", "2"), ("--rigid-motion", "--rigid-threshold", "-1")):
        with pytest.raises(SystemExit):
            demo_amd.rigid_motion_from_args(parse(*bad))
    s = {"query_points_3d": torch.zeros(1, 2, 4), "object_poses": np.zeros((1, 3, 4, 4), np.float32), "rigid_inliers": np.ones((3, 2), bool),
         "rigid_status": np.zeros((1, 3), np.int32)}
    sample_io.save_result(str(tmp_path / "r.npz"), torch.zeros(1, 3, 2, 3), torch.ones(1, 3, 2, dtype=torch.bool), s, include_clip=False)
    z = np.load(tmp_path / "r.npz")
    assert z["object_poses"].shape == (1, 3, 4, 4) and z["rigid_inliers"].dtype == bool and z["rigid_status"].dtype == np.int32


def test_entries_refuse_bad_arguments_without_a_launch():
    """Every mvt_rigid_* entry returns MVT_ERR_ARG (1) for null or misaligned pointers and for sizes and options it refuses, before any
    HIP call (so this runs without a device)."""
    import ctypes
    from mvtracker_amd import hip
    lib = hip._lib
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.addressof(buf) + 15) // 16 * 16  # host memory: only looked at for alignment, never launched on
    fit = lambda **kw: lib.mvt_rigid_fit(*[kw.get(k, v) for k, v in dict(
        tracks=a, vis=a, qf=a, ids=a, off=a, mem=a, ref=a, T=2, N=8, G=1, thr=0.02, it=3, mp=4, uv=1, ms=1e-3, lb=0, poses=a, res=a, inl=a, used=a,
        cnt=a, rmse=a, st=a, stream=None).items()])
    rc = {
        "members null ids": lib.mvt_rigid_members(None, a, 8, 1, 2, a, a, a, a, None),
        "members misaligned": lib.mvt_rigid_members(a, a + 2, 8, 1, 2, a, a, a, a, None),
        "members no object": lib.mvt_rigid_members(a, a, 8, 0, 2, a, a, a, a, None),
        "members too many objects": lib.mvt_rigid_members(a, a, 8, 65536, 2, a, a, a, a, None),
        "members no track": lib.mvt_rigid_members(a, a, 0, 1, 2, a, a, a, a, None),
        "members too many tracks": lib.mvt_rigid_members(a, a, (1 << 30) + 1, 1, 2, a, a, a, a, None),
        "fit null tracks": fit(tracks=None),
        "fit null visibility": fit(vis=None),
        "fit misaligned poses": fit(poses=a + 2),
        "fit no frame": fit(T=0),
        "fit too many frames": fit(T=65536),
        "fit negative threshold": fit(thr=-1.0),
        "fit nan threshold": fit(thr=float("nan")),
        "fit no iteration": fit(it=0),
        "fit too many iterations": fit(it=65),
        "fit two points": fit(mp=2),
        "fit nan spread": fit(ms=float("nan")),
        "fit flag": fit(uv=2),
        "compose null": lib.mvt_rigid_compose(None, a, 1, 2, -1, a, None),
        "compose misaligned xf": lib.mvt_rigid_compose(a, a, 1, 2, -1, a + 4, None),
        "compose frame beyond": lib.mvt_rigid_compose(a, a, 1, 2, 2, a, None),
        "compose frame below": lib.mvt_rigid_compose(a, a, 1, 2, -2, a, None),
        "move null out": lib.mvt_rigid_move(a, a, a, 8, 2, 1, None, None),
        "move misaligned xf": lib.mvt_rigid_move(a, a, a + 4, 8, 2, 1, a, None),
        "move no point": lib.mvt_rigid_move(a, a, a, 0, 2, 1, a, None),
        "fill in place": lib.mvt_rigid_fill(a, a, a, a, a, a, a, a, 2, 8, 1, 1, 0, a, a, None),
        "fill replace": lib.mvt_rigid_fill(a, a, a, a, a, a, a, a, 2, 8, 1, 4, 0, a + 512, a, None),
        "fill null filled": lib.mvt_rigid_fill(a, a, a, a, a, a, a, a, 2, 8, 1, 1, 0, a + 512, None, None),
    }
    assert all(v == 1 for v in rc.values()), {k: v for k, v in rc.items() if v != 1}


def test_restatement_equals_align_umeyama(golden):
    """The reference's align_umeyama(model=Q, data=P, known_scale=True) on unweighted clouds, some of which take the determinant
    correction: the restatement's one fit with all weights 1 gives its R and t."""
    z = golden("rigid_umeyama")
    n_flipped = 0
    for k in range(len(z["n"])):
        n = int(z["n"][k])
        P, Q = z["P"][k, :n], z["Q"][k, :n]
        Rm, tv, info = R.kabsch(P, Q)
        n_flipped += info["flipped"]
        assert bool(z["flipped"][k]) == info["flipped"]
        assert np.abs(Rm - z["R"][k]).max() <= 1e-12 and np.abs(tv - z["t"][k]).max() <= 1e-12, k
        # and through the whole restatement: iteration count 1, all weights 1
        tr = np.stack([P, Q]).astype(np.float32)
        if np.array_equal(tr.astype(np.float64), np.stack([P, Q])):  # (the fixture's clouds are fp32 numbers)
            ref = R.rigid_motion(tr, np.ones((2, n), bool), np.zeros(n, np.int32), np.zeros(n, np.int32), R.options(iterations=1, inlier_threshold=10.0))
            assert ref["status"][0, 1] == R.OK and np.abs(ref["poses"][0, 1, :3, :3] - z["R"][k]).max() <= EPS  # (one fp32 rounding)
    assert len(z["n"]) >= 10 and n_flipped >= 2
