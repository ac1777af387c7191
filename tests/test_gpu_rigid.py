"""Rigid object motion on the device (`-m gpu`): mvt_rigid_members / fit / compose / move / fill through mvtracker_amd/rigid.py against
the fp64 restatement tests/rigid_ref.py.

The bars are derived, not measured.  The device and the restatement both sum in fp64: sums of at most 4096 fp32 terms on clouds whose
H has sigma_1 / (sigma_2 + sigma_3) <= 100 (asserted on the inputs below) differ by less than 1e-10, far below half an fp32 ulp, so
both round to the same fp32 number except at a rounding boundary: rotation entries (|r| <= 1) agree within 2 * 2^-23, translations
within 2 * 2^-23 * (1 + |pbar| + |qbar|), residuals and rmse within that same absolute bar; status, used, inlier_count, inliers and
reference_frames are equal -- the restatement asserts that no base member's residual lies within 5 % of the threshold in any
iteration, so no flag hangs on the last bits.  Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rigid_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 2.0 ** -23
SEED, PLANAR_SEED = 4, 0  # chosen by the margins asserted in ``clip`` and ``test_determinant_correction``, not by the recipe alone


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(c, opt_kw=None, num_objects=None):
    from mvtracker_amd import RigidMotion, rigid_motion
    return rigid_motion(dev(c["tracks"]), dev(c["visibility"]), dev(c["query_frames"]), dev(c["object_ids"]), RigidMotion(**(opt_kw or {})),
                        num_objects=num_objects)


def host(res):
    return {k: getattr(res, k).cpu().numpy() for k in ("poses", "reference_frames", "inliers", "residual", "used", "inlier_count", "rmse", "status")}


def same_bits(a, b):
    """torch.equal on the bit patterns: NaN equals NaN."""
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.is_floating_point() else torch.equal(a, b)


def ulp(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def check_against(got, ref, ids):
    """The bars of the module docstring, every figure printed before it is asserted."""
    tr = ref["trace"]
    for k in ("status", "used", "inlier_count", "inliers", "reference_frames"):
        assert np.array_equal(got[k], ref[k]), k
    ok = ref["status"] == R.OK
    assert np.isnan(got["poses"][~ok]).all() and np.isnan(got["rmse"][~ok]).all()
    bar = 2 * EPS * (1 + np.linalg.norm(tr["pbar"], axis=-1) + np.linalg.norm(tr["qbar"], axis=-1))  # (G,T)
    dR = np.abs(got["poses"][ok][:, :3, :3].astype(np.float64) - ref["poses"][ok][:, :3, :3]).max()
    dt = (np.abs(got["poses"][ok][:, :3, 3].astype(np.float64) - ref["poses"][ok][:, :3, 3]).max(-1) / bar[ok]).max()
    assert np.array_equal(got["poses"][ok][:, 3], np.tile(np.array([0, 0, 0, 1], np.float32), (ok.sum(), 1)))
    Rm = got["poses"][ok][:, :3, :3].astype(np.float64)
    det, orth = np.linalg.det(Rm), np.abs(np.einsum("nki,nkj->nij", Rm, Rm) - np.eye(3)).reshape(len(Rm), -1).max(1)
    member = ids >= 0
    g = np.where(member, ids, 0)
    assert np.array_equal(np.isnan(got["residual"]), np.isnan(ref["residual"]))
    assert np.isnan(got["residual"][:, ~member]).all() and not got["inliers"][:, ~member].any()
    with np.errstate(invalid="ignore"):
        dres = np.nanmax(np.abs(got["residual"].astype(np.float64) - ref["residual"]) / bar[g].T)
        drmse = np.nanmax(np.abs(got["rmse"].astype(np.float64) - ref["rmse"]) / bar)
    print(f"rotation {dR / EPS:.2f} eps, translation {dt:.3f} bars, residual {dres:.3f} bars, rmse {drmse:.3f} bars, det in [{det.min():.9f}, "
          f"{det.max():.9f}], |R^T R - I| {orth.max() / EPS:.2f} eps, conditioning {max(tr['cond']):.1f}, margin {min(tr['margin']):.3f}")
    assert max(tr["cond"]) <= 100
    assert dR <= 2 * EPS and dt <= 1 and dres <= 1 and drmse <= 1
    assert (det > 0).all() and (orth <= 4 * EPS).all()


@pytest.fixture(scope="module")
def clip():
    c = R.planted_clip(SEED)
    c["ref"] = R.rigid_motion(c["tracks"], c["visibility"], c["query_frames"], c["object_ids"])
    tr = c["ref"]["trace"]
    assert min(tr["margin"]) > 0.05 and max(tr["cond"]) <= 100  # the condition for exact flags, and the bars' conditioning
    return c


def test_small_clip(clip):
    ref, ids = clip["ref"], clip["object_ids"]
    T, N = clip["visibility"].shape
    counts = np.bincount(ids[ids >= 0], minlength=9)
    print("T", T, "N", N, "members", counts.tolist(), "reference frames", ref["reference_frames"].tolist())
    assert counts.tolist() == list(R.COUNTS) + [20] and (ids < 0).sum() == R.NO_OBJECT and (np.diff(ids) < 0).any()
    assert (ref["reference_frames"][1:] > 0).any() and (ref["reference_frames"] == 0).any() and np.isnan(clip["tracks"]).sum() == 1
    res = run(clip)
    got = host(res)
    check_against(got, ref, ids)
    st = ref["status"]
    assert (st[0] == R.TOO_FEW).all() and ref["reference_frames"][0] == -1 and (st[1] == R.TOO_FEW).all()  # no member; three members
    assert (st[2] == R.OK).any() and (st[3:8] == R.OK).all()
    assert (st[R.COLLINEAR][ref["used"][R.COLLINEAR] >= 4] == R.DEGENERATE).all() and (st[R.COLLINEAR] == R.DEGENERATE).any()
    # the planted outliers, and only they, are dropped wherever they are displaced (every frame but the reference frame)
    g = np.where(ids >= 0, ids, 0)
    moved = (np.arange(T)[:, None] != ref["reference_frames"][g][None]) & (st[g].T == R.OK) & (ids >= 0)[None]
    assert not got["inliers"][moved & clip["outlier"][None]].any() and clip["outlier"].sum() == sum(c // 16 for c in R.COUNTS if c >= 32)
    live = moved & ~clip["outlier"][None] & clip["visibility"] & clip["visibility"][ref["reference_frames"][g], np.arange(N)][None] \
        & (np.arange(T)[:, None] >= clip["query_frames"][None]) & np.isfinite(clip["tracks"]).all(-1)
    assert got["inliers"][live].all() and live.sum() > 1000
    t, i = clip["nan_at"]
    assert np.isnan(got["residual"][t, i]) and not got["inliers"][t, i] and got["status"][7, t] == R.OK
    # two runs: the same bits; num_objects given: the same result, and two more objects without a member
    again = run(clip)
    for k in got:
        assert same_bits(getattr(again, k), getattr(res, k)), k
    more = host(run(clip, num_objects=11))
    assert all(np.array_equal(more[k][:9] if more[k].shape[0] == 11 else more[k], got[k], equal_nan=True) for k in got)
    assert (more["status"][9:] == R.TOO_FEW).all() and (more["reference_frames"][9:] == -1).all()
    print(res.summary())
    print(res.table())


@pytest.mark.parametrize("kw", [dict(iterations=1), dict(use_visibility=False, iterations=2), dict(live_before_query=True), dict(min_points=5)])
def test_options(clip, kw):
    ref = R.rigid_motion(clip["tracks"], clip["visibility"], clip["query_frames"], clip["object_ids"], R.options(**kw))
    assert min(ref["trace"]["margin"]) > 0.05
    check_against(host(run(clip, kw)), ref, clip["object_ids"])
    if "min_points" in kw:
        assert (ref["status"][2] == R.TOO_FEW).all()


def test_a_frame_alone_equals_the_whole_call(clip):
    """Object 7 (600 members: more than one pass of the workgroup), a frame after its reference frame: the call on the rows
    tracks[[r, t]] gives that frame's bits."""
    res = run(clip)
    r = int(clip["ref"]["reference_frames"][7])
    t = r + 1
    sub = dict(tracks=clip["tracks"][[r, t]], visibility=clip["visibility"][[r, t]], query_frames=np.zeros_like(clip["query_frames"]),
               object_ids=np.where(clip["object_ids"] == 7, 7, -1).astype(np.int32))
    alone = run(sub)
    assert int(alone.reference_frames[7]) == 0 and int(alone.status[7, 1]) == R.OK
    m = dev(clip["object_ids"] == 7)
    assert same_bits(alone.poses[7, 1].contiguous(), res.poses[7, t].contiguous()) and same_bits(alone.residual[1][m], res.residual[t][m])
    assert torch.equal(alone.inliers[1][m], res.inliers[t][m]) and same_bits(alone.rmse[7, 1], res.rmse[7, t])
    assert int(alone.used[7, 1]) == int(res.used[7, t]) and int(alone.inlier_count[7, 1]) == int(res.inlier_count[7, t])


def test_planted_exact_poses():
    """Integer-grid points under rotations by multiples of 90 degrees and integer translations: every sum is exact."""
    rng = np.random.default_rng(1)
    T, counts = 6, (5, 70, 300)
    ids = np.concatenate([np.full(c, g) for g, c in enumerate(counts)])
    ids = ids[rng.permutation(len(ids))].astype(np.int32)
    N = len(ids)
    P = rng.integers(-8, 9, size=(N, 3)).astype(np.float64)
    tracks, poses = np.zeros((T, N, 3)), np.zeros((3, T, 4, 4))
    quarter = [R.rotation(a, k * np.pi / 2).round() for a in np.eye(3) for k in range(4)]
    for g in range(3):
        for t in range(T):
            Rm, tv = (np.eye(3), np.zeros(3)) if t == 0 else (quarter[rng.integers(len(quarter))], rng.integers(-20, 21, size=3).astype(np.float64))
            poses[g, t] = np.eye(4)
            poses[g, t, :3, :3], poses[g, t, :3, 3] = Rm, tv
            tracks[t, ids == g] = P[ids == g] @ Rm.T + tv
    c = dict(tracks=tracks.astype(np.float32), visibility=np.ones((T, N), bool), query_frames=np.zeros(N, np.int32), object_ids=ids)
    got = host(run(c))
    dR = np.abs(got["poses"][:, :, :3, :3] - poses[:, :, :3, :3]).max()
    pbar = np.stack([P[ids == g].mean(0) for g in range(3)])
    qbar = np.stack([[tracks[t, ids == g].mean(0) for t in range(T)] for g in range(3)])
    bar = 2 * EPS * (1 + np.linalg.norm(pbar, axis=-1)[:, None] + np.linalg.norm(qbar, axis=-1))
    dt = (np.abs(got["poses"][:, :, :3, 3] - poses[:, :, :3, 3]).max(-1) / bar).max()
    print(f"rotation {dR / EPS:.3f} eps, translation {dt:.3f} bars, residual max {got['residual'].max():.3g}")
    assert (got["status"] == R.OK).all() and dR <= 2 * EPS and dt <= 1 and got["residual"].max() <= 2.0 ** -20 and got["inliers"].all()


def test_determinant_correction():
    """Near-planar clouds with noise: some take the determinant correction (the restatement says which); the device agrees there too."""
    c = R.planar_clip(PLANAR_SEED)
    kw = dict(iterations=1, inlier_threshold=1.0)
    ref = R.rigid_motion(c["tracks"], c["visibility"], c["query_frames"], c["object_ids"], R.options(**kw))
    flipped = [(g, t) for g, t, _, f in ref["trace"]["flipped"] if f]
    print("objects that take the correction", flipped)
    assert len(flipped) >= 1 and (ref["status"] == R.OK).all()
    got = host(run(c, kw))
    check_against(got, ref, c["object_ids"])
    for g, t in flipped:  # (and without the correction the answer would have been another: a reflection)
        assert np.linalg.det(got["poses"][g, t, :3, :3].astype(np.float64)) > 0.999


@pytest.fixture(scope="module")
def motion(clip):
    return run(clip)


@pytest.mark.parametrize("M,frame", [(1000, None), (1000, 3), (1003, 3)])
def test_move_points(clip, motion, M, frame):
    """Mixed ids (-1 and ids beyond G among them), M a multiple of four (16-byte accesses) and not."""
    from mvtracker_amd import move_points
    rng = np.random.default_rng(M)
    pts = rng.uniform(-1, 1, size=(M, 3)).astype(np.float32)
    oid = rng.integers(-1, 10, size=M).astype(np.int32)
    got = move_points(dev(pts), dev(oid), motion, frame=frame).cpu().numpy()
    ref = R.move_points(pts, oid, clip["ref"]["poses"], clip["ref"]["status"], frame)
    poses = motion.poses.cpu().numpy()
    ref_dev = R.move_points(pts, oid, poses, clip["ref"]["status"], frame)  # (from the device's own fp32 poses: one rounding apart at most)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(got).any() and np.isfinite(got).sum() > M
    with np.errstate(invalid="ignore"):
        d = np.nanmax(np.abs(got.astype(np.float64) - ref_dev) / ulp(ref_dev))
    print(f"M {M} frame {frame}: {d:.2f} ulp, finite {int(np.isfinite(got).sum()) // 3} of {got.size // 3}")
    assert got.shape == (5, M, 3) and d <= 1
    if frame is not None:  # at t = frame the composed transform is R R^T ~ I: the points come back
        ok = np.isfinite(got[frame]).all(-1)
        t_norm = np.linalg.norm(poses[np.clip(oid, 0, 8), frame, :3, 3], axis=-1)[ok]
        back = np.abs(got[frame][ok] - pts[ok]).max(-1)
        assert (back <= 4 * EPS * 3 * (np.linalg.norm(pts[ok], axis=-1) + t_norm) + np.spacing(np.abs(pts[ok]).max(-1))).all()


def test_move_points_many_objects():
    """More objects than the kernel keeps in LDS (128): the transforms are read from memory."""
    from mvtracker_amd import move_points
    rng = np.random.default_rng(9)
    G, n = 150, 4
    ids = np.repeat(np.arange(G), n).astype(np.int32)
    P = rng.integers(-4, 5, size=(G, 3)).astype(np.float64)[ids] + np.tile(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]), (G, 1)) * 3.0
    tv = rng.integers(-9, 10, size=(G, 3)).astype(np.float64)
    c = dict(tracks=np.stack([P, P + tv[ids]]).astype(np.float32), visibility=np.ones((2, G * n), bool), query_frames=np.zeros(G * n, np.int32),
             object_ids=ids)
    res = run(c)
    assert bool((res.status == 0).all())
    pts = rng.integers(-5, 6, size=(601, 3)).astype(np.float32)
    oid = rng.integers(0, G, size=601).astype(np.int32)
    got = move_points(dev(pts), dev(oid), res).cpu().numpy()
    ref = R.move_points(pts, oid, res.poses.cpu().numpy(), res.status.cpu().numpy())
    # against the planted translations: 2 eps per rotation entry on |p|_1 <= 15, and the translation's bar with |pbar| <= 7 sqrt(3),
    # |qbar| <= 16 sqrt(3)
    bar = 2 * EPS * (15 + 1 + 23 * np.sqrt(3))
    assert (np.abs(got - ref) <= ulp(ref)).all() and np.abs(got[0] - pts).max() <= bar and np.abs(got[1] - (pts + tv[oid])).max() <= bar


@pytest.mark.parametrize("replace", [("occluded",), ("outliers",), ("occluded", "outliers")])
def test_fill_tracks(clip, motion, replace):
    from mvtracker_amd import fill_tracks
    tracks, vis = dev(clip["tracks"]), dev(clip["visibility"])
    out, filled = fill_tracks(tracks, vis, motion, replace)
    m = host(motion)
    ref_out, ref_filled = R.fill_tracks(clip["tracks"], clip["visibility"], clip["query_frames"], clip["object_ids"], m, replace)
    got, f = out.cpu().numpy(), filled.cpu().numpy()
    print(replace, "filled", int(f.sum()), "of", f.size)
    assert filled.dtype == torch.bool and np.array_equal(f, ref_filled) and 0 < f.sum() < f.size
    assert np.array_equal(got[~f].view(np.uint32), clip["tracks"][~f].view(np.uint32))  # everything else keeps its bits (the NaN too)
    assert (np.abs(got[f].astype(np.float64) - ref_out[f]) <= ulp(ref_out[f])).all() and np.isfinite(got[f]).all()
    if replace == ("occluded",):
        assert not (f & clip["visibility"]).any()
    # an odd track count takes the element-wise path: the same answers
    sub = {k: (v[:, :-1] if k in ("tracks", "visibility") else v[:-1]) for k, v in clip.items() if k in ("tracks", "visibility", "query_frames", "object_ids")}
    res = run(sub)
    o2, f2 = fill_tracks(dev(sub["tracks"]), dev(sub["visibility"]), res, replace)
    r2 = R.fill_tracks(sub["tracks"], sub["visibility"], sub["query_frames"], sub["object_ids"], host(res), replace)
    assert sub["tracks"].shape[1] % 4 and np.array_equal(f2.cpu().numpy(), r2[1])
    assert np.array_equal(o2.cpu().numpy()[~r2[1]].view(np.uint32), sub["tracks"][~r2[1]].view(np.uint32))
    assert (np.abs(o2.cpu().numpy()[r2[1]].astype(np.float64) - r2[0][r2[1]]) <= ulp(r2[0][r2[1]])).all()


def test_predictor_end_to_end():
    """The tiny synthetic clip of the mask-query test: forward(..., query_groups=ids, rigid_motion=RigidMotion()): at every object's
    reference frame the tracks are the reference configuration, so the status there is 0 and the pose the identity."""
    from mvtracker_amd import EvaluationPredictor, RigidMotion, synth
    from mvtracker_amd.tracker import MVTracker
    m = MVTracker(hidden_size=256).eval()
    sd = synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.to(DEV)
    m.precision = "fp32"
    c = synth.make_clip(62, V=2, T=12, H=128, W=128, N=9, late_queries=True, query_frames=(3,))
    a = [dev(c[k][0])[None] for k in ("rgbs", "depths", "query_points", "intrs", "extrs")]
    ids = torch.tensor([1, 0, 1, 1, 0, 0, 0, 1, 1], dtype=torch.int32, device=DEV)
    pred = EvaluationPredictor(m, interp_shape=None, grid_size=2, n_iters=2)
    opt = RigidMotion(use_visibility=False, min_spread=1e-4)
    res = pred(rgbs=a[0], depths=a[1], query_points_3d=a[2], intrs=a[3], extrs=a[4], query_groups=ids, rigid_motion=opt)
    rm = pred.last_rigid_motion
    assert rm is not None and rm.poses.shape == (2, 12, 4, 4) and rm.residual.shape == (12, 9)
    ref = R.rigid_motion(res["traj_e"][0].cpu().numpy(), res["vis_e"][0].cpu().numpy(), a[2][0, :, 0].cpu().numpy().astype(np.int32),
                         ids.cpu().numpy(), R.options(use_visibility=False, min_spread=1e-4))
    got = host(rm)
    print("reference frames", got["reference_frames"], "status", got["status"].tolist())
    assert np.array_equal(got["reference_frames"], ref["reference_frames"])
    for g in range(2):
        r = int(got["reference_frames"][g])
        centre = np.linalg.norm(ref["trace"]["pbar"][g, r])
        assert got["status"][g, r] == R.OK
        assert np.abs(got["poses"][g, r, :3, :3] - np.eye(3)).max() <= 2 * EPS and np.abs(got["poses"][g, r, :3, 3]).max() <= 2 * EPS * (1 + 2 * centre)
    pred(rgbs=a[0], depths=a[1], query_points_3d=a[2], intrs=a[3], extrs=a[4])
    assert pred.last_rigid_motion is None
