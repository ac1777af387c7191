"""mvt_track_metrics (csrc/metrics.hip) and mvt_adapter_best_view (csrc/pyramid.hip) on inputs whose right answer is exact.

GPU tests (`-m gpu`) go through `mvtracker_amd.hip`, `mvtracker_amd.metrics` and `mvtracker_amd.adapter`; the tests without the
marker are the CPU-only checks of the scalar restatement (tests/metrics_view_exact_ref.py, which also states the input rules and
why they are exact) against oracle/, of what the case lists reach, and the probes.  Every output buffer is poisoned before the
launch (NaN; -7777 for the int32 views): the metrics table gets five extra columns and a guard row, the view and projection
buffers a guard tail, and whatever the kernel must not write has to stay poisoned.  Every comparison is an equality, NaN equal
to NaN in the same place.

A. mvt_track_metrics: every track of every shape, the refusals, and the planted tracks one by one
B. the tables of evaluate_predictions / evaluate_3dpt against oracle.metrics_oracle on the same exact tracks
C. mvt_adapter_best_view: workgroup edge, per-frame cameras and maps, image edges, camera z, ties, half pixels, the wrapper
D. CPU: restatement == oracle bit for bit on every input of A and C, hand-computed values of the planted tracks, reach, probes.
   One difference of association is known and stated, not a rounding bar: at K = 8 numpy's mean adds eight values pairwise, the
   kernel (and the restatement) in ascending k; there the oracle's two averages are compared with numpy's mean of the RESTATED
   per-threshold columns, at K < 8 (numpy adds in order) with the restatement's own averages.
"""
import functools

import numpy as np
import pytest
import torch

import metrics_view_exact_ref as R
from oracle import metrics_oracle as MO
from oracle import mvt_oracle as O

gpu = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
SENT_V = -7777
PAD = 5  # extra columns of the metrics table
F32 = np.float32


@pytest.fixture(scope="module")
def hip():
    from mvtracker_amd import hip as h
    assert torch.cuda.is_available()
    return h


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def assert_same(got, ref, what):
    """Equality, NaN equal to NaN in the same place; names the first place that differs."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
    if bad.any():
        i = tuple(int(k) for k in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} differ, first at {i}: got {got[i]!r}, expected {ref[i]!r}")


# ================================================================== A: mvt_track_metrics

@functools.lru_cache(maxsize=None)
def expected_rows(T, N, D, K):
    return R.track_rows(R.random_clip(T, N, D, K))


@functools.lru_cache(maxsize=None)
def expected_planted(D):
    c, names = R.planted_clip(D)
    return R.track_rows(c), names


def run_track_metrics(hip, c):
    """The kernel's (N, 11 + 2K) table from a poisoned (N + 1, 11 + 2K + PAD) buffer; guard columns and guard row must stay NaN."""
    T, N, D = c["gt"].shape
    K = len(c["thr"])
    out = torch.full((N + 1, 11 + 2 * K + PAD), NAN, device=DEV)
    hip.track_metrics(G(c["gt"]), G(c["pred"]), G(c["vis"]), G(c["occ"]), G(c["qt"]), T, N, D, c["thr"], c["surv"], out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[N]).all()) and bool(torch.isnan(out[:, 11 + 2 * K:]).all()), "guard region written"
    return out[:N, :11 + 2 * K].cpu().numpy()


@gpu
@pytest.mark.parametrize("T,N,D,K", R.SHAPES)
def test_track_metrics_shapes(hip, T, N, D, K):
    got = run_track_metrics(hip, R.random_clip(T, N, D, K))
    assert_same(got, expected_rows(T, N, D, K), f"track_metrics T={T} N={N} D={D} K={K} (track, column)")


def _refusal_inputs(kind):
    T, N, D, K = 65, 5, 3, 5
    c = dict(R.random_clip(T, N, D, K))
    width = None
    if kind == "T1025":
        z = lambda a: np.zeros((1025,) + a.shape[1:], a.dtype)
        c.update(gt=z(c["gt"]), pred=z(c["pred"]), vis=z(c["vis"]), occ=z(c["occ"]))
    elif kind == "K0":
        c["thr"] = []
    elif kind == "K9":
        c["thr"] = R.THRESH + [32.0]
    elif kind == "D4":
        c.update(gt=np.zeros((T, N, 4), F32), pred=np.zeros((T, N, 4), F32))
    elif kind == "ldo_short":
        width = 11 + 2 * K - 1
    return c, width


@gpu
@pytest.mark.parametrize("kind", ["T1025", "K0", "K9", "D4", "ldo_short"])
def test_track_metrics_refusals(hip, kind):
    c, width = _refusal_inputs(kind)
    T, N, D = c["gt"].shape
    K = len(c["thr"])
    out = torch.full((N + 1, 11 + 2 * K + PAD if width is None else width), NAN, device=DEV)
    with pytest.raises(hip.HipError, match="arguments rejected"):
        hip.track_metrics(G(c["gt"]), G(c["pred"]), G(c["vis"]), G(c["occ"]), G(c["qt"]), T, N, D, c["thr"], c["surv"], out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


@pytest.fixture(scope="module")
def planted_gpu(hip):
    return {D: run_track_metrics(hip, R.planted_clip(D)[0]) for D in (2, 3)}


PLANTED = [(D, name) for D in (2, 3) for name in R.planted_clip(D)[1]]


@gpu
@pytest.mark.parametrize("D,name", PLANTED)
def test_track_metrics_planted(planted_gpu, D, name):
    ref, names = expected_planted(D)
    n = names.index(name)
    assert_same(planted_gpu[D][n], ref[n], f"planted track {name} D={D} (column)")


def _flags_01(c):
    return dict(c, vis=(c["vis"] != 0).astype(np.uint8), occ=(c["occ"] != 0).astype(np.uint8))


def _finite_pred(c):
    p = c["pred"].copy()
    bad = ~np.isfinite(p)
    p[bad] = c["gt"][bad]
    return dict(c, pred=p)


@gpu
@pytest.mark.parametrize("D", [2, 3])
def test_track_metrics_flag_bytes_and_non_finite(hip, planted_gpu, D):
    """Bytes 2 and 255 mean the same as 1.  NaN / Inf predictions on gt-occluded frames and before the query move no column: not the
    trajectory errors, not a within count, and where they are not flagged occluded they are the false positives that finite
    predictions on a gt-occluded frame are (`~within` is true for NaN)."""
    c, names = R.planted_clip(D)
    assert_same(run_track_metrics(hip, _flags_01(c)), planted_gpu[D], "flags as 0 / 1")
    n = names.index("nonfinite")
    fin = run_track_metrics(hip, _finite_pred(c))
    assert_same(fin[n], planted_gpu[D][n], "non-finite predictions moved a column")


# ================================================================== B: the tables

def assert_tables_equal(got, ref):
    gr, gp = got
    rr, rp = ref
    assert list(gr) == list(rr), (list(gr), list(rr))
    for col in rr:
        assert sorted(gr[col]) == sorted(rr[col]), col
        for k in rr[col]:
            assert_same(np.float64(gr[col][k]), np.float64(rr[col][k]), f"results[{col}][{k}]")
    assert list(gp) == list(rp)
    for col in rp:
        assert sorted(gp[col]) == sorted(rp[col]), col
        assert np.array_equal(gp[col]["indices"], rp[col]["indices"]), (col, gp[col]["indices"], rp[col]["indices"])
        for k in rp[col]:
            assert_same(np.asarray(gp[col][k], np.float64), np.asarray(rp[col][k], np.float64), f"per_track[{col}][{k}]")


def table_args(c, **over):
    kw = dict(R.TABLE_THR)
    kw.update(over)
    return (c["gt"], c["vis"] != 0, c["pred"], c["occ"] != 0, R.query_points_of(c)), kw


TABLE_CASES = {
    "edges": ("edges", {}),
    "no_static": ("no_static", {}),
    "all_visible": ("all_visible", {}),
    "static_none": ("edges", dict(static_threshold=None)),
    "dynamic_none": ("edges", dict(dynamic_threshold=None)),
    "very_none": ("edges", dict(very_dynamic_threshold=None)),
    "all_none": ("edges", dict(static_threshold=None, dynamic_threshold=None, very_dynamic_threshold=None)),
    "no_query_points": ("edges", {}),
}


@functools.lru_cache(maxsize=None)
def oracle_table(case):
    kind, over = TABLE_CASES[case]
    a, kw = table_args(R.table_clip(kind)[0], **over)
    if case == "no_query_points":
        a = a[:4] + (None,)
    return MO.evaluate_predictions(*a, **kw)


@gpu
@pytest.mark.parametrize("case", list(TABLE_CASES))
def test_evaluate_predictions_tables(hip, case):
    from mvtracker_amd import metrics as M
    kind, over = TABLE_CASES[case]
    a, kw = table_args(R.table_clip(kind)[0], **over)
    if case == "no_query_points":
        a = a[:4] + (None,)
    assert_tables_equal(M.evaluate_predictions(*a, device=DEV, **kw), oracle_table(case))


SETTING_CASES = [(s, f, q) for s in ("kubric-multiview", "2dpt_ablation") for f in (2.0, 0.5) for q in (True, False)]


@gpu
@pytest.mark.parametrize("setting,factor,with_qp", SETTING_CASES)
def test_evaluate_3dpt_settings(hip, setting, factor, with_qp):
    from mvtracker_amd import metrics as M
    c = R.setting_clip(setting, factor)
    qp = R.query_points_of(c) if with_qp else None
    a = (c["gt"], c["vis"] != 0, c["pred"], c["occ"] == 0, setting, factor, qp)
    ref = MO.evaluate_3dpt(*a)
    got = M.evaluate_3dpt(*a, add_per_track_results=False, device=DEV)
    assert list(got) == list(ref) and len(ref) > 0
    for k in ref:
        assert_same(np.float64(got[k]), np.float64(ref[k]), k)


# ================================================================== C: mvt_adapter_best_view

TAIL = 64


def run_best_view(hip, c, with_xyz=True):
    V, T, H, W, N = c["V"], c["T"], c["H"], c["W"], len(c["qp"])
    view = torch.full((N + TAIL,), SENT_V, device=DEV, dtype=torch.int32)
    xyz = torch.full((V * N * 3 + TAIL,), NAN, device=DEV) if with_xyz else None
    hip.adapter_best_view(G(c["depths"]), G(c["intrs"]), G(c["extrs"]), G(c["qp"]), V, T, H, W, N, view, xyz)
    torch.cuda.synchronize()
    assert bool((view[N:] == SENT_V).all()), "view guard written"
    if with_xyz:
        assert bool(torch.isnan(xyz[V * N * 3:]).all()), "projection guard written"
        xyz = xyz[:V * N * 3].reshape(V, N, 3).cpu()
    return view[:N].cpu().numpy().astype(np.int64), xyz


@functools.lru_cache(maxsize=None)
def expected_views(name):
    c = R.view_cases()[name]
    views, xyz, _ = R.best_view(c)
    return c, views, torch.from_numpy(xyz.astype(F32))


VIEW_CASES = list(R.view_cases())


@gpu
@pytest.mark.parametrize("name", VIEW_CASES)
def test_best_view(hip, name):
    c, views, xyz = expected_views(name)
    got_v, got_xyz = run_best_view(hip, c, True)
    assert_same(got_v, views, f"{name}: view of query")
    assert torch.equal(got_xyz, xyz), name
    got_v2, _ = run_best_view(hip, c, False)
    assert_same(got_v2, views, f"{name}: view of query without xyz_out")


@gpu
def test_best_view_permuted_winner_follows(hip):
    """The views in another order: the winner's new index is where the old winner went (ties: the lowest new index of the tie)."""
    c = R.ties_clip()
    order = (2, 0, 1)
    got, _ = run_best_view(hip, R.permute_views(c, order))
    assert_same(got, R.best_view(c, order=order)[0], "permuted views")


@gpu
def test_assign_views_wrapper(hip):
    from mvtracker_amd import adapter
    c, views, xyz = expected_views("sized_V3_N129")
    V, T, H, W, N = c["V"], c["T"], c["H"], c["W"], len(c["qp"])
    a = (G(c["depths"]).reshape(1, V, T, 1, H, W), G(c["qp"])[None], G(c["intrs"])[None], G(c["extrs"])[None])
    only = adapter.assign_views(*a)
    v, xy, z = adapter.assign_views(*a, return_projections=True)
    assert only.dtype == torch.int64 and v.dtype == torch.int64 and tuple(only.shape) == (1, N) and tuple(v.shape) == (1, N)
    assert tuple(xy.shape) == (1, V, N, 2) and tuple(z.shape) == (1, V, N, 1)
    assert_same(only[0].cpu().numpy(), views, "assign_views")
    assert_same(v[0].cpu().numpy(), views, "assign_views with projections")
    _, raw = run_best_view(hip, c, True)
    assert torch.equal(xy[0].cpu(), raw[..., :2]) and torch.equal(z[0].cpu(), raw[..., 2:]) and torch.equal(raw, xyz)


# ================================================================== D: CPU checks

def oracle_rows_check(c, rows, what):
    mv = R.masked_vis(c)
    o = MO.track_metrics(c["gt"], mv, c["pred"], c["occ"] != 0, R.query_points_of(c), c["thr"], c["surv"])
    names = R.column_names(c["thr"])
    assert sorted(o) == sorted(names)
    K = len(c["thr"])
    for j, k in enumerate(names):
        ref = rows[:, 2 + j]
        if K == 8 and k in ("average_jaccard", "average_pts_within_thresh"):  # numpy adds eight values pairwise (module docstring)
            cols = rows[:, 11 + K:11 + 2 * K] if k == "average_jaccard" else rows[:, 11:11 + K]
            ref = np.ascontiguousarray(cols).mean(-1, dtype=F32)
        assert_same(o[k].astype(F32), ref, f"{what}: oracle column {k} (track)")
    assert_same(MO.point_movement(c["gt"], mv), rows[:, 0].astype(np.float64), f"{what}: point_movement")
    assert_same(mv.sum(0).astype(F32), rows[:, 1], f"{what}: visible frames")


@pytest.mark.parametrize("T,N,D,K", R.SHAPES)
def test_restatement_equals_oracle_shapes(T, N, D, K):
    oracle_rows_check(R.random_clip(T, N, D, K), expected_rows(T, N, D, K), f"T={T} N={N} D={D} K={K}")


@pytest.mark.parametrize("D", [2, 3])
def test_restatement_equals_oracle_planted(D):
    c, _ = R.planted_clip(D)
    oracle_rows_check(c, expected_planted(D)[0], f"planted D={D}")
    oracle_rows_check(_flags_01(c), expected_planted(D)[0], f"planted D={D}, flags as 0 / 1")
    for kind in ("edges", "no_static", "all_visible"):
        t = R.table_clip(kind)[0]
        oracle_rows_check(t, R.track_rows(t), f"table {kind}")


@pytest.mark.parametrize("D", [2, 3])
def test_planted_values_by_hand(D):
    """The restatement on the planted tracks against numbers worked out by hand from the construction."""
    rows, names = expected_planted(D)
    K, T = len(R.PLANT_THR), R.PLANT_T
    col = dict(move=0, nvis=1, occ=2, occ0=3, occ1=4, mte=7, ate=8, fde=9, surv=10, pw_050=11 + 1, pw_100=11 + 2)
    ln = lambda d: float(np.sqrt((R.dirs(D)[d] ** 2).sum()))
    want = {
        "thr_at": dict(pw_050=0, pw_100=1, surv=1, mte=0.5), "thr_below": dict(pw_050=1, surv=1, mte=R.dn(0.5)),
        "thr_above": dict(surv=R.ratio(70, T)), "med_odd": dict(mte=3 / 16, nvis=5), "med_even": dict(mte=3 / 16, nvis=6),
        "med_dup_same": dict(mte=3 / 16), "med_dup_split": dict(mte=2 / 16, ate=3 / 16),
        "one_vis": dict(nvis=1, mte=3 / 16, ate=3 / 16, fde=3 / 16, move=0, surv=1),
        "none_vis": dict(nvis=0, mte=NAN, ate=NAN, fde=NAN, surv=1, move=0, occ1=NAN),
        "move_3_200": dict(move=99 * ln(2), nvis=2), "move_63_64": dict(move=ln(3), nvis=2), "move_lane0_only": dict(move=0, nvis=1),
        "move_lane0s": dict(move=94 * ln(5 if D == 3 else 2), nvis=3),
        "last_63": dict(fde=3 / 16), "last_64": dict(fde=4 / 16), "last_end": dict(fde=1 / 16),
        "fail_64": dict(surv=R.ratio(64, T)), "fail_masked": dict(surv=R.ratio(125, 252)),
        "qt_last": dict(occ=NAN, occ0=NAN, occ1=NAN, surv=1, nvis=1, fde=1 / 16), "qt_mid": dict(surv=1, nvis=T - 100, mte=2 / 16),
    }
    for name, d in want.items():
        for k, v in d.items():
            assert_same(rows[names.index(name), col[k]], F32(v), f"{name}.{k}")
    n = names.index("nonfinite")
    c = R.planted_clip(D)[0]
    fin = R.track_rows(_finite_pred(c))
    assert_same(fin[n], rows[n], "non-finite predictions moved a column")


def test_tables_by_hand():
    """Which subset each planted track of the `edges` clip lands in, read off the oracle's per-track table."""
    c, names = R.table_clip("edges")
    res, per = oracle_table("edges")
    idx = {col: {names[i] for i in per[col]["indices"]} for col in per}
    mv = [f"move_{i}" for i in range(9)]
    assert idx["all_static"] & set(mv) == {mv[1]}                  # one step below the static threshold; at it: excluded
    assert idx["all_dynamic"] & set(mv) == set(mv[5:])             # at the dynamic threshold: excluded; one step above: kept
    assert idx["all_very_dynamic"] & set(mv) == {mv[8]}
    assert "one_visible" not in idx["all_any"] and "two_visible" in idx["all_any"]
    assert list(res) == ["all_any", "all_static", "all_dynamic", "all_very_dynamic", "all_dynamic-static-mean"]
    assert list(oracle_table("no_static")[0]) == ["all_any", "all_dynamic", "all_very_dynamic"]
    assert list(oracle_table("static_none")[0]) == ["all_any", "all_dynamic", "all_very_dynamic"]
    assert list(oracle_table("all_none")[0]) == ["all_any"]
    av = oracle_table("all_visible")[0]
    assert all(np.isnan(av[col]["occlusion_accuracy_for_vis0"]) and not np.isnan(av[col]["occlusion_accuracy"]) for col in av)
    for s, f, _ in SETTING_CASES:
        R.setting_clip(s, f)  # the builder's own assertions


@pytest.mark.parametrize("name", VIEW_CASES)
def test_view_restatement_equals_oracle(name):
    c, views, xyz = expected_views(name)
    T_ = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    dep, intr, extr, qp = T_(c["depths"])[:, :, None], T_(c["intrs"]), T_(c["extrs"]), T_(c["qp"])
    assert_same(O.adapter_best_view(dep, qp, intr, extr).numpy(), views, f"{name}: oracle view")
    _, _, blend = R.best_view(c)
    qt = qp[:, 0].long()
    for t in qt.unique():
        m = qt == t
        world = qp[m, 1:][None].expand(c["V"], -1, -1)
        xy, z = O.project_to_view(world, intr[:, t], extr[:, t])
        assert torch.equal(xy, xyz[:, m, :2]) and torch.equal(z, xyz[:, m, 2:]), name
        for v in range(c["V"]):
            s = O.bilinear_sample2d(dep[v, t][None], xy[v, :, 0][None], xy[v, :, 1][None])[0, 0].numpy()
            b = blend[v, m.numpy()]
            assert_same(s[~np.isnan(b)], b[~np.isnan(b)].astype(F32), f"{name}: bilinear_sample2d, view {v}")


def test_cases_reach_what_they_claim():
    tr = set()
    for D in (2, 3):
        tr |= R.reach_tracks(R.planted_clip(D)[0])
    assert tr >= {"median_on_duplicate", "median_between_distinct", "one_visible", "none_visible", "carry_across_empty_step",
                  "pair_across_step_edge", "last_visible_in_later_step", "distance_at_threshold", "distance_below_threshold",
                  "distance_at_survival", "non_finite", "visible_before_query"}
    rnd = set()
    for sh in R.SHAPES:
        rnd |= R.reach_tracks(R.random_clip(*sh))
    assert rnd >= {"full_buffer", "distance_at_threshold", "distance_at_survival", "median_on_duplicate", "carry_across_empty_step",
                   "none_visible", "one_visible"}
    assert {s[0] for s in R.SHAPES} == {1, 2, 63, 64, 65, 128, 129, 1024} and {s[1] for s in R.SHAPES} == {1, 3, 4, 5, 9}
    assert {s[2:] for s in R.SHAPES} == set(R.DK)
    cases = R.view_cases()
    assert R.reach_views(cases["edges"]) >= {"x=" + k for k in ("0", "W-1", "W-0.5", "W", "-0.125")} | \
        {"y=" + k for k in ("0", "H-1", "H-0.5", "H", "-0.125")}
    assert R.reach_views(cases["z"]) >= {"behind_in_box", "small_z_inside"}
    assert R.reach_views(cases["ties"]) >= {"two_way_tie", "three_way_tie", "all_outside", "all_outside_negative_z_wins"}
    assert R.reach_views(cases["outside"]) >= {"two_way_tie_outside", "three_way_tie_outside"}
    assert "fractional_frame" in R.reach_views(cases["frames"])
    c, views, _ = expected_views("frames")
    assert views.tolist() == [0, 1, 2, 0, 1, 2]  # the same world point, three frames, three planted winners; 1.9 reads frame 1
    c, views, _ = expected_views("half")
    assert views.tolist() == [0, 0, 0] and np.array_equal(R.scores_of(c)[:, 0], [4.0, 3.875, 4.0])
    c, views, _ = expected_views("z")
    assert views.tolist() == [0, 1, 0]
    c, order = R.ties_clip(), (2, 0, 1)  # the views in another order: where the maximum is single, the winner's index follows it
    old, new, sc = R.best_view(c)[0], R.best_view(c, order=order)[0], R.scores_of(c)
    single = (sc == sc.max(0, keepdims=True)).sum(0) == 1
    assert single.any() and (~single).any() and np.array_equal(np.array(order)[new[single]], old[single])
    assert np.array_equal(new, R.best_view(R.permute_views(c, order))[0])
    for V in (1, 3, 6):  # the cameras of a (view, frame) are read: no view and no frame is a bystander in the pool
        v = expected_views(f"sized_V{V}_N300")[1]
        assert set(v.tolist()) == set(range(V))


@pytest.mark.parametrize("fault", R.METRIC_FAULTS)
def test_probe_metrics(fault):
    """The planted mistake changes the expected table of section A on section A's inputs."""
    seen = []
    for D in (2, 3):
        c, names = R.planted_clip(D)
        ref, bad = expected_planted(D)[0], R.track_rows(c, fault)
        seen += [names[n] for n in range(len(names)) if not np.array_equal(ref[n], bad[n], equal_nan=True)]
    must = dict(le_dist="thr_at", ge_survival="thr_at", upper_median="med_even", carry_dropped="move_3_200", last_first_step="last_64",
                pre_query_visible="qt_mid")[fault]
    assert seen.count(must) == 2, (fault, seen)
    if fault != "ge_survival":  # the random clips see it too (there a track with a distance on the survival threshold has failed before)
        assert any(not np.array_equal(expected_rows(*sh), R.track_rows(R.random_clip(*sh), fault), equal_nan=True) for sh in R.SHAPES)


@pytest.mark.parametrize("fault", R.VIEW_FAULTS)
def test_probe_views(fault):
    """The planted mistake changes the expected views of section C on section C's inputs, in the case built for it."""
    case = dict(frame0_cams="frames", frame0_depth="frames", clamped_weights="edges", x_gt_w="edges", last_max="ties", no_z_test="z")[fault]
    c, views, _ = expected_views(case)
    assert not np.array_equal(R.best_view(c, fault)[0], views), fault
    if fault == "last_max":
        assert not np.array_equal(R.best_view(R.half_clip(), fault)[0], expected_views("half")[1])
        assert not np.array_equal(R.best_view(R.outside_tie_clip(), fault)[0], expected_views("outside")[1])
