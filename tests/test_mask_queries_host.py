"""Mask queries, host side (no GPU): the host code of mvtracker_amd/masks.py and the ``query_groups`` path of the predictor on mocked
kernels (tests/hip_mock_masks.py) against the restatement tests/mask_ref.py: option validation, label refusals before any launch,
``labels_from_instances``, the anchor arithmetic, skipped frames, row order, ``split``, one generator consumed in (object, frame)
order, the single readback, ``query_groups`` scatter and refusals, and that without a mask argument no new entry is called."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hip_mock_masks  # noqa: E402
import mask_ref as R  # noqa: E402

from mvtracker_amd import synth  # noqa: E402

V, T, H, W = 2, 5, 12, 16


def band_labels(depths, edges=(1.5, 2.5, 3.5)):
    """Labels from depth bands per view: 0 below the first edge, then 1, 2, ...; view 1's ids are shifted by one (local ids)."""
    d = depths[:, :, 0]
    lab = np.digitize(d, edges).astype(np.uint8)
    lab[1] = np.where(lab[1] > 0, lab[1] % len(edges) + 1, 0)
    return lab


@pytest.fixture(scope="module")
def clip():
    c = synth.make_clip(5, V, T, H, W, 1)
    c = {k: v for k, v in c.items()}
    c["depths"][0, 0, 3] = 0.0  # view 0 has no valid depth in frame 3
    c["labels"] = band_labels(c["depths"][0])
    return c


def tensors(clip):
    return [torch.from_numpy(clip[k]) for k in ("labels", "depths", "intrs", "extrs")]


def ref_args(clip):
    return clip["labels"], clip["depths"][0], clip["intrs"][0], clip["extrs"][0]


def test_exports_and_option_validation():
    import mvtracker_amd
    from mvtracker_amd import MaskQueries, hip, masks
    names = {"masks", "MaskQueries", "MaskStatistics", "MaskMatching", "MaskQueryReport", "labels_from_instances", "mask_statistics", "match_mask_ids",
             "global_masks", "lift_masks", "mask_queries", "object_colors"}
    assert names <= set(mvtracker_amd.__all__) and all(getattr(mvtracker_amd, n) is getattr(masks, n) for n in names - {"masks"})
    assert all(n in hip.SIGNATURES for n in ("mvt_mask_stats", "mvt_mask_centroids", "mvt_mask_match", "mvt_mask_relabel", "mvt_mask_pool"))
    assert hip.abi_version() == 9 and hip.MASK_MAX_LABEL == 255
    o = MaskQueries()
    assert (o.anchor, o.frames_before, o.frames_after, o.min_depth, o.max_depth, o.conf_thresh, o.min_pixels, o.match, o.distance_threshold,
            o.min_common_frames, o.max_points_per_frame, o.method) == tuple(R.DEFAULTS.values())
    with pytest.raises(Exception):
        o.match = False  # frozen
    for kw in (dict(anchor="last"), dict(anchor=-1), dict(anchor=1.5), dict(anchor=True), dict(anchor={(0,): 1}), dict(anchor={(0, 0): 1}),
               dict(anchor={(0, 256): 1}), dict(anchor={(0, 1): -1}), dict(frames_before=-1), dict(frames_after=0.5), dict(min_depth=float("nan")),
               dict(max_depth=float("inf")), dict(min_depth=2.0, max_depth=2.0), dict(conf_thresh=float("nan")), dict(min_pixels=0),
               dict(match=1), dict(distance_threshold=-0.1), dict(distance_threshold=float("nan")), dict(min_common_frames=0),
               dict(max_points_per_frame=0), dict(max_points_per_frame=2.5), dict(method="fps"), dict(method="kmeans", max_points_per_frame=5000)):
        with pytest.raises(ValueError):
            MaskQueries(**kw)
    assert MaskQueries(anchor=2.0, frames_before=1.0, max_points_per_frame=8.0).anchor == 2
    assert MaskQueries(anchor={(np.int64(1), 2): 3}).anchor == {(1, 2): 3}


def test_label_refusals_before_any_launch(monkeypatch, clip):
    from mvtracker_amd import MaskQueries, mask_queries, mask_statistics
    hip_mock_masks.install(monkeypatch)
    lab, d, k, e = tensors(clip)
    bad = [lab.float(), lab.to(torch.int32) + 255, lab.to(torch.int64) - 1, lab.to(torch.int16) * 200, lab[0], torch.stack([lab, lab]), lab[:, :, :4]]
    for x in bad:
        with pytest.raises(ValueError):
            mask_statistics(x, d, k, e)
    with pytest.raises(ValueError):
        mask_queries(lab, d[0], k, e)
    with pytest.raises(ValueError):
        mask_queries(lab, d, k, e, "first")
    with pytest.raises(ValueError):
        mask_queries(lab, d, k, e, MaskQueries(conf_thresh=0.5))  # no confidence map
    with pytest.raises(ValueError):
        mask_queries(lab, d, k, e, MaskQueries(anchor=T))
    with pytest.raises(ValueError):
        mask_queries(lab, d, k, e, depths_conf=d[:, :1])
    assert hip_mock_masks.calls == []
    with pytest.raises(ValueError, match="depth bounds"):  # nothing valid: the message names the likely causes
        mask_queries(lab, d, k, e, MaskQueries(max_depth=1e-3))
    with pytest.raises(ValueError, match="masks are empty"):
        mask_queries(torch.zeros_like(lab), d, k, e)


def test_labels_from_instances_overlap_order():
    from mvtracker_amd import labels_from_instances
    m = torch.zeros(3, 1, 1, 2, 4, dtype=torch.bool)
    m[0, ..., 0, :2] = True
    m[1, ..., 0, 1:3] = True
    m[2] = True
    exp = torch.tensor([[1, 1, 2, 3], [3, 3, 3, 3]], dtype=torch.uint8)
    got = labels_from_instances(m)
    assert got.dtype == torch.uint8 and got.shape == (1, 1, 2, 4) and torch.equal(got[0, 0], exp)
    assert torch.equal(labels_from_instances({"cup": m[0], "hand": m[1], "table": m[2]}), got)
    assert torch.equal(labels_from_instances({"table": m[2], "cup": m[0]})[0, 0], torch.full((2, 4), 1, dtype=torch.uint8))
    for bad in (m.float(), m[0], {}):
        with pytest.raises(ValueError):
            labels_from_instances(bad)


def test_anchor_arithmetic_and_clipping():
    from mvtracker_amd import MaskQueries
    from mvtracker_amd.masks import object_frames
    valid = np.array([0, 0, 4, 9, 0, 7, 1, 0])
    mem = [(0, 1), (1, 3)]
    cases = [(dict(), ([2], [2, 3], [0, 1])),
             (dict(frames_before=0, frames_after=0), ([2], [2], [])),
             (dict(anchor=6, frames_before=1, frames_after=5), ([6], [5, 6], [7])),
             (dict(anchor=0, frames_before=3, frames_after=2), ([0], [2], [0, 1])),
             (dict(anchor={(0, 1): 5, (1, 3): 3, (1, 9): 0}, frames_before=1, frames_after=0), ([5, 3], [2, 3, 5], [4])),
             (dict(anchor={(1, 9): 0}), ([2], [2, 3], [0, 1]))]  # no entry for a member: the "first" rule
    for kw, exp in cases:
        got = object_frames(valid, mem, MaskQueries(**kw), len(valid))
        print(kw, got)
        assert got == exp and got == R.object_frames(valid, mem, R.options(**kw), len(valid))


def _compare(got, clip, opt_kw, seed=0):
    q, ids, report = got
    rows, rids, objects, pools, mt = R.mask_queries(*ref_args(clip), R.options(**opt_kw), seed=seed)
    assert q.shape == (1, len(rows), 4) and q.dtype == torch.float32 and ids.dtype == torch.int32
    # (the mock's points are torch's, the restatement's numpy's: the same rows to the last bits but one or two)
    assert np.array_equal(q[0, :, 0].numpy(), rows[:, 0]) and np.allclose(q[0, :, 1:].numpy(), rows[:, 1:], rtol=0, atol=2e-5)
    assert np.array_equal(ids.numpy(), rids)
    assert report.objects == objects and report.matching.num_objects == mt["num_objects"] and report.matching.members == mt["members"]
    assert np.array_equal(report.matching.global_id.numpy(), mt["global_id"])
    return rows, rids, objects


@pytest.mark.parametrize("opt_kw", [dict(), dict(max_points_per_frame=7), dict(anchor=3, frames_before=1), dict(anchor={(0, 1): 4, (1, 2): 1}, frames_after=0),
                                    dict(match=False, max_points_per_frame=5), dict(min_pixels=3, distance_threshold=1.0)])
def test_mask_queries_rows_report_and_single_read(monkeypatch, clip, opt_kw):
    from mvtracker_amd import MaskQueries, mask_queries
    hip_mock_masks.install(monkeypatch)
    items = []
    real_item = torch.Tensor.item
    monkeypatch.setattr(torch.Tensor, "item", lambda self: items.append(1) or real_item(self))
    got = mask_queries(*tensors(clip), MaskQueries(**opt_kw), seed=11)
    assert len(hip_mock_masks.reads) == 1 and items == []  # the tables are read once and nothing else is
    rows, rids, objects = _compare(got, clip, opt_kw, seed=11)
    assert hip_mock_masks.calls[:3] == ["mask_stats", "mask_centroids", "mask_match"]
    assert hip_mock_masks.calls[3:] == ["mask_pool"] * sum(len(o["frames_used"]) for o in objects)
    # rows: by object, then frame; inside a pool that is kept whole, raster order (checked by equality with the reference above)
    key = list(zip(rids.tolist(), rows[:, 0].tolist()))
    assert key == sorted(key) and len(objects) >= 2
    parts = got[2].split(got[0])
    assert [p.shape[1] for p in parts] == [o["rows"] for o in objects if o["rows"]] and torch.equal(torch.cat(parts, 1), got[0])
    with pytest.raises(ValueError):
        got[2].split(got[0][:, :-1])
    print(got[2].summary())
    print(got[2].table())
    print(got[2].matching.table())
    assert str(len(rows)) in got[2].summary()


def test_skipped_frames_are_reported(monkeypatch, clip):
    """View 0 has no valid depth in frame 3: an object seen by view 0 alone there skips the frame."""
    from mvtracker_amd import MaskQueries, mask_queries
    hip_mock_masks.install(monkeypatch)
    lab = clip["labels"].copy()
    lab[1] = 0
    c = dict(clip, labels=lab)
    got = mask_queries(*tensors(c), MaskQueries(anchor=3, frames_before=1, frames_after=1))
    _compare(got, c, dict(anchor=3, frames_before=1, frames_after=1))
    assert all(o["frames_skipped"] == [3] and o["frames_used"] == [2, 4] for o in got[2].objects)
    assert not (got[0][0, :, 0] == 3).any()


def test_one_generator_in_object_frame_order(monkeypatch, clip):
    """The draws of a call come from one generator: cutting the first pool only moves every later draw."""
    from mvtracker_amd import MaskQueries, mask_queries
    hip_mock_masks.install(monkeypatch)
    q, ids, rep = mask_queries(*tensors(clip), MaskQueries(max_points_per_frame=6), seed=3)
    sizes = [m for o in rep.objects for m in o["pool_sizes"]]
    assert sum(m > 6 for m in sizes) >= 3
    g = torch.Generator().manual_seed(3)
    full = mask_queries(*tensors(clip), MaskQueries())[0][0]
    o, r = 0, 0
    for m in sizes:
        pool = full[o:o + m]
        exp = pool[torch.randperm(m, generator=g)[:6]] if m > 6 else pool
        assert torch.equal(q[0, r:r + len(exp)], exp)
        o, r = o + m, r + len(exp)
    assert r == q.shape[1]


def test_statistics_matching_lift_and_relabel(monkeypatch, clip):
    from mvtracker_amd import MaskQueries, global_masks, lift_masks, mask_statistics, match_mask_ids
    hip_mock_masks.install(monkeypatch)
    lab, d, k, e = tensors(clip)
    st = mask_statistics(lab, d, k, e)
    ref = R.statistics(*ref_args(clip), R.options())
    assert hip_mock_masks.reads == []
    for name in ("pixels", "count", "sums"):
        assert tuple(getattr(st, name).shape) == ref[name].shape
    assert np.array_equal(st.pixels.numpy(), ref["pixels"]) and np.array_equal(st.count.numpy(), ref["count"]) and st.out_of_range == 0
    # (the mock's points are torch's, the restatement's numpy's: 2e-5 per point, the bar of the pool tests)
    assert (np.abs(st.sums.numpy() - ref["sums"]) <= ref["count"][..., None] * 2e-5 * 2 ** 20).all()
    assert np.array_equal(np.isnan(st.centroid.numpy()), np.isnan(ref["centroid"]))
    assert np.allclose(st.centroid.numpy(), ref["centroid"], rtol=0, atol=2e-5, equal_nan=True)
    mt = match_mask_ids(st, MaskQueries(distance_threshold=1.0))
    rm = R.matching(ref["centroid"], R.options(distance_threshold=1.0))
    assert len(hip_mock_masks.reads) == 1 and mt.members == rm["members"] and 0 < mt.num_objects < 6
    assert rm["margin"] > 1e-3 and np.allclose(mt.distance.numpy(), rm["distance"], rtol=0, atol=1e-4, equal_nan=True)
    for wide in (lab, lab.to(torch.int32), lab[None].to(torch.int64)):
        gm = global_masks(wide, mt)
        assert gm.dtype == torch.int32 and np.array_equal(gm.numpy(), np.where(clip["labels"] > 0, np.stack([rm["global_id"][v][clip["labels"][v]] for v in range(V)]), -1))
    pts, oid, pix = lift_masks(lab, d, k, e, 1, matching=mt, options=MaskQueries(distance_threshold=1.0))
    exp = [R.object_pool(*ref_args(clip), R.options(), rm["global_id"], g, 1) for g in range(rm["num_objects"])]
    assert np.array_equal(pix.numpy(), np.concatenate([i for i, _ in exp])) and np.allclose(pts.numpy(), np.concatenate([p for _, p in exp]), rtol=0, atol=2e-5)
    assert np.array_equal(oid.numpy(), np.concatenate([np.full(len(i), g, np.int32) for g, (i, _) in enumerate(exp)]))
    with pytest.raises(ValueError):
        lift_masks(lab, d, k, e, T, matching=mt)
    with pytest.raises(ValueError):
        global_masks(lab, "table")


def test_object_colors():
    from mvtracker_amd import object_colors
    from mvtracker_amd.overlay import GIST_RAINBOW
    ids = torch.tensor([0, 0, 2, 1, 2], dtype=torch.int32)
    c = object_colors(ids)
    lut = np.frombuffer(GIST_RAINBOW, np.uint8).reshape(256, 3)
    assert c.dtype == torch.uint8 and c.shape == (5, 3) and torch.equal(c[0], c[1]) and torch.equal(c[2], c[4])
    assert len({tuple(r) for r in c.tolist()}) == 3 and np.array_equal(c[3].numpy(), lut[128])
    assert object_colors(torch.zeros(0, dtype=torch.int32)).shape == (0, 3)
    for bad in (ids.float(), ids[None], ids - 1):
        with pytest.raises(ValueError):
            object_colors(bad)


class _GroupedModel(torch.nn.Module):
    """A model whose tracks are its queries' positions plus the frame number, and whose visibility is the set's size."""

    def __init__(self):
        super().__init__()
        self.sets, self.plain = [], 0

    @staticmethod
    def _result(q, frames):
        t = torch.arange(frames, dtype=torch.float32)[None, :, None, None]
        return {"traj_e": q[:, None, :, 1:] + t, "vis_e": torch.full((1, frames, q.shape[1]), float(q.shape[1]))}

    def forward(self, rgbs, depths, query_points, **kw):
        self.plain += 1
        return self._result(query_points, rgbs.shape[2])

    def forward_grouped(self, rgbs, depths, query_points_list, **kw):
        self.sets.append([q.clone() for q in query_points_list])
        return [self._result(q, rgbs.shape[2]) for q in query_points_list]


def _predictor_inputs(clip, n):
    g = torch.Generator().manual_seed(0)
    q = torch.cat([torch.zeros(1, n, 1), torch.randn(1, n, 3, generator=g)], 2)
    rgbs = torch.zeros(1, V, T, 3, H, W)
    return rgbs, torch.from_numpy(clip["depths"]), q, torch.from_numpy(clip["intrs"]), torch.from_numpy(clip["extrs"])


def test_query_groups_scatter_and_refusals(monkeypatch, clip):
    from mvtracker_amd import EvaluationPredictor
    hip_mock_masks.install(monkeypatch)
    model = _GroupedModel()
    p = EvaluationPredictor(model, interp_shape=None, grid_size=2, visibility_threshold=0.5)
    rgbs, d, q, k, e = _predictor_inputs(clip, 7)
    ids = torch.tensor([4, 0, 4, 9, 0, 4, 9], dtype=torch.int32)
    res = p(rgbs, d, q, k, e, query_groups=ids)
    assert model.plain == 0 and len(model.sets) == 1 and len(model.sets[0]) == 3
    n_support = 4 * V
    for rows, qs in zip(([1, 4], [0, 2, 5], [3, 6]), model.sets[0]):  # ascending id, every set = [its queries; the support rows]
        assert qs.shape == (1, len(rows) + n_support, 4) and torch.equal(qs[0, :len(rows)], q[0, rows])
        assert torch.equal(qs[0, len(rows):], model.sets[0][0][0, 2:])
        assert torch.equal(res["vis_e_as_prob"][0, :, rows], torch.full((T, len(rows)), float(len(rows) + n_support)))
    t = torch.arange(T, dtype=torch.float32)[:, None, None]
    assert res["traj_e"].shape == (1, T, 7, 3) and torch.equal(res["traj_e"][0], q[0, None, :, 1:] + t) and bool(res["vis_e"].all())
    # None: the joint forward, and not one grouped call
    res0 = p(rgbs, d, q, k, e)
    assert model.plain == 1 and len(model.sets) == 1 and torch.equal(res0["traj_e"], res["traj_e"])
    for bad in (ids[:-1], ids.float(), ids[None], ids > 0):
        with pytest.raises(ValueError):
            p(rgbs, d, q, k, e, query_groups=bad)
    with pytest.raises(NotImplementedError, match="single_point"):
        EvaluationPredictor(model, interp_shape=None, single_point=True)(rgbs, d, q, k, e, query_groups=ids)
    with pytest.raises(NotImplementedError, match="backward_tracking"):
        EvaluationPredictor(model, interp_shape=None, backward_tracking=True)(rgbs, d, q, k, e, query_groups=ids)
    plain = torch.nn.Linear(1, 1)
    with pytest.raises(NotImplementedError, match="forward_grouped"):
        EvaluationPredictor(plain, interp_shape=None)(rgbs, d, q, k, e, query_groups=ids)
    assert model.plain == 1 and len(model.sets) == 1


def test_predictor_pass_through_and_no_mask_no_entry(monkeypatch, clip):
    from mvtracker_amd import EvaluationPredictor, MaskQueries, mask_queries, sample_queries
    hip_mock_masks.install(monkeypatch)
    lab, d, k, e = tensors(clip)
    sample_queries(d, k, e, [(0, -10.0, 10.0, 100.0, 5, "")])
    model = _GroupedModel()
    rgbs, _, q, _, _ = _predictor_inputs(clip, 3)
    EvaluationPredictor(model, interp_shape=None, grid_size=0)(rgbs, d, q, k, e)
    assert hip_mock_masks.calls == [] and hip_mock_masks.reads == [] and model.sets == []
    a = EvaluationPredictor.mask_queries(lab, d, k, e, MaskQueries(max_points_per_frame=4), seed=2)
    b = mask_queries(lab, d, k, e, MaskQueries(max_points_per_frame=4), seed=2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2].objects == b[2].objects
    assert torch.equal(EvaluationPredictor.mask_queries(lab, d, k, e)[0], mask_queries(lab, d, k, e)[0])


def test_demo_flags(tmp_path):
    import demo_amd
    from mvtracker_amd import MaskQueries
    parse = lambda *a: demo_amd.build_parser().parse_args(["--synthetic", *a])
    assert demo_amd.query_masks_from_args(parse()) is None
    assert demo_amd.query_masks_from_args(parse("--query-masks", "bands")) == MaskQueries(max_points_per_frame=256)
    got = demo_amd.query_masks_from_args(parse("--query-masks", "m", "--mask-frames-before", "0", "--mask-frames-after", "2", "--mask-anchor", "4",
                                               "--mask-distance-threshold", "0.3", "--mask-no-match", "--mask-max-points", "64", "--mask-method", "kmeans",
                                               "--per-mask-tracking", "--print-masks"))
    assert got == MaskQueries(anchor=4, frames_before=0, frames_after=2, distance_threshold=0.3, match=False, max_points_per_frame=64, method="kmeans")
    assert demo_amd.query_masks_from_args(parse("--query-masks", "m", "--mask-anchor", "first")).anchor == "first"
    for bad in (("--mask-no-match",), ("--per-mask-tracking",), ("--print-masks",), ("--mask-frames-before", "1"), ("--query-masks", "m", "--mask-anchor", "last"),
                ("--query-masks", "m", "--mask-max-points", "0"), ("--query-masks", "m", "--sample-queries", "random"),
                ("--query-masks", "m", "--per-mask-tracking", "--streaming"), ("--query-masks", "m", "--per-mask-tracking", "--single-point")):
        with pytest.raises(SystemExit):
            demo_amd.query_masks_from_args(parse(*bad))
    # --synthetic: depth bands per view, the odd views numbered from the far band
    d = torch.tensor([0.2, 1.0, 3.0, 4.0, 5.5]).reshape(1, 1, 1, 1, 1, 5).repeat(1, 2, 1, 1, 1, 1)
    lab = demo_amd.mask_labels(parse("--query-masks", "bands"), {"depths": d})
    assert lab.dtype == torch.uint8 and lab.shape == (2, 1, 1, 5) and lab[:, 0, 0].tolist() == [[0, 1, 2, 3, 0], [0, 3, 2, 1, 0]]
    # a sample file: a label map, or a stack of boolean instance masks
    m = np.zeros((2, 2, 4, 3, 5), bool)
    m[0, :, :, 0] = True
    m[1, :, :, :2] = True
    np.savez(tmp_path / "s.npz", labels=np.arange(2 * 4 * 3 * 5, dtype=np.int32).reshape(2, 4, 3, 5) % 3, inst=m)
    args = demo_amd.build_parser().parse_args(["--sample-path", str(tmp_path / "s.npz"), "--query-masks", "inst", "--temporal_stride", "2"])
    lab = demo_amd.mask_labels(args, {"depths": d})
    assert lab.shape == (2, 2, 3, 5) and lab[0, 0].tolist() == [[1] * 5, [2] * 5, [0] * 5]
    args.query_masks = "labels"
    assert demo_amd.mask_labels(args, {"depths": d}).shape == (2, 2, 3, 5)
    args.query_masks = "nothing"
    with pytest.raises(SystemExit):
        demo_amd.mask_labels(args, {"depths": d})


def test_entries_refuse_bad_arguments_without_a_launch():
    """Every mvt_mask_* entry returns MVT_ERR_ARG (1) for null or misaligned pointers and shapes it refuses, before any HIP call (so
    this runs without a device)."""
    import ctypes
    from mvtracker_amd import hip
    lib = hip._lib
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.addressof(buf) + 15) // 16 * 16  # host memory: only looked at for alignment, never launched on
    nan = float("nan")
    rc = {
        "stats null labels": lib.mvt_mask_stats(None, a, None, a, a, 1, 1, 8, 8, 0.0, 1.0, 0.0, a, None),
        "stats misaligned labels": lib.mvt_mask_stats(a + 4, a, None, a, a, 1, 1, 8, 8, 0.0, 1.0, 0.0, a, None),
        "stats null depths": lib.mvt_mask_stats(a, None, None, a, a, 1, 1, 8, 8, 0.0, 1.0, 0.0, a, None),
        "stats misaligned conf": lib.mvt_mask_stats(a, a, a + 2, a, a, 1, 1, 8, 8, 0.0, 1.0, 0.0, a, None),
        "stats null table": lib.mvt_mask_stats(a, a, None, a, a, 1, 1, 8, 8, 0.0, 1.0, 0.0, None, None),
        "stats misaligned table": lib.mvt_mask_stats(a, a, None, a, a, 1, 1, 8, 8, 0.0, 1.0, 0.0, a + 8, None),
        "stats no view": lib.mvt_mask_stats(a, a, None, a, a, 0, 1, 8, 8, 0.0, 1.0, 0.0, a, None),
        "stats too many views": lib.mvt_mask_stats(a, a, None, a, a, 65, 1, 8, 8, 0.0, 1.0, 0.0, a, None),
        "stats too many images": lib.mvt_mask_stats(a, a, None, a, a, 64, 1024, 8, 8, 0.0, 1.0, 0.0, a, None),
        "stats too many pixels": lib.mvt_mask_stats(a, a, None, a, a, 1, 1, 8192, 4096, 0.0, 1.0, 0.0, a, None),
        "stats nan bound": lib.mvt_mask_stats(a, a, None, a, a, 1, 1, 8, 8, nan, 1.0, 0.0, a, None),
        "centroids null": lib.mvt_mask_centroids(None, 1, 1, 1, a, None),
        "centroids min_pixels": lib.mvt_mask_centroids(a, 1, 1, 0, a, None),
        "centroids misaligned": lib.mvt_mask_centroids(a, 1, 1, 1, a + 4, None),
        "match null": lib.mvt_mask_match(a, 1, 1, 1, 0.1, 1, None, a, a, a, None),
        "match misaligned distance": lib.mvt_mask_match(a, 1, 1, 1, 0.1, 1, a, a, a + 4, a, None),
        "match min_common": lib.mvt_mask_match(a, 1, 1, 0, 0.1, 1, a, a, a, a, None),
        "match nan threshold": lib.mvt_mask_match(a, 1, 1, 1, nan, 1, a, a, a, a, None),
        "match flag": lib.mvt_mask_match(a, 1, 1, 1, 0.1, 2, a, a, a, a, None),
        "relabel null": lib.mvt_mask_relabel(a, None, 1, 1, 8, 8, a, None),
        "relabel misaligned out": lib.mvt_mask_relabel(a, a, 1, 1, 8, 8, a + 4, None),
        "relabel no pixel": lib.mvt_mask_relabel(a, a, 1, 1, 0, 8, a, None),
        "pool frame": lib.mvt_mask_pool(a, a, None, a, a, 1, 2, 2, 8, 8, 0.0, 1.0, 0.0, a, 0, 4, a, a, a, a, None),
        "pool negative object": lib.mvt_mask_pool(a, a, None, a, a, 1, 2, 0, 8, 8, 0.0, 1.0, 0.0, a, -1, 4, a, a, a, a, None),
        "pool negative capacity": lib.mvt_mask_pool(a, a, None, a, a, 1, 2, 0, 8, 8, 0.0, 1.0, 0.0, a, 0, -1, a, a, a, a, None),
        "pool null pool": lib.mvt_mask_pool(a, a, None, a, a, 1, 2, 0, 8, 8, 0.0, 1.0, 0.0, a, 0, 4, None, a, a, a, None),
        "pool null count": lib.mvt_mask_pool(a, a, None, a, a, 1, 2, 0, 8, 8, 0.0, 1.0, 0.0, a, 0, 4, a, a, None, a, None),
        "pool null table": lib.mvt_mask_pool(a, a, None, a, a, 1, 2, 0, 8, 8, 0.0, 1.0, 0.0, None, 0, 4, a, a, a, a, None),
    }
    print(rc)
    assert all(v == 1 for v in rc.values()), rc
