"""Mask queries on the device (`-m gpu`): mvt_mask_stats / centroids / match / relabel / pool and the host code on top of them
against the restatement tests/mask_ref.py.  Exact statistics on planted scenes whose unprojection is exact in fp32 (every label
pattern that takes another path through the statistics kernel), statistics and points on the synthetic clip at the pool tests' bar
(2e-5), the matching on planted lattices with exact distances (threshold equality, ties, no common frame, min_common_frames, three
cameras, match=False) and on the explainer's worked example, the relabelled clip, mask_queries end to end, and query_groups against
one forward per object.  Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_ref as R  # noqa: E402
import query_sampling_ref as Q  # noqa: E402
from mvtracker_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
V, T, H, W = 2, 3, 37, 53  # the query-sampling tests' shape: 1961 pixels per image, no multiple of 16, 64 or 256


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def api_args(labels, depths, intrs, extrs):
    """(V,T,..) numpy arrays -> the tensors the public entries take."""
    return dev(labels), dev(depths)[None], dev(intrs)[None], dev(extrs)[None]


def opts(**kw):
    from mvtracker_amd import MaskQueries
    return MaskQueries(**kw)


def host_stats(st):
    return {k: getattr(st, k).cpu().numpy() for k in ("pixels", "count", "sums", "centroid")}


# ------------------------------------------------------------------------------------------------------------------ exact statistics
def _exact_case(name):
    """-> (labels, depths, intrs, extrs, conf or None, option keywords)."""
    v, t, h, w = (V, T, 64, 64) if name == "multiple_64x64" else (V, 2, 9, 200) if name == "stripes_64" else (V, T, H, W)
    depths, intrs, extrs = R.exact_scene(v, t, h, w, seed=len(name))
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    lab = np.zeros((v, t, h, w), np.uint8)
    conf, kw = None, {}
    if name in ("one_label", "multiple_64x64", "bounds", "confidence"):
        lab[:] = 7
    elif name == "stripes_64":
        lab[:] = xs // 64 + 1
    elif name == "stripes_1":
        lab[:] = xs + 1
    elif name == "every_lane_another":
        lab[:] = (xs + ys) % 7 + 1
    elif name == "labels_1_128_255":
        lab[:] = np.where(ys < 12, 1, np.where(ys < 25, 128, 255))
        lab[:, :, ::5, ::3] = 0
    elif name == "background_view":
        lab[0] = (xs + ys) % 3 + 1
    elif name == "invalid_object":
        lab[:] = np.where(xs < 20, 1, 2)
        bad = np.array([0.0, np.nan, np.inf, -1.0, 1e-7, 2.0 ** 21], np.float32)  # none of them inside (1e-6, 2^20]
        depths[:, :, 0][lab == 2] = bad[np.arange((lab == 2).sum()) % len(bad)]
        depths[0, 1, 0, 3, 2] = 2.0 ** 19  # label 1: valid under max_depth = 2^20, but its point leaves the fixed-point range
        kw = dict(max_depth=2.0 ** 20)
    if name == "bounds":
        kw = dict(min_depth=0.5, max_depth=4.0)
        assert (depths == 0.5).sum() > 10 and (depths == 4.0).sum() > 10
    if name == "confidence":
        conf = (np.random.default_rng(3).integers(1, 4, size=depths.shape) / 4.0).astype(np.float32)
        kw = dict(conf_thresh=0.5)
        assert (conf == 0.5).sum() > 10
    return lab, depths, intrs, extrs, conf, kw


EXACT = ["one_label", "stripes_64", "stripes_1", "every_lane_another", "labels_1_128_255", "background_view", "invalid_object", "bounds", "confidence",
         "multiple_64x64"]


@pytest.mark.parametrize("name", EXACT)
def test_exact_statistics(name):
    from mvtracker_amd import mask_statistics
    lab, depths, intrs, extrs, conf, kw = _exact_case(name)
    # the planted scene first: fp32 and fp64 arithmetic give the same points, so the reference's integer sums are exact
    p32, p64 = R.clip_points(depths, intrs, extrs), R.clip_points(depths, intrs, extrs, np.float64)
    ok = R.valid_pixels(lab.astype(np.int64), depths, R.options(**kw), conf)
    assert np.array_equal(p32[ok].astype(np.float64), p64[ok]) and ok.sum() > 1000
    ref = R.statistics(lab, depths, intrs, extrs, R.options(**kw), conf)
    args = api_args(lab, depths, intrs, extrs)
    c = None if conf is None else dev(conf)[None]
    st = mask_statistics(*args, opts(**kw), depths_conf=c)
    got = host_stats(st)
    print(name, "labelled", int(ref["pixels"].sum()), "valid", int(ref["count"].sum()), "out of range", int(ref["out_of_range"].sum()),
          "labels", int((ref["pixels"].sum((0, 1)) > 0).sum()))
    for k in ("pixels", "count", "sums"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["centroid"], ref["centroid"], equal_nan=True)
    assert st.out_of_range == int(ref["out_of_range"].sum())
    assert ref["pixels"].sum() > 0 and ref["pixels"][:, :, 0].sum() == 0
    if name == "invalid_object":
        assert ref["pixels"][:, :, 2].min() > 0 and ref["count"][:, :, 2].sum() == 0 and np.isnan(ref["centroid"][:, :, 2]).all()
        assert ref["out_of_range"].sum() == 1 and ref["out_of_range"][0, 1, 1] == 1
    if name == "bounds":
        d = depths[:, :, 0]
        assert ref["count"].sum() == ((d > 0.5) & (d <= 4.0)).sum() < ref["pixels"].sum()
    if name == "confidence":
        assert ref["count"].sum() == (conf > 0.5).sum() < ref["pixels"].sum()
    if name == "background_view":
        assert ref["pixels"][1].sum() == 0 and np.isnan(ref["centroid"][1]).all()
    # two runs, and a wider label type: the same bits
    again = mask_statistics(args[0].to(torch.int32), *args[1:], opts(**kw), depths_conf=c)
    assert torch.equal(again._tables.buf, st._tables.buf)


# ------------------------------------------------------------------------------------------------------------------ the synthetic clip
def world_labels(c):
    """Labels from world-space regions (what rises above the ground, then rings of the ground around the origin), so that the two
    cameras see the same things; view 1 numbers them in another order (local ids)."""
    pts = R.clip_points(c["depths"], c["intrs"], c["extrs"])
    r = np.sqrt(pts[..., 0] ** 2 + pts[..., 1] ** 2)
    lab = np.where(pts[..., 2] > 0.2, 1, np.where(r < 1.2, 2, np.where(r < 2.5, 3, 4))).astype(np.uint8)
    lab[1] = lab[1] % 4 + 1
    lab[:, :, :, :5] = 0  # a strip of background
    lab[c["depths"][:, :, 0] == 0] = 2  # (the clip's invalid pixels are labelled too)
    return lab


@pytest.fixture(scope="module")
def clip():
    c = synth.make_clip(11, V=V, T=T, H=H, W=W, N=4, invalid_frac=0.02)
    c = {k: v[0] for k, v in c.items()}
    c["labels"] = world_labels(c)
    assert len(np.unique(c["labels"])) >= 4
    return c


def clip_args(clip):
    return api_args(clip["labels"], clip["depths"], clip["intrs"], clip["extrs"])


def ref_args(clip):
    return clip["labels"], clip["depths"], clip["intrs"], clip["extrs"]


def test_statistics_on_the_synthetic_clip(clip):
    from mvtracker_amd import mask_statistics
    ref = R.statistics(*ref_args(clip), R.options())
    got = host_stats(mask_statistics(*clip_args(clip)))
    err = np.nanmax(np.abs(got["centroid"] - ref["centroid"]))
    print("valid", int(ref["count"].sum()), "of", int(ref["pixels"].sum()), "centroid error", err)
    assert np.array_equal(got["pixels"], ref["pixels"]) and np.array_equal(got["count"], ref["count"]) and 0 < ref["count"].sum() < ref["pixels"].sum()
    assert np.array_equal(np.isnan(got["centroid"]), np.isnan(ref["centroid"])) and err < 2e-5


def test_lift_equals_frame_pool_bit_for_bit(clip):
    """One label over everything, match=False: the lifted points are frame_pool's rows, the pixels the raster indices it kept."""
    from mvtracker_amd import hip, lift_masks, queries
    lab = np.ones_like(clip["labels"])
    args = api_args(lab, clip["depths"], clip["intrs"], clip["extrs"])
    kinv, einv = torch.empty(V * T, 9, device=DEV), torch.empty(V * T, 12, device=DEV)
    hip.invert_cameras(args[2][0].reshape(V * T, 9).contiguous(), args[3][0].reshape(V * T, 12).contiguous(), kinv, einv, V * T)
    for t in range(T):
        pts, oid, pix = lift_masks(*args, t, options=opts(match=False))
        pool = queries.frame_pool(args[1][0], kinv, einv, t)
        keep = np.nonzero(clip["depths"][:, t, 0].reshape(-1) > 0)[0]
        print("frame", t, "pool", tuple(pool.shape))
        assert 0 < len(keep) < V * H * W and torch.equal(pts, pool) and not oid.any() and oid.dtype == torch.int32
        assert pix.dtype == torch.int32 and np.array_equal(pix.cpu().numpy(), keep)


def test_lift_several_objects(clip):
    from mvtracker_amd import lift_masks, mask_statistics, match_mask_ids
    o = dict(distance_threshold=1.0)
    mt = match_mask_ids(mask_statistics(*clip_args(clip), opts(**o)), opts(**o))
    rm = R.matching(R.statistics(*ref_args(clip), R.options(**o))["centroid"], R.options(**o))
    assert rm["margin"] > 1e-9 and np.array_equal(mt.global_id.cpu().numpy(), rm["global_id"]) and rm["num_objects"] >= 3
    assert max(len(m) for m in rm["members"].values()) >= 3  # an object with members of both cameras, two of them of one camera
    pts, oid, pix = lift_masks(*clip_args(clip), 1, matching=mt, options=opts(**o))
    exp = [R.object_pool(*ref_args(clip), R.options(**o), rm["global_id"], g, 1) for g in range(rm["num_objects"])]
    print("objects", rm["num_objects"], "pools", [len(i) for i, _ in exp])
    assert np.array_equal(pix.cpu().numpy(), np.concatenate([i for i, _ in exp]))
    assert np.array_equal(oid.cpu().numpy(), np.concatenate([np.full(len(i), g, np.int32) for g, (i, _) in enumerate(exp)]))
    assert np.abs(pts.cpu().numpy() - np.concatenate([p for _, p in exp])).max() < 2e-5
    again = lift_masks(*clip_args(clip), 1, options=opts(**o))  # the matching computed inside: the same rows
    assert all(torch.equal(a, b) for a, b in zip(again, (pts, oid, pix)))


@pytest.mark.parametrize("h,w,nb", [(241, 272, 257), (399, 449, 700)])
def test_pool_of_more_than_256_workgroups(h, w, nb):
    """More than 65 536 pixels: every thread of mvt_mask_pool's one-workgroup scan owns a chunk of 2 (257 workgroups) or 3 (700: the
    last chunk partial) counts.  The object covers a hashed half of the pixels, with runs of whole workgroups empty in the middle and
    at the end; the scene's unprojection is exact in fp32, so the points are compared for equality."""
    from mvtracker_amd import lift_masks, mask_statistics, match_mask_ids
    depths, intrs, extrs = R.exact_scene(1, 2, h, w, seed=nb)
    n = h * w
    assert (n + 255) // 256 == nb
    i = np.arange(n, dtype=np.uint64)
    blk = (i // 256).astype(np.int64)
    on = (((i * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)) & np.uint64(1) == 1) & ~((blk >= nb // 3) & (blk < nb // 3 + 7)) & (blk < nb - 5)
    lab = np.zeros((1, 2, h, w), np.uint8)
    lab[0, 1] = on.reshape(h, w)
    lab[0, 0, :3] = 1  # (frame 0 is not the frame read)
    o = dict(match=False)
    args = api_args(lab, depths, intrs, extrs)
    mt = match_mask_ids(mask_statistics(*args, opts(**o)), opts(**o))
    gid = mt.global_id.cpu().numpy()
    assert gid[0][1] == 0
    idx, ref = R.object_pool(lab, depths, intrs, extrs, R.options(**o), gid, 0, 1)
    per = np.bincount(idx // 256, minlength=nb)
    print(f"{h} x {w}: {nb} workgroups, pool {len(idx)} of {n}, {int((per == 0).sum())} workgroups empty")
    assert np.array_equal(idx, np.flatnonzero(on)) and 0.4 * n < len(idx) < 0.55 * n and (per == 0).sum() == 12
    pts, oid, pix = lift_masks(*args, 1, matching=mt, options=opts(**o))
    assert pts.shape == (len(idx), 3) and np.array_equal(pix.cpu().numpy(), idx) and not oid.any()  # count, pixel
    assert np.array_equal(pts.cpu().numpy(), ref)


# ------------------------------------------------------------------------------------------------------------------ matching
def _all(frames, rect):
    return {t: rect for t in frames}


# name -> (instances per camera, frames, option keywords, expected tables per camera, planted tie)
LATTICE = {
    # 3-4-5 at focal 32: (3, 4) pixels apart = 5 / 32 = the threshold exactly -> not matched; (0, 3) apart = 3 / 32 -> matched
    "threshold_equality": ([{1: _all(range(4), (0, 0, 1, 1))}, {1: _all(range(4), (3, 4, 1, 1)), 2: _all(range(4), (0, 3, 1, 1))}], 4,
                           dict(distance_threshold=5 / 32), [{1: 0}, {1: 1, 2: 0}], True),
    # two objects of camera 0 at 5 / 32 each from camera 1's blob: the lowest global id wins (camera 0 lists the far-sorted label first)
    "tie_lowest_id": ([{1: _all(range(2), (6, 8, 1, 1)), 2: _all(range(2), (0, 0, 1, 1))}, {5: _all(range(2), (3, 4, 1, 1))}], 2,
                      dict(distance_threshold=0.25), [{1: 0, 2: 1}, {5: 0}], True),
    "no_common_frame": ([{1: _all(range(2), (2, 2, 1, 1))}, {1: _all(range(2, 4), (2, 2, 1, 1))}], 4, dict(), [{1: 0}, {1: 1}], False),
    "min_common_2_of_1": ([{1: _all(range(4), (2, 2, 1, 1))}, {1: _all(range(3, 4), (2, 5, 1, 1)), 2: _all(range(2, 4), (5, 6, 1, 1))}], 4,
                          dict(min_common_frames=2, distance_threshold=0.25), [{1: 0}, {1: 1, 2: 0}], False),
    "min_common_1_of_1": ([{1: _all(range(4), (2, 2, 1, 1))}, {1: _all(range(3, 4), (2, 5, 1, 1)), 2: _all(range(2, 4), (5, 6, 1, 1))}], 4,
                          dict(min_common_frames=1, distance_threshold=0.25), [{1: 0}, {1: 0, 2: 0}], False),
    # camera 2 is 6 / 32 from camera 0's blob and 3 / 32 from camera 1's, which joined object 0: the minimum over the members
    "third_camera_via_second": ([{3: _all(range(2), (0, 0, 1, 1))}, {1: _all(range(2), (0, 3, 1, 1))}, {2: _all(range(2), (0, 6, 1, 1)), 9: _all(range(2), (12, 5, 1, 1))}], 2,
                                dict(distance_threshold=0.125), [{3: 0}, {1: 0}, {2: 0, 9: 1}], False),
    "match_false": ([{1: _all(range(2), (0, 0, 1, 1)), 4: _all(range(2), (9, 9, 1, 1))}, {4: _all(range(2), (0, 0, 1, 1))}], 2, dict(match=False),
                    [{1: 0, 4: 3}, {4: 3}], False),
}


def _worked_example():
    """AVERAGE_DISTANCE_MATCHING.md: camera 0 has ids 1 and 2 over ten frames; camera 1 has id 1 in frames 2-9 and ids 2 and 4 in frames
    5-9; 2 x 2 blobs on the plane at focal 64, two pixels (0.031) between the matching blobs, 18 pixels (0.281) to the third."""
    cam0 = {1: _all(range(10), (4, 4, 2, 2)), 2: _all(range(10), (30, 4, 2, 2))}
    cam1 = {1: _all(range(2, 10), (6, 4, 2, 2)), 2: _all(range(5, 10), (30, 6, 2, 2)), 4: _all(range(5, 10), (4, 22, 2, 2))}
    return R.lattice_scene([cam0, cam1], 10, H=32, W=40, focal=64.0), dict(), [{1: 0, 2: 1}, {1: 0, 2: 1, 4: 2}]


@pytest.mark.parametrize("name", list(LATTICE) + ["worked_example"])
def test_matching(name):
    from mvtracker_amd import mask_statistics, match_mask_ids
    if name == "worked_example":
        scene, kw, tables = _worked_example()
        tie = False
    else:
        inst, frames, kw, tables, tie = LATTICE[name]
        scene = R.lattice_scene(inst, frames)
    nT = scene[0].shape[1]
    ref_st = R.statistics(*scene, R.options(**kw))
    rm = R.matching(ref_st["centroid"], R.options(**kw))
    exp = np.full((len(tables), 256), -1, np.int32)
    for v, tb in enumerate(tables):
        for l, g in tb.items():
            exp[v, l] = g
    print(name, "expected", tables, "margin", rm["margin"], "distances", rm["distance"][np.isfinite(rm["distance"])])
    assert np.array_equal(rm["global_id"], exp)  # the restatement gives the tables written down here
    assert rm["margin"] == 0.0 if tie else rm["margin"] > 1e-9  # outside the planted ties no decision is close
    st = mask_statistics(*api_args(*scene), opts(**kw))
    assert np.array_equal(st.sums.cpu().numpy(), ref_st["sums"]) and np.array_equal(st.centroid.cpu().numpy(), ref_st["centroid"], equal_nan=True)
    mt = match_mask_ids(st, opts(**kw))
    assert np.array_equal(mt.global_id.cpu().numpy(), exp) and mt.num_objects == rm["num_objects"] and mt.members == rm["members"]
    d, rd = mt.distance.cpu().numpy(), rm["distance"]
    assert np.array_equal(np.isnan(d), np.isnan(rd))
    ok = np.isfinite(rd)
    assert (np.abs(d[ok] - rd[ok]) <= (nT + 8) * 2.0 ** -52 * np.abs(rd[ok])).all()
    if name == "worked_example":
        assert abs(rd[1, 1] - 2 / 64) < 1e-12 and abs(rd[1, 2] - 2 / 64) < 1e-12 and np.isnan(rd[1, 4])
    again = match_mask_ids(mask_statistics(*api_args(*scene), opts(**kw)), opts(**kw))
    assert torch.equal(again._tables.buf, mt._tables.buf)


def test_global_masks_is_the_table_lookup(clip):
    from mvtracker_amd import global_masks, mask_statistics, match_mask_ids
    o = dict(distance_threshold=1.0)
    mt = match_mask_ids(mask_statistics(*clip_args(clip), opts(**o)), opts(**o))
    gid = mt.global_id.cpu().numpy()
    lab = clip["labels"]
    exp = np.where(lab > 0, np.stack([gid[v][lab[v]] for v in range(V)]), -1).astype(np.int32)
    got = global_masks(dev(lab), mt)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), exp) and (exp >= 0).any() and (exp < 0).any()
    assert torch.equal(global_masks(dev(lab).to(torch.int64)[None], mt), got)
    big = np.tile(lab, (1, 1, 3, 5))  # 29415 pixels per image: whole 16-pixel groups and a tail
    assert np.array_equal(global_masks(dev(big), mt).cpu().numpy(), np.tile(exp, (1, 1, 3, 5)))


# ------------------------------------------------------------------------------------------------------------------ end to end
E2E = [dict(distance_threshold=1.0), dict(distance_threshold=1.0, max_points_per_frame=50), dict(distance_threshold=1.0, max_points_per_frame=100000),
       dict(distance_threshold=1.0, anchor=2, frames_before=1, frames_after=3, max_points_per_frame=33),
       dict(distance_threshold=1.0, anchor={(0, 1): 2, (1, 3): 0, (0, 200): 1}, frames_before=0, frames_after=0),
       dict(match=False, frames_before=0, frames_after=0, min_pixels=40)]


@pytest.mark.parametrize("kw", E2E)
def test_mask_queries_end_to_end(clip, kw):
    from mvtracker_amd import mask_queries
    rows, rids, objects, pools, rm = R.mask_queries(*ref_args(clip), R.options(**kw), seed=5)
    assert rm["margin"] > 1e-9
    q, ids, report = mask_queries(*clip_args(clip), opts(**kw), seed=5)
    print(kw, "rows", len(rows), "objects", [(o["object"], o["frames_used"], o["pool_sizes"], o["rows"]) for o in objects])
    assert q.shape == (1, len(rows), 4) and q.dtype == torch.float32 and ids.dtype == torch.int32 and ids.device == q.device
    g = q[0].cpu().numpy()
    assert np.array_equal(g[:, 0], rows[:, 0]) and np.abs(g[:, 1:] - rows[:, 1:]).max() < 2e-5
    assert np.array_equal(ids.cpu().numpy(), rids) and report.objects == objects and report.matching.members == rm["members"]
    assert [p.shape[1] for p in report.split(q)] == [o["rows"] for o in objects if o["rows"]]
    q2, ids2, _ = mask_queries(*clip_args(clip), opts(**kw), seed=5)
    assert torch.equal(q, q2) and torch.equal(ids, ids2)


def test_mask_queries_kmeans(clip):
    """The rows of method "kmeans" are kmeans_centres of the very pools the random method draws from, seeded seed + k."""
    from mvtracker_amd import kmeans_centres, mask_queries
    kw = dict(distance_threshold=1.0, frames_before=0, frames_after=0)
    full, _, rep = mask_queries(*clip_args(clip), opts(**kw))
    sizes = [m for o in rep.objects for m in o["pool_sizes"]]
    q, ids, rep_k = mask_queries(*clip_args(clip), opts(**kw, max_points_per_frame=12, method="kmeans"), seed=3)
    o, exp = 0, []
    for k, m in enumerate(sizes):
        pool = full[0, o:o + m]
        exp.append(torch.cat([pool[:, :1][:min(m, 12)], kmeans_centres(pool[:, 1:].contiguous(), 12, seed=3 + k)[0]], 1) if m > 12 else pool)
        o += m
    print("pools", sizes)
    assert sum(m > 12 for m in sizes) >= 2 and torch.equal(q[0], torch.cat(exp)) and [o["pool_sizes"] for o in rep_k.objects] == [o["pool_sizes"] for o in rep.objects]
    assert torch.equal(mask_queries(*clip_args(clip), opts(**kw, max_points_per_frame=12, method="kmeans"), seed=3)[0], q)


def test_no_row_raises(clip):
    from mvtracker_amd import mask_queries
    a = clip_args(clip)
    with pytest.raises(ValueError, match="depth bounds"):
        mask_queries(*a, opts(min_depth=50.0, max_depth=60.0))
    with pytest.raises(ValueError):
        mask_queries(a[0].to(torch.int32) + 300, *a[1:])


# ------------------------------------------------------------------------------------------------------------------ query_groups
def test_query_groups_equal_one_forward_per_object():
    """fp32, synthetic weights: forward(query_groups=ids) returns per object the bits of a forward on that object's queries alone."""
    from mvtracker_amd import EvaluationPredictor
    from mvtracker_amd.tracker import MVTracker
    m = MVTracker(hidden_size=256).eval()
    sd = synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.to(DEV)
    m.precision = "fp32"
    c = synth.make_clip(62, V=2, T=12, H=128, W=128, N=9, late_queries=True, query_frames=(3,))
    a = [dev(c[k][0])[None] for k in ("rgbs", "depths", "query_points", "intrs", "extrs")]
    ids = torch.tensor([2, 0, 2, 2, 5, 0, 5, 2, 2], dtype=torch.int32, device=DEV)
    pred = EvaluationPredictor(m, interp_shape=None, grid_size=2, n_iters=2)
    res = pred(rgbs=a[0], depths=a[1], query_points_3d=a[2], intrs=a[3], extrs=a[4], query_groups=ids)
    assert res["traj_e"].shape == (1, 12, 9, 3) and bool(torch.isfinite(res["traj_e"]).all())
    for g in (0, 2, 5):
        rows = torch.nonzero(ids == g)[:, 0]
        own = pred(rgbs=a[0], depths=a[1], query_points_3d=a[2][:, rows], intrs=a[3], extrs=a[4])
        for key in ("traj_e", "vis_e_as_prob", "vis_e"):
            assert torch.equal(res[key][:, :, rows], own[key]), (g, key)
    joint = pred(rgbs=a[0], depths=a[1], query_points_3d=a[2], intrs=a[3], extrs=a[4])
    assert not torch.equal(joint["traj_e"], res["traj_e"])  # (the groups really were tracked apart)
