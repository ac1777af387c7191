"""Exact inputs and scalar restatements for csrc/metrics.hip and the view assignment of csrc/pyramid.hip -- TEST INFRASTRUCTURE ONLY.

For tests/test_gpu_metrics_view_exact.py.  No torch device use.  Two things live here:

* the input builders.  Tracks: gt[t, n] = base[n] + s[t, n] * dir[n] with an integer walk s, |s| <= 100, an integer base and a
  direction from a Pythagorean triple over 16; pred = gt + m * dir', m a small integer.  Every difference is a multiple of 1/16,
  every squared length a perfect square over 256 below 2^24, so each distance and each step of the path length is exact in fp32
  whether the products are fused or not (a track that turned would put two visible frames at a distance that is no triple: each
  track stays on its line).  The one-fp32-step cases use an error along one axis on which gt is 0, where sqrt(fl(x * x)) == |x|.
  Cameras: signed permutation rotations, dyadic translations, power-of-two focal lengths, (half-)integer principal points,
  integer depth maps 0..15 -- different for every (view, frame).  In frame t every view's optical axis reads world axis
  (2, 0, 1)[t] and the queries of that frame differ from the frame's anchor point by integers along the other two axes, so a
  query's camera z is the power of two planted for (view, frame), pixel x / y are multiples of 1/8, the bilinear weights
  multiples of 1/64 and the blend and the score exact.  ``assert_tracks_exact`` / ``best_view(check=True)`` assert all of that
  in fp64: every product and partial sum is a float32.

* the scalar restatements ``track_rows`` and ``best_view``: one plain Python loop per track / per query in fp64 and integers,
  written from the kernels' header comments and the reference's rules (metrics.py:10-58, 61-171, 327-330;
  monocular_baselines.py:630-680 with bilinear_sample2d), not vectorised like oracle/.  Rules worth stating:
    - gt visibility is masked to frames >= the query frame; the query frame is not an evaluation point, but counts for the
      trajectory errors, the visible-frame count and the movement;
    - `within` is dist < thr; it is false for a NaN distance (`~within` is true for NaN, the reference's rule), so a non-finite
      prediction that is not flagged occluded is a false positive at every threshold.  Where gt is occluded a finite one is a
      false positive too, and before the query nothing is counted: such predictions move no column at all;
    - ratios are float32(a) / float32(b) of the integer counts (0/0 = NaN); the averages over K are summed in float32 in
      ascending k and divided by float32(K);
    - MTE is the LOWER median; ATE is the fp64 mean rounded once; FDE is the distance at the last visible frame; survival is
      (first visible frame with dist > thr, else T, minus qt) / (T - qt);
    - a view is outside for x < 0, x >= W, y < 0, y >= H or z < 0; its score is then -1e4 - z, else the blend of four clamped
      taps with weights from the unclamped corners, minus z; the first maximum wins.

``fault=`` plants one named mistake; the probes show that the tests' own inputs see it:

    le_dist            dist <= thr counts as within                       ge_survival     dist >= thr fails
    upper_median       the upper of the two middle values                 carry_dropped   a step without a visible frame loses
    last_first_step    the last visible frame is searched in frames 0..63                 the previous visible position
    pre_query_visible  gt visibility is not masked to frames >= the query frame
    frame0_cams        every query reads frame 0's cameras                frame0_depth    ... frame 0's depth maps
    clamped_weights    bilinear weights from the clamped corners          x_gt_w          outside for x > W, not x >= W
    last_max           the last maximum wins                              no_z_test       see below

A probe for `z <= 0 in place of z < 0` was wanted as well.  No input can show that fault: z == 0 makes x and y infinite (outside on
either reading) or NaN (no defined answer), which is why z == 0 is not used.  ``no_z_test`` (a view behind the camera whose x and
y land in the box counts as inside) stands in its place and is what the negative-z queries pin.
"""
import functools
import itertools
import math
import zlib

import numpy as np

F32 = np.float32
NAN = float("nan")
INF = float("inf")

METRIC_FAULTS = ("le_dist", "ge_survival", "upper_median", "carry_dropped", "last_first_step", "pre_query_visible")
VIEW_FAULTS = ("frame0_cams", "frame0_depth", "clamped_weights", "x_gt_w", "last_max", "no_z_test")


def rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def is_f32(x):
    """fp64 array / scalar: every finite value is a float32."""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return bool(np.all((x.astype(F32).astype(np.float64) == x) | ~np.isfinite(x)))


def up(x):
    return float(np.nextafter(F32(x), F32(INF)))


def dn(x):
    return float(np.nextafter(F32(x), F32(-INF)))


def ratio(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return F32(a) / F32(b)


# ================================================================== tracks

DIRS16 = np.array([(1, 0, 0), (0, -2, 0), (3, 4, 0), (0, -3, 4), (4, 0, -3), (5, 12, 0), (8, 0, 15)], np.float64) / 16
THRESH = [0.25, 0.5, 1.0, 2.0, 4.0, 0.125, 8.0, 16.0]  # dyadic; the first K are used
SMAX = 100  # |s|: (2 * SMAX * 17)^2 < 2^24, the squared length of the longest step in units of 1/256


def dirs(D):
    """The directions cut to D components: (0,-3,4) -> (0,-3), (4,0,-3) -> (4,0), (8,0,15) -> (8,0) are single axes, the rest keep
    their triple."""
    d = DIRS16[:, :D]
    ln = np.sqrt((d * d).sum(-1)) * 16
    assert np.array_equal(ln, np.round(ln)) and ln.min() >= 1
    return d


def walk(r, T, n=None):
    """Integer walk with steps in -2..2 (zero steps included), reflected into [-SMAX, SMAX]."""
    shape = (T,) if n is None else (T, n)
    s = np.cumsum(r.integers(-2, 3, shape), 0) + r.integers(-20, 21, shape[1:])
    s = np.abs((s + SMAX) % (4 * SMAX) - 2 * SMAX) - SMAX  # triangle wave: steps keep their size
    assert np.abs(s).max() <= SMAX and (T == 1 or np.abs(np.diff(s, axis=0)).max() <= 2)
    return s


def make_clip(gt, pred, vis, occ, qt, thr, surv):
    T, N, D = gt.shape
    c = dict(gt=np.ascontiguousarray(gt, F32), pred=np.ascontiguousarray(pred, F32), vis=np.ascontiguousarray(vis, np.uint8),
             occ=np.ascontiguousarray(occ, np.uint8), qt=np.ascontiguousarray(qt, np.int32), thr=[float(t) for t in thr], surv=float(surv))
    assert c["vis"].shape == (T, N) and c["occ"].shape == (T, N) and c["qt"].shape == (N,)
    assert c["qt"].min() >= 0 and c["qt"].max() <= T - 1
    assert is_f32(np.asarray(gt, np.float64)) and is_f32(np.asarray(pred, np.float64))
    assert_tracks_exact(c)
    return c


def _assert_lengths_exact(diff):
    """diff (..., D) fp64: fma(dz,dz,fma(dy,dy,dx*dx)) and the unfused chain give the exact length in fp32."""
    assert is_f32(diff)
    nz = (diff != 0).sum(-1)
    one = nz <= 1
    a = np.abs(diff).max(-1)
    a32 = a.astype(F32)
    with np.errstate(over="ignore"):
        assert np.array_equal(np.sqrt(a32[one] * a32[one]), a32[one])  # single axis: sqrt(fl(x * x)) == |x|
    d = diff[~one]
    sq = d * d
    part = np.cumsum(sq, -1)
    assert is_f32(sq) and is_f32(part)
    ln = np.sqrt(part[..., -1])
    assert is_f32(ln) and np.array_equal(ln * ln, part[..., -1])


def assert_tracks_exact(c):
    gt, pr = c["gt"].astype(np.float64), c["pred"].astype(np.float64)
    T, N, D = gt.shape
    fin = np.isfinite(pr).all(-1)
    _assert_lengths_exact((pr - gt)[fin])
    masked = (c["vis"] != 0) & (np.arange(T)[:, None] >= c["qt"][None, :])
    assert not (masked & ~fin).any(), "non-finite predictions only where gt is occluded or before the query"
    for n in range(N):
        p = gt[masked[:, n], n]
        if len(p) > 1:
            _assert_lengths_exact(p[1:] - p[:-1])


def track_rows(c, fault=None):
    """(N, 11 + 2K) float32 in the column order of mvt_track_metrics: the scalar restatement."""
    gt, pr = c["gt"].astype(np.float64), c["pred"].astype(np.float64)
    T, N, D = gt.shape
    thr = [float(F32(t)) for t in c["thr"]]
    surv = float(F32(c["surv"]))
    K = len(thr)
    out = np.full((N, 11 + 2 * K), NAN, F32)
    for n in range(N):
        q = int(c["qt"][n])
        g, p = gt[:, n].tolist(), pr[:, n].tolist()
        gv, po = c["vis"][:, n].tolist(), c["occ"][:, n].tolist()
        dist = [math.sqrt(sum((p[t][a] - g[t][a]) ** 2 for a in range(D))) for t in range(T)]
        vis = [gv[t] != 0 and (t >= q or fault == "pre_query_visible") for t in range(T)]
        n_eval = n_agree = n_occ = n_occ_agree = n_vis = n_vis_agree = 0
        n_within, n_tp, n_fp = [0] * K, [0] * K, [0] * K
        for t in range(q + 1, T):  # the evaluation points: after the query frame
            pocc, gocc = po[t] != 0, not vis[t]
            n_eval += 1
            n_agree += pocc == gocc
            n_occ += gocc
            n_occ_agree += gocc and pocc
            n_vis += not gocc
            n_vis_agree += (not gocc) and (not pocc)
            for k in range(K):
                within = dist[t] <= thr[k] if fault == "le_dist" else dist[t] < thr[k]  # False for NaN
                n_within[k] += within and not gocc
                n_tp[k] += within and not pocc and not gocc
                n_fp[k] += ((not within) and not pocc) or ((not pocc) and gocc)
        frames = [t for t in range(T) if vis[t]]
        move, prev = 0.0, None
        for t in frames:
            if prev is not None and not (fault == "carry_dropped" and t // 64 - prev // 64 > 1):
                move += math.sqrt(sum((g[t][a] - g[prev][a]) ** 2 for a in range(D)))
            prev = t
        o = out[n]
        o[0] = F32(move)
        o[1] = F32(len(frames))
        o[2], o[3], o[4] = ratio(n_agree, n_eval), ratio(n_occ_agree, n_occ), ratio(n_vis_agree, n_vis)
        pw = [ratio(n_within[k], n_vis) for k in range(K)]
        jc = [ratio(n_tp[k], n_vis + n_fp[k]) for k in range(K)]
        spw = sjc = F32(0)
        for k in range(K):
            spw = F32(spw + pw[k])
            sjc = F32(sjc + jc[k])
        o[5], o[6] = sjc / F32(K), spw / F32(K)
        if frames:
            v = sorted(dist[t] for t in frames)
            o[7] = F32(v[len(v) // 2 if fault == "upper_median" else (len(v) - 1) // 2])
            o[8] = F32(sum(v) / len(v))
            cand = [t for t in frames if t < 64] if fault == "last_first_step" else frames
            if cand:
                o[9] = F32(dist[cand[-1]])
        fail = [t for t in frames if (dist[t] >= surv if fault == "ge_survival" else dist[t] > surv)]
        o[10] = ratio((fail[0] if fail else T) - q, T - q)
        o[11:11 + K] = pw
        o[11 + K:11 + 2 * K] = jc
    return out


def column_names(thr):
    th = [f"{float(F32(t)):.2f}" for t in thr]
    return ["occlusion_accuracy", "occlusion_accuracy_for_vis0", "occlusion_accuracy_for_vis1", "average_jaccard",
            "average_pts_within_thresh", "mte_visible", "ate_visible", "fde_visible", "survival"] + \
        [f"pts_within_{t}" for t in th] + [f"jaccard_{t}" for t in th]


def query_points_of(c):
    """(N, 1 + D) float32: the query frame and the gt position there."""
    N = c["gt"].shape[1]
    return np.concatenate([c["qt"][:, None].astype(F32), c["gt"][c["qt"], np.arange(N)]], -1)


def masked_vis(c):
    return (c["vis"] != 0) & (np.arange(c["gt"].shape[0])[:, None] >= c["qt"][None, :])


# ------------------------------------------------------------------ random clips on lines

@functools.lru_cache(maxsize=None)
def random_clip(T, N, D, K):
    r = rng("clip", T, N, D, K)
    dd = dirs(D)
    s = walk(r, T, N)
    base = r.integers(-8, 9, (N, D)).astype(np.float64)
    gt = base[None] + s[..., None] * dd[r.integers(0, len(dd), N)][None]
    e = r.integers(-3, 4, (T, N, 1)) * dd[r.integers(0, len(dd), (T, N))]
    vis = (r.random((T, N)) < r.choice([0.7, 0.7, 0.03], N)[None]).astype(np.uint8)  # a sparse track has whole steps without a visible frame
    occ = (r.random((T, N)) < 0.4).astype(np.uint8)
    qt = r.integers(0, T, N)
    if T == 1024:  # the full LDS buffer of the median: every frame of track 0 is visible
        vis[:, 0], qt[0] = 1, 0
    return make_clip(gt, gt + e, vis, occ, qt, THRESH[:K], [1.0, 0.5, 2.0][K % 3])


DK = list(itertools.product((2, 3), (1, 5, 8)))
# every (T, N) with (D, K) in rotation, and every (D, K) at one shape
SHAPES = list(dict.fromkeys([(T, N) + DK[i % 6] for i, (T, N) in enumerate(itertools.product((1, 2, 63, 64, 65, 128, 129, 1024), (1, 3, 4, 5, 9)))] +
                            [(65, 5, D, K) for D, K in DK]))


# ------------------------------------------------------------------ planted tracks

PLANT_T = 257
PLANT_THR = [0.25, 0.5, 1.0, 2.0, 4.0]
PLANT_SURV = 0.5


def _plant(D):
    """name -> (s, dir index, errors (T, D), gt_visible bytes, pred_occluded bytes, query frame), T = 257.  Errors lie along axis 0;
    every track but `ramp` ones moves along direction 1, (0,-2,0)/16, so gt is 0 on axis 0 and pred = gt + e is exact."""
    T = PLANT_T
    fr = np.arange(T)
    ramp = np.minimum(fr // 2, SMAX)  # s[3] = 1, s[63] = 31, s[64] = 32, s[128] = 64, s[200] = 100
    tr = {}

    def add(name, vis, qt=0, err=None, occ=None, s=None, d=1):
        r = rng("plant", name)
        e = np.zeros((T, D))
        if err is not None:
            e[:, 0] = err
        v = np.zeros(T, np.uint8)
        if isinstance(vis, str) and vis == "all":
            v[:] = 1
        elif isinstance(vis, np.ndarray):
            v[:] = vis
        else:
            v[list(vis)] = 1
        o = (r.random(T) < 0.4).astype(np.uint8) if occ is None else np.asarray(occ, np.uint8)
        tr[name] = (walk(r, T) if s is None else s, d, e, v, o, qt)

    # thresholds: 0.5 is both a distance threshold and the survival threshold
    add("thr_at", "all", err=0.5)
    add("thr_below", "all", err=dn(0.5))
    add("thr_above", "all", err=np.where(fr >= 70, up(0.5), 0.0))
    # median
    six = [2, 9, 70, 130, 200, 256]
    add("med_odd", six[:5], err=_at(T, six[:5], [5, 1, 4, 2, 3]))
    add("med_even", six, err=_at(T, six, [6, 1, 5, 2, 4, 3]))
    add("med_dup_same", six, err=_at(T, six, [3, 1, 3, 2, 5, 3]))   # sorted 1 2 3|3 3 5
    add("med_dup_split", six, err=_at(T, six, [4, 2, 4, 2, 2, 4]))  # sorted 2 2 2|4 4 4
    add("one_vis", [40], qt=40, err=3 / 16)
    add("none_vis", (fr < 50).astype(np.uint8), qt=50, err=1 / 16)
    # movement
    add("move_3_200", [3, 200], s=ramp, d=2)
    add("move_63_64", [63, 64], s=ramp, d=3)
    add("move_lane0_only", [128], s=ramp, d=4)
    add("move_lane0s", [5, 128, 192], s=ramp, d=5 if D == 3 else 2)
    # final error and survival
    e5 = (fr % 5) / 16
    add("last_63", [10, 63], err=e5)
    add("last_64", [10, 63, 64], err=e5)
    add("last_end", [10, 64, T - 1], err=e5)
    add("fail_64", "all", err=np.where(fr >= 64, 1.0, 0.0))
    v = np.ones(T, np.uint8)
    v[10] = 0
    add("fail_masked", v, qt=5, err=_at(T, [2, 10, 130], [16, 16, 16]))
    # query frame
    add("qt0", (rng("qt0").random(T) < 0.6).astype(np.uint8), err=e5)
    add("qt_last", "all", qt=T - 1, err=e5)
    add("qt_mid", "all", qt=100, err=np.where(fr < 100, 3.0, e5))
    v = (rng("qt_occ").random(T) < 0.6).astype(np.uint8)
    v[30] = 0
    add("qt_occ", v, qt=30, err=e5)
    # flags: any non-zero byte is true
    r = rng("flags")
    add("flags", r.choice(np.array([0, 1, 2, 255], np.uint8), T), qt=7, err=e5, occ=r.choice(np.array([0, 1, 2, 255], np.uint8), T))
    # non-finite predictions where gt is occluded and before the query
    v = ((fr % 3 != 0) | (fr < 20)).astype(np.uint8)
    e = e5.copy()
    e[[3, 30, 66, 129]] = NAN
    e[[7, 33, 63, 192]] = INF
    e[[36, 255]] = -INF
    o = (fr % 2).astype(np.uint8)  # of the poisoned frames after the query, 30, 36, 66, 192 are not flagged occluded
    add("nonfinite", v, qt=20, err=e, occ=o)
    return tr


def _at(T, frames, sixteenths):
    e = np.zeros(T)
    e[list(frames)] = np.asarray(sixteenths, np.float64) / 16
    return e


@functools.lru_cache(maxsize=None)
def planted_clip(D):
    tr = _plant(D)
    dd = dirs(D)
    names = list(tr)
    T, N = PLANT_T, len(names)
    gt, pred = np.zeros((T, N, D)), np.zeros((T, N, D))
    vis, occ, qt = np.zeros((T, N), np.uint8), np.zeros((T, N), np.uint8), np.zeros(N, np.int64)
    for n, name in enumerate(names):
        s, d, e, v, o, q = tr[name]
        base = np.array([0, 3, -2][:D], np.float64)
        gt[:, n] = base + s[:, None] * dd[d]
        pred[:, n] = gt[:, n] + e
        vis[:, n], occ[:, n], qt[n] = v, o, q
    return make_clip(gt, pred, vis, occ, qt, PLANT_THR, PLANT_SURV), names


def reach_tracks(c):
    """What the tracks of a clip exercise, from the inputs alone."""
    got = set()
    m = masked_vis(c)
    d = np.sqrt(((c["pred"].astype(np.float64) - c["gt"]) ** 2).sum(-1))
    thr = [float(F32(t)) for t in c["thr"]]
    for n in range(m.shape[1]):
        fr = np.where(m[:, n])[0]
        v = np.sort(d[fr, n])
        if len(v) >= 2 and len(v) % 2 == 0 and v[len(v) // 2 - 1] == v[len(v) // 2]:
            got.add("median_on_duplicate")
        if len(v) >= 2 and len(v) % 2 == 0 and v[len(v) // 2 - 1] != v[len(v) // 2]:
            got.add("median_between_distinct")
        if len(v) == 1:
            got.add("one_visible")
        if len(v) == 0:
            got.add("none_visible")
        if len(v) == 1024:
            got.add("full_buffer")
        if len(fr) >= 2 and (np.diff(fr // 64) > 1).any():
            got.add("carry_across_empty_step")
        if len(fr) >= 2 and ((fr[:-1] % 64 == 63) & (np.diff(fr) == 1)).any():
            got.add("pair_across_step_edge")
        if len(fr) and fr[-1] >= 64:
            got.add("last_visible_in_later_step")
        ev = m[c["qt"][n] + 1:, n]
        dv = d[c["qt"][n] + 1:, n][ev]
        if any((dv == t).any() for t in thr):
            got.add("distance_at_threshold")
        if any((dv == dn(t)).any() for t in thr):
            got.add("distance_below_threshold")
        if (v == float(F32(c["surv"]))).any():
            got.add("distance_at_survival")
        if (~np.isfinite(d[:, n])).any():
            got.add("non_finite")
        if (c["vis"][:c["qt"][n], n] != 0).any():
            got.add("visible_before_query")
    return got


# ------------------------------------------------------------------ clips for the tables (section B)

TABLE_THR = dict(distance_thresholds=[0.25, 0.5, 1.0, 2.0, 4.0], survival_distance_threshold=1.0, static_threshold=0.25,
                 dynamic_threshold=1.0, very_dynamic_threshold=4.0)
TABLE_MOVES = [0.25, dn(0.25), up(0.25), 1.0, dn(1.0), up(1.0), 4.0, dn(4.0), up(4.0)]


def first_visible_query(c):
    """The clip with the first flagged frame as the query frame (what the tables do without query points)."""
    return dict(c, qt=(c["vis"] != 0).argmax(0).astype(np.int32))


def table_margin(c, static, dynamic, very):
    """The tables round 100 * (a float32 mean of per-track float32 ratios) to two decimals, and the order of that sum is not part
    of the contract (the reference adds in torch's order, the oracle in numpy's, the device in its own).  A float32 mean of n
    values of one sign is within (n + 1) * 2^-24 of the true mean, relatively, in any order, so two of them round alike when the
    fp64 mean of the restated rows keeps that far from every boundary k/100 + 0.005.  Returns the smallest ratio of an entry's
    distance from a boundary to that bound; the builders ask for 1.  A column of multiples of 2^-8 below 2^8 (every
    distance here) adds up exactly in any order and is decided wherever it lies."""
    rows = track_rows(c).astype(np.float64)
    mv, nv = rows[:, 0], rows[:, 1]
    sub = {"any": np.ones(len(mv), bool)}
    if static is not None:
        sub["static"] = mv.astype(F32) < F32(static)
    if dynamic is not None:
        sub["dynamic"] = mv.astype(F32) > F32(dynamic)
    if very is not None:
        sub["very"] = mv.astype(F32) > F32(very)
    means, tols = {}, {}
    for k, m in sub.items():
        m = m & (nv >= 2)
        if not m.any():
            continue
        mean, tol = [], []
        for col in rows[m, 2:].T:
            col = col[~np.isnan(col)]
            if len(col) == 0 or (np.all((col * 256) % 1 == 0) and np.all(np.abs(col) < 256)):
                mean.append(NAN), tol.append(0.0)
            else:
                mean.append(col.mean() * 100), tol.append((len(col) + 1) * 2.0 ** -24 * col.mean() * 100)
        means[k], tols[k] = np.array(mean), np.array(tol)
    if "static" in means and "dynamic" in means:  # (a column that is exact in either part is taken as decided in their mean)
        means["mix"], tols["mix"] = (means["static"] + means["dynamic"]) / 2, (tols["static"] + tols["dynamic"]) / 2
    mean, tol = np.concatenate(list(means.values())), np.concatenate(list(tols.values()))
    ok = ~np.isnan(mean)
    if not ok.any():
        return INF
    return float((np.abs((mean[ok] * 100) % 1.0 - 0.5) / 100 / tol[ok]).min())


# the first seeds whose clips pass the builder's assertions (table_margin)
TABLE_SEED = dict(edges=2, no_static=1, all_visible=1)


@functools.lru_cache(maxsize=None)
def table_clip(kind="edges", T=12, D=3):
    """(clip, names).  `edges`: one track per entry of TABLE_MOVES (it sits at 0 in frame 0 and at that value on axis 0 from
    frame 1 on, so its path length is that float32), a track with one and one with two visible frames, and tracks on lines.
    `no_static`: the tracks on lines that move by 1/4 or more.  `all_visible`: `edges` with every frame visible and query frame 0."""
    r = rng("table", kind, T, D, TABLE_SEED[kind])
    dd = dirs(D)
    names, gts, viss, qts = [], [], [], []
    if kind != "no_static":
        for i, mv in enumerate(TABLE_MOVES):
            g = np.zeros((T, D))
            g[1:, 0] = mv
            g[:, 1] = i - 4
            v = np.ones(T, np.uint8)
            v[r.integers(2, T, 3)] = 0
            names.append(f"move_{i}")
            gts.append(g), viss.append(v), qts.append(0)
        for name, frames in (("one_visible", [4]), ("two_visible", [4, 9])):
            g = np.array([2.0, 1.0, -1.0][:D]) + np.arange(T)[:, None] * dd[2]
            v = np.zeros(T, np.uint8)
            v[frames] = 1
            names.append(name)
            gts.append(g), viss.append(v), qts.append(frames[0])
    for i in range(8):
        s = walk(r, T) * (i % 3)  # every third track stands still
        if kind == "no_static" and i % 3 == 0:
            continue
        g = r.integers(-8, 9, D).astype(np.float64) + s[:, None] * dd[r.integers(0, len(dd))]
        v = (r.random(T) < 0.8).astype(np.uint8)
        q = int(r.integers(0, T // 2))
        v[q] = 1
        names.append(f"line_{i}")
        gts.append(g), viss.append(v), qts.append(q)
    gt, vis, qt = np.stack(gts, 1), np.stack(viss, 1), np.array(qts)
    N = len(names)
    if kind == "all_visible":
        vis[:], qt[:] = 1, 0
    e = np.zeros((T, N, D))
    e[..., 1] = r.integers(-3, 4, (T, N)) * r.choice([1, 2, 5, 13], (T, N)) / 16  # along axis 1, where every gt is a multiple of 1/16
    occ = (r.random((T, N)) < 0.4).astype(np.uint8)
    c = make_clip(gt, gt + e, vis, occ, qt, TABLE_THR["distance_thresholds"], TABLE_THR["survival_distance_threshold"])
    if kind == "no_static":
        assert track_rows(c)[:, 0].min() >= 0.25
    th = [TABLE_THR[k] for k in ("static_threshold", "dynamic_threshold", "very_dynamic_threshold")]
    assert min(table_margin(c, *th), table_margin(first_visible_query(c), *th)) >= 1, "a table mean sits on a rounding boundary"
    return c, names


SETTING_SEED = {("2dpt_ablation", 2.0): 7, ("2dpt_ablation", 0.5): 13}  # likewise; 0 elsewhere


@functools.lru_cache(maxsize=None)
def setting_clip(setting, factor, T=20, N=14):
    """Tracks on lines for `evaluate_3dpt`: the thresholds of a setting are not dyadic, so every scaled distance keeps 1/16 from
    each distance threshold and from the survival threshold (asserted), and no scaled path length is rounded across a movement
    threshold (asserted: fp32 and fp64 agree on every subset)."""
    from oracle.metrics_oracle import SETTINGS
    th, surv, st, dy, vd, D = SETTINGS[setting]
    r = rng("setting", setting, factor, T, N, SETTING_SEED.get((setting, factor), 0))
    dd = dirs(D)
    ln = np.sqrt((dd * dd).sum(-1))
    far = lambda x: all(abs(x - t) >= 1 / 16 for t in list(th) + [surv])
    cand = [(m, j) for j in range(len(dd)) for m in range(0, 400) if far(m * ln[j] * factor) and m * ln[j] * factor < 4 * surv and m * ln[j] * 16 <= 4000]  # squared length in 1/256 below 2^24
    assert len(cand) >= 4
    w = np.array([1.0 / (1.0 + m * ln[j] * factor / th[0]) for m, j in cand])
    pick = r.choice(len(cand), (T, N), p=w / w.sum())
    e = np.array([[cand[k][0] * dd[cand[k][1]] * r.choice([-1, 1]) for k in row] for row in pick])
    s = walk(r, T, N) * (np.arange(N) % 3 != 0)  # every third track stands still
    gt = r.integers(-8, 9, (N, D)).astype(np.float64)[None] + s[..., None] * dd[r.integers(0, len(dd), N)][None]
    vis = (r.random((T, N)) < 0.8).astype(np.uint8)
    qt = r.integers(0, T // 2, N)
    vis[qt, np.arange(N)] = 1
    occ = (r.random((T, N)) < 0.4).astype(np.uint8)
    c = make_clip(gt, gt + e, vis, occ, qt, th, surv)
    dist = np.sqrt(((c["pred"].astype(np.float64) - c["gt"]) ** 2).sum(-1)) * factor
    assert all(np.abs(dist - t).min() >= 1 / 16 for t in list(th) + [surv])
    sc = make_clip(gt * factor, (gt + e) * factor, vis, occ, qt, th, surv)  # the scaled clip is exact too
    mv = track_rows(sc)[:, 0].astype(np.float64)
    for t in (st, dy, vd):
        if t is not None:
            assert np.array_equal(mv < t, mv.astype(F32) < F32(t)) and np.array_equal(mv > t, mv.astype(F32) > F32(t))
    assert min(table_margin(sc, st, dy, vd), table_margin(first_visible_query(sc), st, dy, vd)) >= 1, "a table mean sits on a rounding boundary"
    return c


# ================================================================== view assignment

VH, VW, VT = 8, 12, 3
ZAXIS = (2, 0, 1)  # the world axis every view's optical axis reads in frame t


def _signed_perm(r, za):
    """A signed permutation matrix whose third row reads world axis za."""
    rest = [a for a in range(3) if a != za]
    if r.integers(2):
        rest.reverse()
    R = np.zeros((3, 3))
    for row, a in enumerate(rest + [za]):
        R[row, a] = r.choice([-1.0, 1.0])
    return R


def make_view_clip(key, V, plant=None, depth=None, deltas=None, queries=None, focal=None):
    """Cameras such that the anchor point (the same in every frame) projects to plant[(v, t)] = (x, y, z) in view v of frame t.
    Queries: per frame, anchor + integer offsets on the two axes that no optical axis reads (`deltas` (n, 2), default the
    11 x 11 grid), or `queries` = [(frame value, d0, d1)]."""
    r = rng("view", key, V)
    T, H, W = VT, VH, VW
    anchor = r.integers(-4, 5, 3).astype(np.float64)
    intrs, extrs = np.zeros((V, T, 3, 3)), np.zeros((V, T, 3, 4))
    for v in range(V):
        for t in range(T):
            R = _signed_perm(r, ZAXIS[t])
            fx, fy = r.choice([1.0, 2.0, 4.0], 2)
            fx, fy = (focal or {}).get((v, t), (fx, fy))
            cx, cy = r.integers(6, 17) / 2, r.integers(4, 11) / 2
            x, y, z = (plant or {}).get((v, t), (r.integers(8, 81) / 8, r.integers(8, 49) / 8, float(r.choice([1.0, 2.0, 4.0, 8.0]))))
            cam = np.array([(x - cx) * z / fx, (y - cy) * z / fy, z])
            intrs[v, t] = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]
            extrs[v, t, :, :3] = R
            extrs[v, t, :, 3] = cam - R @ anchor
    dm = r.integers(0, 16, (V, T, H, W)).astype(np.float64)
    for (v, t), fn in (depth or {}).items():
        dm[v, t] = fn(dm[v, t]) if callable(fn) else fn
    if queries is None:
        g = np.arange(-5, 6)
        deltas = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2) if deltas is None else np.asarray(deltas)
        queries = [(t, a, b) for t in range(T) for a, b in deltas]
    qp = np.zeros((len(queries), 4))
    for i, (tv, a, b) in enumerate(queries):
        free = [ax for ax in range(3) if ax != ZAXIS[int(tv)]]
        qp[i, 0] = float(F32(tv))
        qp[i, 1:] = anchor
        qp[i, 1 + free[0]] += a
        qp[i, 1 + free[1]] += b
    c = dict(V=V, T=T, H=H, W=W, depths=dm.astype(F32), intrs=intrs.astype(F32), extrs=extrs.astype(F32), qp=qp.astype(F32))
    assert is_f32(dm) and is_f32(intrs) and is_f32(extrs) and is_f32(qp)
    assert len({(intrs[v, t].tobytes(), extrs[v, t].tobytes()) for v in range(V) for t in range(T)}) == V * T  # cameras differ everywhere
    assert len({dm[v, t].tobytes() for v in range(V) for t in range(T)}) == V * T or depth is not None
    best_view(c, check=True)
    return c


def best_view(c, fault=None, check=False, order=None):
    """(views (N,) int64, xyz (V, N, 3) fp64, depth (V, N) fp64: the blend, NaN where the view is outside).  `check` asserts that
    every intermediate is a float32, that z is a power of two and x, y multiples of 1/8.  `order`: a permutation of the views."""
    V, T, H, W = c["V"], c["T"], c["H"], c["W"]
    dm, Ks, Es, qp = (c[k].astype(np.float64).tolist() for k in ("depths", "intrs", "extrs", "qp"))
    order = list(range(V)) if order is None else list(order)
    N = len(qp)
    views = np.zeros(N, np.int64)
    xyz = np.zeros((V, N, 3))
    dep = np.full((V, N), NAN)

    def f(x):
        if check:
            assert float(F32(x)) == x, x
        return x

    for n in range(N):
        t = int(qp[n][0])  # .long(): truncation
        assert 0 <= t < T
        p = qp[n][1:]
        best, bv = -INF, 0
        for vi, v in enumerate(order):
            E, K = Es[v][0 if fault == "frame0_cams" else t], Ks[v][0 if fault == "frame0_cams" else t]
            cam = [f(f(f(f(E[i][0] * p[0]) + f(E[i][1] * p[1])) + f(E[i][2] * p[2])) + E[i][3]) for i in range(3)]
            ph = [f(f(f(K[i][0] * cam[0]) + f(K[i][1] * cam[1])) + f(K[i][2] * cam[2])) for i in range(3)]
            z = cam[2]
            assert z != 0
            x, y = f(ph[0] / ph[2]), f(ph[1] / ph[2])
            if check:
                assert math.frexp(abs(z))[0] == 0.5 and x * 8 == int(x * 8) and y * 8 == int(y * 8), (x, y, z)
            xyz[vi, n] = x, y, z
            outside = x < 0 or (x > W if fault == "x_gt_w" else x >= W) or y < 0 or y >= H or (z < 0 and fault != "no_z_test")
            if outside:
                d = -1e4
            else:
                x0, y0 = math.floor(x), math.floor(y)
                cx0, cx1 = min(max(x0, 0), W - 1), min(max(x0 + 1, 0), W - 1)
                cy0, cy1 = min(max(y0, 0), H - 1), min(max(y0 + 1, 0), H - 1)
                ax0, ax1, ay0, ay1 = (cx0, cx1, cy0, cy1) if fault == "clamped_weights" else (x0, x0 + 1, y0, y0 + 1)
                im = dm[v][0 if fault == "frame0_depth" else t]
                w00, w01 = f((ax1 - x) * (ay1 - y)), f((x - ax0) * (ay1 - y))
                w10, w11 = f((ax1 - x) * (y - ay0)), f((x - ax0) * (y - ay0))
                d = f(f(f(f(w00 * im[cy0][cx0]) + f(w01 * im[cy0][cx1])) + f(w10 * im[cy1][cx0])) + f(w11 * im[cy1][cx1]))
                dep[vi, n] = d
            score = f(d - z)
            if score >= best if fault == "last_max" and vi else score > best:
                best, bv = score, vi
        views[n] = bv
    return views, xyz, dep


def scores_of(c):
    """(V, N) fp64 scores of the restatement."""
    _, xyz, dep = best_view(c)
    return np.where(np.isnan(dep), -1e4, dep) - xyz[..., 2]


def permute_views(c, order):
    o = list(order)
    return dict(c, depths=np.ascontiguousarray(c["depths"][o]), intrs=np.ascontiguousarray(c["intrs"][o]),
                extrs=np.ascontiguousarray(c["extrs"][o]))


def take_queries(c, idx):
    return dict(c, qp=np.ascontiguousarray(c["qp"][idx]))


# ------------------------------------------------------------------ the view cases

VIEW_N = (1, 127, 128, 129, 300)


@functools.lru_cache(maxsize=None)
def pool_clip(V):
    """363 queries, three frames, random plants: the pool of the workgroup-edge cases."""
    return make_view_clip("pool", V)


@functools.lru_cache(maxsize=None)
def sized_clip(V, N):
    c = pool_clip(V)
    return take_queries(c, rng("sized", V, N).permutation(len(c["qp"]))[:N])


@functools.lru_cache(maxsize=None)
def frames_clip():
    """The anchor queried at frames 0, 1, 2 and at 0.5, 1.9, 2.0: view t wins frame t.  In frame t the anchor sits on an integer
    pixel of every view, different per frame, at z = 1; the winner's map holds 15 there, every other map at most 7.  At the
    pixel of another frame the maps are planted so that a kernel reading frame 0's cameras or maps picks the third view."""
    pix = {0: (3.0, 2.0), 1: (7.0, 5.0), 2: (10.0, 1.0)}
    plant = {(v, t): pix[t] + (1.0,) for v in range(3) for t in range(3)}

    def dmap(v, t):
        def fn(m):
            m = np.minimum(m, 7.0)
            for tt, (x, y) in pix.items():
                if tt == t:
                    m[int(y), int(x)] = 15.0 if v == t else m[int(y), int(x)]
                else:  # another frame's pixel: that frame's winner holds 0 there, this frame's winner 1, the third view 7
                    m[int(y), int(x)] = 0.0 if v == tt else (1.0 if v == t else 7.0)
            return m
        return fn
    depth = {(v, t): dmap(v, t) for v in range(3) for t in range(3)}
    return make_view_clip("frames", 3, plant, depth, queries=[(t, 0, 0) for t in (0.0, 1.0, 2.0, 0.5, 1.9, 2.0)])


EDGE_X = (0.0, VW - 1.0, VW - 0.5, float(VW), -0.125)
EDGE_Y = (0.0, VH - 1.0, VH - 0.5, float(VH), -0.125)


@functools.lru_cache(maxsize=None)
def edges_clip():
    """View 0 carries the edge: its anchor pixel is (W - 1, 3) in frame 0 and (5, H - 1) in frame 1 with fx / z = fy / z = 1/2,
    so the offsets walk x (frame 0) or y (frame 1) over size - 1, size - 0.5 and size; in frame 2 it starts at (0, 0) with a
    step of 1/8 and reaches -0.125 on either axis.  View 0's maps hold 8..15, the other two views' maps 0..3 at z = 4: view 0
    wins wherever it is inside."""
    plant = {(0, 0): (VW - 1.0, 3.0, 2.0), (0, 1): (5.0, VH - 1.0, 2.0), (0, 2): (0.0, 0.0, 8.0)}
    for v in (1, 2):
        for t in range(3):
            plant[(v, t)] = (5.0 + v, 3.0 + t / 2, 4.0)
    depth = {(v, t): (lambda m: 8.0 + m // 2) if v == 0 else (lambda m: m // 4) for v in range(3) for t in range(3)}
    g = np.arange(-3, 4)
    return make_view_clip("edges", 3, plant, depth, deltas=np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2),
                          focal={(0, t): (1.0, 1.0) for t in range(3)})


@functools.lru_cache(maxsize=None)
def depth_z_clip():
    """Camera z: view 0 at z = 1/8 (small and positive: inside, and it wins), view 1 at z = -2 with x, y in the box (outside: were it
    inside, its map of 15s would win), view 2 ordinary.  Frame 1: views 0 and 1 exchange roles."""
    plant, depth = {}, {}
    for t in range(3):
        a, b = (0, 1) if t != 1 else (1, 0)
        plant[(a, t)], plant[(b, t)], plant[(2, t)] = (4.0, 3.0, 0.125), (6.0, 4.0, -2.0), (5.0, 2.0, 4.0)
        depth[(a, t)], depth[(b, t)], depth[(2, t)] = (lambda m: 6.0 + m // 8), (lambda m: 15.0 + 0 * m), (lambda m: m // 4)
    return make_view_clip("z", 3, plant, depth, deltas=[(0, 0)])


@functools.lru_cache(maxsize=None)
def ties_clip():
    """Constant maps and planted z with map - z equal: 4 - 2, 3 - 1 and 6 - 4 in frame 0 (a three-way tie wherever all three views
    are inside, two-way where one has left the image), in frame 1 views 1 and 2 tie above view 0, in frame 2 every view is
    outside (z = -4 with the pixel in the box, and z = 2, 2 with the pixel far off the image): the score is -1e4 - z, views 1 and 2
    tie and view 0 wins with its negative z."""
    plant = {(0, 0): (5.0, 4.0, 2.0), (1, 0): (6.0, 3.0, 1.0), (2, 0): (4.0, 4.0, 4.0),
             (0, 1): (5.0, 4.0, 4.0), (1, 1): (6.0, 3.0, 1.0), (2, 1): (4.0, 4.0, 4.0),
             (0, 2): (5.0, 4.0, -4.0), (1, 2): (-40.0, 3.0, 2.0), (2, 2): (4.0, 90.0, 2.0)}
    const = {0: 4.0, 1: 3.0, 2: 6.0}
    depth = {(v, t): (lambda m, v=v: const[v] + 0 * m) for v in range(3) for t in range(3)}
    return make_view_clip("ties", 3, plant, depth)


@functools.lru_cache(maxsize=None)
def outside_tie_clip():
    """Every view outside, two of them at the same z: -1e4 - z ties and the lowest view wins.  V = 6: views 1 and 4 share the
    smallest z (1/2) in frame 0, views 2, 3 and 5 share z = -1 in frame 1, frame 2 has distinct z."""
    zs = {0: [2.0, 0.5, 1.0, 4.0, 0.5, 8.0], 1: [1.0, 2.0, -1.0, -1.0, 0.5, -1.0], 2: [4.0, 2.0, 8.0, 1.0, -2.0, 0.25]}
    plant = {(v, t): (-50.0 - v, 3.0, zs[t][v]) if v % 2 else (4.0, 60.0 + v, zs[t][v]) for v in range(6) for t in range(3)}
    g = np.arange(-1, 2)
    return make_view_clip("outside", 6, plant, deltas=np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2))


@functools.lru_cache(maxsize=None)
def half_clip():
    """View 0 at (4.5, 2.5): the four corners 1, 2, 5, 10 blend to 4.5, minus z = 1/2 is 4; view 1 holds 4 everywhere at z = 1/8,
    a score of 3.875, 1/8 lower; view 2 holds 5 at z = 1, a score of 4 -- a tie that view 0 wins only with the exact mean."""
    plant = {(v, t): [(4.5, 2.5, 0.5), (6.0, 3.0, 0.125), (3.0, 3.0, 1.0)][v] for v in range(3) for t in range(3)}

    def corners(m):
        m = m.copy()
        m[2, 4], m[2, 5], m[3, 4], m[3, 5] = 1.0, 2.0, 5.0, 10.0
        return m
    depth = {(v, t): [corners, (lambda m: 4.0 + 0 * m), (lambda m: 5.0 + 0 * m)][v] for v in range(3) for t in range(3)}
    return make_view_clip("half", 3, plant, depth, deltas=[(0, 0)])


def view_cases():
    """name -> clip: every input of section C."""
    cases = {f"sized_V{V}_N{N}": sized_clip(V, N) for V in (1, 3, 6) for N in VIEW_N}
    cases.update(frames=frames_clip(), edges=edges_clip(), z=depth_z_clip(), ties=ties_clip(), outside=outside_tie_clip(), half=half_clip())
    cases["ties_permuted"] = permute_views(ties_clip(), (2, 0, 1))
    return cases


def reach_views(c):
    """What the queries of a clip exercise, from the restatement's projections and scores."""
    got = set()
    _, xyz, dep = best_view(c)
    sc = np.where(np.isnan(dep), -1e4, dep) - xyz[..., 2]
    x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    okx, oky = (x >= 0) & (x < c["W"]), (y >= 0) & (y < c["H"])
    for name, val in zip(("0", "W-1", "W-0.5", "W", "-0.125"), EDGE_X):
        if ((x == val) & oky & (z > 0)).any():
            got.add("x=" + name)
    for name, val in zip(("0", "H-1", "H-0.5", "H", "-0.125"), EDGE_Y):
        if ((y == val) & okx & (z > 0)).any():
            got.add("y=" + name)
    if ((z < 0) & okx & oky).any():
        got.add("behind_in_box")
    if ((z > 0) & (z <= 0.125) & okx & oky).any():
        got.add("small_z_inside")
    top = (sc == sc.max(0, keepdims=True)).sum(0)
    allout = np.isnan(dep).all(0)
    for k, name in ((2, "two_way_tie"), (3, "three_way_tie")):
        if ((top == k) & ~allout).any():
            got.add(name)
        if ((top == k) & allout).any():
            got.add(name + "_outside")
    if allout.any():
        got.add("all_outside")
    if (allout & (z.min(0) < 0) & (sc.argmax(0) == z.argmin(0))).any():
        got.add("all_outside_negative_z_wins")
    if (qp_frac(c) != 0).any():
        got.add("fractional_frame")
    return got


def qp_frac(c):
    return c["qp"][:, 0] - np.floor(c["qp"][:, 0])
