"""Scene normalisation on the device: mvt_select_kth against np.sort (bit for bit), mvt_scene_stats / mvt_scene_apply /
mvt_scene_tracks against the fp64 restatement (tests/scene_norm_ref.py) inside 4 x d_ref, the restatement's own recorded distance
from the reference (tests/golden/scene_norm.npz), and the predictor / streaming wiring end to end.

The bar: d_ref is how far the reference's fp32 result lies from exact arithmetic on the same inputs; the device departs from exact
arithmetic in the same places (fp32 inputs, fp32 unprojection) plus one final rounding, so its own distance from the restatement
may be 4 x d_ref and no more.  Integers (kept count, ranks) must be equal.  Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_norm_ref as R  # noqa: E402
from mvtracker_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
V, T, H, W = 3, 2, 37, 53
CASES = [(c, r) for c in (1, 2, 3) for r in ("cam", "rad")]
BAR = 4.0


@pytest.fixture(scope="module")
def hip():
    from mvtracker_amd import hip as h
    return h


@pytest.fixture(scope="module")
def fx(golden):
    g = golden("scene_norm")
    clip = synth.make_clip(int(g["clip_seed"][0]), V=V, T=T, H=H, W=W, N=4, invalid_frac=0.02)
    return g, clip


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ select
NS = [1, 2, 63, 64, 65, 256, 257, 4099, 70001]


def _finite_bits(rng, n):
    b = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    return np.where((b & 0x7F800000) == 0x7F800000, b & 0xBFFFFFFF, b)  # no inf / NaN exponent


def dataset(name, n):
    rng = np.random.default_rng(1000 + n)
    if name == "normals":
        return rng.standard_normal(n).astype(np.float32)
    if name == "all_equal":
        return np.full(n, 1.25, np.float32)
    if name == "two_values":
        return rng.choice(np.array([-3.5, 7.0], np.float32), size=n)
    if name == "zeros":  # mixed signs and both zeros
        x = rng.standard_normal(n).astype(np.float32)
        x[::5], x[2::5] = 0.0, -0.0
        return x
    if name == "low_bits":  # bit patterns over the whole range, half of them copies that differ in the lowest three mantissa bits:
        b = _finite_bits(rng, n)  # all four radix passes have something to decide, the last one between neighbours
        h = n // 2
        b[h:2 * h] = b[:h] ^ rng.integers(1, 8, size=h).astype(np.uint32)
        return b.view(np.float32)
    if name == "denormals":
        b = rng.integers(0, 1 << 23, size=n).astype(np.uint32) | (rng.integers(0, 2, size=n).astype(np.uint32) << 31)
        return b.view(np.float32)
    if name == "infinities":
        x = rng.standard_normal(n).astype(np.float32)
        x[::7], x[3::7] = np.inf, -np.inf
        return x
    raise KeyError(name)


def ranks(n):
    return sorted({k for k in (0, n // 8, n - 2, n - 1) if 0 <= k < n})


@pytest.mark.parametrize("name", ["normals", "all_equal", "two_values", "zeros", "low_bits", "denormals", "infinities"])
def test_select_equals_numpy_sort(hip, name):
    ws = torch.empty(hip.SELECT_WS_WORDS, device=DEV, dtype=torch.int32)
    for n in NS:
        x = dataset(name, n)
        assert not np.isnan(x).any()
        xd, ks = dev(x), ranks(n)
        out = torch.zeros(len(ks), device=DEV)
        for j, k in enumerate(ks):
            hip.select_kth(xd, n, k, out[j:j + 1], ws)
        want = np.sort(x)[ks]
        got = out.cpu().numpy()
        assert np.array_equal(bits(got), bits(want)), (name, n, ks, got, want)


def test_select_order_rule_and_argument_errors(hip):
    ws = torch.empty(hip.SELECT_WS_WORDS, device=DEV, dtype=torch.int32)
    x = dev(np.array([0.0, -0.0, 1.0, -1.0], np.float32))
    out = torch.zeros(4, device=DEV)
    for k in range(4):
        hip.select_kth(x, 4, k, out[k:k + 1], ws)
    assert np.array_equal(bits(out.cpu().numpy()), bits(np.array([-1.0, -0.0, 0.0, 1.0], np.float32)))  # the header's rule: -0.0 < +0.0
    out.fill_(-7.0)
    for n, k in ((4, -1), (4, 4), (0, 0)):
        with pytest.raises(hip.HipError, match="arguments rejected"):
            hip.select_kth(x, n, k, out, ws)
    assert bool((out == -7.0).all())  # refused before any launch


# ------------------------------------------------------------------------------------------------------------------ stats
def conf_of(g, case):
    return {1: g["conf"], 2: g["conf_case2"], 3: None, 4: g["conf_case4"]}[case]


def inputs(g, clip, case):
    conf = conf_of(g, case)
    return [dev(clip[k]) for k in ("depths", "intrs", "extrs")], None if conf is None else dev(conf)[None]


def check(name, value, bar):
    print(f"  {name:24s} {value:.3e}   bar {bar:.3e}   ratio to d_ref {BAR * value / bar:.2f}")
    return value <= bar


@pytest.mark.parametrize("case,rule", CASES)
def test_stats_on_the_fixture(fx, case, rule):
    from mvtracker_amd import scene
    g, clip = fx
    k = f"c{case}_{rule}_"
    (d, i, e), conf = inputs(g, clip, case)
    thr, radius = float(g["conf_thresh"][0]), float(g["target_radius"][0])
    m = R.auto_scene_normalization(clip["depths"][0], clip["intrs"][0], clip["extrs"][0], conf_of(g, case), thr, radius, rule == "cam")
    state, _ = scene.scene_statistics(d, i, e, conf, thr, 0, None if rule == "cam" else scene.RADIUS_QUANTILE)
    st = scene.read_statistics(state)
    t = scene.auto_scene_normalization(d, i, e, depths_conf=conf, conf_thresh=thr, target_radius=radius, rescale_by_camera_radius=rule == "cam")
    state2, _ = scene.scene_statistics(d, i, e, conf, thr, 0, None if rule == "cam" else scene.RADIUS_QUANTILE)
    assert torch.equal(state, state2)  # two runs: the same bits
    assert st["M"] == int(g[k + "M"][0]) and st["z_rank"] == int(g[k + "z_rank"][0]) and st["nonfinite"] == 0
    ext = float(g[k + "extent"][0])
    dref = lambda q: BAR * float(g[k + "dref_" + q][0])
    print(f"\ncase {case} / {rule}: M {st['M']}, z rank {st['z_rank']}")
    ok = [check("scale", abs(t.scale - m["scale"]) / m["scale"], dref("scale")),
          check("centroid", R.rel_inf(st["centroid"], m["centroid"], ext), dref("centroid")),
          check("floor_z", R.rel_inf(st["floor_z"], m["floor_z"], ext), dref("floor_z")),
          check("translate", R.rel_inf(t.translation, m["translate"], ext), dref("translate")),
          check("zc_order", R.rel_inf(np.array([st["z_lo"], st["z_hi"]]) - st["centroid"][2],
                                      np.array([m["z_lo"], m["z_hi"]]) - m["centroid"][2], ext), dref("zc_order"))]
    if rule == "rad":
        assert st["r_rank"] == int(g[k + "r_rank"][0])
        ok.append(check("r_order", R.rel_inf(np.array([st["r_lo"], st["r_hi"]]), np.array([m["r_lo"], m["r_hi"]]), ext), dref("r_order")))
    assert all(ok)


def test_stats_skip_a_thin_view_and_refuse_an_empty_pool(fx):
    from mvtracker_amd import scene
    g, clip = fx
    (d, i, e), c1 = inputs(g, clip, 1)
    _, c2 = inputs(g, clip, 2)
    _, c4 = inputs(g, clip, 4)
    a, b = scene.auto_scene_normalization(d, i, e, depths_conf=c1), scene.auto_scene_normalization(d, i, e, depths_conf=c2)
    s1 = scene.read_statistics(scene.scene_statistics(d, i, e, c1)[0])
    s2 = scene.read_statistics(scene.scene_statistics(d, i, e, c2)[0])
    assert s1["M"] - s2["M"] > 1000 and a != b and abs(a.scale - b.scale) > 1e-4  # view 1 (99 valid pixels) is out, whole
    with pytest.raises(RuntimeError, match="Too few valid points for normalization."):
        scene.auto_scene_normalization(d, i, e, depths_conf=c4)
    bad = d.clone()
    bad[0, 0, 0, 0, 5, 5] = float("inf")
    with pytest.raises(ValueError, match="not finite"):
        scene.auto_scene_normalization(bad, i, e)


@pytest.mark.parametrize("shape", [(2, 32, 64), (2, 33, 61)])  # V*H*W = 4096 = 16 workgroups exactly; 4026: a ragged last one
def test_stats_pixel_counts_around_the_workgroup(shape):
    """No fixture here: every unprojected point lies within 2e-5 of its exact position (the unprojection bound of
    tests/test_gpu_ops.py), a mean and an order statistic move by no more than their inputs, so both are held to 2e-5."""
    from mvtracker_amd import scene
    v, h, w = shape
    clip = synth.make_clip(11, V=v, T=2, H=h, W=w, N=4, invalid_frac=0.05)
    d, i, e = (dev(clip[k]) for k in ("depths", "intrs", "extrs"))
    state, _ = scene.scene_statistics(d, i, e, None, 4.8, 1, scene.RADIUS_QUANTILE)
    st = scene.read_statistics(state)
    m = R.auto_scene_normalization(clip["depths"][0], clip["intrs"][0], clip["extrs"][0], None, 4.8, 6.3, False, frame=1)
    assert st["M"] == m["M"] == int((clip["depths"][0][:, 1] > 0).sum()) and st["z_rank"] == m["z_rank"] and st["r_rank"] == m["r_rank"]
    for name in ("centroid", "floor_z", "z_lo", "z_hi", "r_lo", "r_hi"):
        assert np.abs(np.asarray(st[name]) - np.asarray(m[name])).max() < 2e-5, name
    assert torch.equal(state, scene.scene_statistics(d, i, e, None, 4.8, 1, scene.RADIUS_QUANTILE)[0])


# ------------------------------------------------------------------------------------------------------------------ apply / tracks
def transform_of(g, name):
    from mvtracker_amd import SceneTransform
    k = f"xf_{name}_"
    return SceneTransform(float(g[k + "scale"][0]), g[k + "rotation"], g[k + "translation"])


@pytest.mark.parametrize("name", ["auto", "manual", "identity"])
def test_apply_and_tracks_on_the_fixture(fx, name):
    g, clip = fx
    t, k = transform_of(g, name), f"xf_{name}_"
    src = dict(depths=dev(clip["depths"]), extrs=dev(clip["extrs"]), queries=dev(g["queries"])[None], tracks=dev(g["tracks"])[None])
    out = t.apply(depths=src["depths"], extrs=src["extrs"], query_points=src["queries"], tracks=src["tracks"])
    want = R.transform_scene(t.scale, t.rotation, t.translation, clip["depths"][0], clip["extrs"][0], g["queries"], g["tracks"])
    print(f"\ntransform {name}")
    ok = []
    for part, o, w_ in zip(("depths", "extrs", "queries", "tracks"), out, want):
        assert o.shape == src[part].shape and o.dtype == torch.float32
        ok.append(check(part, R.rel_inf(o[0].cpu().numpy(), w_), BAR * float(g[k + "dref_" + part][0])))
        if name == "identity":  # bit for bit
            assert torch.equal(o.view(torch.int32), src[part].view(torch.int32)), part
    back = t.inverse().apply(tracks=out[3])[3]
    ok.append(check("tracks, there and back", R.rel_inf(back[0].cpu().numpy(), g["tracks"]), BAR * float(g[k + "dref_tracks"][0])))
    assert torch.equal(back, t.restore_tracks(out[3]))
    assert all(ok)


def test_apply_vector_and_tail_paths(fx):
    """depths counts that are no multiple of four, and a view that starts off a 16-byte boundary (the scalar path)."""
    g, _ = fx
    t = transform_of(g, "manual")
    x = torch.randn(4099 + 1, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))
    for n, off in ((4099, 0), (4099, 1), (3, 0), (4096, 0)):
        v = x[off:off + n]
        got = t.apply(depths=v)[0]
        assert torch.equal(got, (v.double() * t.scale).float())  # fp64 product, rounded once


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def predictor():
    from mvtracker_amd import EvaluationPredictor
    from mvtracker_amd.tracker import MVTracker
    m = MVTracker(hidden_size=256).eval()
    sd = synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return EvaluationPredictor(m.to(DEV), interp_shape=None, grid_size=2, n_iters=2)


@pytest.fixture(scope="module")
def e2e_clip():
    c = synth.make_clip(5, V=2, T=8, H=128, W=128, N=12, late_queries=True, query_frames=(2,))
    return {k: dev(v) for k, v in c.items()}


def _fwd(pred, c, **kw):
    d, e, q = kw.pop("depths", c["depths"]), kw.pop("extrs", c["extrs"]), kw.pop("queries", c["query_points"])
    return pred(rgbs=c["rgbs"], depths=d, query_points_3d=q, intrs=c["intrs"], extrs=e, **kw)


def test_forward_with_a_transform_is_apply_forward_restore(fx, predictor, e2e_clip):
    g, _ = fx
    t, c = transform_of(g, "manual"), e2e_clip
    out = _fwd(predictor, c, scene_transform=t)
    assert predictor.last_scene_transform is t
    d, e, q, _ = t.apply(depths=c["depths"], extrs=c["extrs"], query_points=c["query_points"])
    by_hand = _fwd(predictor, c, depths=d, extrs=e, queries=q)
    assert predictor.last_scene_transform is None
    assert torch.equal(out["traj_e"], t.restore_tracks(by_hand["traj_e"])) and torch.equal(out["vis_e_as_prob"], by_hand["vis_e_as_prob"])
    assert bool(torch.isfinite(out["traj_e"]).all()) and not torch.equal(out["traj_e"], by_hand["traj_e"])
    # the streaming session: the same chunks
    st = predictor.open_stream(c["query_points"], scene_transform=t)
    outs = [st.push(*(c[k][:, :, a:a + 3] for k in ("rgbs", "depths", "intrs", "extrs"))) for a in range(0, 8, 3)]
    outs.append(st.finish())
    assert torch.equal(torch.cat([o["traj_e"] for o in outs], 1), out["traj_e"])
    assert torch.equal(torch.cat([o["vis_e_as_prob"] for o in outs], 1), out["vis_e_as_prob"])


def test_identity_transform_is_the_plain_call_and_auto_is_the_function(predictor, e2e_clip):
    from mvtracker_amd import SceneTransform, auto_scene_normalization
    c = e2e_clip
    plain = _fwd(predictor, c)
    same = _fwd(predictor, c, scene_transform=SceneTransform(1.0, np.eye(3), (0.0, 0.0, 0.0)))
    assert torch.equal(plain["traj_e"], same["traj_e"]) and torch.equal(plain["vis_e_as_prob"], same["vis_e_as_prob"])
    auto = _fwd(predictor, c, scene_transform="auto")
    want = auto_scene_normalization(c["depths"], c["intrs"], c["extrs"])
    assert predictor.last_scene_transform == want and want.scale != 1.0
    assert torch.equal(auto["traj_e"], _fwd(predictor, c, scene_transform=want)["traj_e"])
    with pytest.raises(ValueError, match="auto_scene_normalization"):
        predictor.open_stream(c["query_points"], scene_transform="auto")
