"""Streaming sessions on the GPU (`-m gpu`): every ring entry against its linear entry on the same frames (bit for bit), a session
against ``forward`` of the same build (bit for bit, in the three precisions) and against the reference's fixtures (the tolerances
of tests/test_gpu_e2e.py), one full-size case, the predictor."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mvtracker_amd import hip, synth  # noqa: E402

DEV = "cuda:0"
S = 12


def T(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def model():
    from mvtracker_amd.tracker import MVTracker
    m = MVTracker(hidden_size=256).eval()
    sd = synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to(DEV)


class precision:
    def __init__(self, model, p):
        self.m, self.p = model, p

    def __enter__(self):
        self.old, self.m.precision = self.m.precision, self.p

    def __exit__(self, *a):
        self.m.precision = self.old


def clip_from_golden(g):
    kw = dict(seed=int(g["seed"]), V=int(g["V"]), T=int(g["T"]), H=int(g["H"]), W=int(g["W"]), N=int(g["N"]))
    if "late_queries" in g.files:
        kw.update(late_queries=bool(g["late_queries"]), query_frames=tuple(int(x) for x in g["query_frames"]))
    return synth.make_clip(**kw)


def dev_clip(c):
    return {k: T(c[k]).to(DEV) for k in ("rgbs", "depths", "query_points", "intrs", "extrs")}


# ------------------------------------------------------------------ ring entries against linear entries
@pytest.fixture(scope="module")
def linear_store(model):
    """A frame store of 30 frames (2 views of 256 x 256: 128 scan tiles at level 0, so the group boxes exist) and query points."""
    c = dev_clip(synth.make_clip(71, V=2, T=30, H=256, W=256, N=40))
    st = model.build_frame_store(c["rgbs"][0], c["depths"][0], c["intrs"][0], c["extrs"][0])
    assert st["gbox"][0] is not None
    torch.cuda.synchronize()
    return st, c["query_points"][0, :, 1:].contiguous()


# (clip frame of linear frame 0, base, R, lo, hi, frame0): the ring holds clip frames [lo, hi]
RINGS = {
    "no_wrap": (0, 0, 18, 0, 11, 0),
    "wraps": (100, 95, 18, 107, 118, 107),          # slots 12 .. 17, 0 .. 5
    "wraps_many_turns": (1000, 7, 24, 1009, 1020, 1010),
    "clamped_tail": (100, 95, 18, 107, 113, 107),   # slots past frame hi repeat it
    "clamped_tail_wraps": (100, 95, 18, 109, 114, 110),
}


def ring_of(st, case, bf16):
    """Ring tensors holding the resident frames of ``case`` (every other slot poisoned), the linear store of exactly those frames,
    and the two frame arguments."""
    F0, base, R, lo, hi, frame0 = RINGS[case]
    fr = torch.arange(lo, hi + 1, device=DEV)
    slots, lin = (fr - base) % R, slice(lo - F0, hi + 1 - F0)

    def ring(t, poison):
        r = torch.full((R, *t.shape[1:]), poison, device=DEV, dtype=t.dtype)
        r[slots] = t[lin]
        return r

    fdt = torch.bfloat16 if bf16 else torch.float32
    rs = dict(xyz=[ring(t, 3.0e4) for t in st["xyz"]], fvec=[ring(t.to(fdt), float("nan")) for t in st["fvec"]],
              box=[ring(t, 0.0) for t in st["box"]], gbox=[None if t is None else ring(t, 0.0) for t in st["gbox"]])
    ls = dict(xyz=[t[lin].contiguous() for t in st["xyz"]], fvec=[t[lin].to(fdt).contiguous() for t in st["fvec"]],
              box=[t[lin].contiguous() for t in st["box"]], gbox=[None if t is None else t[lin].contiguous() for t in st["gbox"]])
    return rs, ls, (base, R, lo, hi), frame0, (frame0 - lo, hi - lo + 1)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("case", sorted(RINGS))
def test_ring_entries_equal_linear_entries(model, linear_store, case, bf16):
    st, q = linear_store
    rs, ls, ring, f0r, (f0l, Tl) = ring_of(st, case, bf16)
    P, grid, L = st["P"], st["tile_grid"], len(st["P"])
    n, K, C = q.shape[0], 16, model.latent_dim
    g = torch.Generator(device="cpu").manual_seed(3)
    coords = (q[:, None, :] + 0.05 * torch.randn(n, S, 3, generator=g).to(DEV)).contiguous()

    # kNN scan (two segments) + merge, level 0
    keys = [torch.zeros(n * S * 2 * K, device=DEV, dtype=torch.int64) for _ in range(2)]
    hip.knn_scan(ls["xyz"][0], P[0], coords, n, S, f0l, 1, Tl, K, 2, keys[0], box=ls["box"][0], grid=grid[0])
    hip.knn_scan_ring(rs["xyz"][0], P[0], coords, n, S, f0r, 1, ring, K, 2, keys[1], box=rs["box"][0], grid=grid[0])
    assert torch.equal(keys[0], keys[1])

    # kNN search (single launch), level 0, unseeded and seeded by its own result
    idx = [torch.zeros(n, S, K, device=DEV, dtype=torch.int32) for _ in range(4)]
    hip.knn_search(ls["xyz"][0], P[0], coords, n, S, f0l, 1, Tl, K, idx[0], ls["box"][0], grid=grid[0], gbox=ls["gbox"][0])
    hip.knn_search_ring(rs["xyz"][0], P[0], coords, n, S, f0r, 1, ring, K, idx[1], rs["box"][0], grid=grid[0], gbox=rs["gbox"][0])
    assert torch.equal(idx[0], idx[1])
    hip.knn_search(ls["xyz"][0], P[0], coords, n, S, f0l, 1, Tl, K, idx[2], ls["box"][0], grid=grid[0], gbox=ls["gbox"][0], seed_idx=idx[0],
                   seed_k=K)
    hip.knn_search_ring(rs["xyz"][0], P[0], coords, n, S, f0r, 1, ring, K, idx[3], rs["box"][0], grid=grid[0], gbox=rs["gbox"][0],
                        seed_idx=idx[0], seed_k=K)
    assert torch.equal(idx[2], idx[3]) and torch.equal(idx[2], idx[0])

    # the *_levels pair: scan + merge of all levels, and the one-launch search
    def levels(s_, idx_, keys_=None, seed=None):
        return [dict(xyz=s_["xyz"][l], P=P[l], keys=None if keys_ is None else keys_[l], nseg=1, seed_idx=None if seed is None else seed[l],
                     box=s_["box"][l], grid=grid[l], idx_out=idx_[l], gbox=s_["gbox"][l]) for l in range(L)]

    il, ir = (torch.zeros(L, n, S, K, device=DEV, dtype=torch.int32) for _ in range(2))
    kl, kr = (torch.zeros(L, n * S * K, device=DEV, dtype=torch.int64) for _ in range(2))
    hip.knn_scan_levels(levels(ls, il, kl), coords, n, S, f0l, 1, Tl, K)
    hip.knn_scan_levels_ring(levels(rs, ir, kr), coords, n, S, f0r, 1, ring, K)
    assert torch.equal(kl, kr)
    hip.knn_merge_levels(levels(ls, il, kl), n, S, K)
    sl, sr = (torch.zeros(L, n, S, K, device=DEV, dtype=torch.int32) for _ in range(2))
    hip.knn_search_levels(levels(ls, sl), coords, n, S, f0l, 1, Tl, K, seed_k=0)
    hip.knn_search_levels_ring(levels(rs, sr), coords, n, S, f0r, 1, ring, K, seed_k=0)
    assert torch.equal(sl, sr) and torch.equal(sl, il)
    hip.knn_search_levels(levels(ls, sl, seed=il), coords, n, S, f0l, 1, Tl, K, seed_k=K)
    hip.knn_search_levels_ring(levels(rs, sr, seed=il), coords, n, S, f0r, 1, ring, K, seed_k=K)
    assert torch.equal(sl, sr) and torch.equal(sl, il)

    # correlation gather, default layout and with options
    tg = torch.randn(n, S, C, generator=g).to(DEV)
    idx_l = [il[l] for l in range(L)]
    Fc = L * K * 4
    ol, orr = torch.zeros(n, S, Fc, device=DEV), torch.zeros(n, S, Fc, device=DEV)
    hip.corr_gather_dot(ls["xyz"], ls["fvec"], P, idx_l, C, tg, coords, n, S, f0l, 1, Tl, K, ol, Fc, 0)
    hip.corr_gather_dot_ring(rs["xyz"], rs["fvec"], P, idx_l, C, tg, coords, n, S, f0r, 1, ring, K, orr, Fc, 0)
    assert torch.equal(ol, orr) and bool(torch.isfinite(ol).all())
    Fo = L * K * (2 + 3 + 3)
    ol, orr = torch.zeros(n, S, Fo, device=DEV), torch.zeros(n, S, Fo, device=DEV)
    hip.corr_gather_dot_opts(ls["xyz"], ls["fvec"], P, idx_l, C, tg, coords, n, S, f0l, 1, Tl, K, 2, True, True, ol, Fo, 0)
    hip.corr_gather_dot_opts_ring(rs["xyz"], rs["fvec"], P, idx_l, C, tg, coords, n, S, f0r, 1, ring, K, 2, True, True, orr, Fo, 0)
    assert torch.equal(ol, orr) and bool(torch.isfinite(ol).all())

    # 1-NN feature init: scan with K = 1 and gather, at the first and the last resident frame
    for fr in (ring[2], ring[3]):
        k1l, k1r = (torch.zeros(n, device=DEV, dtype=torch.int64) for _ in range(2))
        hip.knn_scan(ls["xyz"][0], P[0], q, n, 1, fr - ring[2], 0, Tl, 1, 1, k1l, box=ls["box"][0], grid=grid[0])
        hip.knn_scan_ring(rs["xyz"][0], P[0], q, n, 1, fr, 0, ring, 1, 1, k1r, box=rs["box"][0], grid=grid[0])
        assert torch.equal(k1l, k1r)
        fl, frr = torch.zeros(n, C, device=DEV), torch.zeros(n, C, device=DEV)
        i1l, i1r = (torch.zeros(n, device=DEV, dtype=torch.int32) for _ in range(2))
        hip.knn1_gather(ls["fvec"][0], P[0], C, k1l, n, 1, fr - ring[2], fl, i1l)
        hip.knn1_gather_ring(rs["fvec"][0], P[0], C, k1r, n, 1, fr, ring, frr, i1r)
        assert torch.equal(fl, frr) and torch.equal(i1l, i1r) and bool(torch.isfinite(fl).all())
    torch.cuda.synchronize()


def test_ring_entries_refuse_frames_that_are_not_resident(model, linear_store):
    st, q = linear_store
    rs, _, ring, f0r, _ = ring_of(st, "wraps", False)
    n = q.shape[0]
    keys = torch.zeros(n, device=DEV, dtype=torch.int64)
    feat = torch.zeros(n, model.latent_dim, device=DEV)
    base, R, lo, hi = ring
    for bad in ((base, R, lo, lo + R), (base, R, base - 1, hi), (base, 0, lo, hi)):  # more frames than slots, before the base, no slots
        with pytest.raises(hip.HipError, match="arguments rejected"):
            hip.knn_scan_ring(rs["xyz"][0], st["P"][0], q, n, 1, f0r, 0, bad, 1, 1, keys)
    for frame in (lo - 1, hi + 1):
        with pytest.raises(hip.HipError, match="arguments rejected"):
            hip.knn1_gather_ring(rs["fvec"][0], st["P"][0], model.latent_dim, keys, n, 1, frame, ring, feat)


# ------------------------------------------------------------------ sessions
def stream(model, clip, block, query_sets, iters=4, ring_blocks=3, watch=None):
    """A session over ``clip`` in blocks of ``block`` frames.  ``query_sets`` = [(frames received when added, rows (1,n,4)), ...],
    the first opens the session.  Returns the whole-clip result assembled from the chunks (zero-padded to the final query count)."""
    st = model.open_stream(query_sets[0][1], iters=iters, ring_blocks=ring_blocks)
    pending = list(query_sets[1:])
    Tn = clip["rgbs"].shape[2]
    outs, t = [], 0
    while t < Tn:
        while pending and pending[0][0] <= t:
            st.add_queries(pending.pop(0)[1])
        b = min(block, Tn - t)
        if pending:
            b = min(b, pending[0][0] - t)
        outs.append(st.push(*(clip[k][:, :, t:t + b] for k in ("rgbs", "depths", "intrs", "extrs"))))
        if watch is not None:
            watch(st)
        t += b
    for _, rows in pending:  # (queries at or beyond the clip's end)
        st.add_queries(rows)
    fin = st.finish()
    outs.append(fin)
    N = fin["traj_e"].shape[2]
    res, a = {}, 0
    for o in outs:
        assert o["frames"][0] == a and o["traj_e"].shape[1] == o["frames"][1] - a
        a = o["frames"][1]
    assert a == Tn
    for k in ("traj_e", "vis_e", "vis_logits"):
        res[k] = torch.cat([torch.cat([o[k], torch.zeros(*o[k].shape[:2], N - o[k].shape[2], *o[k].shape[3:], device=DEV)], 2) for o in outs], 1)
    res["feat_init"] = fin["feat_init"]
    return res, st


def mid_stream_sets(q):
    """Half of the rows up front, the others added as late as the rules allow: a row of frame t > 0 right before frame t is pushed,
    a row of frame 0 after three frames (no window has run by then) when the up-front half keeps the first window at frame 0.
    Returns (query sets for ``stream``, all rows in order of addition)."""
    qt = q[0, :, 0].long().cpu().numpy()
    a_rows = np.arange(0, len(qt), 2)
    b_rows = np.arange(1, len(qt), 2)
    zero_at = 3 if (qt[a_rows] == 0).any() else 0
    when = np.where(qt[b_rows] > 0, qt[b_rows], zero_at)
    sets = [(0, q[:, a_rows])]
    for r in sorted(set(when.tolist())):
        sets.append((int(r), q[:, b_rows[when == r]]))
    return sets, torch.cat([s[1] for s in sets], 1)


def check_equal(model, clip, q_all, res, iters=4):
    r = model(clip["rgbs"], clip["depths"], q_all, clip["intrs"], clip["extrs"], iters=iters)
    for k in ("traj_e", "vis_e", "feat_init"):
        assert torch.equal(res[k], r[k]), k
    assert torch.equal(res["vis_logits"], model.last_vis_logits)
    return r


def two_window_clip(golden):
    return dev_clip(clip_from_golden(golden("e2e_two_windows")))


def frames_0_to_14_clip():
    c = synth.make_clip(83, V=2, T=31, H=128, W=128, N=30)
    c["query_points"][0, :, 0] = np.arange(30) % 15
    return dev_clip(c)


@pytest.mark.parametrize("prec", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("which", ["two_windows", "frames_0_14"])
def test_session_equals_forward(model, golden, prec, which):
    clip = two_window_clip(golden) if which == "two_windows" else frames_0_to_14_clip()
    q = clip["query_points"]
    sets, q_mid = mid_stream_sets(q)
    with precision(model, prec):
        for block in (1, S // 2, 7):
            res, st = stream(model, clip, block, [(0, q)])
            windows = list(model.last_windows)
            check_equal(model, clip, q, res)
            assert model.last_windows == windows and len(windows) >= 2
            st.check_finite()
            res, _ = stream(model, clip, block, sets)
            check_equal(model, clip, q_mid, res)
    torch.cuda.synchronize()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_queries_in_the_last_half_window_give_zeros(model, prec):
    c = synth.make_clip(84, V=2, T=16, H=128, W=128, N=6)
    c["query_points"][0, :, 0] = np.array([10, 12, 15, 11, 13, 10], dtype=np.float32)  # all >= T - S/2: no window runs
    clip = dev_clip(c)
    with precision(model, prec):
        for block in (1, 6, 7):
            res, _ = stream(model, clip, block, [(0, clip["query_points"])])
            assert model.last_windows == []
            r = check_equal(model, clip, clip["query_points"], res)
            assert model.last_windows == [] and float(r["traj_e"].abs().max()) == 0.0 and float(res["traj_e"].abs().max()) == 0.0


def test_session_against_reference_fixture_fp32(model, golden):
    """tests/test_gpu_e2e.py::test_forward_golden's tolerances, on the streamed result."""
    g = golden("e2e_two_windows")
    clip = dev_clip(clip_from_golden(g))
    res, st = stream(model, clip, 7, [(0, clip["query_points"])])
    st.check_finite()
    assert len(model.last_windows) == int(g["n_windows"])
    ref = g["traj_exact"]
    rel = np.abs(res["traj_e"].cpu().numpy() - ref).max() / np.abs(ref).max()
    print(f"streamed e2e_two_windows: tracks rel {rel:.3e}")
    assert rel < 1e-4, rel
    assert np.abs(res["vis_e"].cpu().numpy() - g["vis_exact"]).max() < 1e-3
    fi = g["feat_init_exact"]
    assert np.abs(res["feat_init"].cpu().numpy() - fi).max() / np.abs(fi).max() < 2e-5


def test_session_against_reference_fixture_bf16(model, golden):
    """tests/test_gpu_e2e.py::test_forward_bf16_vs_reference_autocast's bars, on the streamed result."""
    g = golden("e2e_two_windows_bf16")
    clip = dev_clip(clip_from_golden(g))
    with precision(model, "bf16"):
        res, st = stream(model, clip, 7, [(0, clip["query_points"])])
        st.check_finite()
    got, gv = res["traj_e"].cpu().numpy(), res["vis_e"].cpu().numpy()
    ref32, refbf = g["traj_fp32_exact"], g["traj_exact"]
    v32, vbf = g["vis_fp32_exact"], g["vis_exact"]
    sc = np.abs(ref32).max()
    d_ref, dv_ref = np.abs(refbf - ref32).max() / sc, np.abs(vbf - v32).max()
    e32, ev32 = np.abs(got - ref32).max() / sc, np.abs(gv - v32).max()
    ebf, evbf = np.abs(got - refbf).max() / sc, np.abs(gv - vbf).max()
    print(f"streamed e2e_two_windows_bf16: vs reference fp32 {e32:.2e} / {ev32:.2e} (autocast itself {d_ref:.2e} / {dv_ref:.2e}), "
          f"vs reference autocast {ebf:.2e} / {evbf:.2e}")
    assert e32 <= max(d_ref, 1e-4) and ev32 <= max(dv_ref, 1e-3), (e32, d_ref, ev32, dv_ref)
    assert ebf <= 2 * d_ref and evbf <= 2 * dv_ref, (ebf, d_ref, evbf, dv_ref)
    assert e32 <= 2.5e-3 and ev32 <= 0.1, (e32, ev32)


def test_full_size_session(model):
    """The benchmark's shape (4 views, 24 frames, 512 x 512, 1 024 queries, bf16) in blocks of 6 frames: the bits of ``forward``,
    and a ring that is allocated once."""
    clip = dev_clip(synth.make_clip(1234, V=4, T=24, H=512, W=512, N=1024))
    ptrs = []

    def watch(st):
        s = st.store
        ptrs.append(tuple(t.data_ptr() for k in ("fvec", "xyz", "box", "gbox") for t in s[k] if t is not None) + (s["depth_s"].data_ptr(),))

    with precision(model, "bf16"):
        res, st = stream(model, clip, 6, [(0, clip["query_points"])], watch=watch)
        watch(st)
        check_equal(model, clip, clip["query_points"], res)
    assert len(ptrs) == 5 and len(set(ptrs)) == 1
    assert st.store["fvec"][0].shape[0] == 18  # 3 blocks of S/2 frames, whatever the clip length


def test_predictor_session_equals_forward(model):
    from mvtracker_amd.predictor import EvaluationPredictor
    c = synth.make_clip(85, V=2, T=20, H=480, W=640, N=12, late_queries=True, query_frames=(3, 7))
    clip = dev_clip(c)
    p = EvaluationPredictor(model, interp_shape=(384, 512), grid_size=5, n_grids_per_view=1, n_iters=4)
    with precision(model, "bf16"):
        r = p(clip["rgbs"], clip["depths"], clip["query_points"], clip["intrs"], clip["extrs"])
        st = p.open_stream(clip["query_points"])
        outs = [st.push(*(clip[k][:, :, t:t + 6] for k in ("rgbs", "depths", "intrs", "extrs"))) for t in range(0, 20, 6)]
        outs.append(st.finish())
    for k in ("traj_e", "vis_e", "vis_e_as_prob"):
        assert torch.equal(torch.cat([o[k] for o in outs], 1), r[k]), k
    assert outs[-1]["frames"][1] == 20 and not p.last_nan
    with pytest.raises(NotImplementedError):
        EvaluationPredictor(model, single_point=True).open_stream(clip["query_points"])
    with pytest.raises(NotImplementedError):
        EvaluationPredictor(model, n_grids_per_view=2).open_stream(clip["query_points"])
