"""Backward tracking on the MI355X (`-m gpu`): ``forward(backward_tracking=True)`` against the host composition of two plain calls
(clip, time-flipped clip) bit for bit, the signed frame step of every store-indexing kernel against the same kernel on the flipped
store, the reference fixture tests/golden/e2e_backward.npz at the end-to-end tolerances, and the predictor option."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mvtracker_amd import hip, synth  # noqa: E402
from mvtracker_amd.backward import reversed_layout  # noqa: E402
from mvtracker_amd.frame_store import nseg  # noqa: E402
from oracle import mvt_oracle as O  # noqa: E402

from test_backward_host import args_of, backward_clip, flip_args, merge, reached_by_reversed  # noqa: E402

DEV = "cuda:0"
CFG = O.TrackerConfig()


@pytest.fixture(scope="module")
def model():
    from mvtracker_amd.tracker import MVTracker
    m = MVTracker(hidden_size=256).eval()
    sd = synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to(DEV)


@pytest.fixture(scope="module")
def clips(golden):
    """name -> device arguments: the fixture's two-window clip, and a clip of the benchmark's size (C3: 4 views x 24 frames x
    512x512, 1024 queries) with query frames spread over the whole clip."""
    out = {"two_windows": args_of(backward_clip(golden("e2e_backward")), DEV)}
    clip = synth.make_clip(7, V=4, T=24, H=512, W=512, N=1024)
    clip["query_points"][0, :, 0] = np.random.default_rng(3).integers(0, 24, size=1024).astype(np.float32)
    out["c3"] = args_of(clip, DEV)
    return out


def compose(model, a, **kw):
    """What a user of plain ``forward`` can do: run the clip and the flipped clip, merge on the host.  Returns (traj, vis, logits)."""
    T, S = a[0].shape[2], model.S
    qt = a[2][0, :, 0].long().cpu()
    rf = model(*a, **kw)
    f = [rf["traj_e"].clone(), rf["vis_e"].clone(), model.last_vis_logits.clone()]
    rb = model(*flip_args(a), **kw)
    b = [rb["traj_e"].clone(), rb["vis_e"].clone(), model.last_vis_logits.clone()]
    reached = reached_by_reversed(qt, S, T)
    return [merge(x, y, qt, reached) for x, y in zip(f, b)], f


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("size", ["two_windows", "c3"])
def test_backward_equals_composition_bit_for_bit(model, clips, size, precision):
    """Derivable, not measured: per-image encoder results do not depend on chunking, the search is exact, and both sides run the
    same launch forms on the same operand values in the same row order."""
    a = clips[size]
    T = a[0].shape[2]
    model.precision = precision
    try:
        want, fwd = compose(model, a, iters=4)
        r = model(*a, iters=4, backward_tracking=True)
        got = [r["traj_e"], r["vis_e"], model.last_vis_logits]
        torch.cuda.synchronize()
        model.check_finite()
    finally:
        model.precision = "fp32"
    assert len(model.last_windows_backward) >= 2
    for name, g, w in zip(("traj_e", "vis_e", "logits"), got, want):
        diff = (g != w)
        print(f"{size}/{precision} {name}: {int(diff.sum())} of {diff.numel()} elements differ, max abs {float((g - w).abs().max()):.3e}")
        assert torch.equal(g, w), name
    # option off = untouched: frames from the query frame on are the plain forward's bits
    qt = a[2][0, :, 0].long()
    keep = torch.arange(T, device=DEV)[:, None] >= qt[None, :]
    for g, f in zip(got, fwd):
        k = keep.reshape(1, T, -1, *([1] * (g.dim() - 3)))
        assert torch.equal(torch.where(k, g, torch.zeros((), device=DEV)), torch.where(k, f, torch.zeros((), device=DEV)))


def test_queries_at_frame_zero_change_nothing(model, clips):
    a = list(clips["two_windows"])
    q = a[2].clone()
    q[0, :, 0] = 0.0
    a[2] = q
    r0 = model(*a, iters=4)
    t0, v0, l0 = r0["traj_e"].clone(), r0["vis_e"].clone(), model.last_vis_logits.clone()
    r1 = model(*a, iters=4, backward_tracking=True)
    assert torch.equal(r1["traj_e"], t0) and torch.equal(r1["vis_e"], v0) and torch.equal(model.last_vis_logits, l0)
    assert torch.equal(r1["feat_init"], r0["feat_init"])


def _flip_store(store):
    fl = lambda t: None if t is None else t.flip(0).contiguous()
    out = dict(store)
    for k in ("xyz", "fvec", "box", "gbox"):
        out[k] = [fl(t) for t in store[k]]
    return out


def test_signed_frame_step_equals_flipped_store(model, clips):
    """Every entry that maps a window slot to a store frame: (frame0 = T-1-w, step = -1) on the store equals (w, +1) on the
    time-flipped store, bit for bit -- a window inside the clip and one that runs past frame 0 (clamp), unseeded and seeded."""
    a = clips["two_windows"]
    st = model.build_frame_store(a[0][0], a[1][0], a[3][0], a[4][0])
    fs = _flip_store(st)
    T, S, K, L, C = st["T"], model.S, model.corr_neighbors, model.corr_n_levels, model.latent_dim
    n = a[2].shape[1]
    gen = torch.Generator().manual_seed(9)
    coords = (a[2][0, :, None, 1:].cpu() + 0.05 * torch.randn(n, S, 3, generator=gen)).to(DEV).contiguous()
    targets = torch.randn(n, S, C, generator=gen).to(DEV)
    for w in (3, 9):  # slots 14..3, and 8..0 then frame 0 repeated
        f0 = T - 1 - w
        sides = []
        for store, fr, step in ((st, f0, -1), (fs, w, 1)):
            res = {}
            lv = lambda seed, out: [dict(xyz=store["xyz"][l], P=store["P"][l], seed_idx=None if seed is None else seed[l], box=store["box"][l],
                                         grid=store["tile_grid"][l], idx_out=out[l], gbox=store["gbox"][l]) for l in range(L)]
            idx0 = torch.empty(L, n, S, K, device=DEV, dtype=torch.int32)
            hip.knn_search_levels(lv(None, idx0), coords, n, S, fr, step, T, K, seed_k=0)
            res["search_levels"] = idx0
            idx1 = torch.empty_like(idx0)
            moved = (coords + 0.01).contiguous()
            hip.knn_search_levels(lv(idx0, idx1), moved, n, S, fr, step, T, K, seed_k=K)
            res["search_levels_seeded"] = idx1
            # the two-launch forms: per-segment keys, then the merge
            nsegs = [nseg(store["P"][l], K) for l in range(L)]
            keys = [torch.empty(n * S * nsegs[l] * K, device=DEV, dtype=torch.int64) for l in range(L)]
            idx2 = torch.empty_like(idx0)
            lv2 = [dict(d, keys=keys[l], nseg=nsegs[l]) for l, d in enumerate(lv(idx0, idx2))]
            hip.knn_scan_levels(lv2, moved, n, S, fr, step, T, K, seed_k=K)
            hip.knn_merge_levels(lv2, n, S, K)
            res["scan_levels_seeded"] = idx2
            idx3 = torch.empty(n, S, K, device=DEV, dtype=torch.int32)
            hip.knn_search(store["xyz"][0], store["P"][0], coords, n, S, fr, step, T, K, idx3, store["box"][0], grid=store["tile_grid"][0],
                           gbox=store["gbox"][0])
            res["search"] = idx3
            k0 = torch.empty(n * S * nsegs[0] * K, device=DEV, dtype=torch.int64)
            hip.knn_scan(store["xyz"][0], store["P"][0], coords, n, S, fr, step, T, K, nsegs[0], k0, box=store["box"][0],
                         grid=store["tile_grid"][0])
            idx4 = torch.empty(n, S, K, device=DEV, dtype=torch.int32)
            hip.knn_merge(k0, n, S, K, nsegs[0], store["P"][0], idx4)
            res["scan"] = idx4
            Fc = L * K * model.corr_width
            fc = torch.empty(n, S, Fc, device=DEV)
            hip.corr_gather_dot(store["xyz"], store["fvec"], store["P"], [idx0[l] for l in range(L)], C, targets, coords, n, S, fr, step, T, K,
                                fc, Fc, 0)
            res["corr"] = fc
            Fo = L * K * (2 + 3)  # two dot groups + the neighbour coordinates, no offsets
            fo = torch.empty(n, S, Fo, device=DEV)
            hip.corr_gather_dot_opts(store["xyz"], store["fvec"], store["P"], [idx0[l] for l in range(L)], C, targets, coords, n, S, fr, step,
                                     T, K, 2, False, True, fo, Fo, 0)
            res["corr_opts"] = fo
            sides.append(res)
        torch.cuda.synchronize()
        assert torch.equal(sides[0]["search"], sides[0]["search_levels"][0]) and torch.equal(sides[0]["scan"], sides[0]["search"])
        assert torch.equal(sides[0]["scan_levels_seeded"], sides[0]["search_levels_seeded"])
        for k in sides[0]:
            assert torch.equal(sides[0][k], sides[1][k]), (w, k)


def test_reversed_window_kernels(model):
    """mvt_window_prepare with frame_step = -1 is frame_step = +1 on flipped times; mvt_window_store with frame_step = -1 and the
    query frames as `before` writes frame T-1-wr-s only where it lies before the row's query frame."""
    T, S, C, n, p0, N = 18, 12, 128, 10, 6, 14
    gen = torch.Generator().manual_seed(2)
    qt = torch.sort(torch.randint(0, T, (n,), generator=gen), descending=True).values.int().to(DEV)
    qxyz, feat = torch.randn(n, 3, generator=gen).to(DEV), torch.randn(n, C, generator=gen).to(DEV)
    pc, pv = torch.randn(p0, S, 3, generator=gen).to(DEV), torch.randn(p0, S, generator=gen).to(DEV)
    for wr in (3, 9):
        outs = []
        for rev in (True, False):
            wc, wm, wf = torch.empty(n, S, 3, device=DEV), torch.empty(n, S, 2, device=DEV), torch.empty(n, S, C, device=DEV)
            if rev:
                hip.window_prepare(qxyz, qt, feat, pc, pv, n, p0, S, C, T - 1 - wr, T, wc, wm, wf, frame_step=-1)
            else:
                hip.window_prepare(qxyz, (T - 1 - qt).int(), feat, pc, pv, n, p0, S, C, wr, T, wc, wm, wf)
            outs.append((wc, wm, wf))
        for x, y in zip(*outs):
            assert torch.equal(x, y)
        order = torch.randperm(N, generator=gen)[:n].to(DEV)
        coords, vis = torch.randn(n, S, 3, generator=gen).to(DEV), torch.randn(n, S, generator=gen).to(DEV)
        traj = torch.full((T, N, 3), 7.0, device=DEV)
        lg, pr = torch.full((T, N), 7.0, device=DEV), torch.full((T, N), 7.0, device=DEV)
        hip.window_store(coords, vis, order, n, S, T - 1 - wr, T, N, traj, lg, pr, frame_step=-1, before=qt)
        want_t, want_l = torch.full((T, N, 3), 7.0), torch.full((T, N), 7.0)
        for i in range(n):
            for s in range(min(S, T - wr)):
                f = T - 1 - wr - s
                if f < int(qt[i]):
                    want_t[f, int(order[i])] = coords[i, s].cpu()
                    want_l[f, int(order[i])] = vis[i, s].cpu()
        assert torch.equal(traj.cpu(), want_t) and torch.equal(lg.cpu(), want_l)
        wrote = want_l != 7.0
        assert torch.equal(pr.cpu()[~wrote], want_l[~wrote])
        assert float((pr.cpu()[wrote] - torch.sigmoid(want_l[wrote])).abs().max()) < 1e-6


def test_backward_golden(model, golden):
    """The reference's two runs merged (tests/golden/make_golden_backward.py), at the tolerances test_forward_golden applies to
    e2e_two_windows: tracks 1e-4 of the track scale, visibilities 1e-3."""
    g = golden("e2e_backward")
    a = args_of(backward_clip(g), DEV)
    r = model(*a, iters=4, backward_tracking=True)
    torch.cuda.synchronize()
    model.check_finite()
    assert model.last_windows == [tuple(int(x) for x in row) for row in g["windows_forward"]]
    assert model.last_windows_backward == [tuple(int(x) for x in row) for row in g["windows_backward"]]
    ref = g["traj_merged"]
    rel = np.abs(r["traj_e"].cpu().numpy() - ref).max() / np.abs(ref).max()
    verr = np.abs(r["vis_e"].cpu().numpy() - g["vis_merged"]).max()
    lerr = np.abs(model.last_vis_logits.cpu().numpy() - g["logits_merged"]).max()
    print(f"backward golden: tracks rel {rel:.3e}, vis {verr:.3e}, logits {lerr:.3e}")
    assert rel < 1e-4, rel
    assert verr < 1e-3, verr
    assert lerr < 1e-3, lerr
    fi = g["feat_init_forward"]
    assert np.abs(r["feat_init"].cpu().numpy() - fi).max() / np.abs(fi).max() < 2e-5


def test_backward_bf16_vs_autocast_oracle(model, golden):
    """Plain bf16 under the existing rule (test_forward_bf16_vs_autocast_oracle): at least as close to the fp32 oracle as 3x the
    oracle under bf16 autocast is -- here for the merged result, the oracle composed from its two runs."""
    g = golden("e2e_backward")
    W = O.make_weights(CFG, seed=0)
    a = args_of(backward_clip(g))
    T, S = a[0].shape[2], CFG.sliding_window_len
    qt = a[2][0, :, 0].long()
    reached = reached_by_reversed(qt, S, T)

    def oracle_merged():
        rf = O.tracker_forward(W, CFG, *a, iters=4, knn_mode="exact")
        rb = O.tracker_forward(W, CFG, *flip_args(a), iters=4, knn_mode="exact")
        return [merge(rf[k].float(), rb[k].float(), qt, reached) for k in ("traj_e", "vis_logits")]

    ro = oracle_merged()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        rb = oracle_merged()
    tol_t = 3 * ((rb[0] - ro[0]).abs().max() / ro[0].abs().max()).item()
    tol_v = 3 * (rb[1] - ro[1]).abs().max().item()
    model.precision = "bf16"
    try:
        r = model(*[t.to(DEV) for t in a], iters=4, backward_tracking=True)
        torch.cuda.synchronize()
    finally:
        model.precision = "fp32"
    et = ((r["traj_e"].cpu() - ro[0]).abs().max() / ro[0].abs().max()).item()
    ev = (model.last_vis_logits.cpu() - ro[1]).abs().max().item()
    print(f"backward bf16: tracks rel err {et:.2e} (autocast-oracle tol {tol_t:.2e}), vis logits {ev:.2e} (tol {tol_v:.2e})")
    assert et < max(tol_t, 1e-4) and ev < max(tol_v, 1e-3)


def test_late_queries_get_their_early_frames(model, golden):
    """The fixture's late queries (t_q >= T - S/2) on their own: no forward window runs, so the rows from the query frame on stay
    the reference's pinned zeros; the reversed pass fills the frames before it with finite, non-zero estimates."""
    g = golden("e2e_backward")
    a = args_of(backward_clip(g), DEV)
    T, S = a[0].shape[2], model.S
    qt = a[2][0, :, 0].long()
    late = torch.nonzero(qt >= T - S // 2)[:, 0]
    assert late.numel() > 0
    al = [a[0], a[1], a[2][:, late].contiguous(), a[3], a[4]]
    off = model(*al, iters=4)
    assert model.last_windows == [] and float(off["traj_e"].abs().max()) == 0.0
    r = model(*al, iters=4, backward_tracking=True)
    torch.cuda.synchronize()
    model.check_finite()
    assert model.last_windows == [] and len(model.last_windows_backward) >= 1
    for i, n in enumerate(late.tolist()):
        t = int(qt[n])
        assert float(r["traj_e"][0, t:, i].abs().max()) == 0.0 and float(r["vis_e"][0, t:, i].abs().max()) == 0.0
        early = r["traj_e"][0, :t, i]
        assert bool(torch.isfinite(early).all()) and float(early.abs().sum(-1).min()) > 0.0
    assert float(r["feat_init"][0, 0].abs().sum(-1).min()) > 0.0
    # and inside the full query set the same queries are tracked in both directions
    rf = model(*a, iters=4, backward_tracking=True)
    for n in late.tolist():
        assert float(rf["traj_e"][0, :, n].abs().sum(-1).min()) > 0.0


def test_frame_store_without_early_frames_is_refused(model, clips):
    a = clips["two_windows"]
    store = model.build_frame_store(a[0][0], a[1][0], a[3][0], a[4][0], t0=2)
    q = a[2].clone()
    q[0, :, 0] = q[0, :, 0].clamp(min=2.0)
    with pytest.raises(ValueError, match="from frame 0"):
        model(a[0], a[1], q, a[3], a[4], iters=1, frame_store=store, backward_tracking=True)
    full = model.build_frame_store(a[0][0], a[1][0], a[3][0], a[4][0])
    r1 = model(a[0], a[1], q, a[3], a[4], iters=4, frame_store=full, backward_tracking=True)
    t1 = r1["traj_e"].clone()
    r2 = model(a[0], a[1], q, a[3], a[4], iters=4, backward_tracking=True)  # (early frames encoded on the second stream)
    assert torch.equal(t1, r2["traj_e"])
    with pytest.raises(NotImplementedError, match="backward_tracking"):
        model.forward_grouped(a[0], a[1], [q], a[3], a[4], backward_tracking=True)


@pytest.mark.parametrize("single_point", [False, True])
def test_predictor_backward_tracking(model, single_point):
    """EvaluationPredictor(backward_tracking=True) against the same composition through the predictor (predictor_small's size:
    2 views x 12 frames x 160x192 resized to 128x160, support grids), and the refusal at single_point_group_size > 1."""
    from mvtracker_amd.predictor import EvaluationPredictor
    clip = synth.make_clip(41, V=2, T=12, H=160, W=192, N=5)
    clip["query_points"][0, :, 0] = np.array([0, 4, 7, 9, 11], np.float32)
    a = args_of(clip, DEV)
    T = 12
    kw = dict(interp_shape=(128, 160), grid_size=3, n_grids_per_view=2, n_iters=2, single_point=single_point,
              local_grid_size=3 if single_point else 8, local_extent=20 if single_point else 50)
    call = lambda p, x: p(rgbs=x[0], depths=x[1], query_points_3d=x[2], intrs=x[3], extrs=x[4])
    got = call(EvaluationPredictor(model, backward_tracking=True, **kw), a)
    # the composition: the predictor's own query set (queries + support points, built on the unflipped clip) through two plain
    # forwards; captured from the plain predictor's model calls
    calls = []
    orig = model.forward

    def spy(rgbs, depths=None, query_points=None, intrs=None, extrs=None, **k):
        calls.append((rgbs, depths, query_points, intrs, extrs, k))
        return orig(rgbs, depths=depths, query_points=query_points, intrs=intrs, extrs=extrs, **k)

    model.forward = spy
    try:
        call(EvaluationPredictor(model, **kw), a)
    finally:
        del model.forward
    assert len(calls) == (5 if single_point else 1)
    qt_all = a[2][0, :, 0].long().cpu()
    for i, (rgbs, depths, q, intrs, extrs, k) in enumerate(calls):
        k = {x: y for x, y in k.items() if x in ("iters",)}
        x = [rgbs, depths, q, intrs, extrs]
        qt = q[0, :, 0].long().cpu()
        rf = model(*x, **k)
        f = [rf["traj_e"].clone(), rf["vis_e"].clone()]
        rb = model(*flip_args(x), **k)
        reached = reached_by_reversed(qt, model.S, T)
        want_t, want_v = [merge(p, q_, qt, reached) for p, q_ in zip(f, [rb["traj_e"], rb["vis_e"]])]
        if single_point:
            assert torch.equal(got["traj_e"][:, :, i], want_t[:, :, 0]) and torch.equal(got["vis_e_as_prob"][:, :, i], want_v[:, :, 0])
        else:
            assert torch.equal(got["traj_e"], want_t[:, :, :5]) and torch.equal(got["vis_e_as_prob"], want_v[:, :, :5])
    assert bool(torch.isfinite(got["traj_e"]).all()) and int(qt_all.max()) == 11
    if single_point:
        p = EvaluationPredictor(model, backward_tracking=True, **kw)
        p.single_point_group_size = 4
        with pytest.raises(NotImplementedError, match="backward_tracking"):
            call(p, a)
