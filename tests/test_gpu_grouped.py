"""Grouped forward (`-m gpu`): G independent query sets through one launch sequence.  Segmented attention against the ungrouped
kernels segment by segment, the grouped updater against one call per set, MVTracker.forward_grouped against one forward per
group, and single_point batching in the evaluation predictor."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mvtracker_amd import hip, synth  # noqa: E402

DEV = "cuda:0"
S, H, DH = 12, 6, 48
INNER = H * DH
NV = 64


def T(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def model():
    from mvtracker_amd.tracker import MVTracker
    m = MVTracker(hidden_size=256).eval()
    sd = synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.to(DEV)


class _Prec:
    def __init__(self, model, prec):
        self.model, self.prec = model, prec

    def __enter__(self):
        self.old = self.model.precision
        self.model.precision = self.prec

    def __exit__(self, *a):
        self.model.precision = self.old


def _args(clip):
    return [T(clip[k]).to(DEV) for k in ("rgbs", "depths", "query_points", "intrs", "extrs")]


# ------------------------------------------------------------------ segmented attention
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("pattern", ["v2p", "vs", "p2v"])
def test_segmented_attention_matches_ungrouped(bf16, pattern):
    """Every segment of one segmented launch is bit-identical to the ungrouped kernel on that segment alone (each segment takes
    its own kernel form; bf16: n_g = 512 / 1024 take the key-split path with its merge launch, 700 does not: 22 key blocks)."""
    segs = [1, 5, 63, 64, 65, 357, 700] + ([512, 1024] if bf16 else [])
    G, n = len(segs), sum(segs)
    Mp, Mv = n * S, G * NV * S
    dt = torch.bfloat16 if bf16 else torch.float32
    g = torch.Generator().manual_seed(7 + len(pattern) + 10 * bf16)
    buf = (torch.randn(Mp + Mv, 3 * INNER, generator=g) * 2).to(DEV, dt)
    offs = np.concatenate([[0], np.cumsum(segs)])
    pts = [(int(offs[i]) * S, segs[i]) for i in range(G)]
    virt = [(Mp + i * NV * S, NV) for i in range(G)]
    qs, ks = {"v2p": (virt, pts), "vs": (virt, virt), "p2v": (pts, virt)}[pattern]
    q, k, v = buf[:, :INNER], buf[:, INNER:2 * INNER], buf[:, 2 * INNER:]
    ld = 3 * INNER
    out = torch.full((Mp + Mv, INNER), float("nan"), device=DEV, dtype=dt)
    q0, nq = zip(*qs)
    k0, nk = zip(*ks)
    if bf16:
        ws = torch.empty(hip.attention_segmented_ws_floats(S, nq, H), device=DEV)
        hip.attention_bf16_segmented(q, ld, 1, S, k, v, ld, 1, S, out, INNER, S, H, DH, q0, nq, k0, nk, ws=ws)
    else:
        hip.attention_segmented(q, ld, 1, S, k, v, ld, 1, S, out, INNER, S, H, DH, q0, nq, k0, nk)
    for (qr, nq_), (kr, nk_) in zip(qs, ks):
        ref = torch.full((nq_ * S, INNER), float("nan"), device=DEV, dtype=dt)
        if bf16:
            ws1 = torch.empty(hip.attention_ws_floats(S, nq_, H), device=DEV)
            hip.attention_bf16(q[qr:], ld, 1, S, k[kr:], v[kr:], ld, 1, S, ref, INNER, S, nq_, nk_, H, DH, ws=ws1)
        else:
            hip.attention(q[qr:], ld, 1, S, k[kr:], v[kr:], ld, 1, S, ref, INNER, S, nq_, nk_, H, DH)
        got = out[qr:qr + nq_ * S]
        assert bool(torch.isfinite(ref.float()).all())
        assert torch.equal(got, ref), (pattern, nq_, nk_, (got.float() - ref.float()).abs().max().item())
    torch.cuda.synchronize()


@pytest.mark.parametrize("bf16", [False, True])
def test_segmented_attention_many_segments(bf16):
    """More segments of one form than a launch's segment table holds (32): the entry splits them over several launches -- in bf16
    with the key-split workspace handed on from launch to launch (every 512-key segment takes the split path)."""
    segs = [(1, 5, 64, 65, 512)[i % 5] for i in range(80)]
    G, n = len(segs), sum(segs)
    Mp, Mv = n * S, G * NV * S
    dt = torch.bfloat16 if bf16 else torch.float32
    buf = torch.randn(Mp + Mv, 3 * INNER, generator=torch.Generator().manual_seed(99 + bf16)).to(DEV, dt)
    offs = np.concatenate([[0], np.cumsum(segs)])
    qs = [(Mp + i * NV * S, NV) for i in range(G)]
    ks = [(int(offs[i]) * S, segs[i]) for i in range(G)]
    q, k, v = buf[:, :INNER], buf[:, INNER:2 * INNER], buf[:, 2 * INNER:]
    ld = 3 * INNER
    out = torch.full((Mp + Mv, INNER), float("nan"), device=DEV, dtype=dt)
    q0, nq = zip(*qs)
    k0, nk = zip(*ks)
    if bf16:
        ws = torch.empty(hip.attention_segmented_ws_floats(S, nq, H), device=DEV)
        hip.attention_bf16_segmented(q, ld, 1, S, k, v, ld, 1, S, out, INNER, S, H, DH, q0, nq, k0, nk, ws=ws)
    else:
        hip.attention_segmented(q, ld, 1, S, k, v, ld, 1, S, out, INNER, S, H, DH, q0, nq, k0, nk)
    ws1 = torch.empty(hip.attention_ws_floats(S, NV, H), device=DEV)
    for (qr, nq_), (kr, nk_) in zip(qs, ks):
        ref = torch.empty(nq_ * S, INNER, device=DEV, dtype=dt)
        if bf16:
            hip.attention_bf16(q[qr:], ld, 1, S, k[kr:], v[kr:], ld, 1, S, ref, INNER, S, nq_, nk_, H, DH, ws=ws1)
        else:
            hip.attention(q[qr:], ld, 1, S, k[kr:], v[kr:], ld, 1, S, ref, INNER, S, nq_, nk_, H, DH)
        assert torch.equal(out[qr:qr + nq_ * S], ref), (nk_, qr)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ grouped updater
def _bar(a, b):
    rel = ((a - b).abs().max() / b.abs().max()).item()
    mean = ((a - b).abs().mean() / b.abs().mean()).item()
    return rel, mean


def test_updater_grouped_fp32(model):
    """fp32: every set's delta equals update_former on that set alone, bit for bit (sizes straddle the kernel forms)."""
    sizes = [16, 37, 342, 512]
    xs = [torch.randn(1, n, S, model.updateformer_input_dim, generator=torch.Generator().manual_seed(n)).to(DEV) for n in sizes]
    with _Prec(model, "fp32"):
        outs = model.update_former_grouped(xs)
        refs = [model.update_former(x) for x in xs]
    torch.cuda.synchronize()
    for n, o, r in zip(sizes, outs, refs):
        assert o.shape == r.shape
        assert torch.equal(o, r), (n, (o - r).abs().max().item())


def test_updater_grouped_bf16(model, monkeypatch):
    """bf16.  Composite entry (mvt_updateformer_forward_grouped): G = 1 bit-identical to mvt_updateformer_forward at equal
    fuse_attention bits; G = 4: each set within the bar of test_updater_fused_attention_matches_separate_launches of update_former
    on that set alone at fuse_attention = 0 (the block kernels pick their form from the total row count, so a set's rows may take
    another form than alone).  Python-sequenced block path: G = 1 bit-identical to the same path ungrouped."""
    sizes = [16, 37, 342, 512]
    xs = [torch.randn(1, n, S, model.updateformer_input_dim, generator=torch.Generator().manual_seed(50 + n)).to(DEV) for n in sizes]
    with _Prec(model, "bf16"):
        assert "updater_struct" in model._pack(torch.device(DEV))
        old = model.fuse_attention
        try:
            for f in (0, 55, 23):
                model.fuse_attention = f
                for x in xs:
                    a, b = model.update_former_grouped([x])[0], model.update_former(x)
                    assert torch.equal(a, b), (f, x.shape[1], (a - b).abs().max().item())
            model.fuse_attention = 55
            outs = model.update_former_grouped(xs)
            model.fuse_attention = 0
            refs = [model.update_former(x) for x in xs]
        finally:
            model.fuse_attention = old
        monkeypatch.setenv("MVT_COMPOSITE", "0")  # the Python-sequenced block path, grouped and ungrouped
        assert "updater_struct" not in model._pack(torch.device(DEV))
        singles = [model.update_former_grouped([x])[0] for x in xs]
        plain = [model.update_former(x) for x in xs]
        py_outs = model.update_former_grouped(xs)
        monkeypatch.delenv("MVT_COMPOSITE")
        model._pack(torch.device(DEV))
    torch.cuda.synchronize()
    for n, o, po, s1, p_, r in zip(sizes, outs, py_outs, singles, plain, refs):
        assert bool(torch.isfinite(o).all())
        assert torch.equal(s1, p_), (n, (s1 - p_).abs().max().item())
        for name, a in (("composite grouped", o), ("python grouped", po)):
            rel, mean = _bar(a, r)
            print(f"n={n} {name}: max {rel:.2e} mean {mean:.2e}")
            assert rel < 1.1e-2 and mean < 9e-3, (n, name, rel, mean)


# ------------------------------------------------------------------ forward_grouped
def _groups(clip):
    """5 groups of unequal size: a one-query group, one whose queries start at frames 9 / 13 (first window 9, not 0), a group with
    a query entering in the second window."""
    qp = T(clip["query_points"]).to(DEV)[0]
    qt = qp[:, 0].long().tolist()
    ids = [[0], [1, 3, 4, 5, 6, 7, 8], [9, 10, 11, 12], [19, 2], list(range(13, 19)) + list(range(20, 24))]
    assert sorted(sum(ids, [])) == list(range(24))
    assert min(qt[i] for i in ids[3]) == 9 and qt[11] == 5 and all(qt[i] == 0 for i in ids[0] + ids[4])
    return [qp[i][None] for i in ids]


@pytest.fixture(scope="module")
def clip():
    return synth.make_clip(71, V=3, T=20, H=128, W=160, N=24, late_queries=True, query_frames=(0, 5, 9, 13))


def test_forward_grouped_fp32_matches_forward(model, clip):
    """Five groups as _groups, plus one whose only query starts at frame 15 >= T - S/2: no window at all, zero outputs."""
    a = _args(clip)
    groups = _groups(clip)
    late = groups[0].clone()
    late[0, 0, 0] = 15.0
    groups.insert(2, late)
    with _Prec(model, "fp32"):
        res = model.forward_grouped(a[0], a[1], groups, a[3], a[4], iters=2)
        refs = [model(a[0], a[1], q, a[3], a[4], iters=2) for q in groups]
    torch.cuda.synchronize()
    assert len(res) == len(groups)
    for g, (r, f) in enumerate(zip(res, refs)):
        for key in ("traj_e", "vis_e", "feat_init"):
            assert r[key].shape == f[key].shape and r[key].dtype == f[key].dtype, (g, key)
            assert torch.equal(r[key], f[key]), (g, key, (r[key] - f[key]).abs().max().item())
    assert all(float(r["traj_e"].abs().sum()) > 0 for g, r in enumerate(res) if g != 2)
    assert not res[2]["traj_e"].any() and not res[2]["vis_e"].any() and not res[2]["feat_init"].any()


def test_forward_grouped_bf16(model, clip):
    """bf16: deterministic and finite; every group's first-iteration neighbours are its own forward's -- all tracks in its first
    window, the tracks that enter in later ones (carried tracks start from estimates that differ by bf16 rounding between the
    two updater paths: a neighbour may flip); the first updater delta of every group's first window within
    the bf16 bar of its own (composite-updater) forward."""
    a = _args(clip)
    groups = _groups(clip)
    with _Prec(model, "bf16"):
        tr = []
        r1 = model.forward_grouped(a[0], a[1], groups, a[3], a[4], iters=2, trace=tr)
        r2 = model.forward_grouped(a[0], a[1], groups, a[3], a[4], iters=2)
        own = []
        for q in groups:
            t_ = []
            model(a[0], a[1], q, a[3], a[4], iters=2, trace=t_)
            own.append(t_)
    torch.cuda.synchronize()
    for x, y in zip(r1, r2):
        for key in ("traj_e", "vis_e", "feat_init"):
            assert torch.equal(x[key], y[key]), key
            assert bool(torch.isfinite(x[key]).all())
    seen = {g: 0 for g in range(len(groups))}
    for wt in tr:
        off = wt["group_offsets"]
        for k, g in enumerate(wt["groups"]):
            ref = own[g][seen[g]]
            seen[g] += 1
            p0 = wt["carried"][k]
            idx = wt["knn_idx"][0][:, off[k]:off[k + 1]]
            assert idx.shape == ref["knn_idx"][0].shape, (g, idx.shape)
            assert torch.equal(idx[:, p0:], ref["knn_idx"][0][:, p0:]), g
            if seen[g] == 1:  # the group's first window
                d, dr = wt["delta"][0][off[k]:off[k + 1]], ref["delta"][0]
                rel, mean = _bar(d, dr)
                print(f"group {g}: first delta max {rel:.2e} mean {mean:.2e}")
                assert rel < 1.1e-2 and mean < 9e-3, (g, rel, mean)
    assert all(seen[g] == len(own[g]) for g in seen)


def test_forward_grouped_bf16_one_group_matches_forward(model, clip):
    """G = 1 through the grouped composite entries (mvt_updateformer_forward_tokens_grouped in every iteration): bit-identical to
    forward, which runs mvt_updateformer_forward_tokens (the searches are exact, so presearch and seeding change nothing)."""
    a = _args(clip)
    q = _groups(clip)[4]
    with _Prec(model, "bf16"):
        r = model.forward_grouped(a[0], a[1], [q], a[3], a[4], iters=2)[0]
        f = model(a[0], a[1], q, a[3], a[4], iters=2)
    torch.cuda.synchronize()
    for key in ("traj_e", "vis_e", "feat_init"):
        assert torch.equal(r[key], f[key]), (key, (r[key] - f[key]).abs().max().item())


def test_forward_grouped_rejects_empty_group(model, clip):
    a = _args(clip)
    q = T(clip["query_points"]).to(DEV)
    with pytest.raises(ValueError):
        model.forward_grouped(a[0], a[1], [q[:, :3], q[:, :0]], a[3], a[4])
    with pytest.raises(ValueError):
        model.forward_grouped(a[0], a[1], [], a[3], a[4])


# ------------------------------------------------------------------ predictor
def test_single_point_grouped_matches_per_query(model, golden):
    """single_point_group_size = 4 against one forward per query (fp32, bit for bit), and against the reference fixture."""
    from mvtracker_amd.predictor import EvaluationPredictor
    clip = synth.make_clip(62, V=2, T=18, H=128, W=128, N=9, late_queries=True, query_frames=(3, 7))
    a = _args(clip)
    with _Prec(model, "fp32"):
        pred = EvaluationPredictor(model, interp_shape=None, grid_size=2, local_grid_size=3, local_extent=20, single_point=True, n_iters=2)
        r1 = pred(rgbs=a[0], depths=a[1], query_points_3d=a[2], intrs=a[3], extrs=a[4])
        t1, v1 = r1["traj_e"].clone(), r1["vis_e_as_prob"].clone()
        pred.single_point_group_size = 4
        r4 = pred(rgbs=a[0], depths=a[1], query_points_3d=a[2], intrs=a[3], extrs=a[4])
        torch.cuda.synchronize()
        assert torch.equal(t1, r4["traj_e"]) and torch.equal(v1, r4["vis_e_as_prob"])
        g = golden("predictor_single_point")
        clip = synth.make_clip(int(g["clip_seed"]), V=2, T=12, H=128, W=128, N=3)
        a = _args(clip)
        a[2] = T(g["query_points"]).to(DEV)
        pred = EvaluationPredictor(model, interp_shape=None, grid_size=2, local_grid_size=3, local_extent=20, single_point=True, n_iters=2)
        pred.single_point_group_size = 4
        r = pred(rgbs=a[0], depths=a[1], query_points_3d=a[2], intrs=a[3], extrs=a[4])
    ref = g["traj_e"]
    assert np.abs(r["traj_e"].cpu().numpy() - ref).max() / np.abs(ref).max() < 1e-4
    assert np.abs(r["vis_e_as_prob"].cpu().numpy() - g["vis_e_as_prob"]).max() < 1e-3
