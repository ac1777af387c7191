"""The window state machine, the token-row kernels and the frame-store kernels on inputs whose right answer is exact.

GPU tests (`-m gpu`) go through `mvtracker_amd.hip`; the tests without the marker are the CPU-only checks of the reference
restatement, of the reference-side exactness claims and of the probes.  Every output buffer is poisoned (NaN, or the sentinel -77.5
where a later launch accumulates into it) before the launch, gets a padded leading dimension where the entry has one and a guard
row behind the last one, and whatever the kernel must not write has to stay poisoned.

A. Window state machine (mvt_window_prepare / mvt_window_store: frame_step +1 and -1, carry map, `before` bound, frame chunks).
   `reference_loop` is the reference's window loop (mvtracker.py:505-531, 537-540, 645-662, 692-698, 710-711) restated tensor for
   tensor for B = 1: the full (T, N) track mask zeroed with `[: w + S, :p1] = 0`, coords_init_ / vis_init_ updated in place, the
   short last window padded by repeating the last mask slot, `coords[:S_local]` stored, the un-sort by inv_sort_inds.  It knows
   nothing of `sp`, `half` or a clamped frame index.  The model is replaced by `standin`, a function of (window start, coords_init,
   vis_init, mask, ffeats) that depends on every input and every slot, returns small integers (exact in fp32) and logits in
   [-18, 18].  The device side takes the schedule from `backward.window_prefixes` and calls the kernels with the stand-in in
   between.  Sweep: S in {2, 4, 6, 12}, T in {2, 3, S/2+1, S-1, S, S+1, 3S/2, 3S/2+1, 2S+1, 3S-1}, C = 4, query frames random (at
   each N in {1, 5, 9, 13}) / all 0 / all T-S/2-1 (N cycling); a layout for which the reference runs no window is not generated.
   All comparisons are torch.equal, except vis_prob, which is within 1e-6 of the fp64 sigmoid of the logit (the bar of
   test_reversed_window_kernels).  On every window the mocks of tests/hip_mock.py give the kernels' outputs bit for bit on CPU
   copies of the same inputs (vis_prob, computed by two different exponentials: both within that 1e-6).  The options combine: the
   reversed sweep (flipped query frames, frame_step = -1, the query frames as `before`) also runs chunked and with a carry map, and
   `before` also runs with frame_step = +1.
B. Row kernels of tokens.hip: layernorm, delta_split, rowdot, broadcast_rows(_repeat), token_assemble, pos_embed; rows in
   {1, 5, 1000}.  LayerNorm / GroupNorm rows are m +- c with half the signs negative (and one entry m for odd C): sum, mean and the
   centred values are exact in any order, and the result is compared with fp64 F.layer_norm under the per-element bar
   32 * 2^-24 * (|w_c| + |b_c|) (at most 8 fp32 roundings of quantities <= |w| + |b|, times 4 for sqrtf and the reciprocal not being
   correctly rounded); a column dropped from the statistics at C = 512 moves an element by about |w_c| / 512, three orders above.
C. Frame-store kernels of pyramid.hip at non-square, non-divisible shapes: depth_subsample, avgpool2 (fp32, bf16), invert_cameras,
   unproject (levels 0, 1, 2); all torch.equal.
Probes (CPU): planted faults in a Python copy of the kernel rules must break the assertions above.
"""
import collections
import functools
import types
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hip_mock
from mvtracker_amd.backward import reversed_layout, window_prefixes

gpu = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
SENT = -77.5  # no integer and no probability: "differs from SENT" is "was written"
CW = 4  # feature width of the window sweep
ULP = 2.0 ** -24


@pytest.fixture(scope="module")
def hip():
    from mvtracker_amd import hip as h
    assert torch.cuda.is_available()
    return h


def G(t):
    return None if t is None else t.to(DEV)


def cpu(t):
    return None if t is None else t.cpu()


def gen(*key):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


def ints(g, lo, hi, *shape):
    """Integers in [lo, hi] as fp32."""
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def poison(*shape, dev="cpu", dtype=torch.float32, value=NAN):
    return torch.full(shape, value, device=dev, dtype=dtype)


def untouched(t):
    return bool(torch.isnan(t).all())


# ================================================================== A: the window state machine

Layout = collections.namedtuple("Layout", "S T N kind qt qxyz feat")


@functools.lru_cache(maxsize=None)
def layouts():
    out = []
    for S in (2, 4, 6, 12):
        for T in sorted({2, 3, S // 2 + 1, S - 1, S, S + 1, 3 * S // 2, 3 * S // 2 + 1, 2 * S + 1, 3 * S - 1}):
            hi = T - S // 2  # the reference runs a window only from a start below this
            if hi < 1:
                continue
            for kind, N in [("random", n) for n in (1, 5, 9, 13)] + [("zero", None), ("last", None)]:
                N = N or (1, 5, 9, 13)[len(out) % 4]
                g = gen("layout", S, T, kind, N)
                if kind == "random":
                    qt = torch.randint(0, T, (N,), generator=g)
                    qt[int(torch.randint(0, N, (1,), generator=g))] = int(torch.randint(0, hi, (1,), generator=g))
                else:
                    qt = torch.full((N,), 0 if kind == "zero" else hi - 1, dtype=torch.int64)
                out.append(Layout(S, T, N, kind, qt, ints(g, -9, 9, N, 3), ints(g, -3, 3, N, CW)))
    return out


def standin(w, coords, vis, mask, ffeats):
    """The model's stand-in: (n, S, 3), (n, S), (n, S), (n, S, C) -> new coords (n, S, 3), logits (n, S).  Small integers, every
    input and the slot observable, logits in [-18, 18]."""
    S, Cc = ffeats.shape[1], ffeats.shape[2]
    dev = coords.device
    slot = torch.arange(S, device=dev, dtype=torch.float32)[None, :]
    fm = torch.remainder((ffeats * torch.arange(1, Cc + 1, device=dev, dtype=torch.float32)).sum(-1), 5.0) - 2.0
    out = coords + mask[..., None] * torch.tensor([1.0, 2.0, 3.0], device=dev) + (fm + slot)[..., None] * torch.tensor([1.0, -1.0, 1.0], device=dev)
    lg = torch.remainder(vis + coords.sum(-1) + 3.0 * mask + fm + 2.0 * slot + float(w), 37.0) - 18.0
    return out.contiguous(), lg.contiguous()


def smart_cat(a, b, dim):
    return b if a is None else torch.cat([a, b], dim=dim)


def reference_loop(qt, qxyz, feat, S, T):
    """mvtracker.py:505-711 for B = 1 with `standin` for forward_iteration.  `feat` is the per-query initial feature (the reference's
    1-NN lookup, :607-643, an input here); the frame axis of the rolling feature maps is carried as a list of frame numbers."""
    batch_size, num_frames, num_points = 1, T, qt.shape[0]
    query_points_t = qt.clone().long()
    query_points_xyz_worldspace = qxyz[None]
    ind_array = torch.arange(num_frames)
    ind_array = ind_array[None, :, None].repeat(batch_size, 1, num_points)
    track_mask = (ind_array >= query_points_t[None, None, :]).unsqueeze(-1)
    coords_init = query_points_xyz_worldspace.unsqueeze(1).repeat(1, S, 1, 1)
    vis_init = qxyz.new_ones((batch_size, S, num_points, 1)) * 10
    _, sort_inds = torch.sort(query_points_t, dim=0, descending=False, stable=True)
    inv_sort_inds = torch.argsort(sort_inds, dim=0)
    assert torch.equal(query_points_t, query_points_t[sort_inds][inv_sort_inds])
    query_points_t_ = query_points_t[sort_inds]
    feat_ = feat[sort_inds]
    coords_init_ = coords_init[..., sort_inds, :].clone()
    vis_init_ = vis_init[:, :, sort_inds].clone()
    track_mask_ = track_mask[:, :, sort_inds].clone()
    traj_e_ = coords_init_.new_zeros((batch_size, num_frames, num_points, 3))
    vis_e_ = coords_init_.new_zeros((batch_size, num_frames, num_points))
    wrote_ = torch.zeros(batch_size, num_frames, num_points, dtype=torch.bool)
    w_idx_start = int(query_points_t_.min())
    p_idx_start = 0
    windows, calls = [], []
    frames_seq, feat_init = None, None
    edges = collections.Counter()
    while w_idx_start < num_frames - S // 2:
        curr_wind_points = torch.nonzero(query_points_t_ < w_idx_start + S)
        assert curr_wind_points.shape[0] > 0
        p_idx_end = curr_wind_points[-1].item() + 1
        windows.append((w_idx_start, p_idx_end))
        if frames_seq is None:
            new_seq_t0 = w_idx_start
        else:
            frames_seq = frames_seq[S // 2:]
            new_seq_t0 = w_idx_start + S // 2
        new_seq_t1 = w_idx_start + S
        frames_seq = smart_cat(frames_seq, torch.arange(num_frames)[new_seq_t0:new_seq_t1], dim=0)
        S_local = frames_seq.shape[0]
        if S_local < S:
            frames_seq = torch.cat([frames_seq, frames_seq[-1:].repeat(S - S_local)], 0)
        if p_idx_end - p_idx_start > 0:
            _feat_init_new = feat_[None, None, p_idx_start:p_idx_end]
            feat_init = smart_cat(feat_init, _feat_init_new.repeat(1, S, 1, 1), dim=2)
        if p_idx_start > 0:
            last_coords = coords[-1][:, S // 2:].clone()
            coords_init_[:, : S // 2, :p_idx_start] = last_coords
            coords_init_[:, S // 2:, :p_idx_start] = last_coords[:, -1].repeat(1, S // 2, 1, 1)
            last_vis = vis[:, S // 2:][..., None]
            vis_init_[:, : S // 2, :p_idx_start] = last_vis
            vis_init_[:, S // 2:, :p_idx_start] = last_vis[:, -1].repeat(1, S // 2, 1, 1)
        track_mask_current = track_mask_[:, w_idx_start: w_idx_start + S, :p_idx_end]
        if S_local < S:
            track_mask_current = torch.cat([track_mask_current, track_mask_current[:, -1:].repeat(1, S - S_local, 1, 1)], 1)
        call = dict(coords=coords_init_[0, :, :p_idx_end].permute(1, 0, 2).clone(), vis=vis_init_[0, :, :p_idx_end, 0].t().clone(),
                    mask=track_mask_current[0, :, :, 0].t().float(), ffeats=feat_init[0, :, :p_idx_end].permute(1, 0, 2).clone())
        calls.append(call)
        out, lg = standin(w_idx_start, call["coords"], call["vis"], call["mask"], call["ffeats"])
        coords, vis = [out.permute(1, 0, 2)[None]], lg.t()[None]
        traj_e_[:, w_idx_start:w_idx_start + S, :p_idx_end] = coords[-1][:, :S_local]
        vis_e_[:, w_idx_start:w_idx_start + S, :p_idx_end] = vis[:, :S_local]  # the logit; the reference's sigmoid is checked apart
        wrote_[:, w_idx_start:w_idx_start + S, :p_idx_end] = True
        track_mask_[:, : w_idx_start + S, :p_idx_end] = 0.0
        edges["windows"] += 1
        edges["short_window"] += S_local < S
        edges["carried"] += p_idx_start > 0
        edges["entering_later"] += p_idx_start > 0 and p_idx_end > p_idx_start
        edges["masked_new_track"] += bool((call["mask"][p_idx_start:] == 0).any())
        w_idx_start = w_idx_start + S // 2
        p_idx_start = p_idx_end
    assert p_idx_start == num_points  # the last window ends at or past the clip's end, so every query enters one
    edges["unwritten_frames"] += int((~wrote_).sum())
    edges["ragged_T"] += num_frames % (S // 2) != 0
    return dict(windows=windows, calls=calls, traj=traj_e_[0][:, inv_sort_inds], logit=vis_e_[0][:, inv_sort_inds],
                wrote=wrote_[0][:, inv_sort_inds], edges=edges)


@functools.lru_cache(maxsize=None)
def references():
    return [reference_loop(l.qt, l.qxyz, l.feat, l.S, l.T) for l in layouts()]


def flip_layout(l):
    """The layout whose REVERSED pass is l's forward pass: query frames T-1-qt."""
    return l._replace(qt=l.T - 1 - l.qt)


def run_windows(ops, lay, dev, reverse=False):
    """The device side: schedule from backward.window_prefixes / reversed_layout, the kernels of `ops` with `standin` in between."""
    S, T, N = lay.S, lay.T, lay.N
    qt = lay.qt.numpy()
    if reverse:
        rl = reversed_layout(qt, S, T)
        order, qt_s, windows = rl["order"], rl["sorted_qt"], rl["windows"]
        assert rl["frame0"] == [T - 1 - w for w, _ in windows] and rl["active"] == (windows[-1][1] if windows else 0)
    else:
        order = np.argsort(qt, kind="stable")
        qt_s = qt[order]
        windows = window_prefixes(qt_s, S, T)
    order_t = torch.from_numpy(order.astype(np.int64))
    r = dict(windows=list(windows), recs=[], order_d=order_t.to(dev), qt_d=torch.from_numpy(qt_s.astype(np.int32)).to(dev),
             qxyz_s=lay.qxyz[order_t].contiguous().to(dev), feat_s=lay.feat[order_t].contiguous().to(dev),
             traj=poison(T, N, 3, dev=dev, value=SENT), logit=poison(T, N, dev=dev, value=SENT), prob=poison(T, N, dev=dev, value=SENT))
    # the reversed pass: slot 0 of the window that starts at w in reversed time is clip frame T-1-w, the slots run downwards, and
    # only the frames before each row's query frame are stored
    r["step"], r["before"] = (-1, r["qt_d"]) if reverse else (1, None)
    prev_c = prev_v = None
    p0 = 0
    for w, p1 in windows:
        f0 = T - 1 - w if reverse else w
        wc, wm, wf = poison(p1, S, 3, dev=dev), poison(p1, S, 2, dev=dev), poison(p1, S, CW, dev=dev)
        ops.window_prepare(r["qxyz_s"], r["qt_d"], r["feat_s"], prev_c, prev_v, p1, p0, S, CW, f0, T, wc, wm, wf, frame_step=r["step"])
        out, lg = standin(w, wc, wm[..., 1], wm[..., 0], wf)
        ops.window_store(out, lg, r["order_d"], p1, S, f0, T, N, r["traj"], r["logit"], r["prob"], frame_step=r["step"], before=r["before"])
        r["recs"].append(dict(w=w, f0=f0, p0=p0, p1=p1, prev_c=prev_c, prev_v=prev_v, wc=wc, wm=wm, wf=wf, out=out, lg=lg))
        prev_c, prev_v, p0 = out, lg, p1
    return r


def check_prob(prob, logit, wrote):
    prob, logit = prob.cpu(), logit.cpu()
    assert torch.equal(prob[~wrote], torch.full_like(prob[~wrote], SENT))
    if bool(wrote.any()):
        assert float((prob[wrote].double() - torch.sigmoid(logit[wrote].double())).abs().max()) < 1e-6


def check_run(run, ref, lay, reverse=False):
    """The sweep's assertions for one layout.  reverse: `ref` is the reference on the flipped query frames, in reversed time."""
    assert run["windows"] == ref["windows"], (lay[:4], run["windows"], ref["windows"])
    for rec, call in zip(run["recs"], ref["calls"]):
        assert torch.equal(rec["wc"].cpu(), call["coords"]), (lay[:4], rec["w"], "coords")
        assert torch.equal(rec["wm"][..., 0].cpu(), call["mask"]), (lay[:4], rec["w"], "mask")
        assert torch.equal(rec["wm"][..., 1].cpu(), call["vis"]), (lay[:4], rec["w"], "vis_init")
        assert torch.equal(rec["wf"].cpu(), call["ffeats"]), (lay[:4], rec["w"], "ffeats")
    traj, logit, wrote = ref["traj"], ref["logit"], ref["wrote"]
    if reverse:  # back into clip time; only the frames before each query frame are the reversed pass's
        traj, logit, wrote = traj.flip(0), logit.flip(0), wrote.flip(0)
        wrote = wrote & (torch.arange(lay.T)[:, None] < lay.qt[None, :])
    assert torch.equal(run["traj"].cpu(), torch.where(wrote[..., None], traj, torch.full_like(traj, SENT))), (lay[:4], "traj")
    assert torch.equal(run["logit"].cpu(), torch.where(wrote, logit, torch.full_like(logit, SENT))), (lay[:4], "vis_logit")
    check_prob(run["prob"], run["logit"], wrote)


# ---- the kernels' rules in torch (the probes' carrier and the vectorised statement of the grid-stride cases)

def rule_prepare(qxyz, qt, feat, prev_c, prev_v, n, p0, S, Cc, frame0, T, coords, mask_vis, ffeats, frame_step=1, carry_src=None, bug=None):
    dev = coords.device
    reverse = frame_step < 0
    w = T - 1 - frame0 if reverse else frame0  # the window start in the pass's own time
    half = S // 2
    s = torch.arange(S, device=dev)
    last = S - 2 if bug == "carry_from_S-2" else S - 1
    sp = torch.where(s < half, half + s, torch.full_like(s, last))
    spv = torch.where(s < half, half + s, torch.full_like(s, S - 1)) if bug != "vis_other_slot" else s
    rows = torch.arange(n, device=dev)
    src = carry_src[:n].long() if carry_src is not None else torch.where(rows < p0, rows, torch.full_like(rows, -1))
    carried = src >= 0
    c = qxyz[:n, None, :].expand(n, S, 3).clone()
    v = torch.full((n, S), 10.0, device=dev)
    if bool(carried.any()):
        sc = src.clamp(min=0)
        c = torch.where(carried[:, None, None], prev_c.reshape(-1, S, 3)[sc][:, sp], c)
        v = torch.where(carried[:, None], prev_v.reshape(-1, S)[sc][:, spv], v)
    s_local = min(S, T - w)
    sl = s.clamp(max=s_local - 1)
    q = qt[:n].long()[:, None]
    if reverse:
        f0 = T - 1 - w
        f = (f0 - sl)[None, :]
        entered = f < q if bug == "rev:f<qt" else f <= q
        first_half = f >= f0 - half if bug == "rev:f>=f0-half" else f > f0 - half
    else:
        f = (w + sl)[None, :]
        entered = f > q if bug == "f>qt" else f >= q
        first_half = f < w + half + {"f<=w+half": 1, "f<w+half-1": -1}.get(bug, 0)
    on = entered & ~(carried[:, None] & first_half)
    coords.reshape(-1)[:n * S * 3].copy_(c.reshape(-1))
    mask_vis.reshape(-1)[:n * S * 2].copy_(torch.stack([on.float(), v], -1).reshape(-1))
    ffeats.reshape(-1)[:n * S * Cc].copy_(feat[:n, None, :].expand(n, S, Cc).reshape(-1))


def rule_store(coords, vis, order, n, S, frame0, T, N, traj, vis_logit, vis_prob, frame_step=1, before=None, frames=None, bug=None):
    """Slot s is frame frame0 + frame_step * s; written to row frame - f0 where the frame lies in `frames` = (f0, f1) (None: the whole
    clip) and before the row's bound, if one is given."""
    dev = coords.device
    f0, f1 = (0, T) if frames is None else frames
    s_local = min(S, T - frame0 if frame_step > 0 else frame0 + 1)
    if bug == "drop_last_short_slot" and s_local < S:
        s_local -= 1
    o = torch.arange(n, device=dev) if bug == "no_order" else order[:n]
    s = torch.arange(s_local, device=dev)
    fr = (frame0 + frame_step * s)[None, :].expand(n, s_local)
    keep = (fr >= f0) & (fr < f1)
    if before is not None:
        keep = keep & (fr < before[:n].long()[:, None])
    fi, ni = fr[keep] - f0, o[:, None].expand(n, s_local)[keep]
    lg = vis.reshape(n, S)[:, :s_local][keep]
    traj.reshape(-1, N, 3)[fi, ni] = coords.reshape(n, S, 3)[:, :s_local][keep]
    vis_logit.reshape(-1, N)[fi, ni] = lg
    # (the sigmoid of the whole window, then the selection: torch's CPU sigmoid is not the same bits for every vector length, and
    #  the chunks of one window are compared side by side with its whole-clip store)
    vis_prob.reshape(-1, N)[fi, ni] = torch.sigmoid(vis.reshape(n, S))[:, :s_local][keep]


def rule_ops(bug=None):
    return types.SimpleNamespace(window_prepare=functools.partial(rule_prepare, bug=bug), window_store=functools.partial(rule_store, bug=bug))


REVERSED_PROBES = ["rev:f<qt", "rev:f>=f0-half"]  # the mirror images of "f>qt" and "f<=w+half": they break the reversed rule only
PROBES = ["f>qt", "f<=w+half", "f<w+half-1", "carry_from_S-2", "vis_other_slot", "no_order", "drop_last_short_slot"] + REVERSED_PROBES


def failing_layouts(ops, reverse=False):
    """Layouts whose sweep fails; reverse: the reversed sweep (each layout's reference against the reversed pass of its flip)."""
    bad = 0
    for lay, ref in zip(layouts(), references()):
        try:
            if reverse:
                rl = flip_layout(lay)
                check_run(run_windows(ops, rl, "cpu", reverse=True), ref, rl, reverse=True)
            else:
                check_run(run_windows(ops, lay, "cpu"), ref, lay)
        except AssertionError:
            bad += 1
    return bad


def test_sweep_reaches_every_window_edge():
    ls, refs = layouts(), references()
    assert len(ls) >= 100 and all(r["windows"] for r in refs)  # no layout without a window is generated
    assert {l.S for l in ls} == {2, 4, 6, 12} and {l.N for l in ls} == {1, 5, 9, 13} and {l.kind for l in ls} == {"random", "zero", "last"}
    total = sum((r["edges"] for r in refs), collections.Counter())
    print(f"{len(ls)} layouts: {dict(total)}")
    for edge in ("short_window", "carried", "entering_later", "masked_new_track", "unwritten_frames", "ragged_T"):
        assert total[edge] > 0, edge
    for r in refs:  # the stand-in's promises: logits within +-18, small integers
        assert float(r["logit"].abs().max()) <= 18.0 and float(r["traj"].abs().max()) < 2 ** 20
        assert torch.equal(r["traj"], r["traj"].round()) and torch.equal(r["logit"], r["logit"].round())


def test_reference_against_mock_and_rule():
    """The reference alone satisfies the sweep's assertions: with tests/hip_mock.py, and with the torch copy of the kernel rules
    that carries the probes, in place of the kernels."""
    assert failing_layouts(hip_mock) == 0
    assert failing_layouts(rule_ops()) == 0


def test_reference_reversed_against_rule():
    for lay in layouts():
        rl = flip_layout(lay)
        check_run(run_windows(rule_ops(), rl, "cpu", reverse=True), reference_loop(lay.qt, lay.qxyz, lay.feat, lay.S, lay.T), rl, reverse=True)
    assert failing_layouts(hip_mock, reverse=True) == 0


@pytest.mark.parametrize("bug", PROBES)
def test_window_probes_break_the_sweep(bug):
    """Each planted fault fails the sweep of its direction, and leaves the other direction's alone."""
    rev = bug in REVERSED_PROBES
    bad = failing_layouts(rule_ops(bug), reverse=rev)
    print(f"{bug}: {bad} of {len(layouts())} layouts fail the {'reversed' if rev else 'forward'} sweep")
    assert bad > 0
    if rev:
        assert failing_layouts(rule_ops(bug)) == 0


def fresh_outputs(f, N, dev):
    return [poison(f, N, 3, dev=dev, value=SENT), poison(f, N, dev=dev, value=SENT), poison(f, N, dev=dev, value=SENT)]


def check_chunks(store, mock_store, rec, run, lay, dev):
    """Chunk stores over partitions of the clip, side by side, are the whole-clip store of the run's pass (and what `mock_store`
    gives chunk by chunk); a chunk outside the window's frames stays at the sentinel."""
    S, T, N, w, fr0, p1 = lay.S, lay.T, lay.N, rec["w"], rec["f0"], rec["p1"]
    opts = dict(frame_step=run["step"], before=run["before"])
    mopts = dict(frame_step=run["step"], before=cpu(run["before"]))
    lo, hi = sorted((fr0, fr0 + run["step"] * (S - 1)))  # the window's frames, before the clip's ends cut them
    whole = fresh_outputs(T, N, dev)
    store(rec["out"], rec["lg"], run["order_d"], p1, S, fr0, T, N, *whole, **opts)
    for L in sorted({1, S // 2, S // 2 + 1, T}):
        parts, mocks = [], []
        for f0 in range(0, T, L):
            f1 = min(f0 + L, T)
            ch = fresh_outputs(f1 - f0, N, dev)
            store(rec["out"], rec["lg"], run["order_d"], p1, S, fr0, T, N, *ch, frames=(f0, f1), **opts)
            if f1 <= lo or f0 > hi:  # a chunk that does not meet the window: success, nothing written
                assert all(float((c - SENT).abs().max()) == 0.0 for c in ch), (lay[:4], w, f0, f1)
            parts.append(ch)
            if mock_store is not None:
                mk = fresh_outputs(f1 - f0, N, "cpu")
                mock_store(cpu(rec["out"]), cpu(rec["lg"]), cpu(run["order_d"]), p1, S, fr0, T, N, *mk, frames=(f0, f1), **mopts)
                mocks.append(mk)
        for k in range(3):
            side = torch.cat([p[k] for p in parts], 0)
            assert torch.equal(side, whole[k]), (lay[:4], w, L, k)
            if mocks:
                mside = torch.cat([m[k] for m in mocks], 0)
                if k < 2:
                    assert torch.equal(side.cpu(), mside), (lay[:4], w, L, k)
                else:
                    wrote = mside != SENT
                    check_prob(side, torch.cat([p[1] for p in parts], 0), wrote)
                    check_prob(mside, torch.cat([m[1] for m in mocks], 0), wrote)


def check_mapped(prepare, rec, run, lay, dev):
    """The carry map: the prefix form written as a map, then the window's rows permuted with the previous window's rows scattered
    over a larger, poisoned buffer, both against the prefix form's outputs in `rec`."""
    S, T = lay.S, lay.T
    fr0, p0, p1 = rec["f0"], rec["p0"], rec["p1"]
    g = gen("mapped", lay[:4], rec["w"])
    carry = torch.where(torch.arange(p1) < p0, torch.arange(p1), torch.full((p1,), -1)).int().to(dev)
    wc, wm, wf = poison(p1, S, 3, dev=dev), poison(p1, S, 2, dev=dev), poison(p1, S, CW, dev=dev)
    prepare(run["qxyz_s"], run["qt_d"], run["feat_s"], rec["prev_c"], rec["prev_v"], p1, 0, S, CW, fr0, T, wc, wm, wf, frame_step=run["step"],
            carry_src=carry)
    assert torch.equal(wc, rec["wc"]) and torch.equal(wm, rec["wm"]) and torch.equal(wf, rec["wf"]), (lay[:4], rec["w"])
    perm = torch.randperm(p1, generator=g)
    pos = torch.randperm(p0 + 2, generator=g)[:p0]
    prev_c = prev_v = None
    if p0:
        prev_c, prev_v = poison(p0 + 2, S, 3, dev=dev), poison(p0 + 2, S, dev=dev)
        prev_c[pos.to(dev)] = rec["prev_c"]
        prev_v[pos.to(dev)] = rec["prev_v"]
    carry = torch.tensor([int(pos[r]) if r < p0 else -1 for r in perm.tolist()], dtype=torch.int32).to(dev)
    pd = perm.to(dev)
    wc, wm, wf = poison(p1, S, 3, dev=dev), poison(p1, S, 2, dev=dev), poison(p1, S, CW, dev=dev)
    prepare(run["qxyz_s"][pd].contiguous(), run["qt_d"][pd].contiguous(), run["feat_s"][pd].contiguous(), prev_c, prev_v, p1, 0, S, CW, fr0, T,
            wc, wm, wf, frame_step=run["step"], carry_src=carry)
    assert torch.equal(wc, rec["wc"][pd]) and torch.equal(wm, rec["wm"][pd]) and torch.equal(wf, rec["wf"][pd]), (lay[:4], rec["w"])


def check_before_forward(store, rec, run, lay, dev):
    """A per-row frame bound on the forward store: `rule_store`'s result, which is the unbounded store with every caller column
    put back to the sentinel from its row's bound on."""
    S, T, N, w, p1 = lay.S, lay.T, lay.N, rec["w"], rec["p1"]
    before = torch.randint(0, T + 2, (p1,), generator=gen("before", lay[:4], w)).int().to(dev)
    before[0] = w + S // 2  # a bound inside the window whatever the draw
    got, want, free = fresh_outputs(T, N, dev), fresh_outputs(T, N, dev), fresh_outputs(T, N, dev)
    store(rec["out"], rec["lg"], run["order_d"], p1, S, w, T, N, *got, before=before)
    rule_store(rec["out"], rec["lg"], run["order_d"], p1, S, w, T, N, *want, before=before)
    rule_store(rec["out"], rec["lg"], run["order_d"], p1, S, w, T, N, *free)
    bound = torch.zeros(N, dtype=torch.long, device=dev)
    bound[run["order_d"][:p1]] = before.long()
    cut = torch.arange(T, device=dev)[:, None] >= bound[None, :]
    free[0][cut], free[1][cut] = SENT, SENT
    assert torch.equal(want[0], free[0]) and torch.equal(want[1], free[1]), (lay[:4], w)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (lay[:4], w)
    wrote = (want[1] != SENT).cpu()
    assert bool(wrote.any()) == bool((before.long() > w).any())
    check_prob(got[2], got[1], wrote)


def cpu_runs(ops, reverse, every=7):
    """(layout, run) of every `every`-th sweep layout on the CPU; reverse: the reversed pass of the flipped layout."""
    for lay in layouts()[::every]:
        lay = flip_layout(lay) if reverse else lay
        yield lay, run_windows(ops, lay, "cpu", reverse=reverse)


def test_mock_ring_chunk_against_mock_store():
    """hip_mock.window_store with `frames` over a partition of the clip lays out its whole-clip result, and the kernel rule's chunk
    by chunk (what the GPU tests assert of the kernels, here of the stand-ins alone), forwards and on the reversed sweep."""
    for reverse in (False, True):
        for lay, run in cpu_runs(hip_mock, reverse):
            for rec in run["recs"]:
                check_chunks(hip_mock.window_store, None, rec, run, lay, "cpu")
                check_chunks(rule_ops().window_store, hip_mock.window_store, rec, run, lay, "cpu")


def test_carry_map_against_rule_and_mock():
    """The carry-map cases of test_window_prepare_mapped on the stand-ins alone, forwards and on the reversed sweep."""
    for ops in (rule_ops(), hip_mock):
        for reverse in (False, True):
            for lay, run in cpu_runs(ops, reverse):
                for rec in run["recs"]:
                    check_mapped(ops.window_prepare, rec, run, lay, "cpu")


def test_before_forward_against_rule_and_mock():
    for ops in (rule_ops(), hip_mock):
        for lay, run in cpu_runs(ops, False):
            for rec in run["recs"]:
                check_before_forward(ops.window_store, rec, run, lay, "cpu")


def device_ops():
    from mvtracker_amd import hip
    return types.SimpleNamespace(window_prepare=lambda *a, **k: hip.window_prepare(*a, **k), window_store=lambda *a, **k: hip.window_store(*a, **k))


@functools.lru_cache(maxsize=None)
def device_runs(reverse=False):
    """The sweep on the device; reverse: the reversed pass of every flipped layout (the reference is the unflipped layout's)."""
    runs = [run_windows(device_ops(), flip_layout(lay) if reverse else lay, DEV, reverse=reverse) for lay in layouts()]
    torch.cuda.synchronize()
    return runs


@gpu
def test_window_sweep(hip):
    for lay, run, ref in zip(layouts(), device_runs(), references()):
        check_run(run, ref, lay)


@gpu
def test_window_mock_conformity(hip):
    for lay, run in zip(layouts(), device_runs()):
        S, T, N = lay.S, lay.T, lay.N
        for rec in run["recs"]:
            w, p0, p1 = rec["w"], rec["p0"], rec["p1"]
            wc, wm, wf = poison(p1, S, 3), poison(p1, S, 2), poison(p1, S, CW)
            hip_mock.window_prepare(cpu(run["qxyz_s"]), cpu(run["qt_d"]), cpu(run["feat_s"]), cpu(rec["prev_c"]), cpu(rec["prev_v"]), p1, p0,
                                    S, CW, w, T, wc, wm, wf)
            assert torch.equal(wc, rec["wc"].cpu()) and torch.equal(wm, rec["wm"].cpu()) and torch.equal(wf, rec["wf"].cpu()), (lay[:4], w)
            dv, mk = fresh_outputs(T, N, DEV), fresh_outputs(T, N, "cpu")
            hip.window_store(rec["out"], rec["lg"], run["order_d"], p1, S, w, T, N, *dv)
            hip_mock.window_store(cpu(rec["out"]), cpu(rec["lg"]), cpu(run["order_d"]), p1, S, w, T, N, *mk)
            assert torch.equal(dv[0].cpu(), mk[0]) and torch.equal(dv[1].cpu(), mk[1]), (lay[:4], w)
            wrote = mk[1] != SENT
            check_prob(dv[2], dv[1], wrote)
            check_prob(mk[2], mk[1], wrote)


@gpu
def test_window_store_chunk(hip):
    for lay, run in zip(layouts(), device_runs()):
        for rec in run["recs"]:
            check_chunks(device_ops().window_store, hip_mock.window_store, rec, run, lay, DEV)


@gpu
def test_window_store_chunk_reversed(hip):
    """Reversed chunks: on the reversed sweep, chunk stores over the same partitions equal the whole-clip reversed store."""
    for lay, run in zip(layouts(), device_runs(reverse=True)):
        for rec in run["recs"]:
            check_chunks(device_ops().window_store, hip_mock.window_store, rec, run, flip_layout(lay), DEV)


@gpu
def test_window_prepare_mapped(hip):
    for lay, run in zip(layouts(), device_runs()):
        for rec in run["recs"]:
            check_mapped(device_ops().window_prepare, rec, run, lay, DEV)


@gpu
def test_window_prepare_mapped_reversed(hip):
    """Reversed carry map: the cases of test_window_prepare_mapped on the reversed sweep."""
    for lay, run in zip(layouts(), device_runs(reverse=True)):
        for rec in run["recs"]:
            check_mapped(device_ops().window_prepare, rec, run, flip_layout(lay), DEV)


@gpu
def test_window_store_before_forward(hip):
    """`before` with frame_step = +1, against rule_store."""
    for lay, run in zip(layouts(), device_runs()):
        for rec in run["recs"]:
            check_before_forward(device_ops().window_store, rec, run, lay, DEV)


@gpu
def test_window_sweep_reversed(hip):
    for lay, run, ref in zip(layouts(), device_runs(reverse=True), references()):
        check_run(run, ref, flip_layout(lay), reverse=True)


@gpu
def test_window_entries_refuse_bad_arguments(hip):
    """frame_step = 0, a carry map together with a carried prefix, and a chunk past the clip's end: return code 1, nothing launched,
    nothing written.  The same calls with the argument put right are accepted."""
    n, p0, S, T, w = 5, 2, 4, 9, 3
    g = gen("refuse")
    qxyz, feat, qt = G(ints(g, -9, 9, n, 3)), G(ints(g, -3, 3, n, CW)), torch.tensor([0, 1, 3, 4, 5], dtype=torch.int32, device=DEV)
    prev_c, prev_v = G(ints(g, -99, 99, p0, S, 3)), G(ints(g, -18, 18, p0, S))
    carry = torch.tensor([0, 1, -1, -1, -1], dtype=torch.int32, device=DEV)
    coords, vis, order = G(ints(g, -99, 99, n, S, 3)), G(ints(g, -18, 18, n, S)), torch.randperm(n, generator=g).to(DEV)

    def prepare(outs, p0=0, **kw):
        hip.window_prepare(qxyz, qt, feat, prev_c, prev_v, n, p0, S, CW, w, T, *outs, **kw)

    def store(outs, T_=T, **kw):
        hip.window_store(coords, vis, order, n, S, w, T_, n, *outs, **kw)

    good = [poison(n, S, 3, dev=DEV), poison(n, S, 2, dev=DEV), poison(n, S, CW, dev=DEV)]
    prepare(good, carry_src=carry)
    stored = fresh_outputs(2, n, DEV)
    store(stored, frames=(w, w + 2))
    torch.cuda.synchronize()
    assert not any(bool(torch.isnan(b).any()) for b in good) and not any(bool((b == SENT).any()) for b in stored)
    bad = [poison(n, S, 3, dev=DEV), poison(n, S, 2, dev=DEV), poison(n, S, CW, dev=DEV)]
    kept = fresh_outputs(2, n, DEV)
    for call in (lambda: prepare(bad, p0=p0, frame_step=0), lambda: prepare(bad, p0=p0, carry_src=carry),
                 lambda: store(kept, frame_step=0, frames=(w, w + 2)), lambda: store(kept, T_=w + 1, frames=(w, w + 2))):
        with pytest.raises(hip.HipError, match="arguments rejected"):
            call()
    torch.cuda.synchronize()
    assert all(untouched(b) for b in bad) and all(bool((b == SENT).all()) for b in kept)


@gpu
def test_window_prepare_grid_stride(hip):
    """n * S * C / 4 above the 256 * 32 blocks of 256 threads: every thread takes a second element."""
    n, p0, S, Cc, w, T = 6000, 2900, 12, 128, 29, 37  # a short window: T - w = 8 < S
    assert n * S * Cc // 4 > 256 * 32 * 256
    g = gen("prepare_grid")
    qt = torch.sort(torch.cat([torch.randint(0, w + S // 2, (p0,), generator=g), torch.randint(w, T + 3, (n - p0,), generator=g)])).values.int().to(DEV)
    qxyz, feat = G(ints(g, -9, 9, n, 3)), G(ints(g, -3, 3, n, Cc))
    prev_c, prev_v = G(ints(g, -99, 99, p0, S, 3)), G(ints(g, -18, 18, p0, S))
    got = [poison(n + 1, S, 3, dev=DEV), poison(n + 1, S, 2, dev=DEV), poison(n + 1, S, Cc, dev=DEV)]
    want = [t.clone() for t in got]
    hip.window_prepare(qxyz, qt, feat, prev_c, prev_v, n, p0, S, Cc, w, T, *got)
    rule_prepare(qxyz, qt, feat, prev_c, prev_v, n, p0, S, Cc, w, T, *want)
    for a, b in zip(got, want):
        assert torch.equal(a[:n], b[:n]) and untouched(a[n:])


@gpu
def test_window_store_grid_stride(hip):
    n, S, T, w = 180000, 12, 18, 3
    assert n * min(S, T - w) > 256 * 32 * 256
    g = gen("store_grid")
    order = torch.randperm(n, generator=g).to(DEV)
    coords, vis = G(ints(g, -99, 99, n, S, 3)), G(ints(g, -18, 18, n, S))
    got, want = fresh_outputs(T, n, DEV), fresh_outputs(T, n, DEV)
    hip.window_store(coords, vis, order, n, S, w, T, n, *got)
    rule_store(coords, vis, order, n, S, w, T, n, *want)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    wrote = (want[1] != SENT).cpu()
    assert int(wrote.sum()) == n * S and not bool(wrote[:w].any())
    check_prob(got[2], got[1], wrote)


# ================================================================== B: the row kernels of tokens.hip

ROWS = (1, 5, 1000)
LN_C = (1, 2, 63, 64, 65, 255, 256, 384, 511, 512)


def balanced_rows(g, rows, C):
    """Rows m +- c, integer m in [-16, 16], c in [1, 8]: half the signs negative, for odd C one entry equal to m.  Every partial
    sum is an integer below 2^24, so sum, mean (= m) and the centred values (+-c, 0) are exact in any order."""
    m, c = ints(g, -16, 16, rows, 1), ints(g, 1, 8, rows, 1)
    pattern = torch.cat([torch.ones(C // 2), -torch.ones(C // 2), torch.zeros(C % 2)])
    sign = pattern[torch.rand(rows, C, generator=g).argsort(1)]
    x = m + c * sign
    assert torch.equal(x.double().mean(1, keepdim=True), m.double()) and torch.equal(x.sum(1, keepdim=True) / C, m)
    return x


def norm_case(rows, C, eps, affine, tag="ln"):
    """x, w, b, the fp64 reference and the bar; the reference-side claims are asserted here, before any device result is looked at."""
    g = gen(tag, rows, C, eps, affine)
    x = balanced_rows(g, rows, C)
    w, b = (ints(g, -8, 8, C), ints(g, -8, 8, C)) if affine else (None, None)
    if tag == "gn":  # one group over the C channels of a row (the update head's GroupNorm(1, C))
        ref = F.group_norm(x.double(), 1, w.double(), b.double(), eps)
    else:
        ref = F.layer_norm(x.double(), (C,), None if w is None else w.double(), None if b is None else b.double(), eps)
    bar = 32 * ULP * ((w.abs() + b.abs()) if affine else torch.ones(C)).double()
    two_pass = (layernorm_two_pass(x, w, b, eps).double() - ref).abs()
    assert bool((two_pass <= bar / 4).all()), (rows, C, eps, affine)
    return x, w, b, ref, bar


def layernorm_two_pass(x, w, b, eps):
    """layernorm_kernel's arithmetic in fp32 torch: mean, then the centred sum of squares, 1 / sqrt, scale and shift."""
    C = x.shape[1]
    d = x - x.sum(1, keepdim=True) / C
    o = d * (1.0 / torch.sqrt((d * d).sum(1, keepdim=True) / C + torch.tensor(eps, dtype=torch.float32)))
    return o if w is None else o * w + b


def padded(x, ld, guard_rows=1):
    """x (rows, C) inside a poisoned (rows + guard, ld) buffer."""
    buf = poison(x.shape[0] + guard_rows, ld)
    buf[:x.shape[0], :x.shape[1]] = x
    return buf


def check_padded(buf, rows, C):
    """The pad columns and the guard row of a poisoned (rows + 1, ld) output."""
    assert untouched(buf[:rows, C:]) and untouched(buf[rows:])


def test_norm_reference_claims():
    """Exact means and the two-pass fp32 emulation inside a quarter of the bar (both asserted in norm_case); torch's own fp32 CPU
    LayerNorm, whose one-pass moments lose bits on the rows with |m| = 16, c = 1 (1.56 of the bar there), is only reported."""
    worst = 0.0
    for C in LN_C:
        for rows in ROWS:
            for eps in (1e-5, 1e-6):
                for affine in (True, False):
                    x, w, b, ref, bar = norm_case(rows, C, eps, affine)
                    err = (F.layer_norm(x, (C,), w, b, eps).double() - ref).abs()
                    worst = max(worst, float((err / bar.clamp(min=1e-30))[:, bar > 0].max()))
    print(f"torch fp32 CPU LayerNorm: worst error / bar {worst:.2f}")
    # the bar separates a column dropped from the statistics at C = 512
    x, w, b, ref, bar = norm_case(5, 512, 1e-5, True)
    xd = x.double()
    mean = xd[:, :511].mean(1, keepdim=True)
    var = ((xd[:, :511] - mean) ** 2).mean(1, keepdim=True)
    wrong = (xd - mean) / torch.sqrt(var + 1e-5) * w.double() + b.double()
    assert bool(((wrong - ref).abs() > 100 * bar)[:, w != 0].any())


@gpu
@pytest.mark.parametrize("C", LN_C)
def test_layernorm(hip, C):
    for rows in ROWS:
        for eps in (1e-5, 1e-6):
            for affine in (True, False):
                x, w, b, ref, bar = norm_case(rows, C, eps, affine)
                ldx, ldy = C + 3, C + 5
                y = poison(rows + 1, ldy, dev=DEV)
                hip.layernorm(G(padded(x, ldx)), ldx, G(w), G(b), y, ldy, rows, C, eps)
                y = y.cpu()
                err = (y[:rows, :C].double() - ref).abs()
                print(f"layernorm rows {rows} C {C} eps {eps} affine {affine}: max err / bar {float((err / bar.clamp(min=1e-30)).max()):.3f}")
                assert bool((err <= bar).all()), (rows, C, eps, affine)
                check_padded(y, rows, C)


DS_C = (64, 96, 128, 255, 256)  # (C = 1 is degenerate in the reference: F.group_norm refuses a single value per group)


@gpu
@pytest.mark.parametrize("C", DS_C)
def test_delta_split(hip, C):
    for rows in ROWS:
        for pad in (0, 5):
            x, gw, gb, ref, bar = norm_case(rows, C, 1e-5, True, tag="gn")
            g = gen("delta", rows, C, pad)
            ldd = 3 + C + pad
            step, c0 = ints(g, -50, 50, rows, 3), ints(g, -1000, 1000, rows, 3)
            delta = padded(torch.cat([step, x], 1), ldd)
            coords, dn = poison(rows + 1, 3, dev=DEV), poison(rows + 1, C, dev=DEV)
            coords[:rows] = G(c0)
            flag = torch.zeros(1, dtype=torch.int32, device=DEV)
            hip.delta_split(G(delta), ldd, G(gw), G(gb), coords, dn, rows, C, flag)
            assert torch.equal(coords[:rows].cpu(), c0 + step) and untouched(coords[rows:])
            assert bool(((dn[:rows].cpu().double() - ref).abs() <= bar).all()) and untouched(dn[rows:]), (rows, C, pad)
            assert int(flag) == 0


@gpu
def test_delta_split_nan_flag(hip):
    rows, C = 5, 64
    x, gw, gb, _, _ = norm_case(rows, C, 1e-5, True, tag="gn")
    g = gen("delta_nan")
    base = torch.cat([ints(g, -50, 50, rows, 3), x], 1)

    def run(r, c, with_flag=True):
        delta = base.clone()
        delta[r, c] = NAN
        coords, dn = G(ints(g, -9, 9, rows, 3)), poison(rows, C, dev=DEV)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV) if with_flag else None
        hip.delta_split(G(delta), 3 + C, G(gw), G(gb), coords, dn, rows, C, flag)
        torch.cuda.synchronize()
        return None if flag is None else int(flag)

    for col in range(3):
        assert run(2, col) == 1
    assert run(2, 3) == 0 and run(0, 3 + C - 1) == 0  # a NaN in a feature column is not the coordinate guard's
    assert run(rows - 1, 0) == 1  # the last row of a block of four with one row only
    assert run(2, 0, with_flag=False) is None


RD_C = (1, 63, 64, 65, 128, 384)


def rowdot_case(rows, C, bias):
    g = gen("rowdot", rows, C, bias)
    x, w = ints(g, -8, 8, rows, C), ints(g, -8, 8, C)
    b = ints(g, -100, 100, 1) if bias else None
    ref = x.double() @ w.double() + (b.double() if bias else 0.0)
    assert float((x.abs().double() @ w.abs().double()).max()) + 100 < 2 ** 24
    return x, w, b, ref


def test_mock_rowdot_without_bias():
    for C in RD_C:
        for bias in (True, False):
            x, w, b, ref = rowdot_case(5, C, bias)
            out = poison(6)
            hip_mock.rowdot(padded(x, C + 3), C + 3, w, b, out, 5, C)
            assert torch.equal(out[:5].double(), ref) and untouched(out[5:])


@gpu
@pytest.mark.parametrize("C", RD_C)
def test_rowdot(hip, C):
    for rows in ROWS:
        for bias in (True, False):
            x, w, b, ref = rowdot_case(rows, C, bias)
            ldx = C + 3
            out = poison(rows + 1, dev=DEV)
            hip.rowdot(G(padded(x, ldx)), ldx, G(w), G(b), out, rows, C)
            assert torch.equal(out[:rows].cpu().double(), ref) and untouched(out[rows:]), (rows, C, bias)


@gpu
@pytest.mark.parametrize("S", [1, 12])
@pytest.mark.parametrize("C", [7, 128])
def test_broadcast_rows(hip, C, S):
    n, ld = 5, C + 3
    v = ints(gen("bcast", C, S), -99, 99, n, C)
    x = poison(n * S + 1, ld, dev=DEV)
    hip.broadcast_rows(G(v), x, ld, n, S, C)
    x = x.cpu()
    assert torch.equal(x[:n * S, :C].reshape(n, S, C), v[:, None, :].expand(n, S, C))
    check_padded(x, n * S, C)
    for reps in (1, 3):
        x = poison(reps * n * S + 1, ld, dev=DEV)
        hip.broadcast_rows_repeat(G(v), x, ld, n, S, C, reps)
        x = x.cpu()
        assert torch.equal(x[:reps * n * S, :C].reshape(reps, n, S, C), v[None, :, None, :].expand(reps, n, S, C))
        check_padded(x, reps * n * S, C)


def token_case(E, Fc, C, S, flows):
    N = 3
    D = 3 * E + 3 + Fc + C + 2
    g = gen("tokens", E, Fc, C, S, flows)
    c0 = ints(g, -20, 20, N, 1, 3)
    coords = c0.repeat(1, S, 1)
    if flows:
        coords = coords + ints(g, -6, 6, N, S, 3)
    fcorr, ffeats, mv = ints(g, -9, 9, N, S, Fc), ints(g, -9, 9, N, S, C), ints(g, -9, 9, N, S, 2)
    pos, te = ints(g, -4, 4, N, D), ints(g, -4, 4, S, D)
    sincos = torch.zeros(N, S, 3 * E)
    sincos[..., 1::2] = 1.0  # sin(0) at the even columns, cos(0) at the odd ones (E is even)
    ref = (torch.cat([sincos, coords - coords[:, :1], fcorr, ffeats, mv], 2).double() + pos[:, None].double()) + te[None].double()
    return N, D, coords, fcorr, ffeats, mv, pos, te, ref.reshape(N * S, D)


@gpu
@pytest.mark.parametrize("S", [1, 12])
@pytest.mark.parametrize("pad", [0, 3, 300])
@pytest.mark.parametrize("dims", [(64, 256, 128), (4, 5, 12), (2, 1, 4)])
def test_token_assemble(hip, dims, pad, S):
    E, Fc, C = dims
    for flows in (False, True):
        N, D, coords, fcorr, ffeats, mv, pos, te, ref = token_case(E, Fc, C, S, flows)
        ldx = D + pad
        x = poison(N * S + 1, ldx, dev=DEV)
        hip.token_assemble(G(coords), G(fcorr), Fc, G(ffeats), C, G(mv), G(pos), G(te), N, S, E, x, ldx)
        x = x.cpu()
        lo = 3 * E if flows else 0  # integer flows: the flow columns and everything after them (the sinusoids have their fixture test)
        assert torch.equal(x[:N * S, lo:D].double(), ref[:, lo:]), (dims, pad, S, flows)
        assert not bool(torch.isnan(x[:N * S, :D]).any())
        assert torch.equal(x[:N * S, D:], torch.zeros(N * S, pad)) and untouched(x[N * S:])  # exact zeros on every pad column


def pos_layout(N, D, dim_padded):
    A = dim_padded // 3
    one_axis = torch.cat([torch.zeros(A // 2), torch.ones(A // 2)])  # sin(0) | cos(0)
    return one_axis.repeat(3)[:D][None, :].expand(N, D)


def omega_table(dim_padded):
    om = np.arange(dim_padded // 6, dtype=np.float64)
    om /= (dim_padded // 3) / 2.0
    return torch.from_numpy(1.0 / 10000 ** om)


@gpu
@pytest.mark.parametrize("dims", [(581, 582), (7, 12), (12, 12)])
def test_pos_embed_zero(hip, dims):
    D, dim_padded = dims
    for N, S in ((1, 1), (5, 12), (1000, 2)):
        coords = poison(N, S, 3)
        coords[:, 0] = 0.0  # only slot 0 of a track is read
        for omega in (G(omega_table(dim_padded)), None):
            pos = poison(N + 1, D, dev=DEV)
            hip.pos_embed(G(coords), N, S, D, dim_padded, pos, omega)
            assert torch.equal(pos[:N].cpu(), pos_layout(N, D, dim_padded)) and untouched(pos[N:]), (dims, N, S, omega is None)


@gpu
def test_pos_embed_omega_table_fixture(hip, golden):
    g = golden("embeddings")
    c0 = torch.from_numpy(g["coords0"]).float().reshape(-1, 3)
    n, S, D = c0.shape[0], 12, 581
    coords = c0[:, None, :].repeat(1, S, 1).contiguous()
    ref = g["pos_embed"].reshape(n, 582)[:, :D].astype(np.float32)
    for omega in (G(omega_table(582)), None):
        pos = poison(n + 1, D, dev=DEV)
        hip.pos_embed(G(coords), n, S, D, 582, pos, omega)
        assert np.abs(pos[:n].cpu().numpy() - ref).max() < 1.5e-7 and untouched(pos[n:])


# ================================================================== C: the frame-store kernels of pyramid.hip

@gpu
@pytest.mark.parametrize("shape", [(2, 3, 37, 53, 4), (3, 2, 64, 40, 8), (1, 1, 4, 4, 4)])
def test_depth_subsample(hip, shape):
    V, T, H, W, s = shape
    hs, ws = H // s, W // s
    depths = torch.randperm(V * T * H * W, generator=gen("depth", shape)).float().reshape(V, T, H, W)  # all distinct, exact
    out = poison(T * V * hs * ws + 7, dev=DEV)
    hip.depth_subsample(G(depths), out, V, T, H, W, s)
    want = depths[:, :, ::s, ::s][:, :, :hs, :ws].permute(1, 0, 2, 3)
    assert torch.equal(out[:-7].cpu().reshape(T, V, hs, ws), want) and untouched(out[-7:])


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(6, 9, 13, 8), (2, 2, 2, 16), (5, 16, 6, 128)])
def test_avgpool2(hip, shape, dtype):
    n, h, w, C = shape
    ho, wo = h // 2, w // 2
    x = 4.0 * ints(gen("pool", shape), -31, 31, n, h, w, C)  # multiples of 4 in [-124, 124]: the mean is an integer <= 124
    xd = x.double()[:, :2 * ho, :2 * wo]  # the odd last row and column are dropped
    want = (xd[:, 0::2, 0::2] + xd[:, 0::2, 1::2] + xd[:, 1::2, 0::2] + xd[:, 1::2, 1::2]) / 4
    assert torch.equal(want, want.round()) and float(want.abs().max()) <= 124
    assert torch.equal(want, F.avg_pool2d(x.double().permute(0, 3, 1, 2), 2, stride=2).permute(0, 2, 3, 1))
    out = poison(n * ho * wo * C + 16, dev=DEV, dtype=dtype)
    hip.avgpool2(G(x.to(dtype)), out, n, h, w, C)
    assert torch.equal(out[:-16].cpu().double().reshape(n, ho, wo, C), want) and untouched(out[-16:])


def exact_cameras(g, n):
    """K = [[2^a, 0, cx], [0, 2^b, cy], [0, 0, 1]] with integer cx, cy; [R | t] a signed permutation with an integer translation:
    both inverses are exact."""
    K = torch.zeros(n, 3, 3)
    K[:, 0, 0] = 2.0 ** ints(g, 0, 4, n)
    K[:, 1, 1] = 2.0 ** ints(g, 0, 4, n)
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = ints(g, -8, 8, n), ints(g, -8, 8, n), 1.0
    E = torch.zeros(n, 3, 4)
    for i in range(n):
        E[i, torch.arange(3), torch.randperm(3, generator=g)] = ints(g, 0, 1, 3) * 2 - 1
    E[:, :, 3] = ints(g, -20, 20, n, 3)
    return K, E


def exact_inverses(K, E):
    n = K.shape[0]
    # LU leaves 1e-15 on some entries of the fp64 inverses; the true ones are multiples of 2^-4 / integers, and the products below
    # prove that the rounded matrices are the inverses, exactly
    kinv = (torch.inverse(K.double()) * 16).round() / 16
    sq = torch.eye(4, dtype=torch.float64).repeat(n, 1, 1)
    sq[:, :3] = E.double()
    einv = torch.inverse(sq).round()
    assert torch.equal(K.double() @ kinv, torch.eye(3, dtype=torch.float64).expand(n, 3, 3))  # exact, not merely close
    assert torch.equal(sq @ einv, torch.eye(4, dtype=torch.float64).expand(n, 4, 4))
    assert torch.equal(kinv.float().double(), kinv) and torch.equal(einv.float().double(), einv)
    return kinv.contiguous(), einv[:, :3].contiguous()  # (torch.inverse returns column-major matrices)


def test_exact_cameras_claim():
    for n in (1, 6, 65):
        exact_inverses(*exact_cameras(gen("cams", n), n))


@gpu
@pytest.mark.parametrize("n", [1, 6, 65])
def test_invert_cameras(hip, n):
    K, E = exact_cameras(gen("cams", n), n)
    kinv, einv = exact_inverses(K, E)
    ko, eo = poison(n + 1, 9, dev=DEV), poison(n + 1, 12, dev=DEV)
    hip.invert_cameras(G(K), G(E), ko, eo, n)
    assert torch.equal(ko[:n].cpu().double(), kinv.reshape(n, 9)) and untouched(ko[n:])
    assert torch.equal(eo[:n].cpu().double(), einv.reshape(n, 12)) and untouched(eo[n:])


UNPROJECT = (2, 3, 9, 13, 4)  # V, T, hs, ws, stride


@functools.lru_cache(maxsize=None)
def unproject_inputs():
    V, T, hs, ws, stride = UNPROJECT
    g = gen("unproject")
    K, E = exact_cameras(g, V * T)  # camera (v, t) at row v * T + t, all different
    assert len({tuple(k.reshape(-1).tolist()) + tuple(e.reshape(-1).tolist()) for k, e in zip(K, E)}) == V * T
    kinv, einv = exact_inverses(K, E)
    # multiples of 0.25 up to 16: only 65 values for 702 cells, so "distinct" means any two cells of the store less than 65 apart
    # differ (a stride coprime to 65 through the values), which every row, column, level and image offset of an image is; some zeros
    i = torch.arange(T * V * hs * ws)
    depth = (0.25 * ((i * 23 + 5) % 65).float()).reshape(T, V, hs, ws)
    assert int((depth == 0).sum()) > 0 and float(depth.max()) == 16.0
    return kinv.float(), einv.float(), depth


def unproject_rule(kinv, einv, depth, level, bug=None):
    """unproject_kernel's indexing in fp64 torch: (T, V, h, w, 4).  The arithmetic is that of common.h / model_utils.py:462-466."""
    V, T, hs, ws, stride = UNPROJECT
    f = 1 << level
    h, w = (ws >> level, hs >> level) if bug == "hw_swapped" else (hs >> level, ws >> level)
    st = float(stride * f)
    out = torch.zeros(T, V, h, w, 4, dtype=torch.float64)
    flat = depth.reshape(-1).double()
    Kd, Ed = kinv.double().reshape(-1, 3, 3), einv.double().reshape(-1, 3, 4)
    y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    pix = torch.stack([(x + 0.5) * st - 0.5, (y + 0.5) * st - 0.5, torch.ones(h, w, dtype=torch.float64)], -1).double()
    ff = 1 if bug == "level_offset" else f
    for t in range(T):
        for v in range(V):
            cam = t * V + v if bug == "vt_swapped" else v * T + t
            d = flat[(((t * V + v) * hs + y * ff) * ws + x * ff).clamp(max=flat.numel() - 1)]
            ray = torch.einsum("ij,hwj->hwi", Kd[cam], pix) * d[..., None]
            out[t, v, :, :, :3] = torch.einsum("ij,hwj->hwi", Ed[cam, :, :3], ray) + Ed[cam, :, 3]
    return out


def unproject_reference(kinv, einv, depth, level):
    """The fp64 formula with the reference's own slicing (no flat index): depth[t, v, ::f, ::f][:h, :w]."""
    V, T, hs, ws, stride = UNPROJECT
    f = 1 << level
    h, w = hs >> level, ws >> level
    d = depth.double()[:, :, ::f, ::f][:, :, :h, :w]
    st = float(stride * f)
    gy, gx = torch.meshgrid((torch.arange(h).double() + 0.5) * st - 0.5, (torch.arange(w).double() + 0.5) * st - 0.5, indexing="ij")
    pix = torch.stack([gx, gy, torch.ones_like(gx)], -1)
    Kd = kinv.double().reshape(V, T, 3, 3).permute(1, 0, 2, 3)
    Ed = einv.double().reshape(V, T, 3, 4).permute(1, 0, 2, 3)
    cam = torch.einsum("tvij,hwj->tvhwi", Kd, pix) * d[..., None]
    world = torch.einsum("tvij,tvhwj->tvhwi", Ed[..., :3], cam) + Ed[:, :, None, None, :, 3]
    out = torch.cat([world, torch.zeros_like(world[..., :1])], -1)
    assert torch.equal(out.float().double(), out)  # the fp64 result is its own fp32 rounding: every product and sum is exact
    return out


@pytest.mark.parametrize("level", [0, 1, 2])
def test_unproject_rule_and_probes(level):
    kinv, einv, depth = unproject_inputs()
    ref = unproject_reference(kinv, einv, depth, level)
    assert torch.equal(unproject_rule(kinv, einv, depth, level), ref)
    for bug in ("hw_swapped", "vt_swapped") + (("level_offset",) if level else ()):
        assert not torch.equal(unproject_rule(kinv, einv, depth, level, bug).reshape(-1), ref.reshape(-1)), bug
    mock = poison(ref.numel())
    hip_mock.unproject(depth, kinv, einv, mock, *UNPROJECT, level)
    assert torch.equal(mock.double().reshape(ref.shape), ref)


@gpu
@pytest.mark.parametrize("level", [0, 1, 2])
def test_unproject(hip, level):
    V, T, hs, ws, stride = UNPROJECT
    kinv, einv, depth = unproject_inputs()
    ref = unproject_reference(kinv, einv, depth, level)
    xyz = poison(ref.numel() + 4, dev=DEV)
    assert kinv.is_contiguous() and einv.is_contiguous() and depth.is_contiguous()
    hip.unproject(G(depth), G(kinv), G(einv), xyz, V, T, hs, ws, stride, level)
    assert torch.equal(xyz[:-4].cpu().double().reshape(ref.shape), ref) and untouched(xyz[-4:])
    assert float(xyz[:-4].reshape(-1, 4)[:, 3].abs().max()) == 0.0
