"""Streaming sessions on the host: the scheduler as a pure function (numpy), the ring slot arithmetic, and a whole session on
the mocked kernels (tests/hip_mock.py + tests/hip_mock_ring.py) against the mocked ``forward`` and the reference's fixtures."""
import numpy as np
import pytest
import torch

from mvtracker_amd import synth
from mvtracker_amd.backward import window_prefixes
from mvtracker_amd.streaming import StreamSchedule
from mvtracker_amd.tracker import MVTracker

import hip_mock_ring


def T(a):
    return torch.from_numpy(np.asarray(a))


# ------------------------------------------------------------------ scheduler
def run_schedule(rng, S, Tn, qt, ring_blocks=3):
    """Drive a StreamSchedule over a clip of Tn frames with random block sizes.  One query opens the session; each of the others
    is added at a random legal time: at the latest right before the push that delivers its frame (a window run in a push that ends
    at frame e starts at or before e - S + 1 and admits t <= e; before the first window, frame t would be skipped in that push).
    Returns (schedule, windows run, emitted ranges)."""
    qt = list(qt)
    rng.shuffle(qt)
    rest = qt[1:]
    sc = StreamSchedule(S, ring_blocks)
    sc.add_queries(qt[:1])
    wins, frames = [], []
    done = 0
    while done < Tn:
        b = min(int(rng.integers(1, 2 * S)), Tn - done)
        now = [t for t in rest if t < done + b or rng.random() < 0.3]
        for t in now:
            rest.remove(t)
            sc.add_queries([t])
        ops, fr = sc.push(b)
        done += b
        for op in ops:
            if op[0] == "encode":
                _, i0, i1, g = op
                assert 0 <= i0 < i1 <= b and g == done - b + i0
                # contiguous in the ring: never across a block boundary, never past the ring's end
                assert (g - sc.base) // sc.half == (g + i1 - i0 - 1 - sc.base) // sc.half
                assert sc.slot(g) + (i1 - i0) <= sc.R
            else:
                _, w, p1, hi = op
                assert hi - w < sc.R and hi >= w + S - 1
                wins.append((w, p1))
        frames.append(fr)
    for t in rest:  # (query frames at or beyond the clip's end)
        sc.add_queries([t])
    ops, fr = sc.finish()
    for op in ops:
        assert op[0] == "window" and op[3] == Tn - 1 and op[3] - op[1] < sc.R
        wins.append(op[1:3])
    frames.append(fr)
    return sc, wins, frames


def test_scheduler_matches_the_window_loop_for_any_schedule():
    rng = np.random.default_rng(0)
    for case in range(400):
        S = int(rng.choice([8, 12, 16]))
        Tn = int(rng.integers(1, 5 * S + 1))
        nq = int(rng.integers(1, 9))
        qt = rng.integers(0, Tn + 3, nq)  # (a few at or beyond the clip's end: never admitted, as in ``forward``)
        sc, wins, frames = run_schedule(rng, S, Tn, qt, ring_blocks=int(rng.choice([3, 4, 6])))
        assert sorted(sc.qt.tolist()) == sorted(qt.tolist())
        assert wins == window_prefixes(np.sort(qt), S, Tn), (case, S, Tn, qt)
        assert wins == sc.windows
        # the emitted ranges tile [0, Tn) exactly once
        assert frames[0][0] == 0 and frames[-1][1] == Tn
        for (a0, b0), (a1, b1) in zip(frames[:-1], frames[1:]):
            assert a0 <= b0 == a1 <= b1


def test_scheduler_latency_is_one_window():
    """With blocks of S/2 frames from frame 0 on, window w runs in the push that delivers frame w + S - 1 and frames [w, w + S/2)
    come back from it."""
    S = 12
    sc = StreamSchedule(S)
    sc.add_queries([0, 0, 3])
    got = [sc.push(6)[1] for _ in range(5)]
    assert got == [(0, 0), (0, 6), (6, 12), (12, 18), (18, 24)]
    assert sc.finish()[1] == (24, 30)


def test_add_queries_refuses_what_forward_would_have_treated_differently():
    S = 8
    sc = StreamSchedule(S)
    sc.add_queries([5])
    sc.push(3)  # frames 0..2 skipped (the first window starts at 5)
    with pytest.raises(ValueError, match="skipped"):
        sc.add_queries([2])
    sc.add_queries([3])  # not yet pushed: the first window now starts at 3
    sc.push(4)  # frames 3..6 stored
    with pytest.raises(ValueError, match="skipped"):
        sc.add_queries([1])
    sc.add_queries([4, 30])  # before the first window runs, anything from its start on is fine
    ops, fr = sc.push(4)  # frames 7..10: window 3 runs (frames 3..10)
    assert [op[1:3] for op in ops if op[0] == "window"] == [(3, 3)] and fr == (0, 7)
    with pytest.raises(ValueError, match="already run"):
        sc.add_queries([10])  # window 3 would have admitted t < 11
    n = len(sc.qt)
    with pytest.raises(ValueError):
        sc.add_queries([40, 10])  # one bad query refuses the whole call
    assert len(sc.qt) == n
    sc.add_queries([11])
    with pytest.raises(ValueError, match="negative"):
        sc.add_queries([-1])
    with pytest.raises(ValueError):
        StreamSchedule(8, ring_blocks=2)
    sc.finish()
    with pytest.raises(ValueError, match="finished"):
        sc.add_queries([50])
    with pytest.raises(ValueError, match="finished"):
        sc.push(1)


def test_ring_slot_arithmetic_against_a_linear_store():
    """Frames written block by block into ring slots (f - base) mod R and read back through the resident range of every window are
    the frames of a linear store; a block never wraps."""
    rng = np.random.default_rng(1)
    for S, blocks, base in ((8, 3, 0), (12, 3, 5), (12, 4, 7), (16, 5, 3)):
        sc = StreamSchedule(S, blocks)
        sc.add_queries([base])
        Tn = 6 * S + 3
        linear = torch.arange(Tn, dtype=torch.float32)[:, None].expand(Tn, 4).contiguous()
        ring = torch.full((sc.R, 4), -1.0)
        done = 0
        while done < Tn:
            b = min(int(rng.integers(1, S)), Tn - done)
            ops, _ = sc.push(b)
            for op in ops:
                if op[0] == "encode":
                    _, i0, i1, g = op
                    ring[sc.slot(g):sc.slot(g) + i1 - i0] = linear[g:g + i1 - i0]
                else:
                    _, w, p1, hi = op
                    r = (sc.base, sc.R, w, hi)
                    got = ring.index_select(0, hip_mock_ring.ring_slots(r))
                    assert torch.equal(got, linear[w:hi + 1])
                    for s in range(S):  # the kernels' slot rule, with off = base + ((lo - base) // R) * R and one conditional subtraction
                        f = min(max(w + s, w), hi)
                        off = sc.base + (w - sc.base) // sc.R * sc.R
                        slot = f - off
                        slot = slot - sc.R if slot >= sc.R else slot
                        assert 0 <= slot < sc.R and ring[slot, 0] == f
            done += b
        ops, _ = sc.finish()
        for _, w, p1, hi in ops:
            assert hi == Tn - 1 and torch.equal(ring.index_select(0, hip_mock_ring.ring_slots((sc.base, sc.R, w, hi))), linear[w:Tn])


def test_frames_of_a_count_and_of_a_ring():
    """What the slot-mapped wrappers accept where T stands: a frame count is the ring (0, T, 0, T-1), a ring passes through,
    anything else is refused."""
    from mvtracker_amd import hip
    assert hip._frames(12) == (0, 12, 0, 11) and hip._frames(1) == (0, 1, 0, 0) and hip._frames(0) == (0, 0, 0, -1)
    assert hip._frames((95, 18, 107, 118)) == (95, 18, 107, 118) and hip._frames([7, 24, 1009, 1020]) == (7, 24, 1009, 1020)
    for bad in ((0, 12, 0), (0, 12, 0, 11, 0), (), None, 12.0, "12"):
        with pytest.raises(hip.HipError, match="frames"):
            hip._frames(bad)


# ------------------------------------------------------------------ the session on mocked kernels
@pytest.fixture()
def model(monkeypatch):
    hip_mock_ring.install(monkeypatch)
    m = MVTracker(hidden_size=256).eval()
    sd = synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m


def clip_with_query_frames(seed, Tn, frames, V=2, H=96, W=96):
    """A synthetic clip whose i-th query starts at frames[i]."""
    c = synth.make_clip(seed=seed, V=V, T=Tn, H=H, W=W, N=len(frames))
    c["query_points"][0, :, 0] = np.asarray(frames, dtype=np.float32)
    return {k: T(c[k]) for k in ("rgbs", "depths", "query_points", "intrs", "extrs")}


def fixture_clip(g):
    kw = dict(seed=int(g["seed"]), V=int(g["V"]), T=int(g["T"]), H=int(g["H"]), W=int(g["W"]), N=int(g["N"]))
    if "late_queries" in g.files:
        kw.update(late_queries=bool(g["late_queries"]), query_frames=tuple(int(x) for x in g["query_frames"]))
    c = synth.make_clip(**kw)
    return {k: T(c[k]) for k in ("rgbs", "depths", "query_points", "intrs", "extrs")}


def stream(model, clip, blocks, query_sets=None, iters=4, ring_blocks=3):
    """Run a session over ``clip`` with the given block sizes (cycled).  ``query_sets``: [(first frame pushed after adding, query
    rows), ...] -- the first set opens the session.  Returns the assembled whole-clip result (chunks zero-padded), the session."""
    q = clip["query_points"]
    query_sets = query_sets or [(0, q)]
    st = model.open_stream(query_sets[0][1], iters=iters, ring_blocks=ring_blocks)
    pending = list(query_sets[1:])
    Tn = clip["rgbs"].shape[2]
    outs, t, i = [], 0, 0
    while t < Tn:
        while pending and pending[0][0] <= t:
            st.add_queries(pending.pop(0)[1])
        b = min(blocks[i % len(blocks)], Tn - t)
        if pending:
            b = min(b, pending[0][0] - t)
        i += 1
        outs.append(st.push(clip["rgbs"][:, :, t:t + b], clip["depths"][:, :, t:t + b], clip["intrs"][:, :, t:t + b], clip["extrs"][:, :, t:t + b]))
        t += b
    assert not pending
    fin = st.finish()
    outs.append(fin)
    N = fin["traj_e"].shape[2]
    res = {}
    for k in ("traj_e", "vis_e", "vis_logits"):
        parts = []
        for o in outs:
            a, b = o["frames"]
            assert o[k].shape[1] == b - a
            pad = torch.zeros(*o[k].shape[:2], N - o[k].shape[2], *o[k].shape[3:])
            parts.append(torch.cat([o[k], pad], 2))
        res[k] = torch.cat(parts, 1)
    a = 0
    for o in outs:
        assert o["frames"][0] == a
        a = o["frames"][1]
    assert a == Tn
    res["feat_init"] = fin["feat_init"]
    return res, st


@pytest.mark.parametrize("name", ["e2e_two_windows", "e2e_short_clip"])
@pytest.mark.parametrize("blocks", [(1,), (6,), (7,), (5, 2, 9)])
def test_session_is_forward_on_mocked_kernels(model, golden, name, blocks):
    g = golden(name)
    clip = fixture_clip(g)
    r = model(clip["rgbs"], clip["depths"], clip["query_points"], clip["intrs"], clip["extrs"], iters=4)
    ref_windows, ref_logits = list(model.last_windows), model.last_vis_logits.clone()
    s, st = stream(model, clip, blocks)
    assert model.last_windows == ref_windows and len(ref_windows) == int(g["n_windows"])
    for k in ("traj_e", "vis_e", "feat_init"):
        assert torch.equal(s[k], r[k]), k
    assert torch.equal(s["vis_logits"], ref_logits)
    st.check_finite()
    assert int(model.last_nan_flag.item()) == 0
    # ... and the reference's own results, within the tolerances of the host test of ``forward``
    ref = g["traj_exact"]
    assert np.abs(s["traj_e"].numpy() - ref).max() / np.abs(ref).max() < 1e-3
    np.testing.assert_allclose(s["vis_e"].numpy(), g["vis_exact"], atol=5e-3)
    np.testing.assert_allclose(s["feat_init"].numpy(), g["feat_init_exact"], rtol=1e-3, atol=1e-4)


def test_session_with_queries_added_mid_stream(model):
    """Queries at frames 0 .. 14, added in three batches as late as allowed: the session equals ``forward`` on all of them in order
    of addition, and a query behind the windows already run is refused."""
    clip = clip_with_query_frames(5, 30, [7, 0, 14, 3, 9, 1, 12, 5, 2, 13, 4, 8, 6, 11, 10])
    q = clip["query_points"]
    qt = q[0, :, 0].long()
    assert sorted(qt.tolist()) == list(range(15))
    first, second, third = q[:, qt < 4], q[:, (qt >= 4) & (qt < 12)], q[:, qt >= 12]
    allq = torch.cat([first, second, third], 1)
    r = model(clip["rgbs"], clip["depths"], allq, clip["intrs"], clip["extrs"], iters=2)
    logits = model.last_vis_logits.clone()
    # window 0 (frames 0..11) admits t < 12: the second batch must be in before frame 11 arrives; the third before window 6 runs
    s, st = stream(model, clip, (4,), [(0, first), (8, second), (16, third)], iters=2)
    for k in ("traj_e", "vis_e", "feat_init"):
        assert torch.equal(s[k], r[k]), k
    assert torch.equal(s["vis_logits"], logits)
    st2 = model.open_stream(first, iters=2)
    for t in range(0, 12, 4):
        st2.push(clip["rgbs"][:, :, t:t + 4], clip["depths"][:, :, t:t + 4], clip["intrs"][:, :, t:t + 4], clip["extrs"][:, :, t:t + 4])
    with pytest.raises(ValueError, match="already run"):
        st2.add_queries(second)


def test_clip_whose_queries_lie_in_its_last_half_window_is_all_zeros(model):
    clip = clip_with_query_frames(6, 16, [11, 12, 10, 15])
    r = model(clip["rgbs"], clip["depths"], clip["query_points"], clip["intrs"], clip["extrs"], iters=2)
    assert model.last_windows == [] and float(r["traj_e"].abs().max()) == 0.0
    s, _ = stream(model, clip, (5,), iters=2)
    for k in ("traj_e", "vis_e", "feat_init"):
        assert torch.equal(s[k], r[k]), k
    assert model.last_windows == []


def test_forms_without_a_session_say_so(model):
    from mvtracker_amd.parallel import ShardedTracker
    q = torch.zeros(1, 2, 4)
    with pytest.raises(NotImplementedError, match="backward_tracking"):
        model.open_stream(q, backward_tracking=True)
    with pytest.raises(NotImplementedError, match="forward_grouped"):
        model.open_stream([q, q])
    with pytest.raises(NotImplementedError, match="ShardedTracker"):
        ShardedTracker(model).open_stream(q)
    with pytest.raises(ValueError):
        model.open_stream(torch.zeros(1, 0, 4))
