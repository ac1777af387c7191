"""Backward tracking without a GPU: the fixture and the merge rule against the oracle, the reversed window layout against a direct
restatement of the reference's window loop, and the host sequencing of ``forward(backward_tracking=True)`` on mocked kernels."""
import numpy as np
import pytest
import torch

from mvtracker_amd import synth
from mvtracker_amd.backward import reversed_layout, window_prefixes
from oracle import mvt_oracle as O

import hip_mock

CFG = O.TrackerConfig()


def T_(a):
    return torch.from_numpy(np.asarray(a))


def backward_clip(g):
    """The fixture's clip: the seeded synthetic clip with the fixture's own query points."""
    clip = synth.make_clip(seed=int(g["seed"]), V=int(g["V"]), T=int(g["T"]), H=int(g["H"]), W=int(g["W"]), N=1)
    clip["query_points"] = np.asarray(g["query_points"])
    return clip


def args_of(clip, dev="cpu"):
    return [T_(clip[k]).to(dev) for k in ("rgbs", "depths", "query_points", "intrs", "extrs")]


def flip_args(a):
    """The time-flipped clip with query times T-1-trunc(t)."""
    rgbs, depths, q, intrs, extrs = a
    T = rgbs.shape[2]
    qf = q.clone()
    qf[0, :, 0] = (T - 1 - q[0, :, 0].long()).to(q.dtype)
    return [rgbs.flip(2).contiguous(), depths.flip(2).contiguous(), qf, intrs.flip(2).contiguous(), extrs.flip(2).contiguous()]


def merge(fwd, rev, qt, reached):
    """The semantics of backward tracking: fwd / rev (1,T,N,...) results on the clip and on the flipped clip."""
    T = fwd.shape[1]
    take = (torch.arange(T)[:, None] < qt[None, :]) & reached[None, :]
    take = take.reshape(1, T, -1, *([1] * (fwd.dim() - 3))).to(fwd.device)
    return torch.where(take, rev.flip(1), fwd)


def reached_by_reversed(qt, S, T):
    lay = reversed_layout(qt.numpy(), S, T)
    r = torch.zeros(len(qt), dtype=torch.bool)
    r[torch.from_numpy(lay["order"][:lay["active"]])] = True
    return r


def test_fixture_covers_the_cases(golden):
    g = golden("e2e_backward")
    T, S = int(g["T"]), CFG.sliding_window_len
    qt = g["query_points"][0, :, 0].astype(np.int64)
    assert (qt == 0).any() and ((qt > 0) & (qt < S // 2)).any() and (qt >= T - S // 2).any()
    assert ((qt >= S // 2) & (qt < T - S // 2)).any()
    wb = g["windows_backward"]
    assert len(wb) >= 2 and int(wb[-1, 0]) + S > T  # at least two reversed windows, the last one runs past frame 0
    lay = reversed_layout(qt, S, T)
    assert [tuple(int(x) for x in r) for r in wb] == lay["windows"]
    assert [tuple(int(x) for x in r) for r in g["windows_forward"]] == window_prefixes(np.sort(qt), S, T)


def test_oracle_composition_reproduces_the_fixture(golden):
    """oracle(clip) and oracle(flipped clip) merged as DESIGN section 8 states, against the reference-generated fixture, at the
    tolerances of the oracle-vs-fixture leg of the end-to-end tests (tracks 1e-4 of the track scale, visibilities 1e-3)."""
    g = golden("e2e_backward")
    W = O.make_weights(CFG, seed=0)
    a = args_of(backward_clip(g))
    T, S = int(g["T"]), CFG.sliding_window_len
    rf = O.tracker_forward(W, CFG, *a, iters=4, knn_mode="exact")
    rb = O.tracker_forward(W, CFG, *flip_args(a), iters=4, knn_mode="exact")
    assert [tuple(x) for x in rf["windows"]] == [tuple(int(v) for v in r) for r in g["windows_forward"]]
    assert [tuple(x) for x in rb["windows"]] == [tuple(int(v) for v in r) for r in g["windows_backward"]]
    qt = a[2][0, :, 0].long()
    reached = reached_by_reversed(qt, S, T)
    for key, name, tol in (("traj_e", "traj", None), ("vis_e", "vis", 1e-3), ("vis_logits", "logits", 1e-3)):
        for leg, got in (("forward", rf[key]), ("backward", rb[key].flip(1)), ("merged", merge(rf[key], rb[key], qt, reached))):
            ref = g[f"{name}_{leg}"]
            err = np.abs(got.numpy() - ref).max()
            if tol is None:
                err, tol_ = err / np.abs(g["traj_merged"]).max(), 1e-4
            else:
                tol_ = tol
            print(f"{name}_{leg}: {err:.3e} (tol {tol_:.0e})")
            assert err < tol_, (name, leg, err)
    np.testing.assert_allclose(rf["feat_init"].numpy(), g["feat_init_forward"], rtol=1e-4, atol=1e-5)


def reference_windows(qt, S, T):
    """mvtracker.py:489-540 restated directly: [(window start, number of queries with t < start + S)]."""
    qs = sorted(int(t) for t in qt)
    out = []
    w = qs[0]
    while w < T - S // 2:
        out.append((w, sum(1 for t in qs if t < w + S)))
        w += S // 2
    return out


def test_reversed_layout_is_the_reference_loop_on_flipped_times():
    rng = np.random.default_rng(5)
    seen_none_rev = seen_none_fwd = seen_multi = 0
    for _ in range(600):
        T = int(rng.integers(1, 41))
        S = int(rng.choice([8, 12, 16]))
        N = int(rng.integers(1, 20))
        lo = int(rng.integers(0, T))
        qt = rng.integers(lo, T, size=N) if rng.uniform() < 0.5 else rng.integers(0, lo + 1, size=N)
        lay = reversed_layout(qt, S, T)
        flipped = T - 1 - qt
        assert lay["windows"] == reference_windows(flipped, S, T)
        assert lay["frame0"] == [T - 1 - w for w, _ in lay["windows"]]
        order = lay["order"]
        assert sorted(order.tolist()) == list(range(N))
        assert np.array_equal(order, np.argsort(flipped, kind="stable"))  # the row order of a forward call on the flipped clip
        assert np.array_equal(lay["sorted_qt"], qt[order]) and np.all(np.diff(lay["sorted_qt"]) <= 0)
        assert lay["active"] == (lay["windows"][-1][1] if lay["windows"] else 0)
        for w, p1 in lay["windows"]:
            assert 0 <= T - 1 - w < T and p1 >= 1
            assert set(order[:p1].tolist()) == {n for n in range(N) if flipped[n] < w + S}
        fwd = window_prefixes(np.sort(qt), S, T)
        assert fwd == reference_windows(qt, S, T)
        seen_none_rev += not lay["windows"]
        seen_none_fwd += not fwd
        seen_multi += len(lay["windows"]) >= 2
    assert seen_none_rev > 10 and seen_none_fwd > 10 and seen_multi > 10
    with pytest.raises(ValueError, match="within the clip"):
        reversed_layout([0, 12], 12, 12)


# ---- the host sequencing on mocked kernels ------------------------------------------------------------------------------------
def _flipped_time(fn, time_args):
    """hip_mock restates slot frames as min(frame0 + s*step, T-1); a negative step reads clamp(frame0 - s, 0, T-1), which is the
    positive-step contract on the time-flipped store."""
    def wrapper(*args, **kw):
        import inspect
        ba = inspect.signature(fn).bind(*args, **kw)
        ba.apply_defaults()
        p = ba.arguments
        if p["frame_step"] < 0:
            assert p["frame_step"] == -1
            fl = lambda t: t.flip(0).contiguous()
            for k in time_args:
                v = p[k]
                if k == "levels":
                    p[k] = [dict(lv, xyz=fl(lv["xyz"])) for lv in v]
                elif isinstance(v, (list, tuple)):
                    p[k] = [fl(t) for t in v]
                elif v is not None:
                    p[k] = fl(v)
            p["frame0"], p["frame_step"] = p["T"] - 1 - p["frame0"], 1
        return fn(*ba.args, **ba.kwargs)
    return wrapper


@pytest.fixture()
def model(monkeypatch):
    from mvtracker_amd import hip
    from mvtracker_amd.tracker import MVTracker
    hip_mock.install(monkeypatch)
    monkeypatch.setattr(hip, "knn_scan", _flipped_time(hip_mock.knn_scan, ["xyz", "box"]))
    monkeypatch.setattr(hip, "knn_search", _flipped_time(hip_mock.knn_search, ["xyz", "box", "gbox"]))
    monkeypatch.setattr(hip, "knn_scan_levels", _flipped_time(hip_mock.knn_scan_levels, ["levels"]))
    monkeypatch.setattr(hip, "knn_search_levels", _flipped_time(hip_mock.knn_search_levels, ["levels"]))
    monkeypatch.setattr(hip, "corr_gather_dot", _flipped_time(hip_mock.corr_gather_dot, ["xyz_l", "fvec_l"]))
    monkeypatch.setattr(hip, "corr_gather_dot_opts", _flipped_time(hip_mock.corr_gather_dot_opts, ["xyz_l", "fvec_l"]))
    m = MVTracker(hidden_size=256).eval()
    sd = synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m


def test_forward_backward_tracking_sequence(model, golden):
    """forward(backward_tracking=True) on the mocked kernels: the host composition of two plain calls (clip, flipped clip) with the
    same mocks, frames from the query frame on untouched, the fixture at the mocks' layout-check tolerance, and the rows of
    feat_init only the reversed pass reaches."""
    g = golden("e2e_backward")
    a = args_of(backward_clip(g))
    T, S = int(g["T"]), model.S
    qt = a[2][0, :, 0].long()
    rf = model(*a, iters=4)
    lf, wf = model.last_vis_logits.clone(), list(model.last_windows)
    rf = {k: v.clone() for k, v in rf.items()}
    rb = model(*flip_args(a), iters=4)
    lb, wb = model.last_vis_logits.clone(), list(model.last_windows)
    rb = {k: v.clone() for k, v in rb.items()}
    r = model(*a, iters=4, backward_tracking=True)
    assert model.last_windows == wf and model.last_windows_backward == wb
    assert wb == [tuple(int(x) for x in row) for row in g["windows_backward"]]
    reached = reached_by_reversed(qt, S, T)
    for got, f_, b_ in ((r["traj_e"], rf["traj_e"], rb["traj_e"]), (r["vis_e"], rf["vis_e"], rb["vis_e"]), (model.last_vis_logits, lf, lb)):
        want = merge(f_, b_, qt, reached)
        assert float((got - want).abs().max()) < 1e-5
        keep = (torch.arange(T)[:, None] >= qt[None, :]).reshape(1, T, -1, *([1] * (got.dim() - 3)))
        assert torch.equal(torch.where(keep, got, torch.zeros(())), torch.where(keep, f_, torch.zeros(())))
    ref = g["traj_merged"]
    assert np.abs(r["traj_e"].numpy() - ref).max() / np.abs(ref).max() < 1e-3
    np.testing.assert_allclose(r["vis_e"].numpy(), g["vis_merged"], atol=2e-2)  # (mocked kernels: torch arithmetic, layout check)
    # the fixture's late queries on their own: no forward window runs (zero rows from the query frame on, the reference's pinned
    # behaviour), the reversed pass fills the frames before the query frame, and feat_init takes the reversed pass's rows
    late = torch.nonzero(qt >= T - S // 2)[:, 0]
    assert late.numel() > 0
    al = [a[0], a[1], a[2][:, late], a[3], a[4]]
    rl = model(*al, iters=4, backward_tracking=True)
    assert model.last_windows == [] and len(model.last_windows_backward) >= 1
    for i, n in enumerate(late.tolist()):
        t = int(qt[n])
        assert float(rl["traj_e"][0, t:, i].abs().max()) == 0.0
        assert bool(torch.isfinite(rl["traj_e"][0, :t, i]).all()) and float(rl["traj_e"][0, :t, i].abs().sum(-1).min()) > 0.0
    assert float(rl["feat_init"][0, 0].abs().sum(-1).min()) > 0.0
    assert float(model(*al, iters=4)["feat_init"].abs().max()) == 0.0
    # feat_init (rows sorted by query frame): the forward pass's rows unchanged, the rows it never reached taken from the reversed pass
    order = torch.argsort(qt, stable=True)
    order_b = torch.argsort(T - 1 - qt, stable=True)
    fi, fi_f, fi_b = r["feat_init"][0, 0], rf["feat_init"][0, 0], rb["feat_init"][0, 0]
    nf = wf[-1][1]
    assert torch.equal(fi[:nf], fi_f[:nf])
    for row in range(nf, len(qt)):
        pos = int(torch.nonzero(order_b == order[row])[0, 0])
        want = fi_b[pos] if pos < wb[-1][1] else torch.zeros_like(fi_b[pos])
        assert float((fi[row] - want).abs().max()) < 1e-6


def test_backward_tracking_refusals(model):
    clip = synth.make_clip(3, V=1, T=16, H=128, W=128, N=4, late_queries=True, query_frames=(9,))
    clip["query_points"][0, 0, 0] = 9.0
    a = args_of(clip)
    with pytest.raises(NotImplementedError, match="backward_tracking"):
        model.forward_grouped(a[0], a[1], [a[2]], a[3], a[4], backward_tracking=True)
    store = model.build_frame_store(a[0][0], a[1][0], a[3][0], a[4][0], t0=4)
    with pytest.raises(ValueError, match="from frame 0"):
        model(*a, iters=1, frame_store=store, backward_tracking=True)
    bad = a[2].clone()
    bad[0, 0, 0] = 16.0
    with pytest.raises(ValueError, match="within the clip"):
        model(a[0], a[1], bad, a[3], a[4], iters=1, backward_tracking=True)


def test_predictor_passes_the_option(monkeypatch):
    from mvtracker_amd.predictor import EvaluationPredictor

    class Spy(torch.nn.Module):
        def forward(self, rgbs, depths=None, query_points=None, intrs=None, extrs=None, **kw):
            self.kw = kw
            T, N = rgbs.shape[2], query_points.shape[1]
            return {"traj_e": torch.zeros(1, T, N, 3), "vis_e": torch.zeros(1, T, N)}

    monkeypatch.setattr("mvtracker_amd.hip.require_device", lambda t: None)
    monkeypatch.setattr("mvtracker_amd.hip.invert_cameras", hip_mock.invert_cameras)
    clip = synth.make_clip(2, V=1, T=8, H=64, W=64, N=3)
    a = args_of(clip)
    call = lambda p: p(rgbs=a[0], depths=a[1], query_points_3d=a[2], intrs=a[3], extrs=a[4])
    for single in (False, True):
        spy = Spy()
        call(EvaluationPredictor(spy, interp_shape=None, grid_size=0, local_grid_size=0, single_point=single, backward_tracking=True))
        assert spy.kw.get("backward_tracking") is True
        spy = Spy()
        call(EvaluationPredictor(spy, interp_shape=None, grid_size=0, local_grid_size=0, single_point=single))
        assert "backward_tracking" not in spy.kw
    p = EvaluationPredictor(Spy(), interp_shape=None, grid_size=0, local_grid_size=0, single_point=True, backward_tracking=True)
    p.single_point_group_size = 4
    with pytest.raises(NotImplementedError, match="backward_tracking"):
        call(p)
