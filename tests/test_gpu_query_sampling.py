"""Query sampling on the device: mvt_query_pool and the mvt_kmeans_* kernels against tests/golden/query_sampling.npz (the
reference's pools, its k-means inertia and sklearn's seed-to-seed spread) and the fp64 restatement in tests/query_sampling_ref.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import query_sampling_ref as R  # noqa: E402
from mvtracker_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
V, T, H, W = 2, 3, 37, 53


@pytest.fixture(scope="module")
def hip():
    from mvtracker_amd import hip as h
    return h


@pytest.fixture(scope="module")
def fx(golden):
    g = golden("query_sampling")
    clip = synth.make_clip(int(g["clip_seed"][0]), V=V, T=T, H=H, W=W, N=4, invalid_frac=0.02)
    return g, clip


def _cams(hip, intrs, extrs):
    n = intrs.shape[0] * intrs.shape[1]
    kinv, einv = torch.empty(n, 9, device=DEV), torch.empty(n, 12, device=DEV)
    hip.invert_cameras(torch.from_numpy(intrs).to(DEV).reshape(n, 9).contiguous(), torch.from_numpy(extrs).to(DEV).reshape(n, 12).contiguous(),
                       kinv, einv, n)
    return kinv, einv


def _pool(fx, row, conf=True):
    from mvtracker_amd import hip, queries
    g, clip = fx
    t, zmin, zmax, radius = g["rows"][row]
    kinv, einv = _cams(hip, clip["intrs"][0], clip["extrs"][0])
    c = torch.from_numpy(g["conf"][0]).to(DEV) if conf else None
    return queries.frame_pool(torch.from_numpy(clip["depths"][0]).to(DEV), kinv, einv, int(t), c, float(g["conf_threshold"][0]), (0.0, 0.0),
                              radius, zmin, zmax)


# ------------------------------------------------------------------------------------------------------------------ pool
@pytest.mark.parametrize("row", [0, 1, 2])
def test_pool_equals_reference(fx, row):
    g, _ = fx
    pool = _pool(fx, row)
    ref = g[f"pool{row}_xyz"]
    assert pool.shape == ref.shape  # membership: the same count ...
    if len(ref):
        assert np.abs(pool.cpu().numpy() - ref).max() < 2e-5  # ... and every row the reference's point at that position (order)
    assert torch.equal(pool, _pool(fx, row))  # two runs


def test_pool_all_and_none(fx, hip):
    from mvtracker_amd import queries
    g, clip = fx
    d = clip["depths"][0].copy()
    d[d <= 0] = 1.0
    kinv, einv = _cams(hip, clip["intrs"][0], clip["extrs"][0])
    dd = torch.from_numpy(d).to(DEV)
    full = queries.frame_pool(dd, kinv, einv, 1)  # no confidence map, every depth positive, no bounds: M = V*H*W
    assert full.shape == (V * H * W, 3)
    assert np.abs(full.cpu().numpy() - R.frame_points(d, clip["intrs"][0], clip["extrs"][0], 1)).max() < 2e-5
    assert queries.frame_pool(torch.zeros_like(dd), kinv, einv, 1).shape == (0, 3)  # M = 0
    assert queries.frame_pool(dd, kinv, einv, 1, conf=torch.zeros_like(dd)).shape == (0, 3)


def test_pool_count_multiple_of_workgroup(hip):
    from mvtracker_amd import queries
    clip = synth.make_clip(5, V=1, T=2, H=64, W=64, N=4)  # 4096 pixels = 16 workgroups of 256, all valid
    kinv, einv = _cams(hip, clip["intrs"][0], clip["extrs"][0])
    d = torch.from_numpy(clip["depths"][0]).to(DEV)
    pool = queries.frame_pool(d, kinv, einv, 1)
    assert pool.shape == (4096, 3)
    assert np.abs(pool.cpu().numpy() - R.frame_points(clip["depths"][0], clip["intrs"][0], clip["extrs"][0], 1)).max() < 2e-5
    idx, pts = R.frame_pool(clip["depths"][0], clip["intrs"][0], clip["extrs"][0], 1, radius=1.0, z_min=-0.1, z_max=0.5)
    part = queries.frame_pool(d, kinv, einv, 1, radius=1.0, z_min=-0.1, z_max=0.5)
    assert 0 < len(idx) < 4096 and part.shape == pts.shape and np.abs(part.cpu().numpy() - pts).max() < 2e-5
    assert torch.equal(part, queries.frame_pool(d, kinv, einv, 1, radius=1.0, z_min=-0.1, z_max=0.5))


# ------------------------------------------------------------------------------------------------------------------ k-means data
def _blobs(n, seed):
    rng = np.random.default_rng(seed)
    c = np.array([[-1.5, 0.2, 0.4], [1.0, 1.2, -0.3], [0.3, -1.4, 1.1]])
    p = c[rng.integers(0, 3, size=n)] + rng.normal(0, 0.25, size=(n, 3))
    return p.astype(np.float32)


@pytest.fixture(scope="module")
def blobs():
    return {5003: _blobs(5003, 11), 20011: _blobs(20011, 12)}


def _assign_once(hip, pts_np, centres_np):
    """stats + one assignment on the device -> (labels, acc (k,4) int64, state dict of raw words, work tensors)."""
    from mvtracker_amd import queries
    pts = torch.from_numpy(pts_np).to(DEV)
    k = len(centres_np)
    w = queries._km_begin(pts, k, 1e-4)
    w["centres"].copy_(torch.from_numpy(centres_np))
    hip.kmeans_assign(pts, len(pts_np), w["centres"], k, w["labels"], w["acc"], w["state"])
    torch.cuda.synchronize()
    return w


@pytest.mark.parametrize("n,k", [(5003, 1), (5003, 7), (5003, 64), (20011, 1000)])
def test_assign_and_update(hip, blobs, n, k):
    from mvtracker_amd import queries
    pts = blobs[n]
    rng = np.random.default_rng(k)
    centres = pts[rng.choice(n, size=k, replace=False)].copy()
    w = _assign_once(hip, pts, centres)
    labels = w["labels"].cpu().numpy().astype(np.int64)
    d = R.sq_dists(pts, centres)
    chosen = d[np.arange(n), labels]
    assert (labels >= 0).all() and (labels < k).all()
    assert (chosen <= (1 + 1e-5) * d.min(1)).all()  # every point sits at (one of) its nearest centres
    acc = w["acc"].cpu().numpy()
    counts = acc[:, 3]
    assert counts.sum() == n and np.array_equal(counts, np.bincount(labels, minlength=k))
    # update: each centre = fp64 mean of ITS assigned points, within 1e-6 x the pool extent; the inertia of this assignment
    hip.kmeans_update(w["centres"], k, w["acc"], w["state"])
    info = queries._km_state(w)
    new, _ = R.lloyd_step(pts, centres, labels)
    extent = float((pts.max(0) - pts.min(0)).max())
    err = np.abs(w["centres"].cpu().numpy().astype(np.float64) - new).max()
    print(f"n={n} k={k}: centre err {err:.3e} (bar {1e-6 * extent:.3e}), inertia {info['inertia']:.9g} vs fp64 {chosen.sum():.9g}")
    assert err <= 1e-6 * extent
    assert abs(info["inertia"] - chosen.sum()) <= 1e-5 * chosen.sum()
    assert info["iterations"] == 1 and info["empty"] == int((counts == 0).sum())
    assert int(w["acc"].abs().max()) == 0  # cleared for the next assignment


def test_assign_tie_goes_to_lower_index(hip, blobs):
    pts = blobs[5003]
    centres = pts[[10, 20, 30, 40, 50, 60]].copy()
    centres[4] = centres[1]  # two identical centres: an exact tie for every point nearest to them
    w = _assign_once(hip, pts, centres)
    labels = w["labels"].cpu().numpy()
    assert (labels == 1).sum() > 0 and (labels == 4).sum() == 0


# ------------------------------------------------------------------------------------------------------------------ whole runs
def test_determinism_and_seed(blobs):
    from mvtracker_amd import queries
    pts = torch.from_numpy(blobs[5003]).to(DEV)
    a, ia = queries.kmeans_centres(pts, 64, seed=0)
    b, ib = queries.kmeans_centres(pts, 64, seed=0)
    assert torch.equal(a, b) and ia == ib  # bit-identical, inertia and iteration count included
    c, _ = queries.kmeans_centres(pts, 64, seed=1)
    assert not torch.equal(a, c)
    assert bool(torch.isfinite(a).all()) and ia["empty"] == 0


@pytest.mark.parametrize("n,k", [(5003, 7), (5003, 64), (20011, 1000)])
def test_convergence(blobs, n, k):
    from mvtracker_amd import queries
    pts_np = blobs[n]
    pts = torch.from_numpy(pts_np).to(DEV)
    c, info = queries.kmeans_centres(pts, k, seed=2)
    print(f"n={n} k={k}: {info}")
    assert info["converged"] and info["iterations"] < 300
    ref = R.inertia(pts_np, c.cpu().numpy())
    assert abs(info["inertia"] - ref) <= 1e-5 * ref
    _, counts = R.lloyd_step(pts_np, c.cpu().numpy())
    assert info["empty"] == int((counts == 0).sum())


def test_one_iteration_is_one_lloyd_step(hip, blobs):
    from mvtracker_amd import queries
    pts_np = blobs[5003]
    pts = torch.from_numpy(pts_np).to(DEV)
    w = queries._km_begin(pts, 7, 1e-4)
    queries._km_seed(w, 5)
    seeds = w["centres"].cpu().numpy().copy()
    assert len(np.unique(seeds, axis=0)) == 7 and (R.sq_dists(seeds, pts_np).min(1) == 0).all()  # seeds are distinct pool points
    c, info = queries.kmeans_centres(pts, 7, seed=5, max_iter=1)
    assert info["iterations"] == 1
    new, _ = R.lloyd_step(pts_np, seeds)
    assert np.abs(c.cpu().numpy() - new).max() <= 1e-6 * float((pts_np.max(0) - pts_np.min(0)).max())


def test_argument_errors_raise_before_any_launch(hip, blobs):
    from mvtracker_amd import queries
    pts = torch.from_numpy(blobs[5003]).to(DEV)
    w = queries._km_begin(pts, 7, 1e-4)
    big = torch.empty(4097, 3, device=DEV)
    acc = torch.zeros(4097, 4, device=DEV, dtype=torch.int64)
    with pytest.raises(hip.HipError, match="arguments rejected"):  # k > 4096
        hip.kmeans_assign(pts, 5003, big, 4097, w["labels"], acc, w["state"])
    with pytest.raises(hip.HipError, match="arguments rejected"):
        hip.kmeans_seed(pts, 5003, 4097, 0, w["min_d2"], w["partials"], big, w["state"])
    with pytest.raises(hip.HipError, match="arguments rejected"):  # k > M
        hip.kmeans_iterate(pts[:5], 5, w["centres"], 7, w["labels"], w["acc"], w["state"], 1, 300)
    with pytest.raises(hip.HipError, match="arguments rejected"):  # M == 0
        hip.kmeans_stats(pts[:0], 0, 1e-4, w["stat"], w["state"])
    with pytest.raises(hip.HipError, match="arguments rejected"):  # misaligned state (8-byte words)
        hip.kmeans_update(w["centres"], 7, w["acc"], _Shifted(), 300)
    with pytest.raises(ValueError):
        queries.kmeans_centres(torch.empty(0, 3, device=DEV), 4)
    with pytest.raises(ValueError):
        queries.kmeans_centres(torch.empty(5000, 3, device=DEV), 4097)
    torch.cuda.synchronize()


class _Shifted:
    """A stand-in tensor whose device pointer is 4 bytes past an int64 allocation (torch cannot view such a slice as int64)."""

    def __init__(self):
        self.base = torch.zeros(40, device=DEV, dtype=torch.int64)
        self.dtype, self.is_cuda = torch.int64, True

    def numel(self):
        return 32

    def data_ptr(self):
        return self.base.data_ptr() + 4


# ------------------------------------------------------------------------------------------------------------------ quality
def test_inertia_against_reference(fx):
    """Device k-means on the reference's pool, k = 64: inertia <= I_ref * (1 + 2 s), I_ref the reference's own kmeans_sample inertia
    and s sklearn's relative spread over random_state 0..9, both read from the fixture."""
    from mvtracker_amd import queries
    g, _ = fx
    pool = torch.from_numpy(g["pool0_xyz"]).to(DEV)
    k = int(g["k"][0])
    i_ref = float(g["kmeans_inertia"][0])
    sk = g["sklearn_inertia"]
    s = float((sk.max() - sk.min()) / sk.min())
    c, info = queries.kmeans_centres(pool, k)
    print(f"I_ref {i_ref:.6f}, s {s:.6f}, bar {i_ref * (1 + 2 * s):.6f}, device inertia {info['inertia']:.6f} after {info['iterations']} iterations")
    assert abs(info["inertia"] - R.inertia(g["pool0_xyz"], c.cpu().numpy())) <= 1e-5 * info["inertia"]
    assert info["inertia"] <= i_ref * (1 + 2 * s)


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_sampled_queries_track(fx):
    """Sampled queries through ``forward`` and through a streaming session.  The fixture clip's frames (37 x 53) are below what the
    tracker accepts (its coarsest point-cloud level needs corr_neighbors = 16 points: 2 views want frames of at least 96 x 96),
    so this runs on the same seeded scene rendered at 128 x 128; sampling on the fixture clip itself is what the pool tests check."""
    from mvtracker_amd import sample_queries
    from mvtracker_amd.tracker import MVTracker
    g, _ = fx
    clip = synth.make_clip(int(g["clip_seed"][0]), V=2, T=8, H=128, W=128, N=4, invalid_frac=0.02)
    rgbs, depths, intrs, extrs = (torch.from_numpy(clip[k]).to(DEV) for k in ("rgbs", "depths", "intrs", "extrs"))
    q = sample_queries(depths, intrs, extrs, [(0, -0.1, 4.2, 2.1, 32, "kmeans")])
    assert q.shape == (1, 32, 4) and bool(torch.isfinite(q).all()) and bool((q[..., 0] == 0).all())
    model = MVTracker(hidden_size=256).eval()
    sd = synth.make_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=0)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model.to(DEV)
    out = model(rgbs, depths, q, intrs, extrs, iters=2)
    torch.cuda.synchronize()
    assert out["traj_e"].shape == (1, 8, 32, 3) and bool(torch.isfinite(out["traj_e"]).all())
    st = model.open_stream(q[:, :16], iters=2)
    st.add_queries(q[:, 16:])
    chunks = [st.push(rgbs[:, :, t:t + 4], depths[:, :, t:t + 4], intrs[:, :, t:t + 4], extrs[:, :, t:t + 4]) for t in (0, 4)]
    chunks.append(st.finish())
    torch.cuda.synchronize()
    tr = torch.cat([c["traj_e"] for c in chunks], 1)
    assert tr.shape == (1, 8, 32, 3) and bool(torch.isfinite(tr).all())
    assert torch.equal(tr, out["traj_e"])  # the session tracked the same 32 queries as the one call
