"""Query sampling, host side (no GPU): the numpy restatement of the pool rule against the reference's pools
(tests/golden/query_sampling.npz), and the spec semantics of mvtracker_amd.queries on CPU tensors through tests/hip_mock_queries.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hip_mock  # noqa: E402
import hip_mock_queries  # noqa: E402
import query_sampling_ref as R  # noqa: E402
from mvtracker_amd import synth  # noqa: E402

V, T, H, W = 2, 3, 37, 53


@pytest.fixture(scope="module")
def fx(golden):
    g = golden("query_sampling")
    clip = synth.make_clip(int(g["clip_seed"][0]), V=V, T=T, H=H, W=W, N=4, invalid_frac=0.02)
    return g, clip


def _tensors(clip, conf=None):
    out = [torch.from_numpy(clip[k]) for k in ("depths", "intrs", "extrs")]
    return out + [None if conf is None else torch.from_numpy(conf)]


def test_fixture_is_what_the_issue_asks(fx):
    g, clip = fx
    assert clip["depths"].shape == (1, V, T, 1, H, W) and g["conf"].shape == (1, V, T, 1, H, W)
    assert float((clip["depths"] == 0).mean()) > 0.005 and 0.0 <= g["conf"].min() and g["conf"].max() <= 1.0
    n = [len(g[f"pool{i}_index"]) for i in range(3)]
    assert n[0] > 4 * int(g["k"][0]) and n[1] > n[0] and n[2] == 0
    assert np.isfinite(g["rows"][0]).all() and np.isinf(g["rows"][1][1:]).all()
    assert g["kmeans_centres"].shape == (int(g["k"][0]), 3) and g["sklearn_inertia"].shape == (10,)


@pytest.mark.parametrize("row", [0, 1, 2])
def test_numpy_pool_rule_equals_reference(fx, row):
    g, clip = fx
    t, zmin, zmax, radius = g["rows"][row]
    idx, pts = R.frame_pool(clip["depths"][0], clip["intrs"][0], clip["extrs"][0], int(t), g["conf"][0], float(g["conf_threshold"][0]),
                            (0.0, 0.0), radius, zmin, zmax)
    assert np.array_equal(idx, g[f"pool{row}_index"])  # membership and order
    if len(idx):
        assert np.abs(pts - g[f"pool{row}_xyz"]).max() < 2e-5  # the bound of the unprojection fixture test (test_gpu_ops.py)


@pytest.mark.parametrize("row", [0, 1, 2])
def test_mock_pool_equals_numpy_rule(fx, row, monkeypatch):
    from mvtracker_amd import queries
    hip_mock_queries.install(monkeypatch)
    g, clip = fx
    t, zmin, zmax, radius = g["rows"][row]
    d, intrs, extrs, conf = _tensors(clip, g["conf"])
    kinv, einv = torch.empty(V * T, 9), torch.empty(V * T, 12)
    hip_mock.invert_cameras(intrs[0].reshape(-1, 9), extrs[0].reshape(-1, 12), kinv, einv, V * T)
    pool = queries.frame_pool(d[0].contiguous(), kinv, einv, int(t), conf[0].contiguous(), float(g["conf_threshold"][0]), (0.0, 0.0), radius, zmin, zmax)
    assert pool.shape == g[f"pool{row}_xyz"].shape
    if len(pool):
        assert np.abs(pool.numpy() - g[f"pool{row}_xyz"]).max() < 2e-5


def test_spec_semantics(fx, monkeypatch):
    from mvtracker_amd import queries
    hip_mock_queries.install(monkeypatch)
    g, clip = fx
    d, intrs, extrs, conf = _tensors(clip, g["conf"])
    n0, n1 = len(g["pool0_index"]), len(g["pool1_index"])
    inf = float("inf")
    spec = [(0, -0.1, 4.2, 2.1, 50, ""),           # random draw of 50
            (7, -inf, inf, inf, 50, ""),            # t >= T: skipped
            (2, -0.1, 4.2, 0.0, 50, "kmeans"),      # empty pool: skipped
            (1, -inf, inf, inf, 10 ** 6, "kmeans"),  # pool smaller than count: whole, in pool order
            (0, -0.1, 4.2, 2.1, 16, "kmeans")]      # 16 centres
    q = queries.sample_queries(d, intrs, extrs, spec, depths_conf=conf, seed=3)
    assert q.shape == (1, 50 + n1 + 16, 4) and q.dtype == torch.float32
    assert torch.equal(q[0, :, 0], torch.cat([torch.zeros(50), torch.ones(n1), torch.zeros(16)]))  # spec order, t in column 0
    pool0, pool1 = torch.from_numpy(g["pool0_xyz"]), torch.from_numpy(g["pool1_xyz"])
    assert (q[0, 50:50 + n1, 1:] - pool1).abs().max() < 2e-5  # returned whole, the pool's order
    d0 = torch.cdist(q[0, :50, 1:].double(), pool0.double()).min(1)
    assert d0.values.max() < 4e-5 and len(set(d0.indices.tolist())) == 50  # 50 distinct pool points
    lo, hi = pool0.min(0).values, pool0.max(0).values
    c = q[0, 50 + n1:, 1:]
    assert bool(((c >= lo - 1e-4) & (c <= hi + 1e-4)).all())  # centres lie in the pool's box
    assert torch.equal(q, queries.sample_queries(d, intrs, extrs, spec, depths_conf=conf, seed=3))
    assert not torch.equal(q[0, :50], queries.sample_queries(d, intrs, extrs, spec, depths_conf=conf, seed=4)[0, :50])
    # without a confidence map validity is depth > 0: more points than with it
    q_all = queries.sample_queries(d, intrs, extrs, [(0, -0.1, 4.2, 2.1, 10 ** 6, "")])
    assert q_all.shape[1] > n0
    with pytest.raises(NotImplementedError):
        queries.sample_queries(d, intrs, extrs, [(0, -0.1, 4.2, 2.1, 10, "fps")], depths_conf=conf)
    with pytest.raises(ValueError, match="empty pool"):
        queries.sample_queries(d, intrs, extrs, [(2, -0.1, 4.2, 0.0, 50, "kmeans"), (9, -inf, inf, inf, 5, "")], depths_conf=conf)
    with pytest.raises(ValueError):
        queries.sample_queries(d[0], intrs, extrs, spec)


def test_kmeans_centres_host_rules(monkeypatch):
    from mvtracker_amd import hip, queries
    hip_mock_queries.install(monkeypatch)
    launches = []
    for name in ("kmeans_stats", "kmeans_seed", "kmeans_iterate", "kmeans_assign", "kmeans_update"):
        monkeypatch.setattr(hip, name, (lambda n, f: lambda *a, **k: (launches.append(n), f(*a, **k))[1])(name, getattr(hip, name)))
    pts = torch.randn(40, 3, generator=torch.Generator().manual_seed(0))
    same, info = queries.kmeans_centres(pts, 40)
    assert same is pts and info["iterations"] == 0 and not launches  # len(points) <= count: unchanged (reference :46-47)
    assert queries.kmeans_centres(pts[:7], 64)[0].shape == (7, 3) and not launches
    with pytest.raises(ValueError):
        queries.kmeans_centres(pts, 0)
    with pytest.raises(ValueError, match="4096"):
        queries.kmeans_centres(torch.randn(5000, 3), 4097)
    with pytest.raises(ValueError):
        queries.kmeans_centres(pts[:0], 4)
    with pytest.raises(ValueError):
        queries.kmeans_centres(torch.full((40, 3), float("nan")), 4)
    with pytest.raises(ValueError):
        queries._km_begin(pts, 41, 1e-4)  # k > M never reaches a launch
    assert not launches
    c, info = queries.kmeans_centres(pts, 5, max_iter=300)
    assert c.shape == (5, 3) and info["converged"] and 1 <= info["iterations"] < 300 and info["empty"] == 0
    assert launches.count("kmeans_iterate") == -(-info["iterations"] // queries.LLOYD_CHUNK)  # the flag is read once per chunk
    import query_sampling_ref as R2
    assert abs(info["inertia"] - R2.inertia(pts.numpy(), c.numpy())) <= 1e-9 * info["inertia"]
    _, one = queries.kmeans_centres(pts, 5, max_iter=1)
    assert one["iterations"] == 1


def _random_queries_before(depths, intrs, extrs, num_queries=512, t0=0, xy_radius=12.0, z_min=-1.0, z_max=10.0, seed=0):
    """demo_amd.random_queries as it stood before it became a call into sample_queries (whole-clip unprojection, eager torch)."""
    from mvtracker_amd import hip
    _, V_, T_, _, H_, W_ = depths.shape
    dev = depths.device
    kinv = torch.empty(V_ * T_, 9, device=dev)
    einv = torch.empty(V_ * T_, 12, device=dev)
    hip.invert_cameras(intrs[0].reshape(V_ * T_, 9).contiguous(), extrs[0].reshape(V_ * T_, 12).contiguous(), kinv, einv, V_ * T_)
    ds = depths[0, :, :, 0].permute(1, 0, 2, 3).contiguous()
    xyz = torch.empty(T_, V_, H_, W_, 4, device=dev)
    hip.unproject(ds, kinv, einv, xyz, V_, T_, H_, W_, 1, 0)
    pts = xyz[t0].reshape(-1, 4)[:, :3]
    r2 = pts[:, 0] ** 2 + pts[:, 1] ** 2
    pool = pts[(r2 <= xy_radius ** 2) & (pts[:, 2] >= z_min) & (pts[:, 2] <= z_max) & (ds[t0].reshape(-1) > 0)]
    assert pool.shape[0] > 0, "cylinder mask removed all points; increase the radius or the z range"
    g = torch.Generator(device="cpu").manual_seed(seed)
    idx = torch.randperm(pool.shape[0], generator=g)[:num_queries].to(dev)
    q = pool[idx]
    return torch.cat([torch.full((q.shape[0], 1), float(t0), device=dev), q], 1)[None]


@pytest.mark.parametrize("kw", [{}, {"num_queries": 64, "t0": 2, "seed": 5}, {"xy_radius": 1.3, "z_min": 0.05, "z_max": 0.9},
                                {"num_queries": 10 ** 6, "xy_radius": 0.8}])
def test_random_queries_unchanged(fx, kw, monkeypatch):
    hip_mock_queries.install(monkeypatch)
    import demo_amd
    _, clip = fx
    d, intrs, extrs, _ = _tensors(clip)
    want = _random_queries_before(d, intrs, extrs, **kw)
    got = demo_amd.random_queries(d, intrs, extrs, **kw)
    assert want.shape[1] > 0 and torch.equal(got, want)
    with pytest.raises(AssertionError, match="cylinder mask removed all points"):
        demo_amd.random_queries(d, intrs, extrs, xy_radius=1e-6, z_min=5.0, z_max=6.0)


def test_public_interface(fx, monkeypatch):
    import inspect
    import mvtracker_amd
    from mvtracker_amd import EvaluationPredictor, queries
    hip_mock_queries.install(monkeypatch)
    assert mvtracker_amd.sample_queries is queries.sample_queries and mvtracker_amd.kmeans_centres is queries.kmeans_centres
    assert mvtracker_amd.DEFAULT_SPEC == [(0, -0.1, 4.2, 2.1, 1000, "kmeans")]
    sig = inspect.signature(queries.sample_queries)
    assert list(sig.parameters)[:8] == ["depths", "intrs", "extrs", "spec", "depths_conf", "conf_threshold", "centre", "seed"]
    assert sig.parameters["conf_threshold"].default == 0.9 and sig.parameters["centre"].default == (0.0, 0.0)
    g, clip = fx
    d, intrs, extrs, conf = _tensors(clip, g["conf"])
    spec = [(0, -0.1, 4.2, 2.1, 8, "kmeans")]
    q = EvaluationPredictor.sample_queries(d, intrs, extrs, spec, depths_conf=conf)
    assert torch.equal(q, queries.sample_queries(d, intrs, extrs, spec, depths_conf=conf)) and q.shape == (1, 8, 4)
    assert EvaluationPredictor.sample_queries(d, intrs, extrs, depths_conf=conf).shape == (1, len(g["pool0_index"]), 4)  # DEFAULT_SPEC: 1000 > pool
