"""CPU stand-ins for the query sampling entries of mvtracker_amd.hip (query_pool, kmeans_*), on top of tests/hip_mock.py: the host
code of mvtracker_amd/queries.py runs on CPU tensors.  The pool mock follows the kernel's rule exactly (hip_mock.unproject's
coordinates, fp32 comparisons, raster order); the k-means mocks are a plain fp64 Lloyd iteration from a seeded draw of distinct
points -- the same state words, not the same numbers as the device."""
import torch

import hip_mock


def query_pool(depths, conf, kinv, einv, V, T, t, H, W, conf_threshold, x0, y0, radius_sq, z_min, z_max, pool, count, block_counts,
               radius_inclusive=False):
    ds = depths.reshape(V, T, H, W).permute(1, 0, 2, 3).contiguous()
    xyz = torch.empty(T, V, H, W, 4)
    hip_mock.unproject(ds, kinv, einv, xyz, V, T, H, W, 1, 0)
    pts = xyz[t].reshape(-1, 4)[:, :3]
    valid = ds[t].reshape(-1) > 0 if conf is None else conf.reshape(V, T, H, W)[:, t].reshape(-1) > conf_threshold
    x, y = pts[:, 0] - x0, pts[:, 1] - y0
    r2 = x ** 2 + y ** 2
    keep = valid & ((r2 <= radius_sq) if radius_inclusive else (r2 < radius_sq)) & (pts[:, 2] >= z_min) & (pts[:, 2] <= z_max)
    kept = pts[keep]
    pool[:kept.shape[0]] = kept
    count[0] = kept.shape[0]


def kmeans_stats(pts, M, tol, partial, state):
    from mvtracker_amd import hip
    state.zero_()
    state.view(torch.float64)[hip.KM_TOL] = tol * pts.double().var(0, unbiased=False).mean()


def kmeans_seed(pts, M, k, seed, min_d2, partials, centres, state):
    g = torch.Generator().manual_seed(seed)
    centres[:k] = pts[torch.randperm(M, generator=g)[:k]]


def _assign(pts, centres, k, labels, acc, state):
    from mvtracker_amd import hip
    d = ((pts.double()[:, None] - centres[:k].double()[None]) ** 2).sum(-1)
    best = d.argmin(1)
    labels[:] = best.int()
    a = acc.view(torch.float64).reshape(-1, 4)  # (the mock keeps fp64 sums in the accumulator's words)
    a.zero_()
    a[:, :3].index_add_(0, best, pts.double())
    a[:, 3] = torch.bincount(best, minlength=k).double()
    state.view(torch.float64)[hip.KM_INERTIA] = d.min(1).values.sum()
    state[hip.KM_EMPTY] = int((a[:, 3] == 0).sum())


def kmeans_assign(pts, M, centres, k, labels, acc, state, max_iter=300, final_pass=False):
    from mvtracker_amd import hip
    if final_pass or not (state[hip.KM_CONVERGED] or state[hip.KM_ITER] >= max_iter):
        _assign(pts, centres, k, labels, acc, state)


def kmeans_update(centres, k, acc, state, max_iter=300, final_pass=False):
    from mvtracker_amd import hip
    if final_pass or state[hip.KM_CONVERGED] or state[hip.KM_ITER] >= max_iter:
        return
    a = acc.view(torch.float64).reshape(-1, 4)
    new = torch.where(a[:, 3:] > 0, a[:, :3] / a[:, 3:].clamp(min=1), centres[:k].double()).float()
    shift = ((new.double() - centres[:k].double()) ** 2).sum()
    centres[:k] = new
    state[hip.KM_ITER] += 1
    if shift <= state.view(torch.float64)[hip.KM_TOL]:
        state[hip.KM_CONVERGED] = 1


def kmeans_iterate(pts, M, centres, k, labels, acc, state, n_iters, max_iter):
    for _ in range(n_iters):
        kmeans_assign(pts, M, centres, k, labels, acc, state, max_iter)
        kmeans_update(centres, k, acc, state, max_iter)


def install(monkeypatch):
    import sys
    from mvtracker_amd import hip
    hip_mock.install(monkeypatch)
    me = sys.modules[__name__]
    for name in "query_pool kmeans_stats kmeans_seed kmeans_assign kmeans_update kmeans_iterate".split():
        monkeypatch.setattr(hip, name, getattr(me, name))
