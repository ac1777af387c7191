"""CPU stand-ins for the region clustering entries of mvtracker_amd.hip (cluster_crop, cluster_count, cluster_link, cluster_border,
cluster_finish), on top of tests/hip_mock_clean.py and tests/hip_mock_queries.py: the host code of mvtracker_amd/cluster.py and the
region path of mvtracker_amd/queries.py run on CPU tensors.  The fake entries follow the kernels' rules stage by stage (the crop's
strict test, the inclusive neighbour test on fp32(eps^2), roots = lowest core index, the fallbacks) with the pieces of the
restatement tests/cluster_ref.py; ``calls`` lists the entries called, in order, and ``shapes`` the (clouds, points) of every count."""
import numpy as np
import torch

import cluster_ref as R
import hip_mock_clean
import hip_mock_queries

calls = []
shapes = []


def cluster_crop(xyz, Cn, Pn, region_T_world, bounds):
    calls.append("cluster_crop")
    assert tuple(region_T_world.shape) == (Cn, 3, 4) and region_T_world.dtype == torch.float32 and len(bounds) == 6
    x = xyz.reshape(Cn, Pn, 4)
    b = np.asarray(bounds, np.float64).reshape(3, 2)
    for c in range(Cn):
        m = region_T_world[c].numpy().astype(np.float64)
        p = x[c, :, :3].numpy().astype(np.float64)
        q = p @ m[:, :3].T + m[:, 3]
        with np.errstate(invalid="ignore"):
            keep = np.isfinite(p).all(1) & ((q > b[:, 0]) & (q < b[:, 1])).all(1)
        x[c, ~torch.from_numpy(keep), :3] = float("nan")


def _pairs(x, r2):
    ok = R.valid_rows(x)
    idx = np.nonzero(ok)[0]
    if len(idx) == 0:
        return idx, idx
    i, j = R.neighbour_pairs(x[idx, :3].astype(np.float64), r2)
    return idx[i], idx[j]


def cluster_count(xyz, Cn, Pn, grid, r2, min_samples, box, gbox, core):
    calls.append("cluster_count")
    shapes.append((Cn, Pn))
    assert grid == (0, 0) or (grid[0] % 8 == 0 and grid[1] % 8 == 0 and grid[0] * grid[1] == Pn)
    assert r2 == float(np.float32(r2)) and r2 > 0 and min_samples >= 1
    x = xyz.reshape(Cn, Pn, 4).numpy()
    for c in range(Cn):
        i, _ = _pairs(x[c], r2)
        core.reshape(Cn, Pn)[c] = torch.from_numpy((np.bincount(i, minlength=Pn) >= min_samples).astype(np.uint8))


def cluster_link(xyz, Cn, Pn, grid, r2, box, gbox, core, parent, state):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    calls.append("cluster_link")
    state.zero_()
    x = xyz.reshape(Cn, Pn, 4).numpy()
    for c in range(Cn):
        k = core.reshape(Cn, Pn)[c].numpy() != 0
        i, j = _pairs(x[c], r2)
        cc = k[i] & k[j]
        comp = connected_components(coo_matrix((np.ones(int(cc.sum()), np.int8), (i[cc], j[cc])), shape=(Pn, Pn)), directed=False)[1]
        first = np.full(comp.max() + 1, Pn, np.int64)
        np.minimum.at(first, comp[k], np.nonzero(k)[0])
        parent.reshape(Cn, Pn)[c] = torch.from_numpy(np.where(k, first[comp], np.arange(Pn)).astype(np.int32))


def cluster_border(xyz, Cn, Pn, grid, r2, box, gbox, core, parent, root):
    calls.append("cluster_border")
    x = xyz.reshape(Cn, Pn, 4).numpy()
    for c in range(Cn):
        k = core.reshape(Cn, Pn)[c].numpy() != 0
        par = parent.reshape(Cn, Pn)[c].numpy().astype(np.int64)
        i, j = _pairs(x[c], r2)
        best = np.full(Pn, Pn, np.int64)
        b = ~k[i] & k[j]
        np.minimum.at(best, i[b], par[j[b]])
        root.reshape(Cn, Pn)[c] = torch.from_numpy(np.where(k, par, np.where(best < Pn, best, -1)).astype(np.int32))


def cluster_finish(xyz, Cn, Pn, min_samples, core, root, sizes, labels, select, state):
    from mvtracker_amd import hip
    calls.append("cluster_finish")
    x = xyz.reshape(Cn, Pn, 4).numpy()
    for c in range(Cn):
        ok = R.valid_rows(x[c])
        k = core.reshape(Cn, Pn)[c].numpy() != 0
        r = root.reshape(Cn, Pn)[c].numpy().astype(np.int64)
        roots = np.nonzero(k & (r == np.arange(Pn)))[0]
        ids = np.full(Pn + 1, -1, np.int64)
        ids[roots] = np.arange(len(roots))
        lab = ids[r]  # (r = -1 reads the spare last entry)
        counts = np.bincount(lab[lab >= 0], minlength=len(roots))
        chosen = int(np.argmax(counts)) if len(roots) else -1
        n = int(ok.sum())
        fb = hip.CLUSTER_EMPTY if n == 0 else (hip.CLUSTER_FEW if n < min_samples else (hip.CLUSTER_NONE if len(roots) == 0 else 0))
        sel = ok if fb in (hip.CLUSTER_FEW, hip.CLUSTER_NONE) else (lab == chosen) & (lab >= 0)
        labels.reshape(Cn, Pn)[c] = torch.from_numpy(lab.astype(np.int32))
        select.reshape(Cn, Pn)[c] = torch.from_numpy(sel.astype(np.uint8))
        st = state.reshape(Cn, hip.CLUSTER_STATE_WORDS)[c]
        st[:7] = torch.tensor([n, int(k.sum()), len(roots), chosen, int(counts[chosen]) if len(roots) else 0, int((ok & (lab < 0)).sum()), fb])


def install(monkeypatch):
    import sys
    from mvtracker_amd import hip
    hip_mock_clean.install(monkeypatch)
    hip_mock_queries.install(monkeypatch)
    me = sys.modules[__name__]
    del calls[:]
    del shapes[:]
    for name in "cluster_crop cluster_count cluster_link cluster_border cluster_finish".split():
        monkeypatch.setattr(hip, name, getattr(me, name))
