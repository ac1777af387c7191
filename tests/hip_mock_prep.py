"""CPU stand-ins for the cloud preparation entries of mvtracker_amd.hip (normals_estimate, voxel_bounds, voxel_insert, voxel_emit), on
top of tests/hip_mock_align.py: the host code of mvtracker_amd/cloud.py and the PCA path of mvtracker_amd/align.py run on CPU tensors.
The fake entries call the restatement tests/cloud_prep_ref.py; ``calls`` lists the entries called, in order, and ``order`` those
together with the box and grid-normal entries (tile_aabb, tile_group_aabb, align_normals), which this module wraps to see the sequence."""
import numpy as np
import torch

import cloud_prep_ref as R
import hip_mock_align

calls = []
order = []


def normals_estimate(xyz, Cn, Pn, grid, max_nn, radius, box, gbox, nrm, viewpoint=None, nbr_idx=None, nbr_cnt=None, cov=None):
    from mvtracker_amd import hip
    calls.append("normals_estimate")
    order.append("normals_estimate")
    assert grid == (0, 0) or (grid[0] % 8 == 0 and grid[1] % 8 == 0 and grid[0] * grid[1] == Pn)
    assert 3 <= max_nn <= hip.NORMALS_MAX_NN and radius > 0
    x = xyz.reshape(Cn, Pn, 4).numpy()
    out = nrm.reshape(Cn, Pn, 4)
    out.zero_()
    for c in range(Cn):
        r = R.estimate(x[c], radius, max_nn, None if viewpoint is None else viewpoint.reshape(Cn, 3)[c].numpy())
        out[c, :, :3] = torch.from_numpy(r["nrm"].astype(np.float32))
        if nbr_idx is not None:
            nbr_idx.reshape(Cn, Pn, max_nn)[c] = torch.from_numpy(r["idx"])
        if nbr_cnt is not None:
            nbr_cnt.reshape(Cn, Pn)[c] = torch.from_numpy(r["cnt"])
        if cov is not None:
            cov.reshape(Cn, Pn, 6)[c] = torch.from_numpy(r["cov"])


def voxel_bounds(xyz, Pn, voxel, partial, state):
    from mvtracker_amd import hip
    calls.append("voxel_bounds")
    x = xyz.reshape(-1, 4)[:Pn].numpy()
    ok = R.valid_rows(x)
    st = state.view(torch.float64)
    lo = x[ok, :3].astype(np.float64).min(0) if ok.any() else np.full(3, np.inf)
    st[hip.VOXEL_ORIGIN:hip.VOXEL_ORIGIN + 3] = torch.from_numpy(lo - voxel * 0.5)
    st[hip.VOXEL_SIZE] = voxel
    state[hip.VOXEL_STATUS], state[hip.VOXEL_POINTS] = 0, int(ok.sum())


def voxel_insert(xyz, Pn, state, table, capacity):
    from mvtracker_amd import hip
    calls.append("voxel_insert")
    assert capacity >= 2 * Pn and capacity & (capacity - 1) == 0
    r = R.voxel(xyz.reshape(-1, 4)[:Pn].numpy(), float(state.view(torch.float64)[hip.VOXEL_SIZE]))
    state[hip.VOXEL_STATUS] = r["status"]


def voxel_emit(xyz, Pn, state, table, capacity, block_counts, points, counts, first, n_out, labels=None):
    from mvtracker_amd import hip
    calls.append("voxel_emit")
    r = R.voxel(xyz.reshape(-1, 4)[:Pn].numpy(), float(state.view(torch.float64)[hip.VOXEL_SIZE]))
    mv = len(r["counts"])
    points.reshape(-1, 4)[:mv, :3] = torch.from_numpy(r["points"])
    points.reshape(-1, 4)[:mv, 3] = 0
    counts[:mv], first[:mv] = torch.from_numpy(r["counts"]), torch.from_numpy(r["first"])
    n_out[0] = mv
    if labels is not None:
        labels[:Pn] = torch.from_numpy(r["labels"])


def install(monkeypatch):
    import sys
    from mvtracker_amd import hip
    hip_mock_align.install(monkeypatch)
    me = sys.modules[__name__]
    del calls[:]
    del order[:]
    for name in "normals_estimate voxel_bounds voxel_insert voxel_emit".split():
        monkeypatch.setattr(hip, name, getattr(me, name))
    for name in "tile_aabb tile_group_aabb align_normals".split():
        inner = getattr(hip, name)
        monkeypatch.setattr(hip, name, (lambda n, f: lambda *a, **k: (order.append(n), f(*a, **k))[1])(name, inner))
