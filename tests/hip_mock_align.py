"""CPU stand-ins for the camera alignment entries of mvtracker_amd.hip (align_normals, align_transform, align_correspond,
align_solve), on top of tests/hip_mock_clean.py: the host code of mvtracker_amd/align.py and the predictor's wiring run on CPU
tensors.  The fake entries follow the kernels' rules (query slots, the done flag, the evaluation counter, the status bits) and call
the restatement tests/camera_align_ref.py for the arithmetic; ``calls`` lists the entries called, in order, and ``searches`` the
(source view, target views) of every correspond call that was not cut short by the done flag, found by the tensors' addresses."""
import numpy as np
import torch

import camera_align_ref as R
import hip_mock_clean

calls = []
searches = []


def align_normals(xyz, Cn, grid, max_edge, nrm):
    calls.append("align_normals")
    gw, gh = grid
    x = xyz.reshape(Cn, gw * gh, 4).numpy()
    out = nrm.reshape(Cn, gw * gh, 4)
    out.zero_()
    for c in range(Cn):
        out[c, :, :3] = torch.from_numpy(R.normals(x[c], gw, gh, max_edge).astype(np.float32))


def align_transform(xyz0, D, n, xyz):
    calls.append("align_transform")
    src = xyz0.reshape(-1, 4)[:n].numpy()
    out = xyz.reshape(-1, 4)
    out[:n, :3] = torch.from_numpy(R.transform(D.reshape(3, 4).numpy(), src))
    out[:n, 3] = 0


def _slots(Pn, grid, s):
    from mvtracker_amd import align
    return align.query_slots(Pn, grid, s).numpy()


def align_correspond(src0, Pn, grid, sample_stride, frames, D, cap2, targets, istate, partial, q_idx=None, q_d2=None):
    from mvtracker_amd import hip
    calls.append("align_correspond")
    if int(istate[hip.ALIGN_I_DONE]):
        return
    searches.append((src0.data_ptr(), tuple(t["xyz"].data_ptr() for t in targets)))
    slots = _slots(Pn, grid, sample_stride)
    ntq = len(slots) // 64
    Dm = D.reshape(3, 4).numpy()
    part = partial.reshape(frames, ntq, hip.ALIGN_ROW)
    for f in range(frames):
        s0 = src0.reshape(frames, Pn, 4)[f].numpy()
        q = np.full((len(slots), 3), np.nan, np.float32)
        q[slots >= 0] = R.transform(Dm, s0[slots[slots >= 0]])
        union = R.target_union([(t["xyz"].reshape(frames, t["P"], 4)[f].numpy(), t["nrm"].reshape(frames, t["P"], 4)[f].numpy()[:, :3])
                                for t in targets])
        corr = R.correspond(q, union, cap2)
        for tile in range(ntq):
            sl = slice(tile * 64, tile * 64 + 64)
            c = {k: v[sl] for k, v in corr.items()}
            part[f, tile] = torch.from_numpy(R.normal_equations(q[sl], c, union))
        if q_idx is not None:
            q_idx.reshape(frames, -1)[f] = torch.from_numpy(corr["idx"].astype(np.int32))
            q_d2.reshape(frames, -1)[f] = torch.from_numpy(corr["d2"].astype(np.float32))


def align_solve(partial, n_rows, n_queries, final_call, D, istate, hist, result, sums=None):
    from mvtracker_amd import hip
    calls.append("align_solve")
    if int(istate[hip.ALIGN_I_DONE]):
        return
    S = partial.reshape(-1, hip.ALIGN_ROW)[:n_rows].numpy().sum(0)
    if sums is not None:
        sums[:hip.ALIGN_ROW] = torch.from_numpy(S)
    ev, iters, status = int(istate[hip.ALIGN_I_EVALS]), int(istate[hip.ALIGN_I_ITERATIONS]), int(istate[hip.ALIGN_I_STATUS])
    fit, rmse = R.figures(S, float(n_queries[0]))
    h = hist.reshape(-1, hip.ALIGN_HIST)
    if ev < h.shape[0]:
        h[ev] = torch.tensor([S[27], fit, rmse, S[28], 0, 0, 0, 0, 0, 0], dtype=torch.float64)
    done = 0
    if ev > 0 and abs(fit - float(result[0])) < 1e-6 and abs(rmse - float(result[1])) < 1e-6:
        done = 1
    elif not final_call:
        x, st = R.solve(S)
        if x is None:
            status |= st
            done = 1
        else:
            Dn = R.transform_of(x) @ np.vstack([D.reshape(3, 4).numpy(), [0, 0, 0, 1]])
            D.reshape(3, 4).copy_(torch.from_numpy(Dn[:3]))
            if ev < h.shape[0]:
                h[ev, 4:] = torch.from_numpy(x)
            iters += 1
    result[:4] = torch.tensor([fit, rmse, iters, status], dtype=torch.float64)
    istate[hip.ALIGN_I_DONE], istate[hip.ALIGN_I_ITERATIONS], istate[hip.ALIGN_I_STATUS], istate[hip.ALIGN_I_EVALS] = done, iters, status, ev + 1


def install(monkeypatch):
    import sys
    from mvtracker_amd import hip
    hip_mock_clean.install(monkeypatch)
    me = sys.modules[__name__]
    del calls[:]
    del searches[:]
    for name in "align_normals align_transform align_correspond align_solve".split():
        monkeypatch.setattr(hip, name, getattr(me, name))
