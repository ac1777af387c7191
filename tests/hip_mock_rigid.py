"""CPU stand-ins for the rigid-motion entries of mvtracker_amd.hip (rigid_members, rigid_fit, rigid_compose, rigid_move, rigid_fill), on
top of tests/hip_mock_masks.py (and with it the predictor's mocks): the host code of mvtracker_amd/rigid.py runs on CPU tensors.  The
fake entries follow the kernels' contract with the pieces of the restatement tests/rigid_ref.py.  ``calls`` lists the entries called,
in order; ``reads`` counts the host reads ``rigid._readback`` made."""
import numpy as np
import torch

import hip_mock_masks
import rigid_ref as R

calls = []
reads = []


def _put(dst, src):
    dst.copy_(torch.from_numpy(np.ascontiguousarray(src)).reshape(dst.shape))


def rigid_members(object_ids, query_frames, N, G, T, counts, offsets, members, reference_frames):
    calls.append("rigid_members")
    assert object_ids.dtype == torch.int32 and query_frames.dtype == torch.int32 and object_ids.numel() == N
    mem = R.member_lists(object_ids.numpy(), G)
    _put(counts, np.array([len(m) for m in mem], np.int32))
    _put(offsets, np.concatenate([[0], np.cumsum([len(m) for m in mem])]).astype(np.int32))
    flat = np.concatenate(mem + [np.zeros(0, np.int64)]).astype(np.int32)
    members[:len(flat)] = torch.from_numpy(flat)
    _put(reference_frames, R.reference_frames(object_ids.numpy(), query_frames.numpy(), G, T))


def rigid_fit(tracks, visibility, query_frames, object_ids, offsets, members, reference_frames, T, N, G, inlier_threshold, iterations, min_points,
              use_visibility, min_spread, live_before_query, poses, residual, inliers, used, inlier_count, rmse, status):
    calls.append("rigid_fit")
    assert tuple(tracks.shape) == (T, N, 3) and tracks.is_contiguous() and visibility.dtype == torch.bool and tuple(visibility.shape) == (T, N)
    ids = object_ids.numpy().copy()
    ids[(ids < 0) | (ids >= G)] = -1
    ref = R.rigid_motion(tracks.numpy(), visibility.numpy(), query_frames.numpy(), ids,
                         R.options(inlier_threshold, iterations, min_points, bool(use_visibility), min_spread, bool(live_before_query)), num_objects=G)
    assert np.array_equal(ref["reference_frames"], reference_frames.numpy())
    for k, dst in dict(poses=poses, residual=residual, inliers=inliers, used=used, inlier_count=inlier_count, rmse=rmse, status=status).items():
        _put(dst, ref[k])


def rigid_compose(poses, status, G, T, frame, xf):
    calls.append("rigid_compose")
    _put(xf, R.transforms(poses.numpy().reshape(G, T, 4, 4), status.numpy().reshape(G, T), frame))


def rigid_move(points, point_objects, xf, M, T, G, out):
    calls.append("rigid_move")
    x = xf.numpy().reshape(G, T, 3, 4)
    ids = point_objects.numpy().astype(np.int64)
    ok = (ids >= 0) & (ids < G)
    o = np.full((T, M, 3), np.nan)
    m = x[ids[ok]]
    with np.errstate(invalid="ignore"):
        o[:, ok] = np.einsum("mtij,mj->tmi", m[..., :3], points.numpy().astype(np.float64)[ok]) + m[..., 3].transpose(1, 0, 2)
    _put(out, o.astype(np.float32))


def rigid_fill(tracks, visibility, inliers, query_frames, object_ids, reference_frames, poses, status, T, N, G, replace, live_before_query, out,
               filled):
    calls.append("rigid_fill")
    motion = dict(status=status.numpy().reshape(G, T), inliers=inliers.numpy(), reference_frames=reference_frames.numpy(),
                  poses=poses.numpy().reshape(G, T, 4, 4))
    names = tuple(n for n, bit in (("occluded", 1), ("outliers", 2)) if replace & bit)
    o, f = R.fill_tracks(tracks.numpy(), visibility.numpy(), query_frames.numpy(), object_ids.numpy(), motion, names, bool(live_before_query))
    _put(out, o)
    _put(filled, f)


def _readback(t):
    reads.append(tuple(t.shape))
    return int(t.item())


def install(monkeypatch):
    import sys
    from mvtracker_amd import hip, rigid
    hip_mock_masks.install(monkeypatch)
    me = sys.modules[__name__]
    del calls[:]
    del reads[:]
    for name in "rigid_members rigid_fit rigid_compose rigid_move rigid_fill".split():
        monkeypatch.setattr(hip, name, getattr(me, name))
    monkeypatch.setattr(rigid, "_readback", _readback)
