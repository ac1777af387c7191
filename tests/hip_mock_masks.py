"""CPU stand-ins for the mask query entries of mvtracker_amd.hip (mask_stats, mask_centroids, mask_match, mask_relabel, mask_pool),
on top of tests/hip_mock_queries.py (and with it the pool and k-means mocks): the host code of mvtracker_amd/masks.py runs on CPU
tensors.  The fake entries follow the kernels' contract with the pieces of the restatement tests/mask_ref.py, on hip_mock.unproject's
points.  ``calls`` lists the entries called, in order; ``reads`` counts the host copies ``masks._readback`` made."""
import numpy as np
import torch

import hip_mock
import hip_mock_queries
import mask_ref as R

calls = []
reads = []


def _points(depths, kinv, einv, V, T, H, W):
    ds = depths.reshape(V, T, H, W).permute(1, 0, 2, 3).contiguous()
    xyz = torch.empty(T, V, H, W, 4)
    hip_mock.unproject(ds, kinv, einv, xyz, V, T, H, W, 1, 0)
    return xyz[..., :3].permute(1, 0, 2, 3, 4).numpy()  # (V,T,H,W,3)


def _valid(labels, depths, conf, V, T, H, W, dmin, dmax, thr):
    opt = R.options(min_depth=dmin, max_depth=dmax, conf_thresh=None if conf is None else thr)
    return R.valid_pixels(labels.numpy().astype(np.int64), depths.reshape(V, T, 1, H, W).numpy(), opt,
                          None if conf is None else conf.reshape(V, T, 1, H, W).numpy())


def mask_stats(labels, depths, conf, kinv, einv, V, T, H, W, min_depth, max_depth, conf_thresh, stats):
    from mvtracker_amd import hip
    calls.append("mask_stats")
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (V, T, H, W) and stats.dtype == torch.int64
    lab = labels.numpy().astype(np.int64)
    ok = _valid(labels, depths, conf, V, T, H, W, min_depth, max_depth, conf_thresh)
    pts = _points(depths, kinv, einv, V, T, H, W)
    with np.errstate(invalid="ignore"):
        in_range = ok & (np.abs(pts) < np.float32(2.0 ** hip.MASK_RANGE_BITS)).all(-1)
    q = np.rint(np.where(in_range[..., None], pts, 0).astype(np.float64) * 2 ** hip.MASK_FRAC_BITS).astype(np.int64)
    s = np.zeros((V, T, hip.MASK_LABELS, hip.MASK_STAT_WORDS), np.int64)
    for v in range(V):
        for t in range(T):
            l = lab[v, t].reshape(-1)
            s[v, t, :, hip.MASK_PIXELS] = np.bincount(l, minlength=256)
            s[v, t, :, hip.MASK_COUNT] = np.bincount(l[in_range[v, t].reshape(-1)], minlength=256)
            s[v, t, :, hip.MASK_OUT_OF_RANGE] = np.bincount(l[(ok & ~in_range)[v, t].reshape(-1)], minlength=256)
            for c in range(3):
                np.add.at(s[v, t, :, hip.MASK_SUM + c], l, q[v, t, :, :, c].reshape(-1))
    s[:, :, 0] = 0
    stats.reshape(s.shape).copy_(torch.from_numpy(s))


def mask_centroids(stats, V, T, min_pixels, centroid):
    from mvtracker_amd import hip
    calls.append("mask_centroids")
    s = stats.reshape(V, T, 256, hip.MASK_STAT_WORDS).numpy()
    centroid.reshape(V, T, 256, 3).copy_(torch.from_numpy(R.centroids(s[..., hip.MASK_COUNT], s[..., hip.MASK_SUM:hip.MASK_SUM + 3], min_pixels)))


def mask_match(centroid, V, T, min_common_frames, distance_threshold, match, ids, global_id, distance, state):
    calls.append("mask_match")
    m = R.matching(centroid.reshape(V, T, 256, 3).numpy(), R.options(min_common_frames=min_common_frames, distance_threshold=distance_threshold,
                                                                    match=bool(match)))
    global_id.reshape(V, 256).copy_(torch.from_numpy(m["global_id"]))
    distance.reshape(V, 256).copy_(torch.from_numpy(m["distance"]))
    state[0] = m["num_objects"]
    state[1] = sum(len(x) for x in m["members"].values())


def mask_relabel(labels, table, V, T, H, W, out):
    calls.append("mask_relabel")
    lab = labels.long()
    o = torch.stack([table.reshape(V, 256)[v][lab[v]] for v in range(V)])
    out.copy_(torch.where(lab != 0, o, torch.full_like(o, -1)))


def mask_pool(labels, depths, conf, kinv, einv, V, T, t, H, W, min_depth, max_depth, conf_thresh, table, obj, pool, pixel, count, block_counts):
    calls.append("mask_pool")
    ok = _valid(labels, depths, conf, V, T, H, W, min_depth, max_depth, conf_thresh)[:, t]
    lab = labels[:, t].long()
    g = torch.stack([table.reshape(V, 256)[v][lab[v]] for v in range(V)]).numpy()
    idx = np.nonzero((ok & (g == obj)).reshape(-1))[0]
    pts = _points(depths, kinv, einv, V, T, H, W)[:, t].reshape(-1, 3)[idx]
    n = min(len(idx), pixel.numel())
    pool[:n] = torch.from_numpy(pts[:n])
    pixel[:n] = torch.from_numpy(idx[:n].astype(np.int32))
    count[0] = len(idx)


def _readback(t):
    reads.append(tuple(t.shape))
    return t.cpu().numpy()


def install(monkeypatch):
    import sys
    from mvtracker_amd import hip, masks
    hip_mock_queries.install(monkeypatch)
    me = sys.modules[__name__]
    del calls[:]
    del reads[:]
    for name in "mask_stats mask_centroids mask_match mask_relabel mask_pool".split():
        monkeypatch.setattr(hip, name, getattr(me, name))
    monkeypatch.setattr(masks, "_readback", _readback)
