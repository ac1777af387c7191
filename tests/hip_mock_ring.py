"""Torch-CPU stand-ins for the ring forms of mvtracker_amd.hip -- TEST INFRASTRUCTURE ONLY (see tests/hip_mock.py).

Each ring entry is restated through its linear one: the resident frames [lo, hi] of the ring -- frame f in slot (f - base) mod R --
are gathered into a linear store of hi - lo + 1 frames, and the matching function of hip_mock.py runs on that with frame0 - lo.
"""
import torch

import hip_mock


def ring_slots(ring):
    """Slots of the resident frames lo .. hi, in frame order."""
    base, R, lo, hi = ring
    assert R > 0 and base <= lo <= hi and hi - lo < R, ring
    return torch.tensor([(f - base) % R for f in range(lo, hi + 1)])


def _linear(t, ring, per_frame):
    """(R, ...) ring tensor -> contiguous (hi - lo + 1, per_frame) linear store of the resident frames."""
    R = ring[1]
    return t.reshape(R, -1)[:, :per_frame].index_select(0, ring_slots(ring)).contiguous()


def _f0(frame0, ring):
    assert ring[2] <= frame0 <= ring[3], (frame0, ring)
    return frame0 - ring[2], ring[3] - ring[2] + 1


def knn_scan_ring(xyz, Pn, coords, N, S, frame0, frame_step, ring, K, nseg, keys, seed_idx=None, seed_k=0, seed_dims=(0, 0, 0, 0), box=None,
                  grid=(0, 0)):
    f0, T = _f0(frame0, ring)
    hip_mock.knn_scan(_linear(xyz, ring, Pn * 4), Pn, coords, N, S, f0, frame_step, T, K, nseg, keys, seed_idx=seed_idx, seed_k=seed_k,
                      seed_dims=seed_dims, box=None, grid=grid)


def knn_search_ring(xyz, Pn, coords, N, S, frame0, frame_step, ring, K, idx_out, box, grid=(0, 0), gbox=None, seed_idx=None, seed_k=0,
                    seed_dims=(0, 0, 0, 0)):
    f0, T = _f0(frame0, ring)
    hip_mock.knn_search(_linear(xyz, ring, Pn * 4), Pn, coords, N, S, f0, frame_step, T, K, idx_out, None, grid=grid, gbox=None,
                        seed_idx=seed_idx, seed_k=seed_k, seed_dims=seed_dims)


def _levels(levels, ring):
    return [dict(lv, xyz=_linear(lv["xyz"], ring, lv["P"] * 4), box=None, gbox=None) for lv in levels]


def knn_scan_levels_ring(levels, coords, N, S, frame0, frame_step, ring, K, seed_k=0):
    f0, T = _f0(frame0, ring)
    hip_mock.knn_scan_levels(_levels(levels, ring), coords, N, S, f0, frame_step, T, K, seed_k=seed_k)


def knn_search_levels_ring(levels, coords, N, S, frame0, frame_step, ring, K, seed_k):
    f0, T = _f0(frame0, ring)
    hip_mock.knn_search_levels(_levels(levels, ring), coords, N, S, f0, frame_step, T, K, seed_k)


def corr_gather_dot_ring(xyz_l, fvec_l, P_l, idx_l, Cc, targets, coords, N, S, frame0, frame_step, ring, K, out, ldo, o_off):
    f0, T = _f0(frame0, ring)
    hip_mock.corr_gather_dot([_linear(x, ring, p * 4) for x, p in zip(xyz_l, P_l)], [_linear(f, ring, p * Cc) for f, p in zip(fvec_l, P_l)],
                             P_l, idx_l, Cc, targets, coords, N, S, f0, frame_step, T, K, out, ldo, o_off)


def corr_gather_dot_opts_ring(xyz_l, fvec_l, P_l, idx_l, Cc, targets, coords, N, S, frame0, frame_step, ring, K, groups, add_offset, add_xyz,
                              out, ldo, o_off):
    f0, T = _f0(frame0, ring)
    hip_mock.corr_gather_dot_opts([_linear(x, ring, p * 4) for x, p in zip(xyz_l, P_l)],
                                  [_linear(f, ring, p * Cc) for f, p in zip(fvec_l, P_l)], P_l, idx_l, Cc, targets, coords, N, S, f0,
                                  frame_step, T, K, groups, add_offset, add_xyz, out, ldo, o_off)


def knn1_gather_ring(fvec, Pn, Cc, keys, n, nseg, frame, ring, feat_out, idx_out=None):
    f0, _ = _f0(frame, ring)
    hip_mock.knn1_gather(_linear(fvec, ring, Pn * Cc), Pn, Cc, keys, n, nseg, f0, feat_out, idx_out)


def conv2d(x, wt, bias, out, n, H, W, Cin, Cout, KH, KW, stride, pad, ldo, act=0):
    """hip_mock.conv2d image by image.  The library's convolutions do not depend on how many images a call holds; torch's CPU
    convolution blocks by batch size and may differ in the last bit between a frame encoded alone and inside a larger call, which
    is what a session and ``forward`` do with the same frame."""
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    xf, of = x.reshape(-1), out.reshape(-1)
    assert out.is_contiguous()
    for i in range(n):
        hip_mock.conv2d(xf[i * H * W * Cin:(i + 1) * H * W * Cin], wt, bias, of[i * Ho * Wo * ldo:], 1, H, W, Cin, Cout, KH, KW, stride, pad,
                        ldo, act)


def install(monkeypatch):
    """hip_mock.install plus the ring forms (and a convolution that does not depend on the batch size)."""
    import sys
    from mvtracker_amd import hip
    hip_mock.install(monkeypatch)
    me = sys.modules[__name__]
    for name in ("knn_scan_ring knn_search_ring knn_scan_levels_ring knn_search_levels_ring corr_gather_dot_ring corr_gather_dot_opts_ring "
                 "knn1_gather_ring conv2d").split():
        monkeypatch.setattr(hip, name, getattr(me, name))
