"""CPU stand-ins for the motion mask entries of mvtracker_amd.hip (motion_temporal, motion_mask, motion_report), on top of
tests/hip_mock_cluster.py (and with it the cleaning and query sampling mocks): the host code of mvtracker_amd/motion.py and the
motion path of mvtracker_amd/queries.py run on CPU tensors.  The fake entries follow the kernels' contract stage by stage with the
pieces of the restatement tests/motion_ref.py: the diff maps or their maximum, the windowed and pooled mask with per-tile counts, the
report's sums.  ``calls`` lists the entries called, in order, and ``args`` what each was called with (shapes and settings)."""
import numpy as np
import torch

import hip_mock_cluster
import motion_ref as R

calls = []
args = []


def motion_temporal(rgbs, V, T, H, W, all_mode, out, partial):
    from mvtracker_amd import hip
    calls.append("motion_temporal")
    args.append(dict(dtype=rgbs.dtype, shape=(V, T, H, W), all_mode=bool(all_mode)))
    assert rgbs.dtype in (torch.uint8, torch.float32) and rgbs.is_contiguous() and tuple(rgbs.shape) == (V, T, 3, H, W) and T >= 2
    d = R.boundary_diffs(rgbs.numpy())
    assert out.numel() == V * (1 if all_mode else T - 1) * H * W and partial.dtype == torch.float64
    out.reshape(V, -1, H, W)[:] = torch.from_numpy(d.max(1, keepdims=True) if all_mode else d)
    x = rgbs.numpy().astype(np.float64)
    rows = partial.reshape(V, hip.motion_blocks(H, W), T - 1)
    rows.zero_()
    rows[:, 0] = torch.from_numpy(np.abs(x[:, 1:] - x[:, :-1]).sum(axis=(2, 3, 4)))  # (a view's whole sum in its first row)


def motion_mask(src, V, T, H, W, win, r, thresh, mask, counts):
    from mvtracker_amd import hip
    calls.append("motion_mask")
    args.append(dict(win=win, r=r, thresh=thresh))
    assert win >= 0 and 0 <= r <= 15 and mask.dtype == torch.bool and tuple(mask.shape) == (V, T, H, W)
    d = src.reshape(V, -1, H, W).numpy()
    assert d.shape[1] == (T - 1 if win > 0 else 1)
    for t in range(T):
        m = d[:, max(0, t - win):min(T - 2, t + win - 1) + 1].max(1) if win > 0 else d[:, 0]
        pad = np.full((V, H + 2 * r, W + 2 * r), -np.inf, np.float32)
        pad[:, r:r + H, r:r + W] = m
        pooled = np.max(np.stack([pad[:, dy:dy + H, dx:dx + W] for dy in range(2 * r + 1) for dx in range(2 * r + 1)]), 0)
        mask[:, t] = torch.from_numpy(pooled < np.float32(thresh))
    c = counts.reshape(V * (T if win > 0 else 1), hip.motion_tiles(H, W))
    c.zero_()
    c[:, 0] = (mask if win > 0 else mask[:, :1]).reshape(c.shape[0], -1).sum(1).int()  # (an image's whole count in its first tile)


def motion_report(partial, counts, V, T, H, W, all_mode, report):
    calls.append("motion_report")
    report[:T - 1] = partial.reshape(-1, T - 1).sum(0)
    c = counts.reshape(V, -1, counts.shape[-1]).sum(-1).double()  # (V, T) or (V, 1)
    report[T - 1:] = c.expand(V, T).reshape(-1)


def install(monkeypatch):
    import sys
    from mvtracker_amd import hip
    hip_mock_cluster.install(monkeypatch)
    me = sys.modules[__name__]
    del calls[:]
    del args[:]
    for name in "motion_temporal motion_mask motion_report".split():
        monkeypatch.setattr(hip, name, getattr(me, name))
