"""numpy restatement of the motion masks ("Motion masks"), written from the rule, not from the reference's code:

    d_b      = ((|dc0| + |dc1|) + |dc2|) / 3.0f     fp32, boundary b between frames b and b + 1, uint8 converted to fp32 first
    change   = max of d_b over b in [t - win, t + win - 1] n [0, T - 2] and over |dy|, |dx| <= r clipped to the image
    static   = change < fp32(thresh)                win = window, or T for window == -1; T == 1: everything static

and of the static-prefix rule of the reference demo.  tests/golden/motion_mask.npz holds what the reference's own functions give."""
import numpy as np


def boundary_diffs(frames):
    """frames (V, T, 3, H, W) uint8 / float -> (V, T-1, H, W) fp32."""
    x = np.asarray(frames).astype(np.float32)
    a = np.abs(x[:, 1:] - x[:, :-1])
    return ((a[:, :, 0] + a[:, :, 1]) + a[:, :, 2]) / np.float32(3.0)


def change_map(frames, window=-1, r=7):
    """(V, T, H, W) fp32; T >= 2."""
    d = boundary_diffs(frames)
    V, B, H, W = d.shape
    T = B + 1
    if not (window == -1 or window >= 1):
        raise ValueError(window)
    win = T if window == -1 else int(window)
    out = np.empty((V, T, H, W), np.float32)
    for t in range(T):
        lo, hi = max(0, t - win), min(T - 2, t + win - 1)
        m = d[:, lo:hi + 1].max(1)
        pad = np.full((V, H + 2 * r, W + 2 * r), -np.inf, np.float32)
        pad[:, r:r + H, r:r + W] = m
        rows = np.max(np.stack([pad[:, :, k:k + W] for k in range(2 * r + 1)]), 0)
        out[:, t] = np.max(np.stack([rows[:, k:k + H] for k in range(2 * r + 1)]), 0)
    return out


def static_mask(frames, window=-1, r=7, thresh=10.0):
    """(V, T, H, W) bool."""
    V, T, _, H, W = np.asarray(frames).shape
    if T == 1:
        return np.ones((V, T, H, W), bool)
    return change_map(frames, window, r) < np.float32(thresh)


def boundary_mean_diff(frames):
    """(T-1,) fp64: the mean of |frame b+1 - frame b| over views, channels and pixels, in fp64 throughout."""
    x = np.asarray(frames).astype(np.float32).astype(np.float64)
    return np.abs(x[:, 1:] - x[:, :-1]).sum(axis=(0, 2, 3, 4)) / float(x.shape[0] * x.shape[2] * x.shape[3] * x.shape[4])


def static_prefix(diffs, n_frames, diff_threshold=0.5, max_frames=10):
    """Frame 0, then frame i + 1 while delta_i <= threshold and fewer than max_frames are taken; stops at the first failure."""
    if n_frames == 0:
        return []
    frames = [0]
    for i in range(n_frames - 1):
        if float(diffs[i]) <= diff_threshold and len(frames) < max_frames:
            frames.append(i + 1)
        else:
            break
    return frames
