"""The clip the track-overlay tests share (tests/test_overlay_host.py, tests/test_gpu_overlay.py): V = 2 views, T = 7 frames, N = 70
tracks (more than one wave), frames of 40 x 56.

View 0 is the camera K = [[8, 0, 0], [0, 8, 0], [0, 0, 1]], E = [I | 0]: a world point (px / 8, py / 8, 1) lands on the integer pixel
(px, py) exactly, so the planted tracks are placed by hand.  View 1 is a rotated, shifted camera with non-dyadic entries: there the
order of the sums matters.  Planted, in view 0 (``SPECIAL`` names the tracks):
  cross_a / cross_b   two tracks on integer pixels that cross each other twice, different rows at their query frame (different
                      rainbow colours)
  nan, inf, zero_z    a NaN coordinate at frame 3; an infinite x at frame 4 (0 * inf makes its row NaN: invalid); camera z == 0 at
                      frame 2 (a division by zero: +-inf, clipped to +-1e4, a segment that leaves the picture)
  behind              camera z = -1 from frame 3 on: drawn mirrored without min_depth, not drawn with it
  x_zero, origin      pixel (0, 12) at frame 3 (no marker, but its segments); pixel (0, 0) at frame 3 (nothing)
  still               the same pixel in every frame: segments with a == b
  diagonal            pixel (1, 1) at frame 3, (54, 38) at frame 4: a segment across the whole picture
Query frames are 0, 2 and 5 by i % 3 (the planted tracks: 0); about a third of the points are invisible; the other tracks drift on
non-integer positions."""
import numpy as np

V, T, N, H, W = 2, 7, 70, 40, 56
SPECIAL = dict(cross_a=0, cross_b=1, nan=2, inf=3, zero_z=4, behind=5, x_zero=6, origin=7, still=8, diagonal=9)


def cameras():
    K = np.zeros((V, T, 3, 3), np.float32)
    E = np.zeros((V, T, 3, 4), np.float32)
    K[0] = np.array([[8, 0, 0], [0, 8, 0], [0, 0, 1]], np.float32)
    E[0, :, :, :3] = np.eye(3, dtype=np.float32)
    a = 0.3
    rot = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    for t in range(T):
        K[1, t] = np.array([[7.3, 0.01, 3.7], [0, 7.1, 1.9], [0, 0, 1]], np.float32)
        E[1, t, :, :3] = rot.astype(np.float32)
        E[1, t, :, 3] = np.array([-0.9 + 0.013 * t, 0.11, 0.37], np.float32)
    return K, E


def pixel(px, py, z=1.0):
    """The world point that view 0 sees at pixel (px, py) with camera z (exact for z = +-1 and coordinates in eighths)."""
    return np.array([px * z / 8.0, py * z / 8.0, z], np.float32)


def clip(seed=0, float_frames=False):
    rng = np.random.default_rng(seed)
    tracks = np.zeros((T, N, 3), np.float32)
    start = rng.uniform((4, 4), (W - 4, H - 4), (N, 2))
    step = rng.uniform(-3.5, 3.5, (N, 2))
    for t in range(T):
        p = start + t * step + rng.normal(0, 0.3, (N, 2))
        tracks[t, :, 0], tracks[t, :, 1], tracks[t, :, 2] = p[:, 0] / 8.0, p[:, 1] / 8.0, 1.0
    S = SPECIAL
    for t in range(T):
        tracks[t, S["cross_a"]] = pixel(6 + 7 * t, 8 + 4 * (t % 2) * 2)       # rows 8, 16, 8, ...
        tracks[t, S["cross_b"]] = pixel(6 + 7 * t, 16 - 4 * (t % 2) * 2)      # rows 16, 8, 16, ...: crosses cross_a between frames
        tracks[t, S["nan"]] = pixel(20 + t, 30)
        tracks[t, S["inf"]] = pixel(30 + t, 32)
        tracks[t, S["zero_z"]] = pixel(12 + 2 * t, 24)
        tracks[t, S["behind"]] = pixel(40 - 2 * t, 10 + 3 * t, 1.0 if t < 3 else -1.0)
        tracks[t, S["x_zero"]] = pixel(3 * abs(t - 3), 12)
        tracks[t, S["origin"]] = pixel(4 * abs(t - 3), 5 * abs(t - 3))
        tracks[t, S["still"]] = pixel(30, 20)
        tracks[t, S["diagonal"]] = pixel(1, 1) if t <= 3 else pixel(54, 38)
    tracks[3, S["nan"], 1] = np.nan
    tracks[4, S["inf"], 0] = np.inf
    tracks[2, S["zero_z"], 2] = 0.0
    query_frames = np.array([0, 2, 5], np.int64)[np.arange(N) % 3]
    query_frames[:len(S)] = 0
    visibility = rng.random((T, N)) > 0.33
    visibility[:, S["cross_a"]] = True
    if float_frames:
        rgbs = rng.uniform(-30.0, 290.0, (V, T, 3, H, W)).astype(np.float32)
        rgbs[0, 1, 2, 5, 7] = np.nan
        rgbs[1, 2, 0, 3, 3] = np.inf
        rgbs[1, 2, 1, 3, 3] = 254.99998
    else:
        rgbs = rng.integers(0, 256, (V, T, 3, H, W), dtype=np.uint8)
    K, E = cameras()
    colors = rng.integers(0, 256, (N, 3), dtype=np.uint8)
    return dict(rgbs=rgbs, tracks=tracks, visibility=visibility, query_frames=query_frames, intrs=K, extrs=E, colors=colors)
