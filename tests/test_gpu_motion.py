"""Motion masks on the device: every comparison is ``torch.equal`` / ``np.array_equal`` against the restatement tests/motion_ref.py
or against the reference's recorded masks (tests/golden/motion_mask.npz).

1. The fixture's three (window, r) configurations on its clips, uint8 and the same frames as float32 (identical masks), the 0..1
   clip with the threshold 10 / 255, and the recorded static prefixes from the report.
2. A planted pixel: V = 2, T = 5, H = 19, W = 70 (one partial tile row, a second tile column of 6 pixels: narrower than any halo
   with r >= 7), constant frames but for one pixel of view 0 that changes by 30 in one channel at boundary 2, so its channel mean is
   exactly 10.0, which is not < 10: the moving set must be exactly the (2r+1)^2 square clipped to the image in the frames
   [b - win + 1, b + win] (all frames for window -1), in view 0 only; with a change of 29 everything is static.  The pixel at
   (0, 0), at (H-1, W-1) and inside; r 0, 7, 15; windows 1, 2, -1.
3. window >= T-1 equals window -1; T == 2 (a single boundary); several tiles in both directions (33 x 65).
4. Non-integer float frames: the (a + b) + c and / 3 order, to the bit.
5. The report on integer frames: boundary_mean_diff equal to the fp64 value, static_fraction equal to the mask's own means, two
   calls the same bits.
6. sample_queries(motion=...) on a synthetic clip with a planted moving block: every query unprojects from a moving pixel.
Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_align_cases as Cs  # noqa: E402
import motion_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "motion_mask.npz")


def device_mask(frames, window, r, thresh=10.0):
    from mvtracker_amd import MotionMask, motion_masks
    static, report = motion_masks(torch.from_numpy(np.ascontiguousarray(frames)).to(DEV), MotionMask(window, r, thresh))
    torch.cuda.synchronize()
    assert static.dtype == torch.bool and static.is_cuda and tuple(static.shape) == frames[:, :, 0].shape
    return static.cpu(), report


def test_fixture_masks_uint8_and_float32():
    g = np.load(GOLDEN)
    configs = [tuple(int(x) for x in c) for c in g["configs"]]
    assert configs == [(-1, 7), (2, 3), (1, 0)]
    for name in ("moving", "prefix", "unit"):
        frames = g[name + "_frames"] if name != "unit" else g["moving_frames"].astype(np.float32) / np.float32(255.0)
        thresh = float(g[name + "_thresh"][0])
        for i, (win, r) in enumerate(configs):
            exp = torch.from_numpy(np.unpackbits(g[f"{name}_static_{i}"])[:frames[:, :, 0].size].reshape(frames[:, :, 0].shape).astype(bool))
            got, report = device_mask(frames, win, r, thresh)
            print(f"{name} window {win} r {r}: static {float(exp.float().mean()):.3f}, mismatches {int((got != exp).sum())}")
            assert torch.equal(got, exp)
            if frames.dtype == np.uint8:
                as_float, report_f = device_mask(frames.astype(np.float32), win, r, thresh)
                assert torch.equal(as_float, exp)
                assert np.array_equal(report.boundary_mean_diff, report_f.boundary_mean_diff) and np.array_equal(report.static_fraction, report_f.static_fraction)
        if name != "unit":
            for j, (thr, mx) in enumerate(g["prefix_rules"]):
                assert report.static_prefix_frames(thr, int(mx)) == g[f"{name}_prefix_{j}"].tolist(), (name, thr, mx)
    assert device_mask(g["prefix_frames"], -1, 7)[1].static_prefix_frames() == [0, 1, 2, 3]


V2, T2, H2, W2, B2 = 2, 5, 19, 70, 2


def planted(y, x, change, dtype=np.uint8):
    f = np.full((V2, T2, 3, H2, W2), 100, dtype)
    f[0, B2 + 1:, 1, y, x] += change
    return f


@pytest.mark.parametrize("r", [0, 7, 15])
def test_planted_pixel(r):
    for y, x in ((0, 0), (H2 - 1, W2 - 1), (9, 62)):
        square = torch.zeros(H2, W2, dtype=torch.bool)
        square[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1] = True
        for window in (1, 2, -1):
            exp = torch.ones(V2, T2, H2, W2, dtype=torch.bool)
            t0, t1 = (0, T2 - 1) if window == -1 else (max(0, B2 - window + 1), min(T2 - 1, B2 + window))
            exp[0, t0:t1 + 1] = ~square
            frames = planted(y, x, 30)
            got = device_mask(frames, window, r)[0]
            print(f"pixel ({y}, {x}) r {r} window {window}: moving frames {t0}..{t1}, {int(square.sum())} pixels each, mismatches {int((got != exp).sum())}")
            assert np.array_equal(exp.numpy(), R.static_mask(frames, window, r))  # (the restatement says the same)
            assert torch.equal(got, exp)
            assert bool(device_mask(planted(y, x, 29), window, r)[0].all())
        assert torch.equal(device_mask(planted(y, x, 30, np.float32), 1, r)[0], device_mask(planted(y, x, 30), 1, r)[0])


def random_u8(V, T, H, W, seed):
    """A fixed image per view with a few percent of the pixels redrawn in every frame: masks that are neither empty nor full."""
    rng = np.random.default_rng(seed)
    f = np.repeat(rng.integers(0, 256, (V, 1, 3, H, W)), T, 1)
    for t in range(T):
        hit = rng.random((V, 1, H, W)) < 0.03
        f[:, t] = np.where(hit, rng.integers(0, 256, (V, 3, H, W)), f[:, t])
    return f.astype(np.uint8)


def test_wide_windows_and_two_frames():
    V, T, H, W = 2, 4, 33, 65  # 2 x 2 tiles, the second ones a single pixel wide / high; 3 blocks of the temporal pass, no whole groups of 4
    frames = random_u8(V, T, H, W, 5)
    for r in (0, 2):
        whole = device_mask(frames, -1, r)[0]
        exp = torch.from_numpy(R.static_mask(frames, -1, r))
        print(f"r {r}: static {float(exp.float().mean()):.3f}")
        assert 0 < exp.float().mean() < 1 and torch.equal(whole, exp)
        for window in (T - 1, T, T + 3):
            assert torch.equal(device_mask(frames, window, r)[0], whole), window
        for window in (1, T - 2):
            assert torch.equal(device_mask(frames, window, r)[0], torch.from_numpy(R.static_mask(frames, window, r))), window
    two = frames[:, :2]
    for window, r in ((-1, 0), (1, 3), (2, 7), (5, 15)):
        assert torch.equal(device_mask(two, window, r)[0], torch.from_numpy(R.static_mask(two, window, r))), (window, r)


def test_non_integer_float_frames():
    rng = np.random.default_rng(9)
    for H, W in ((33, 65), (24, 40)):  # element-wise and 16-byte loads
        frames = rng.random((2, 4, 3, H, W), dtype=np.float32)
        for window, r, thresh in ((1, 0, 0.4), (-1, 0, 0.55), (2, 1, 0.75)):
            exp = torch.from_numpy(R.static_mask(frames, window, r, thresh))
            got = device_mask(frames, window, r, thresh)[0]
            print(f"{H} x {W} window {window} r {r} thresh {thresh}: static {float(exp.float().mean()):.3f}, mismatches {int((got != exp).sum())}")
            assert 0 < exp.float().mean() < 1 and torch.equal(got, exp)
    # diffs a single ulp either side of a threshold: the division must be the correctly rounded one
    d = R.boundary_diffs(frames)
    thresh = float(np.sort(d.reshape(-1))[d.size // 2])
    for th in (thresh, float(np.nextafter(np.float32(thresh), np.float32(1)))):
        assert torch.equal(device_mask(frames, 1, 0, th)[0], torch.from_numpy(R.static_mask(frames, 1, 0, th)))


def test_report_exact_and_deterministic():
    for H, W in ((33, 65), (40, 72)):
        frames = random_u8(2, 5, H, W, 7)
        for window, r in ((-1, 3), (2, 3)):
            static, report = device_mask(frames, window, r)
            again, report2 = device_mask(frames, window, r)
            exp_diff = R.boundary_mean_diff(frames)
            print(f"{H} x {W} window {window}: boundary mean diffs {report.boundary_mean_diff.tolist()} static fraction {report.static_fraction.mean():.4f}")
            assert report.boundary_mean_diff.dtype == np.float64 and np.array_equal(report.boundary_mean_diff, exp_diff)
            assert np.array_equal(report.static_fraction, static.sum((2, 3)).numpy() / float(H * W))
            assert torch.equal(static, again) and np.array_equal(report.static_fraction, report2.static_fraction)
            assert np.array_equal(report.boundary_mean_diff, report2.boundary_mean_diff)
            assert report.static_prefix_frames(1e9, 3) == [0, 1, 2] and report.static_prefix_frames(0.0) == [0]


def test_sample_queries_on_moving_pixels():
    from mvtracker_amd import MotionMask, motion_masks, sample_queries, synth
    V, T, H, W = 2, 4, 32, 48
    clip = synth.make_clip(21, V=V, T=T, H=H, W=W, N=4, rgb_dtype=np.uint8)
    rgbs = np.repeat(clip["rgbs"][:, :, :1], T, 2)  # a still clip ...
    for t in range(T):
        rgbs[0, 0, t, :, 10:16, 8 + 3 * t:16 + 3 * t] += 128  # ... and a block (every channel off by 128, modulo 256) that moves in view 0
    d, K, E = (torch.from_numpy(clip[k]).to(DEV) for k in ("depths", "intrs", "extrs"))
    cfg = MotionMask(1, 1)
    t = 1
    q = sample_queries(d, K, E, [(t, -100.0, 100.0, 1000.0, 40, "")], seed=3, motion=cfg, rgbs=torch.from_numpy(rgbs).to(DEV))
    static = motion_masks(torch.from_numpy(rgbs).to(DEV), cfg)[0].cpu().numpy()
    assert np.array_equal(static, R.static_mask(rgbs[0], 1, 1))
    pts = Cs.unproject(clip["depths"], clip["intrs"], clip["extrs"])[:, t].reshape(-1, 3)
    moving = ~static[:, t].reshape(-1)
    valid = np.isfinite(pts).all(1)
    got = q[0].cpu().numpy().astype(np.float64)
    dist = np.linalg.norm(np.where(valid[None, :, None], pts[None], 1e9) - got[:, None, 1:], axis=-1)
    nearest = dist.argmin(1)
    print(f"{len(got)} queries, moving valid pixels {int((moving & valid).sum())} of {int(valid.sum())}, largest distance to a pixel's point {dist.min(1).max():.3g}")
    assert len(got) == 40 and (got[:, 0] == t).all() and 40 < (moving & valid).sum() < valid.sum() / 2
    assert dist.min(1).max() < 1e-4 and moving[nearest].all() and (nearest < H * W).all()  # view 0 only: nothing moves in view 1
    plain = sample_queries(d, K, E, [(t, -100.0, 100.0, 1000.0, 40, "")], seed=3)
    assert not torch.equal(plain, q)
