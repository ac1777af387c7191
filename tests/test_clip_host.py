"""The depth-clip front end, host side (no GPU): ``clip.DepthClip``'s rank and shape rules, its lazy conversions, the padded-cloud
chunking and cropping, and ``clip.list_cloud``, on the mocked kernels of tests/hip_mock_clean.py.  The clip is V=2, T=3, H=5, W=9: the
smallest one whose padding matters (Hp=8, Wp=16, P=128)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hip_mock_clean  # noqa: E402

V, T, H, W = 2, 3, 5, 9
HP, WP, P = 8, 16, 128


@pytest.fixture
def launches(monkeypatch):
    """The mocks, with ``hip.invert_cameras`` and ``hip.clean_points`` recording (name, scalar arguments) before they run."""
    from mvtracker_amd import hip
    hip_mock_clean.install(monkeypatch)
    seen = []
    for name in ("invert_cameras", "clean_points"):
        inner = getattr(hip, name)
        monkeypatch.setattr(hip, name, (lambda n, f: lambda *a: (seen.append((n,) + tuple(x for x in a if not isinstance(x, torch.Tensor))), f(*a))[1])(
            name, inner))
    return seen


def make_clip(dtype=torch.float64):
    """(depths, intrs, extrs, conf) with the leading batch of 1; fp64, so that the conversions have something to do."""
    g = torch.Generator().manual_seed(0)
    depths = 1.0 + torch.rand(1, V, T, 1, H, W, generator=g, dtype=dtype)
    conf = torch.rand(1, V, T, 1, H, W, generator=g, dtype=dtype)
    intrs = torch.tensor([[8.0, 0.0, W / 2], [0.0, 8.0, H / 2], [0.0, 0.0, 1.0]], dtype=dtype).expand(1, V, T, 3, 3).clone()
    extrs = torch.zeros(1, V, T, 3, 4, dtype=dtype)
    extrs[..., :3, :3] = torch.eye(3, dtype=dtype)
    extrs[0, :, :, 0, 3] = 0.05 * torch.arange(V, dtype=dtype)[:, None] + 0.01 * torch.arange(T, dtype=dtype)[None]
    return depths, intrs, extrs, conf


# ----------------------------------------------------------------------------------------------------------------------- ranks
def test_both_ranks_give_the_same_clip(launches):
    from mvtracker_amd.clip import DepthClip
    d, k, e, c = make_clip()
    a = DepthClip(d, k, e, c)
    b = DepthClip(d[0], k[0], e[0], c[0])
    assert launches == []  # construction checks; it converts and launches nothing
    assert (a.batched, b.batched) == (True, False)
    for clip in (a, b):
        assert (clip.V, clip.T, clip.H, clip.W, clip.dev) == (V, T, H, W, d.device)
        assert clip.d.shape == (V, T, 1, H, W) and clip.d.dtype == torch.float32 and clip.d.is_contiguous()
        assert clip.K.shape == (V, T, 9) and clip.E.shape == (V, T, 12) and clip.K.dtype == clip.E.dtype == torch.float32
        assert clip.kinv.shape == (V * T, 9) and clip.einv.shape == (V * T, 12)
    assert torch.equal(a.d, b.d) and torch.equal(a.d, d[0].float())
    assert torch.equal(a.kinv, b.kinv) and torch.equal(a.einv, b.einv)
    assert launches == [("invert_cameras", V * T)] * 2  # one launch per clip, at the first request, however often it is asked
    x = torch.zeros(V, T, 1, H, W)
    assert a.rebatch(x).shape == (1, V, T, 1, H, W) and b.rebatch(x) is x
    assert DepthClip(d, k, e, c, batch="required").batched


def test_ranks_that_are_refused(launches):
    from mvtracker_amd.clip import DepthClip
    d, k, e, c = make_clip()
    bad = [dict(args=(d[0], k[0], e[0], c[0]), batch="required"),            # "required" refuses the clip rank
           dict(args=(d.expand(2, -1, -1, -1, -1, -1), k.expand(2, -1, -1, -1, -1), e.expand(2, -1, -1, -1, -1), None)),   # a batch of 2
           dict(args=(d.expand(2, -1, -1, -1, -1, -1), k.expand(2, -1, -1, -1, -1), e.expand(2, -1, -1, -1, -1), None), batch="required"),
           dict(args=(d, k[0], e[0], None)), dict(args=(d[0], k, e, None)),   # mixed ranks
           dict(args=(d, k, e[0], None)), dict(args=(d, k, e, c[0])), dict(args=(d[0], k[0], e[0], c)),
           dict(args=(d, k[0], e[0], None), batch="required"),
           dict(args=(d[0, 0], k[0, 0], e[0, 0], None))]                      # no views
    for case in bad:
        with pytest.raises(ValueError):
            DepthClip(*case["args"], batch=case.get("batch", "either"))
    assert launches == []


# -------------------------------------------------------------------------------------------------------------- shape refusals
@pytest.mark.parametrize("batch", ["either", "required"])
def test_shape_defects_raise_before_any_launch(launches, batch):
    from mvtracker_amd.clip import DepthClip
    d, k, e, c = make_clip()
    defects = [(d.expand(-1, -1, -1, 2, -1, -1), k, e, None),  # depths with two channels
               (d, k[..., :2], e, None), (d, k[:, :1], e, None), (d, k[:, :, :2], e, None),  # wrong intrs
               (d, k, e[..., :3], None), (d, k, e[:, :, :2], None), (d, k, k, None),         # wrong extrs
               (d, k, e, c[..., :4, :]), (d, k, e, c[:, :1]), (d, k, e, c[:, :, :, 0])]       # wrong depths_conf
    for args in defects:
        with pytest.raises(ValueError):
            DepthClip(*args, batch=batch)
        if batch == "either":
            with pytest.raises(ValueError):
                DepthClip(*(None if t is None else t[0] for t in args))
    assert launches == []


# ------------------------------------------------------------------------------------------------------------------------ conf
def test_conf_is_converted_only_under_a_threshold(launches):
    from mvtracker_amd.clip import DepthClip
    d, k, e, c = make_clip()
    clip = DepthClip(d, k, e, c)
    assert clip.conf(None) is None and "_conf32" not in vars(clip)  # a map without a threshold: not read, not converted
    got = clip.conf(0.5)
    assert got.dtype == torch.float32 and got.is_contiguous() and got.shape == clip.d.shape and torch.equal(got, c[0].float())
    assert clip.conf(0.0) is got
    assert DepthClip(d, k, e).conf(0.5) is None
    assert launches == []


# ---------------------------------------------------------------------------------------------------------------- padded clouds
def test_padded_grid_and_frame_chunks(launches):
    from mvtracker_amd.clip import DepthClip, frames_per_chunk
    clip = DepthClip(*make_clip())
    assert clip.padded_grid() == (HP, WP, P)
    assert clip.frame_chunks(V * P) == [(0, 1), (1, 1), (2, 1)]
    assert clip.frame_chunks(2 * V * P) == [(0, 2), (2, 1)]
    assert clip.frame_chunks(1 << 40) == [(0, 3)]
    assert clip.frame_chunks(1) == [(0, 1), (1, 1), (2, 1)]  # never less than a frame
    # today's rule, max(1, min(T, max_points // (V * P), 65535 // V)), on the arithmetic alone
    assert frames_per_chunk(40000, 100, 64, 1 << 40) == 1       # 65535 clouds a launch
    assert frames_per_chunk(2, 100000, 64, 1 << 40) == 32767
    assert frames_per_chunk(3, 100, 64, 3 * 64 * 7 + 5) == 7     # the workspace bound
    assert frames_per_chunk(3, 5, 64, 1 << 40) == 5              # the clip
    big = torch.zeros(1).expand(1, 1, 1, 1, 46341, 46337)  # (one float of storage); padded to 46344 x 46344 >= 2^31 - 64 points
    with pytest.raises(ValueError, match="too large"):
        DepthClip(big, torch.eye(3).reshape(1, 1, 1, 3, 3), torch.eye(4)[:3].reshape(1, 1, 1, 3, 4)).padded_grid()
    assert launches == []


def test_clouds_launch_through_the_module_and_crop_cuts_the_padding(launches):
    from mvtracker_amd.clip import DepthClip
    d, k, e, c = make_clip()
    clip = DepthClip(d, k, e, c)
    xyz = clip.clouds(1, 2, 0.25, sphere=(0.0, 0.0, 1.5, 9.0))
    assert launches == [("invert_cameras", V * T), ("clean_points", V, T, 1, 2, H, W, 0.25, (0.0, 0.0, 1.5, 9.0))]
    assert xyz.shape == (V * 2, P, 4) and xyz.dtype == torch.float32
    valid = clip.crop(torch.isfinite(xyz[..., 0]), 2)  # the pixels that entered the clouds: conf > 0.25 (all depths are valid)
    assert torch.equal(valid, c[0, :, 1:3, 0].float() > 0.25)
    grid = xyz.reshape(V, 2, HP, WP, 4)[..., :3]  # the padding holds NaN rows
    assert bool(torch.isnan(grid[:, :, H:]).all()) and bool(torch.isnan(grid[:, :, :, W:]).all())
    clip.clouds(0, 1, None)
    # the cameras are inverted once; without a threshold no confidence map is passed (the None in front)
    assert launches[2:] == [("clean_points", None, V, T, 0, 1, H, W, None, None)]
    for nt in (1, 3):
        ramp = torch.arange(V * nt * P).reshape(V * nt, P)
        got = clip.crop(ramp, nt)
        assert got.shape == (V, nt, H, W) and torch.equal(got, ramp.reshape(V, nt, HP, WP)[:, :, :H, :W])
        assert int(got[1, nt - 1, 2, 3]) == ((1 * nt + nt - 1) * HP + 2) * WP + 3
        rows = torch.stack([ramp, -ramp], -1)  # trailing dimensions are kept
        assert torch.equal(clip.crop(rows, nt), torch.stack([got, -got], -1))


# ------------------------------------------------------------------------------------------------------------------ list_cloud
def test_list_cloud(launches):
    from mvtracker_amd import DepthCleaning, align_point_clouds, clean_point_cloud, cluster_points, estimate_normals
    from mvtracker_amd.clip import list_cloud
    p = torch.arange(18, dtype=torch.float64).reshape(6, 3) / 7
    p[1, 2] = float("inf")
    p[4, 0] = float("nan")
    xyz = list_cloud(p)
    assert xyz.shape == (1, 6, 4) and xyz.dtype == torch.float32
    assert bool(torch.isnan(xyz[0, [1, 4], :3]).all())                  # one bad coordinate takes the whole row out
    assert torch.equal(xyz[0, [0, 2, 3, 5], :3], p[[0, 2, 3, 5]].float())  # finite rows are copied
    assert bool((xyz[0, :, 3] == 0).all())
    for bad in (torch.zeros(6), torch.zeros(6, 4), torch.zeros(1, 6, 3), torch.zeros(3, 6)):
        with pytest.raises(ValueError, match="source must be"):
            list_cloud(bad, "source")
    # M = 0: refused with the caller's name for it, or, for the callers that answer an empty list themselves, an empty cloud
    with pytest.raises(ValueError, match="target is empty"):
        list_cloud(p[:0], "target")
    assert list_cloud(p[:0], empty_ok=True).shape == (1, 0, 4)
    assert clean_point_cloud(p[:0], DepthCleaning()).shape == (0,)
    assert cluster_points(p[:0]).shape == (0,)
    with pytest.raises(ValueError, match="points is empty"):
        estimate_normals(p[:0])
    with pytest.raises(ValueError, match="source is empty"):
        align_point_clouds(p[:0], p, p, 0.05, 3)
    assert launches == [] and hip_mock_clean.calls == []
