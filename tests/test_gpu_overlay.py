"""Track overlays on the device: every picture comparison is ``torch.equal`` against the restatement tests/overlay_ref.py (a
sequential painter that redraws every frame from scratch; the device scatters keys into a line layer that persists over the frames).

The clip is tests/overlay_cases.py: V = 2, T = 7, N = 70 (more than one wave of tracks), 40 x 56, uint8 and float frames, with
integer-placed crossing tracks, query frames 0, 2 and 5, a NaN point, an inf point, a division by zero, a point behind the camera, a
point with x == 0 and one at (0, 0), a segment with a == b, a segment across the whole picture diagonal and invisible points.

1. The integer points equal a numpy float32 replay of the stated operation sequence, exactly (pad 0 / 16, min_depth None / 0.05),
   and ``project_tracks`` gives the replay's bits.
2. CONFIGS: trail -1 / 0 / 1 / 3, pad 0 / 16, linewidth 1 / 2 (and 3 and 8), min_depth None / 0.05, explicit colours and "rainbow",
   max_tracks 5: the overlay and the colours equal the restatement, a second run gives the same bits, and a session in blocks of
   1, 3 and the rest gives the whole clip's bits.
3. ``project_tracks`` against the fixture tests/golden/overlay.npz: its maximum error against the fp64 values must not exceed twice
   the maximum error of the reference's own fp32 output against the same values (only the order of the sums differs).
   Measured on MI355X: see DESIGN section 8 "Track overlays".
4. One predictor call with ``track_overlay=TrackOverlay()`` on a synthetic clip.
Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlay_cases as Cs  # noqa: E402
import overlay_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "overlay.npz")

# (float frames, TrackOverlay arguments; colors="explicit" stands for the clip's own colour table)
CONFIGS = [
    (False, dict()),
    (True, dict(trail=0, pad=16, linewidth=1, min_depth=0.05, colors="explicit")),
    (False, dict(trail=1, pad=16, colors="explicit")),
    (True, dict(trail=3, linewidth=1)),
    (False, dict(trail=3, pad=16, min_depth=0.05)),
    (False, dict(trail=1, linewidth=1, min_depth=0.05, max_tracks=5)),
    (True, dict(pad=16, linewidth=1, min_depth=0.05, colors="explicit")),
    (False, dict(max_tracks=5, colors="explicit")),
    (False, dict(trail=3, linewidth=3, pad=3, color_view=1)),
    (True, dict(linewidth=8, trail=1)),
]

_clips = {}


def clip(float_frames):
    """(numpy clip, device tensors), built once per frame type and left unchanged."""
    if float_frames not in _clips:
        c = Cs.clip(float_frames=float_frames)
        _clips[float_frames] = (c, {k: torch.from_numpy(v).to(DEV) for k, v in c.items()})
    return _clips[float_frames]


def args_of(c):
    return c["rgbs"], c["tracks"], c["visibility"], c["query_frames"], c["intrs"], c["extrs"]


def test_integer_points_equal_the_float32_replay():
    from mvtracker_amd import overlay, project_tracks
    n, d = clip(False)
    px, py, z = R.project(n["tracks"], n["intrs"], n["extrs"])
    xyz = project_tracks(d["tracks"], d["intrs"], d["extrs"]).cpu().numpy()
    same = np.array_equal(xyz, np.stack([px, py, z], -1), equal_nan=True)
    print("project_tracks equals the float32 replay:", same, "; NaN values", int(np.isnan(xyz).sum()), "infinite", int(np.isinf(xyz).sum()))
    assert xyz.shape == (Cs.V, Cs.T, Cs.N, 3) and same and np.isnan(xyz).any() and np.isinf(xyz).any() and (xyz[..., 2] < 0).any()
    for pad in (0, 16):
        for min_depth in (None, 0.05):
            got = overlay.track_pixels(d["tracks"], d["intrs"], d["extrs"], pad=pad, min_depth=min_depth).cpu().numpy()
            x, y, valid = R.integer_points(px, py, z, pad, min_depth)
            want = np.stack([x, y, valid], -1)
            print(f"pad {pad} min_depth {min_depth}: {int((~valid).sum())} invalid points, mismatches {int((got != want).any(-1).sum())}")
            assert got.dtype == np.int32 and np.array_equal(got, want) and (~valid).any()


@pytest.mark.parametrize("case", range(len(CONFIGS)))
def test_overlay_equals_the_restatement(case):
    from mvtracker_amd import TrackOverlay, open_track_overlay, render_track_overlays
    float_frames, kw = CONFIGS[case]
    n, d = clip(float_frames)
    lut = np.load(GOLDEN)["lut"]
    explicit = kw.get("colors") == "explicit"
    o = TrackOverlay(**(dict(kw, colors=d["colors"]) if explicit else kw))
    want, want_cols = R.render(*args_of(n), lut=lut, **(dict(kw, colors=n["colors"]) if explicit else kw))
    video, cols = render_track_overlays(*args_of(d), o)
    torch.cuda.synchronize()
    pad = o.pad
    drawn = int((want[:, :, :, pad:pad + Cs.H, pad:pad + Cs.W] != R.to_u8(n["rgbs"])).any(2).sum())
    bad = int((video.cpu().numpy() != want).any(2).sum())
    print(f"{'float' if float_frames else 'uint8'} frames {kw}: {drawn} pixels drawn, {bad} pixels differ from the restatement")
    assert video.dtype == torch.uint8 and tuple(video.shape) == (Cs.V, Cs.T, 3, Cs.H + 2 * pad, Cs.W + 2 * pad) and drawn > 200
    assert torch.equal(video.cpu(), torch.from_numpy(want)) and torch.equal(cols.cpu(), torch.from_numpy(want_cols))
    again, cols2 = render_track_overlays(*args_of(d), o)
    assert torch.equal(again, video) and torch.equal(cols2, cols)
    s = open_track_overlay(d["query_frames"], Cs.V, Cs.H, Cs.W, o)
    parts, a = [], 0
    for b in (1, 3, Cs.T - 4):
        parts.append(s.push(d["rgbs"][:, a:a + b], d["tracks"][a:a + b], d["visibility"][a:a + b], d["intrs"][:, a:a + b], d["extrs"][:, a:a + b]))
        a += b
    assert torch.equal(torch.cat(parts, 1), video) and torch.equal(s.colors, cols) and int((s.marker_keys != 0).sum()) == 0


def test_visibility_none_draws_discs():
    from mvtracker_amd import render_track_overlays
    n, d = clip(False)
    a, na = list(args_of(d)), list(args_of(n))
    a[2] = na[2] = None
    video = render_track_overlays(*a)[0]
    assert torch.equal(video.cpu(), torch.from_numpy(R.render(*na, lut=np.load(GOLDEN)["lut"])[0]))


def test_project_tracks_error_bar():
    from mvtracker_amd import project_tracks
    g = np.load(GOLDEN)
    got = project_tracks(*(torch.from_numpy(g[k]).to(DEV) for k in ("proj_tracks", "proj_intrs", "proj_extrs"))).cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - g["proj_f64"]).max())
    err_ref = float(np.abs(g["proj_ref"].astype(np.float64) - g["proj_f64"]).max())
    print(f"project_tracks max |error| vs fp64 {err:.4g}; the reference's own fp32 output {err_ref:.4g}; bound {2 * err_ref:.4g}")
    assert got.shape == (3, 5, 64, 3) and g["proj_f64"][..., 2].min() >= 0.5
    assert err <= 2 * err_ref


def test_predictor_track_overlay():
    from mvtracker_amd import EvaluationPredictor, TrackOverlay, project_tracks, synth
    from mvtracker_amd.tracker import MVTracker
    m = MVTracker(hidden_size=256).eval()
    sd = synth.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    p = EvaluationPredictor(m.to(DEV), interp_shape=(96, 96), grid_size=2, n_iters=2)  # the tracker works at 96 x 96, the overlay at 128 x 128
    V, T, H, W, N = 2, 8, 128, 128, 12
    c = {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_clip(5, V=V, T=T, H=H, W=W, N=N, late_queries=True, query_frames=(2,), rgb_dtype=np.uint8).items()}
    kw = dict(rgbs=c["rgbs"], depths=c["depths"], query_points_3d=c["query_points"], intrs=c["intrs"], extrs=c["extrs"])
    plain = p(**kw)
    assert p.last_track_overlay is None
    res = p(**kw, track_overlay=TrackOverlay())
    video, cols = p.last_track_overlay
    torch.cuda.synchronize()
    assert all(torch.equal(res[k], plain[k]) for k in ("traj_e", "vis_e", "vis_e_as_prob"))
    assert tuple(video.shape) == (V, T, 3, H, W) and video.dtype == torch.uint8 and video.is_cuda and tuple(cols.shape) == (N, 3) and cols.dtype == torch.uint8
    # a visible track whose query-frame point lies inside a view: the marker's centre has the track's colour, which the frame has not
    qf = c["query_points"][0, :, 0].long()
    pix = project_tracks(res["traj_e"][0], c["intrs"][0], c["extrs"][0])  # (V,T,N,3)
    # (an invisible point is a ring: there the pixel 4 to the right of the centre, which a disc covers too)
    assert bool(torch.isfinite(pix).all())
    pix = pix.cpu().numpy().astype(np.int64)  # truncation toward zero, as the rule's
    hits = {True: 0, False: 0}
    for v in range(V):
        for n in range(N):
            t = int(qf[n])
            visible = bool(res["vis_e"][0, t, n])
            x, y = int(pix[v, t, n, 0]) + (0 if visible else 4), int(pix[v, t, n, 1])
            later = [i for i in range(n + 1, N) if int(qf[i]) <= t and (pix[v, t, i, 0] - x) ** 2 + (pix[v, t, i, 1] - y) ** 2 <= 25]
            if 8 < x < W - 8 and 8 < y < H - 8 and not later:
                hits[visible] += 1
                assert torch.equal(video[v, t, :, y, x], cols[n]) and not torch.equal(c["rgbs"][0, v, t, :, y, x], cols[n]), (v, n, t, x, y, visible)
    print("query pixels checked (visible, invisible):", hits[True], hits[False], "; pixels drawn:", int((video != c["rgbs"][0]).any(2).sum()))
    assert hits[True] >= 1 and hits[True] + hits[False] >= 4 and bool((video != c["rgbs"][0]).any())
