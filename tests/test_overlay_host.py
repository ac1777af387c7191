"""Track overlays, host side (no GPU): the restatement tests/overlay_ref.py against hand counts, literal bitmaps and the fixture
tests/golden/overlay.npz (matplotlib's gist_rainbow and its Normalize rule); that the shared clip can catch a wrong painter's order;
then the host code of mvtracker_amd/overlay.py and the predictor's wiring on mocked kernels (tests/hip_mock_overlay.py): exports,
validation before any launch, ``track_overlay=None`` calls nothing, sessions in blocks, the demo's flags.  Every figure is printed
before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hip_mock_overlay as M  # noqa: E402
import overlay_cases as Cs  # noqa: E402
import overlay_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "overlay.npz")


def bitmap(ys, xs, h, w):
    a = np.zeros((h, w), int)
    a[ys, xs] = 1
    return ["".join(".#"[v] for v in row) for row in a]


def test_hand_counts_and_literal_bitmaps():
    ys, xs = R.stroke((2, 3), (6, 3), 2, 20, 20)
    got = sorted(zip(xs.tolist(), ys.tolist()))
    want = sorted([(x, y) for y in (2, 3, 4) for x in range(2, 7)] + [(1, 3), (7, 3)])
    print("w = 2 stroke (2,3)-(6,3):", len(got), "pixels; disc R = 4:", len(R.disc((10, 10), 4, 30, 30)[0]), "ring R = 4:", len(R.ring((10, 10), 4, 30, 30)[0]))
    assert got == want and len(got) == 17
    assert len(R.disc((10, 10), 4, 30, 30)[0]) == 49 and len(R.ring((10, 10), 4, 30, 30)[0]) == 32
    assert not set(zip(*R.ring((10, 10), 4, 30, 30))) & set(zip(*R.disc((10, 10), 3, 30, 30)))  # a ring is hollow
    assert bitmap(*R.stroke((1, 1), (6, 4), 2, 7, 9), 7, 9) == [
        ".#.......",
        "###......",
        ".####....",
        "...####..",
        ".....###.",
        "......#..",
        "........."]
    assert bitmap(*R.stroke((6, 4), (1, 1), 2, 7, 9), 7, 9) == bitmap(*R.stroke((1, 1), (6, 4), 2, 7, 9), 7, 9)  # either direction
    assert bitmap(*R.stroke((3, 3), (3, 3), 2, 7, 7), 7, 7) == [".......", ".......", "...#...", "..###..", "...#...", ".......", "......."]
    assert bitmap(*R.stroke((3, 3), (3, 3), 3, 7, 7), 7, 7) == [".......", ".......", "..###..", "..###..", "..###..", ".......", "......."]
    assert bitmap(*R.stroke((3, 3), (3, 3), 1, 7, 7), 7, 7) == [".......", ".......", ".......", "...#...", ".......", ".......", "......."]
    # clipped to the picture: a disc at a corner, a stroke that starts far outside
    assert len(R.disc((0, 0), 4, 30, 30)[0]) == 17 and len(R.stroke((-10000, 3), (2, 3), 1, 8, 8)[0]) == 3
    assert len(R.stroke((100, 100), (200, 200), 2, 8, 8)[0]) == 0


def test_colour_table_and_index_rule_equal_the_fixture():
    from mvtracker_amd import overlay
    g = np.load(GOLDEN)
    table = np.frombuffer(overlay.GIST_RAINBOW, np.uint8).reshape(256, 3)
    assert g["lut"].shape == (256, 3) and np.array_equal(table, g["lut"]) and os.path.getsize(GOLDEN) < 256 * 1024
    rows, rgb = g["color_y_hp"], g["color_rgb"]
    assert len(rows) > 700 and rows[:, 0].min() == -5 and (rows[:, 0] >= rows[:, 1]).sum() >= 20 and {72, 40} <= set(rows[:, 1].tolist())
    mine = np.array([table[overlay.rainbow_index(y, hp)] for y, hp in rows])
    print("colour rows", len(rows), "mismatches", int((mine != rgb).any(1).sum()))
    assert np.array_equal(mine, rgb)
    c = Cs.clip()
    x, y, valid = R.integer_points(*R.project(c["tracks"], c["intrs"], c["extrs"]), 16)
    cols = R.rainbow_colors(table, x, y, valid, c["query_frames"], 0, 16, Cs.H + 32)
    n = Cs.SPECIAL["cross_a"]
    assert y[0, 0, n] == 8 + 16 and np.array_equal(cols[n], table[(24 * 256) // 72]) and not np.array_equal(cols[n], cols[Cs.SPECIAL["cross_b"]])


def test_projection_restatement_against_the_fixture():
    g = np.load(GOLDEN)
    px, py, z = R.project(g["proj_tracks"], g["proj_intrs"], g["proj_extrs"])
    mine = np.stack([px, py, z], -1)
    assert mine.dtype == np.float32 and mine.shape == (3, 5, 64, 3) and g["proj_f64"][..., 2].min() >= 0.5
    err_mine, err_ref = np.abs(mine - g["proj_f64"]).max(), np.abs(g["proj_ref"] - g["proj_f64"]).max()
    print(f"restatement max |error| vs fp64 {err_mine:.3g}, the reference's own {err_ref:.3g}")
    assert err_mine <= 2 * err_ref


def test_the_clip_can_catch_a_wrong_order():
    g = np.load(GOLDEN)
    c = Cs.clip()
    kw = dict(lut=g["lut"], colors=c["colors"])
    a = (c["rgbs"], c["tracks"], c["visibility"], c["query_frames"], c["intrs"], c["extrs"])
    ops = {}
    video, cols = R.render(*a, ops_out=ops, **kw)
    found = dict(newer_over_older=0, higher_index_same_s=0, marker_over_line=0, ring=0)
    for (v, t), lst in ops.items():
        top = {}  # pixel -> the op that owns it so far
        for op in lst:
            for p in zip(op["ys"].tolist(), op["xs"].tolist()):
                prev = top.get(p)
                if prev is not None and not np.array_equal(cols[prev["i"]], cols[op["i"]]):
                    if op["kind"] == "line" and prev["kind"] == "line":
                        found["newer_over_older" if op["s"] > prev["s"] else "higher_index_same_s"] += 1
                        assert op["s"] > prev["s"] or (op["s"] == prev["s"] and op["i"] > prev["i"])
                    elif op["kind"] != "line" and prev["kind"] == "line":
                        found["marker_over_line"] += 1
                top[p] = op
            found["ring"] += len(op["ys"]) if op["kind"] == "ring" else 0
    # trail = 1: a pixel of the last frame that an older segment covers and no segment of the window does, and no marker
    t = Cs.T - 1
    outside = 0
    for v in range(Cs.V):
        old = set(p for op in ops[(v, t)] if op["kind"] == "line" and op["s"] < t - 1 for p in zip(op["ys"].tolist(), op["xs"].tolist()))
        new = set(p for op in ops[(v, t)] if op["kind"] != "line" or op["s"] >= t - 1 for p in zip(op["ys"].tolist(), op["xs"].tolist()))
        outside += len(old - new)
    print(found, "pixels covered only from outside a trail of 1:", outside)
    assert all(n > 0 for n in found.values()) and outside > 0
    backwards = R.render(*a, reverse=True, **kw)[0]
    diff = int((backwards != video).any(2).sum())
    print("pixels that change when every frame is painted in reversed order:", diff)
    assert diff > 0
    short = R.render(*a, trail=1, **kw)[0]
    assert (short[:, t] != video[:, t]).any() and np.array_equal(short[:, 1], video[:, 1])
    assert np.array_equal(R.render(*a, trail=Cs.T, **kw)[0], video)
    # what the special tracks are there for
    x, y, valid = R.integer_points(*R.project(c["tracks"], c["intrs"], c["extrs"]))
    S = Cs.SPECIAL
    assert not valid[0, 3, S["nan"]] and not valid[0, 4, S["inf"]] and valid[0, 2, S["zero_z"]] and x[0, 2, S["zero_z"]] == 10000
    assert (x[0, 3, S["x_zero"]], y[0, 3, S["x_zero"]]) == (0, 12) and (x[0, 3, S["origin"]], y[0, 3, S["origin"]]) == (0, 0)
    assert (x[0, 3, S["diagonal"]], y[0, 3, S["diagonal"]], x[0, 4, S["diagonal"]], y[0, 4, S["diagonal"]]) == (1, 1, 54, 38)
    assert valid[0, 4, S["behind"]] and not R.integer_points(*R.project(c["tracks"], c["intrs"], c["extrs"]), 0, 0.05)[2][0, 4, S["behind"]]
    kinds = {(op["kind"], op["i"]) for op in ops[(0, 3)] if op["s"] >= 2}
    assert ("line", S["x_zero"]) in kinds and not {("disc", S["x_zero"]), ("ring", S["x_zero"])} & kinds  # x == 0: the segment, no marker
    assert not any(op["i"] == S["origin"] and op["s"] in (2, 3) for op in ops[(0, 4)])  # (0, 0): nothing touches it
    assert not (c["visibility"].all() or not c["visibility"].any()) and sorted(set(c["query_frames"].tolist())) == [0, 2, 5]


def test_exports_and_constants(tmp_path):
    import shutil
    import subprocess
    import mvtracker_amd
    from mvtracker_amd import TrackOverlay, TrackOverlaySession, hip, open_track_overlay, overlay, project_tracks, render_track_overlays, stack_views
    assert TrackOverlay is overlay.TrackOverlay and render_track_overlays is overlay.render_track_overlays and project_tracks is overlay.project_tracks
    assert open_track_overlay is overlay.open_track_overlay and stack_views is overlay.stack_views and TrackOverlaySession is overlay.TrackOverlaySession
    assert {"overlay", "TrackOverlay", "TrackOverlaySession", "project_tracks", "render_track_overlays", "open_track_overlay", "stack_views"} <= set(mvtracker_amd.__all__)
    assert all(n in hip.SIGNATURES for n in ("mvt_overlay_project", "mvt_overlay_draw", "mvt_overlay_compose")) and hip.abi_version() == 9
    o = TrackOverlay()
    assert (o.trail, o.linewidth, o.pad, o.colors, o.color_view, o.min_depth, o.max_tracks) == (-1, 2, 0, "rainbow", 0, None, None)
    with pytest.raises(Exception):
        o.trail = 3  # frozen
    v = torch.arange(2 * 3 * 3 * 4 * 5, dtype=torch.uint8).reshape(2, 3, 3, 4, 5)
    s = stack_views(v)
    assert tuple(s.shape) == (3, 3, 8, 5) and torch.equal(s[:, :, :4], v[0]) and torch.equal(s[:, :, 4:], v[1])
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    names = dict(MVT_OVERLAY_MAX_LINEWIDTH=hip.OVERLAY_MAX_LINEWIDTH, MVT_OVERLAY_MAX_PAD=hip.OVERLAY_MAX_PAD, MVT_OVERLAY_MAX_SIDE=hip.OVERLAY_MAX_SIDE,
                 MVT_OVERLAY_MAX_INDEX=hip.OVERLAY_MAX_INDEX)
    lines = ['#include <stdio.h>', '#include "mvtracker_hip.h"', 'int main(void) {'] + [f'  printf("{n} %d\\n", {n});' for n in names] + ['  return 0;', '}']
    (tmp_path / "probe.c").write_text("\n".join(lines))
    p = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True).stdout.strip().split("\n"))
    assert {k: int(v) for k, v in got.items()} == names == dict(MVT_OVERLAY_MAX_LINEWIDTH=8, MVT_OVERLAY_MAX_PAD=64, MVT_OVERLAY_MAX_SIDE=8192,
                                                               MVT_OVERLAY_MAX_INDEX=1 << 20)


def test_entries_refuse_bad_arguments_without_a_launch():
    """Every mvt_overlay_* entry returns MVT_ERR_ARG (1) for null or misaligned pointers and for the shapes it refuses, before any HIP
    call (so this runs without a device)."""
    import ctypes
    from mvtracker_amd import hip
    lib = hip._lib
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.addressof(buf) + 15) // 16 * 16  # host memory: only looked at for alignment, never launched on
    proj = lambda *over: lib.mvt_overlay_project(*[over[i] if i < len(over) and over[i] is not ... else d for i, d in enumerate(
        (a, a, a, 2, 3, 4, a, a, 0, 0, 0.0, a, 0, a, 0, 40, a, None))])
    draw = lambda *over: lib.mvt_overlay_draw(*[over[i] if i < len(over) and over[i] is not ... else d for i, d in enumerate(
        (a, a, a, a, a, 2, 4, 4, 1, 2, 40, 56, a, a, None))])
    comp = lambda *over: lib.mvt_overlay_compose(*[over[i] if i < len(over) and over[i] is not ... else d for i, d in enumerate(
        (a, 1, 2, 3, 0, 40, 56, 0, a, 0, a, a, None))])
    E = ...
    rc = {
        "project null tracks": proj(None),
        "project misaligned extrs": proj(E, E, a + 2),
        "project no views": proj(E, E, E, 0),
        "project too many tracks": proj(E, E, E, E, E, 1 << 20),
        "project no output": proj(E, E, E, E, E, E, None, None, E, E, E, E, E, None),
        "project misaligned points": proj(E, E, E, E, E, E, E, a + 4),
        "project pad": proj(E, E, E, E, E, E, E, E, 65),
        "project nan depth": proj(E, E, E, E, E, E, E, E, E, 1, float("nan")),
        "project colour view": proj(E, E, E, E, E, E, E, E, E, E, E, E, E, E, 2),
        "project picture height": proj(E, E, E, E, E, E, E, E, 20, E, E, E, E, E, E, 40),
        "project lut without colours": proj(E, E, E, E, E, E, E, E, E, E, E, E, E, E, E, E, None),
        "draw null points": draw(E, None),
        "draw lines without a plane": draw(E, E, E, E, E, E, E, E, E, E, E, E, None),
        "draw plane without lines": draw(None),
        "draw lines at frame 0": draw(E, E, E, E, E, E, E, E, 0),
        "draw more drawn than tracks": draw(E, E, E, E, E, E, E, 5),
        "draw no track drawn": draw(E, E, E, E, E, E, E, 0),
        "draw linewidth 0": draw(E, E, E, E, E, E, E, E, E, 0),
        "draw linewidth 9": draw(E, E, E, E, E, E, E, E, E, 9),
        "draw picture too large": draw(E, E, E, E, E, E, E, E, E, E, 8193),
        "draw frame number": draw(E, E, E, E, E, E, E, E, 1 << 20),
        "draw misaligned markers": draw(E, E, E, E, E, E, E, E, E, E, E, E, E, a + 4),
        "compose null frames": comp(None),
        "compose misaligned floats": comp(a + 2, 0),
        "compose frame outside": comp(E, E, E, E, 3),
        "compose pad": comp(E, E, E, E, E, E, E, 65),
        "compose picture too large": comp(E, E, E, E, E, 8193),
        "compose null markers": comp(E, E, E, E, E, E, E, E, E, E, None),
        "compose null out": comp(E, E, E, E, E, E, E, E, E, E, E, None),
        "compose negative window": comp(E, E, E, E, E, E, E, E, E, -1),
    }
    print(rc)
    assert all(v == 1 for v in rc.values()), rc


def clip_tensors(**kw):
    c = Cs.clip(**kw)
    return {k: torch.from_numpy(v) for k, v in c.items()}, c


def args_of(c):
    return c["rgbs"], c["tracks"], c["visibility"], c["query_frames"], c["intrs"], c["extrs"]


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    from mvtracker_amd import TrackOverlay, open_track_overlay, project_tracks, render_track_overlays
    M.install(monkeypatch)
    for kw in (dict(trail=-2), dict(trail=1.5), dict(trail=True), dict(linewidth=0), dict(linewidth=9), dict(pad=-1), dict(pad=65), dict(colors="cool"),
               dict(colors=torch.zeros(4, 3)), dict(colors=torch.zeros(4, 4, dtype=torch.uint8)), dict(color_view=-1), dict(min_depth=float("nan")),
               dict(min_depth="near"), dict(max_tracks=0), dict(max_tracks=2.5)):
        with pytest.raises(ValueError):
            TrackOverlay(**kw)
    assert TrackOverlay(trail=3.0, min_depth=1).trail == 3 and TrackOverlay(min_depth=1).min_depth == 1.0
    c, _ = clip_tensors()
    rgbs, tracks, vis, qf, K, E = args_of(c)
    bad = [(rgbs[0], tracks, vis, qf, K, E), (rgbs[:, :, :2], tracks, vis, qf, K, E), (rgbs.to(torch.int32), tracks, vis, qf, K, E),
           (rgbs, tracks[:-1], vis, qf, K, E), (rgbs, tracks[..., :2], vis, qf, K, E), (rgbs, tracks[:, :-1], vis, qf, K, E),
           (rgbs, tracks, vis[:, :-1], qf, K, E), (rgbs, tracks, vis.float(), qf, K, E), (rgbs, tracks, vis, qf[:-1], K, E),
           (rgbs, tracks, vis, qf[None], K, E), (rgbs, tracks, vis, qf, K[:1], E), (rgbs, tracks, vis, qf, K, E[:, :, :, :3]),
           (rgbs, tracks, vis, qf, K[:, :-1], E), (rgbs, tracks, vis, qf, K, E, "rainbow"), (rgbs, tracks, vis, qf, K, E, None),
           (rgbs, tracks, vis, qf, K, E, TrackOverlay(color_view=2)), (rgbs, tracks, vis, qf, K, E, TrackOverlay(colors=c["colors"][:-1]))]
    for a in bad:
        with pytest.raises(ValueError):
            render_track_overlays(*a)
    with pytest.raises(ValueError):
        render_track_overlays(torch.zeros(1, 1, 3, 8200, 8, dtype=torch.uint8), tracks[:1], None, qf, K[:1, :1], E[:1, :1])  # larger than the integers allow
    for a in ((tracks[0], K, E), (tracks, K[0], E), (tracks, K, E[:, :3])):
        with pytest.raises(ValueError):
            project_tracks(*a)
    with pytest.raises(ValueError):
        open_track_overlay(qf, 2, Cs.H, Cs.W, "rainbow")
    with pytest.raises(ValueError):
        open_track_overlay(qf, 0, Cs.H, Cs.W, TrackOverlay())
    s = open_track_overlay(qf, 2, Cs.H, Cs.W, TrackOverlay())
    for a in ((rgbs[:, :2, :, :-1], tracks[:2], vis[:2], K[:, :2], E[:, :2]), (rgbs[:, :2], tracks[:3], vis[:2], K[:, :2], E[:, :2]),
              (rgbs[:1, :2], tracks[:2], vis[:2], K[:1, :2], E[:1, :2])):
        with pytest.raises(ValueError):
            s.push(*a)
    print("entries called", M.calls)
    assert M.calls == [] and s.frames == 0


def test_render_on_the_mock_equals_the_restatement(monkeypatch):
    from mvtracker_amd import TrackOverlay, project_tracks, render_track_overlays
    from mvtracker_amd import overlay
    M.install(monkeypatch)
    g = np.load(GOLDEN)
    for float_frames, kw in ((False, dict()), (True, dict(trail=1, pad=16, linewidth=1, min_depth=0.05)), (False, dict(trail=0, max_tracks=5)),
                             (False, dict(trail=3, colors="explicit", pad=3))):
        c, n = clip_tensors(float_frames=float_frames)
        if kw.get("colors") == "explicit":
            kw = dict(kw, colors=c["colors"])
        del M.calls[:], M.args[:]
        video, cols = render_track_overlays(*args_of(c), TrackOverlay(**kw))
        ref_kw = dict(kw, colors=n["colors"]) if "colors" in kw else kw
        want, want_cols = R.render(*args_of(n), lut=g["lut"], **ref_kw)
        pad = kw.get("pad", 0)
        print(kw.keys(), "calls", len(M.calls), "pixels drawn", int((want[:, :, :, pad:pad + Cs.H, pad:pad + Cs.W] != R.to_u8(n["rgbs"])).any(2).sum()))
        assert video.dtype == torch.uint8 and tuple(video.shape) == (Cs.V, Cs.T, 3, Cs.H + 2 * pad, Cs.W + 2 * pad)
        assert np.array_equal(video.numpy(), want) and np.array_equal(cols.numpy(), want_cols) and tuple(cols.shape) == (Cs.N, 3)
        # one projection for the block, then a scatter and a compose per frame
        assert M.calls == ["overlay_project"] + ["overlay_draw", "overlay_compose"] * Cs.T
        assert M.args[0] == dict(shape=(Cs.V, Cs.T, Cs.N), pad=pad, min_depth=kw.get("min_depth"), frame0=0, color_view=0, Hp=Cs.H + 2 * pad,
                                 rainbow="colors" not in kw)
        draws = M.args[1::2]
        assert [d["t"] for d in draws] == list(range(Cs.T)) and all(d["M"] == kw.get("max_tracks", Cs.N) for d in draws)
        assert [d["lines"] for d in draws] == [kw.get("trail", -1) != 0 and t >= 1 for t in range(Cs.T)]
        trail = kw.get("trail", -1)
        assert [d["first_segment"] for d in M.args[2::2]] == [0 if trail < 0 else max(0, t - trail) for t in range(Cs.T)]
        assert all(d["dtype"] == (torch.float32 if float_frames else torch.uint8) for d in M.args[2::2])
    # visibility None: every marker a disc; a batch axis of 1 and double frames are taken
    c, n = clip_tensors()
    a = list(args_of(c))
    a[2] = None
    v0 = render_track_overlays(*a)[0]
    na = list(args_of(n))
    na[2] = None
    assert np.array_equal(v0.numpy(), R.render(*na, lut=g["lut"])[0])
    a[0] = a[0][None].double()
    assert torch.equal(render_track_overlays(*a)[0], v0)
    xyz = project_tracks(c["tracks"], c["intrs"], c["extrs"])
    assert tuple(xyz.shape) == (Cs.V, Cs.T, Cs.N, 3) and xyz.dtype == torch.float32
    assert np.array_equal(xyz.numpy(), np.stack(R.project(n["tracks"], n["intrs"], n["extrs"]), -1), equal_nan=True)
    px = overlay.track_pixels(c["tracks"], c["intrs"], c["extrs"], pad=16, min_depth=0.05)
    x, y, valid = R.integer_points(*R.project(n["tracks"], n["intrs"], n["extrs"]), 16, 0.05)
    assert px.dtype == torch.int32 and np.array_equal(px.numpy(), np.stack([x, y, valid], -1))


def test_session_blocks_equal_one_call(monkeypatch):
    from mvtracker_amd import TrackOverlay, open_track_overlay, render_track_overlays
    M.install(monkeypatch)
    for kw in (dict(), dict(trail=1, pad=16), dict(trail=3, linewidth=1, min_depth=0.05, max_tracks=40)):
        c, _ = clip_tensors()
        o = TrackOverlay(**kw)
        whole, cols = render_track_overlays(*args_of(c), o)
        s = open_track_overlay(c["query_frames"], Cs.V, Cs.H, Cs.W, o)
        parts, a = [], 0
        for b in (1, 3, Cs.T - 4):
            parts.append(s.push(c["rgbs"][:, a:a + b], c["tracks"][a:a + b], c["visibility"][a:a + b], c["intrs"][:, a:a + b], c["extrs"][:, a:a + b]))
            a += b
            late = c["query_frames"] >= a  # a track's colour is there once its query frame was pushed, not before
            assert not s.colors[late].any() and torch.equal(s.colors[~late], cols[~late])
        assert s.frames == Cs.T and torch.equal(torch.cat(parts, 1), whole) and torch.equal(s.colors, cols)
        assert int(s.marker_keys.abs().sum()) == 0  # the marker plane is clean between the frames
    # scratch does not grow with the clip
    assert tuple(s.marker_keys.shape) == tuple(s.line_keys.shape) == (Cs.V, Cs.H, Cs.W)
    assert open_track_overlay(c["query_frames"], Cs.V, Cs.H, Cs.W, TrackOverlay(trail=0)).line_keys is None


class FakeModel(torch.nn.Module):
    """Tracks in the world the model is given: the queries' own points, repeated over the frames."""

    def forward(self, rgbs, depths=None, query_points=None, intrs=None, extrs=None, **kw):
        self.seen = dict(rgbs=rgbs, extrs=extrs, kw=kw)
        T, n = rgbs.shape[2], query_points.shape[1]
        vis = torch.zeros(1, T, n)
        vis[:, :, ::2] = 1.0
        return {"traj_e": query_points[:, None, :, 1:].repeat(1, T, 1, 1).contiguous(), "vis_e": vis}


def predictor_inputs():
    rng = np.random.default_rng(3)
    V, T, H, W = 2, 3, 24, 32
    K = torch.tensor([[8.0, 0, 0], [0, 8.0, 0], [0, 0, 1]]).expand(1, V, T, 3, 3).contiguous()
    E = torch.zeros(1, V, T, 3, 4)
    E[..., :3] = torch.eye(3)
    E[:, 1, :, 0, 3] = 0.5  # view 1: shifted by 4 pixels
    q = torch.tensor([[[0.0, 10 / 8, 12 / 8, 1.0], [1.0, 20 / 8, 6 / 8, 1.0], [0.0, 5 / 8, 18 / 8, 1.0]]])
    return dict(rgbs=torch.from_numpy(rng.integers(0, 256, (1, V, T, 3, H, W), dtype=np.uint8)), depths=torch.ones(1, V, T, 1, H, W), query_points_3d=q,
                intrs=K, extrs=E)


def test_predictor_wiring(monkeypatch):
    import types
    from mvtracker_amd import EvaluationPredictor, SceneTransform, TrackOverlay, hip, render_track_overlays
    M.install(monkeypatch)
    order = []
    for name in [n for n in dir(hip) if n[0] != "_" and isinstance(getattr(hip, n), types.FunctionType)]:
        if name in ("require_device", "device_guard", "guarded"):
            continue
        monkeypatch.setattr(hip, name, (lambda n, f: lambda *a_, **k: (order.append(n), f(*a_, **k))[1])(name, getattr(hip, name)))
    c = predictor_inputs()
    pred = EvaluationPredictor(FakeModel(), interp_shape=(12, 16), grid_size=2)  # the tracker sees resized frames, the overlay the raw ones
    res = pred(**c)
    plain = list(order)
    assert plain and not any(n.startswith("overlay") for n in plain) and pred.last_track_overlay is None
    del order[:]
    res_none = pred(**c, track_overlay=None)
    assert order == plain and M.calls == [] and "track_overlay" not in pred.model.seen["kw"] and pred.last_track_overlay is None
    with pytest.raises(ValueError, match="TrackOverlay"):
        pred(**c, track_overlay="rainbow")
    del order[:]
    o = TrackOverlay(pad=2)
    res_o = pred(**c, track_overlay=o, save_debug_logs=False)
    own = ["overlay_project"] + ["overlay_draw", "overlay_compose"] * 3
    assert order[:len(plain)] == plain and order[len(plain):] == own  # after the tracking, and nothing the tracker does has changed
    assert all(torch.equal(res_o[k], res[k]) and torch.equal(res_none[k], res[k]) for k in ("traj_e", "vis_e", "vis_e_as_prob"))
    assert tuple(pred.model.seen["rgbs"].shape[-2:]) == (12, 16)
    video, cols = pred.last_track_overlay
    assert tuple(video.shape) == (2, 3, 3, 24 + 4, 32 + 4) and video.dtype == torch.uint8 and tuple(cols.shape) == (3, 3)
    want = render_track_overlays(c["rgbs"][0], res["traj_e"][0], res["vis_e"][0], c["query_points_3d"][0, :, 0], c["intrs"][0], c["extrs"][0], o)
    assert torch.equal(video, want[0]) and torch.equal(cols, want[1])
    # raw resolution: query 0 sits at pixel (10, 12) of view 0 and (14, 12) of view 1, + pad
    for v, (x, y) in enumerate(((10, 12), (14, 12))):
        assert torch.equal(video[v, 0, :, y + 2, x + 2], cols[0]) and not torch.equal(c["rgbs"][0, v, 0, :, y, x], cols[0])
    # a scene transform: the tracker works in the normalised world, the overlay is drawn with the restored tracks and the caller's cameras
    xf = SceneTransform(scale=2.0, rotation=torch.eye(3), translation=torch.tensor([0.1, -0.2, 0.3]))
    res_x = pred(**c, track_overlay=o, scene_transform=xf)
    assert not torch.equal(pred.model.seen["extrs"], c["extrs"]) and torch.allclose(res_x["traj_e"], res["traj_e"], atol=1e-5)
    assert torch.equal(pred.last_track_overlay[0], render_track_overlays(c["rgbs"][0], res_x["traj_e"][0], res_x["vis_e"][0], c["query_points_3d"][0, :, 0],
                                                                         c["intrs"][0], c["extrs"][0], o)[0])
    assert "stream" in EvaluationPredictor.forward.__doc__ and "track_overlay" in EvaluationPredictor.forward.__doc__
    pred(**c)
    assert pred.last_track_overlay is None


def test_demo_flags(tmp_path):
    import demo_amd
    from mvtracker_amd import TrackOverlay
    ap = demo_amd.build_parser()
    a = ap.parse_args(["--synthetic"])
    assert demo_amd.track_overlay_from_args(a) is None
    a = ap.parse_args(["--synthetic", "--save-overlay", str(tmp_path)])
    o = demo_amd.track_overlay_from_args(a)
    assert isinstance(o, TrackOverlay) and (o.trail, o.linewidth, o.pad, o.min_depth, o.max_tracks) == (-1, 2, 0, None, None)
    a = ap.parse_args(["--synthetic", "--save-overlay", str(tmp_path), "--overlay-trail", "10", "--overlay-linewidth", "1", "--overlay-pad", "8",
                       "--overlay-min-depth", "0.05", "--overlay-max-tracks", "36"])
    o = demo_amd.track_overlay_from_args(a)
    assert (o.trail, o.linewidth, o.pad, o.min_depth, o.max_tracks) == (10, 1, 8, 0.05, 36)
    for bad in (["--synthetic", "--overlay-trail", "3"], ["--synthetic", "--save-overlay", str(tmp_path), "--overlay-linewidth", "9"],
                ["--synthetic", "--save-overlay", str(tmp_path), "--overlay-pad", "65"]):
        with pytest.raises(SystemExit):
            demo_amd.track_overlay_from_args(ap.parse_args(bad))
    video = torch.arange(2 * 2 * 3 * 4 * 5, dtype=torch.uint8).reshape(2, 2, 3, 4, 5)
    files = demo_amd.save_overlay(video, str(tmp_path / "out"))
    print(files)
    try:
        from PIL import Image
    except ImportError:
        assert sorted(os.path.basename(f) for f in files) == ["view0.npy", "view1.npy"]
        assert np.array_equal(np.load(files[1]), video[1].numpy())
    else:
        assert sorted(os.path.basename(f) for f in files) == ["view0_frame0000.png", "view0_frame0001.png", "view1_frame0000.png", "view1_frame0001.png"]
        assert np.array_equal(np.asarray(Image.open(os.path.join(str(tmp_path / "out"), "view1_frame0001.png"))), video[1, 1].permute(1, 2, 0).numpy())
