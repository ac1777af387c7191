"""CPU stand-ins for the track-overlay entries of mvtracker_amd.hip (overlay_project, overlay_draw, overlay_compose), on top of
tests/hip_mock_scene.py (and with it tests/hip_mock.py): the host code of mvtracker_amd/overlay.py and the predictor's wiring run on CPU tensors.  The fake entries follow
the kernels' contract (the point layout, the key planes kept by a maximum, the persistent line plane, the marker plane reset by
compose) and take the arithmetic and the primitives from the restatement tests/overlay_ref.py.  ``calls`` lists the entries called,
in order, and ``args`` what each was called with."""
import numpy as np
import torch

import hip_mock_scene
import overlay_ref as R

calls = []
args = []


def _keys(k):
    return k.numpy().view(np.uint64)


def overlay_project(tracks, intrs, extrs, V, T, N, xyz=None, points=None, pad=0, min_depth=None, query_frames=None, frame0=0, lut=None,
                    color_view=0, Hp=0, colors=None):
    calls.append("overlay_project")
    args.append(dict(shape=(V, T, N), pad=pad, min_depth=min_depth, frame0=frame0, color_view=color_view, Hp=Hp, rainbow=lut is not None))
    assert tuple(tracks.shape) == (T, N, 3) and tuple(intrs.shape) == (V, T, 3, 3) and tuple(extrs.shape) == (V, T, 3, 4)
    assert all(a.dtype == torch.float32 and a.is_contiguous() for a in (tracks, intrs, extrs))
    px, py, z = R.project(tracks.numpy(), intrs.numpy(), extrs.numpy())
    if xyz is not None:
        xyz.copy_(torch.from_numpy(np.stack([px, py, z], -1)))
    x, y, valid = R.integer_points(px, py, z, pad, min_depth)
    if points is not None:
        assert points.dtype == torch.int32 and tuple(points.shape) == (T, V, N, 4)
        points.copy_(torch.from_numpy(np.stack([x, y, valid.astype(np.int64), np.zeros_like(x)], -1).transpose(1, 0, 2, 3).astype(np.int32)))
    if lut is not None:
        q = np.maximum(query_frames.numpy(), 0)
        for n in range(N):
            t = int(q[n]) - frame0
            if 0 <= t < T:
                yy = int(y[color_view, t, n]) if valid[color_view, t, n] else pad
                colors[n] = lut[min(255, max(0, (yy * 256) // Hp))]


def overlay_draw(prev, cur, visibility, query_frames, colors, V, N, M, t, linewidth, Hp, Wp, line_keys, marker_keys):
    calls.append("overlay_draw")
    args.append(dict(t=t, M=M, linewidth=linewidth, lines=prev is not None, visibility=visibility is not None))
    assert (prev is None) == (line_keys is None) and 1 <= M <= N and tuple(cur.shape) == (V, N, 4) and tuple(marker_keys.shape) == (V, Hp, Wp)
    q, c = query_frames.numpy(), colors.numpy().astype(np.uint64)
    rgb = (c[:, 0] << np.uint64(16)) | (c[:, 1] << np.uint64(8)) | c[:, 2]
    for v in range(V):
        mk = _keys(marker_keys[v])
        for i in range(M):
            bx, by, ok, _ = (int(e) for e in cur[v, i])
            if not ok:
                continue
            if not (q[i] > t or bx == 0 or by == 0):
                ys, xs = (R.disc if visibility is None or bool(visibility[i]) else R.ring)((bx, by), 2 * linewidth, Hp, Wp)
                key = np.uint64(((i + 1) << 24) | int(rgb[i]))
                mk[ys, xs] = np.maximum(mk[ys, xs], key)
            if prev is None:
                continue
            ax, ay, ok_a, _ = (int(e) for e in prev[v, i])
            if t - 1 < q[i] or not ok_a or (ax, ay) == (0, 0) or (bx, by) == (0, 0):
                continue
            ys, xs = R.stroke((ax, ay), (bx, by), linewidth, Hp, Wp)
            lk = _keys(line_keys[v])
            key = np.uint64((((t << 20) | i) << 24) | int(rgb[i]))
            lk[ys, xs] = np.maximum(lk[ys, xs], key)


def overlay_compose(frames, V, T, t_local, H, W, pad, line_keys, first_segment, marker_keys, out):
    calls.append("overlay_compose")
    args.append(dict(t_local=t_local, first_segment=first_segment, dtype=frames.dtype, lines=line_keys is not None))
    Hp, Wp = H + 2 * pad, W + 2 * pad
    assert tuple(frames.shape) == (V, T, 3, H, W) and tuple(out.shape) == (V, T, 3, Hp, Wp) and frames.dtype in (torch.uint8, torch.float32)
    pic = np.full((V, 3, Hp, Wp), 255, np.uint8)
    pic[:, :, pad:pad + H, pad:pad + W] = R.to_u8(frames[:, t_local].numpy())
    mk = _keys(marker_keys)
    lk = _keys(line_keys) if line_keys is not None else np.zeros_like(mk)
    take_line = (lk != 0) & (lk >= np.uint64((first_segment + 1) << 44))
    key = np.where(mk != 0, mk, np.where(take_line, lk, np.uint64(0)))
    for c in range(3):
        ch = ((key >> np.uint64(16 - 8 * c)) & np.uint64(255)).astype(np.uint8)
        pic[:, c] = np.where(key != 0, ch, pic[:, c])
    out[:, t_local] = torch.from_numpy(pic)
    marker_keys.zero_()


def install(monkeypatch):
    import sys
    from mvtracker_amd import hip
    hip_mock_scene.install(monkeypatch)
    me = sys.modules[__name__]
    del calls[:]
    del args[:]
    for name in "overlay_project overlay_draw overlay_compose".split():
        monkeypatch.setattr(hip, name, getattr(me, name))
