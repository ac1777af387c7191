"""Scene normalisation timing at 4 views x 512x512 and 6 views x 720x1280: ``auto_scene_normalization`` (both scale rules) and
``SceneTransform.apply`` on a clip of --frames frames plus 1 000 query rows, with HIP events, warm (2 warm-ups, then median [min,
max] of --reps calls).  Beside each, the same step written with torch ops on the device: boolean-mask unprojection, ``mean`` and a
sort-based quantile (``torch.quantile`` itself refuses more than 16 M values, so the rank rule is restated over ``torch.sort``), and
elementwise / matmul ops for the transform.

    python tools/time_scene_norm.py [--out profiles/r09_scene_norm.json] [--reps 15] [--frames 8]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvtracker_amd import scene, synth  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stat(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def torch_quantile(x, q):
    s = torch.sort(x).values
    rank = torch.tensor(q, dtype=torch.float32) * (s.numel() - 1)
    kb = int(rank.floor())
    return torch.lerp(s[kb], s[min(kb + 1, s.numel() - 1)], (rank - rank.floor()).to(x.device))


def torch_auto(depths, intrs, extrs, by_camera, target_radius=6.3):
    """The reference's steps with torch ops on the device (valid = depth > 0, frame 0)."""
    V, _, _, H, W = depths[0].shape
    dev = depths.device
    e4 = torch.eye(4, device=dev).repeat(V, 1, 1)
    e4[:, :3] = extrs[0, :, 0]
    einv, kinv = torch.inverse(e4), torch.inverse(intrs[0, :, 0])
    y, x = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    homog = torch.stack([x, y, torch.ones_like(x)], -1).reshape(-1, 3).float()
    pts = []
    for v in range(V):
        d = depths[0, v, 0, 0].reshape(-1)
        cam = (homog @ kinv[v].T) * d[:, None]
        pts.append((cam @ einv[v, :3, :3].T + einv[v, :3, 3])[d > 0])
    pts = torch.cat(pts)
    c = pts.mean(0)
    floor = torch_quantile(pts[:, 2] - c[2], 0.12)
    if by_camera:
        cc = extrs[0, :, 0, :, 3] - c
        cc[:, 2] -= floor
        radius = cc.norm(dim=1).median()
    else:
        lifted = pts - c
        lifted[:, 2] -= floor
        radius = torch_quantile(lifted.norm(dim=1), 0.95)
    scale = target_radius / radius
    t = -scale * c
    t[2] -= scale * floor
    return torch.cat([scale[None], t]).cpu()


def torch_apply(xf, depths, extrs, queries):
    dev = depths.device
    R = torch.tensor(xf.rotation, device=dev, dtype=torch.float32)
    t = torch.tensor(xf.translation, device=dev, dtype=torch.float32)
    d = depths * xf.scale
    rot = extrs[..., :3] @ R.T
    e = torch.cat([rot, (xf.scale * extrs[..., 3] - rot @ t)[..., None]], -1)
    q = torch.cat([queries[..., :1], (xf.scale * queries[..., 1:]) @ R.T + t], -1)
    return d, e, q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--frames", type=int, default=8)
    args = ap.parse_args()
    res = dict(reps=args.reps, frames=args.frames, configs={},
               statistic="median [min, max] of HIP-event times after 2 warm-ups, ms; the clip is on the device; auto includes its one host read")
    for name, (V, H, W) in {"4x512x512": (4, 512, 512), "6x720x1280": (6, 720, 1280)}.items():
        clip = synth.make_clip(1234, V=V, T=args.frames, H=H, W=W, N=4, invalid_frac=0.02, frame_period=1)
        depths, intrs, extrs = (torch.from_numpy(clip[k]).cuda() for k in ("depths", "intrs", "extrs"))
        queries = torch.rand(1, 1000, 4, device="cuda")
        xf = scene.auto_scene_normalization(depths, intrs, extrs)
        steps = {"auto_camera_radius": lambda: scene.auto_scene_normalization(depths, intrs, extrs),
                 "auto_scene_radius": lambda: scene.auto_scene_normalization(depths, intrs, extrs, rescale_by_camera_radius=False),
                 "apply": lambda: xf.apply(depths=depths, extrs=extrs, query_points=queries),
                 "torch_auto_camera_radius": lambda: torch_auto(depths, intrs, extrs, True),
                 "torch_auto_scene_radius": lambda: torch_auto(depths, intrs, extrs, False),
                 "torch_apply": lambda: torch_apply(xf, depths, extrs, queries)}
        t = {k: [] for k in steps}
        for rep in range(args.reps + 2):
            for k, fn in steps.items():
                ms, _ = timed(fn)
                if rep >= 2:
                    t[k].append(ms)
        ref = torch_auto(depths, intrs, extrs, True)
        r = dict(views=V, height=H, width=W, pixels=V * H * W, scale=xf.scale, torch_scale=float(ref[0]), **{k + "_ms": stat(v) for k, v in t.items()})
        res["configs"][name] = r
        print(name, json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
