"""Reprojection check timing at the benchmark clip's size: 4 views x 384x512, one frame.  Each launch of the render and the scores
(``mvt_reproject_clear`` + ``mvt_reproject_splat_depths`` for both source modes and splat 1 / 3, ``mvt_reproject_resolve``,
``mvt_photometric_score``) and the whole ``reprojection_report`` call, timed with device events around --inner back-to-back calls
after 2 warm-ups: median [min, max] of --reps windows, microseconds per call, with the bytes each launch must move over its time.

Bytes a launch must move (from the shapes; what it cannot avoid, not what it issues):
  clear    the key images, written once: targets * H*W * 8
  splat    the source depth maps read once and one 8-byte atomic per drawn (point, target, sprite pixel): V * H*W * 4 + 8 * atomics
           (the atomics are counted by ``drawn``: the device's own points projected with torch in fp64 by the rule's formula, each
           drawn point counting the pixels of its sprite that lie in the image)
  resolve  keys read; index, depth and colour written; three gathered channel values per covered pixel: H*W * targets * (8 + 4 + 4 + 3) + 3 * covered
  score    two images, index and two depth maps read: pairs * H*W * (3 + 3 + 4 + 4 + 4)

    python tools/time_reprojection.py [--out profiles/reprojection.json] [--reps 7] [--inner 50]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvtracker_amd import ReprojectionCheck, hip, reprojection_report, synth  # noqa: E402

V, T, H, W = 4, 2, 384, 512


def window_us(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def measure(fn, reps, inner):
    t = [window_us(fn, inner) for _ in range(reps + 2)][2:]
    return dict(median=round(statistics.median(t), 2), min=round(min(t), 2), max=round(max(t), 2))


def with_rate(m, nbytes):
    return dict(m, bytes=int(nbytes), gb_per_s=round(nbytes / (m["median"] * 1e-6) / 1e9, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_reprojection.py needs an MI355X: there is no CPU path")
    clip = synth.make_clip(1234, V=V, T=T, H=H, W=W, N=4, invalid_frac=0.02, rgb_dtype=np.uint8)
    rgbs, depths, intrs, extrs = (torch.from_numpy(clip[k]).cuda()[0].contiguous() for k in ("rgbs", "depths", "intrs", "extrs"))
    HW = H * W
    K, E = intrs.reshape(V, T, 9)[:, 0].contiguous(), extrs.reshape(V, T, 12)[:, 0].contiguous()
    kinv, einv = torch.empty(V * T, 9, device="cuda"), torch.empty(V * T, 12, device="cuda")
    hip.invert_cameras(intrs.reshape(-1, 9).contiguous(), extrs.reshape(-1, 12).contiguous(), kinv, einv, V * T)
    keys = torch.empty(V, HW, dtype=torch.int64, device="cuda")
    index = torch.empty(V, H, W, dtype=torch.int32, device="cuda")
    depth = torch.empty(V, H, W, device="cuda")
    color = torch.empty(V, 3, H, W, dtype=torch.uint8, device="cuda")
    views = list(range(V))

    def splat(others, s):
        hip.reproject_splat_depths(depths, None, kinv, einv, V, T, 0, H, W, None, views, K, E, others, 0.01, s, keys)

    def drawn(others, s):
        """Atomics of one splat, for the byte count: the device's own points (mvt_clean_points) projected with torch in fp64 by the
        rule's formula (a matmul here: a point on a pixel border may fall the other way, which a byte count does not see), each drawn
        point counting the pixels of its s x s sprite inside the image."""
        r = s // 2
        xyz = torch.empty(V, ((H + 7) // 8 * 8) * ((W + 7) // 8 * 8), 4, device="cuda")
        hip.clean_points(depths, None, kinv, einv, V, T, 0, 1, H, W, None, None, xyz)
        p = xyz.reshape(V, -1, 4)[..., :3].double()
        n = 0
        for tv in range(V):
            Em, Km = E[tv].reshape(3, 4).double(), K[tv].reshape(3, 3).double()
            for sv in range(V):
                if others and sv == tv:
                    continue
                c = p[sv] @ Em[:, :3].T + Em[:, 3]
                u, v = c[:, 0] * Km[0, 0] / c[:, 2] + Km[0, 2], c[:, 1] * Km[1, 1] / c[:, 2] + Km[1, 2]
                ok = (c[:, 2] > 0.01) & (u > -1) & (u < W) & (v > -1) & (v < H)
                ui, vi = u[ok].trunc().long(), v[ok].trunc().long()  # (toward zero, as the rule)
                wide = (ui + r).clamp(max=W - 1) - (ui - r).clamp(min=0) + 1
                high = (vi + r).clamp(max=H - 1) - (vi - r).clamp(min=0) + 1
                n += int((wide * high).sum())
        return n

    res = dict(views=V, height=H, width=W, reps=args.reps, inner=args.inner,
               statistic="median [min, max] over windows of `inner` back-to-back calls, device events, after 2 warm-up windows, microseconds per call",
               launches={})
    out = res["launches"]
    out["clear"] = with_rate(measure(lambda: hip.reproject_clear(keys, V * HW), args.reps, args.inner), V * HW * 8)
    for others in (True, False):
        for s in (1, 3):
            atomics = drawn(others, s)
            name = f"clear+splat_{'others' if others else 'all'}_splat{s}"
            m = measure(lambda: (hip.reproject_clear(keys, V * HW), splat(others, s)), args.reps, args.inner)
            out[name] = with_rate(m, V * HW * 8 + V * HW * 4 + 8 * atomics)
            out[name]["atomics"] = atomics
    hip.reproject_clear(keys, V * HW)
    splat(True, 1)
    resolve = lambda: hip.reproject_resolve(keys, V, H, W, index, depth, color, rgbs=rgbs, V=V, T=T, t=0)  # noqa: E731
    resolve()
    covered = int((index >= 0).sum())
    out["resolve"] = with_rate(measure(resolve, args.reps, args.inner), V * HW * (8 + 4 + 4 + 3) + 3 * covered)
    out["resolve"]["coverage"] = round(covered / (V * HW), 4)
    real, own = rgbs[:, 0].contiguous(), depths[:, 0, 0].contiguous()
    scores = torch.empty(V, hip.SCORE_WORDS, dtype=torch.int64, device="cuda")
    partial = torch.empty(V * hip.photometric_blocks(H, W) * hip.SCORE_WORDS, dtype=torch.int64, device="cuda")
    score = lambda: hip.photometric_score(color, real, index, depth, own, V, H, W, 0.05, scores, partial=partial)  # noqa: E731
    out["score (2 launches)"] = with_rate(measure(score, args.reps, args.inner), V * HW * (3 + 3 + 4 + 4 + 4))
    ck = ReprojectionCheck(frames=(0,))
    res["reprojection_report_call"] = measure(lambda: reprojection_report(rgbs, depths, intrs, extrs, ck), args.reps, max(1, args.inner // 10))
    for k, v in out.items():
        print(k, json.dumps(v), flush=True)
    print("reprojection_report (render + scores + one readback)", json.dumps(res["reprojection_report_call"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
