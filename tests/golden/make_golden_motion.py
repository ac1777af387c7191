"""Writes tests/golden/motion_mask.npz: small clips and what the reference's own ``_static_bg_mask_from_window``
(mvtracker/datasets/generic_scene_dataset.py) and ``_detect_static_prefix_frames`` (demo.py) give them, generated from
/root/reference in the build container (the path is the one tests/golden/_ref_import.py names).

    python tests/golden/make_golden_motion.py

Both files import much that is absent here and that the two functions never touch (PIL, torchvision, tqdm, rerun, huggingface_hub,
the monocular baselines), so each function's own definition is compiled from its file's syntax tree into a namespace that holds
what it uses (torch, torch.nn.functional, typing.List), as make_golden_reproject.py does.

Clips, uint8 (2, 6, 3, 40, 70): a fixed random image per view, plus noise of up to +-6 on a quarter of the pixels of every frame,
plus a 6 x 6 blob that moves one pixel per frame and touches a corner in frame 0.  ``moving``: noise in every frame.  ``prefix``:
frames 0..3 are the same noise-free image with the blob at rest, so the first three boundaries are exactly 0.  ``unit``: the first
clip divided by 255 as float32, with the threshold 10 / 255 (a threshold that fp32 does not hold exactly).  Masks are bit-packed
(np.packbits over the flattened mask).  Data only."""
import ast
import os
import sys
from typing import List

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..")]
from _ref_import import REF_ROOT  # noqa: E402
import motion_ref as R  # noqa: E402

CONFIGS = ((-1, 7), (2, 3), (1, 0))
PREFIX_RULES = ((0.5, 10), (0.5, 3), (100.0, 10), (100.0, 4), (0.0, 10))
V, T, H, W = 2, 6, 40, 70


def ref_function(path, name):
    tree = ast.parse(open(path).read(), path)
    node = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name]
    ns = {"torch": torch, "F": F, "List": List}
    exec(compile(ast.Module(body=node, type_ignores=[]), path, "exec"), ns)
    return ns[name]


def make_clip(seed, still_frames):
    """``still_frames``: leading frames without noise and with the blob at rest."""
    rng = np.random.default_rng(seed)
    base = rng.integers(20, 200, (V, 1, 3, H, W))
    clip = np.repeat(base, T, 1)
    for t in range(T):
        step = max(0, t - (still_frames - 1)) if still_frames else t
        for v in range(V):
            y, x = (step, step) if v == 0 else (H - 6 - step, W - 6 - step)  # view 0: the top left corner, view 1: the bottom right
            clip[v, t, :, y:y + 6, x:x + 6] += 50
        if t >= still_frames:
            noisy = rng.random((V, 1, H, W)) < 0.25
            clip[:, t] += np.where(noisy, rng.integers(-6, 7, (V, 3, H, W)), 0)
    return clip.astype(np.uint8)


def main():
    mask_fn = ref_function(os.path.join(REF_ROOT, "mvtracker", "datasets", "generic_scene_dataset.py"), "_static_bg_mask_from_window")
    prefix_fn = ref_function(os.path.join(REF_ROOT, "demo.py"), "_detect_static_prefix_frames")
    out = {"configs": np.array(CONFIGS, np.int64), "prefix_rules": np.array(PREFIX_RULES, np.float64)}
    clips = {"moving": (make_clip(11, 0), 10.0), "prefix": (make_clip(12, 4), 10.0)}
    clips["unit"] = ((clips["moving"][0].astype(np.float32) / np.float32(255.0)), 10.0 / 255.0)
    for name, (frames, thresh) in clips.items():
        if frames.dtype == np.uint8:  # (the unit clip is derived by the tests: moving_frames.astype(float32) / float32(255))
            out[name + "_frames"] = frames
        out[name + "_thresh"] = np.array([thresh], np.float64)
        for i, (win, r) in enumerate(CONFIGS):
            m = mask_fn(torch.from_numpy(frames), win, r, thresh).numpy()
            mine = R.static_mask(frames, win, r, thresh)
            print(f"{name} window {win} r {r}: static {m.mean():.3f}, per frame of view 0 {np.round(m[0].mean((1, 2)), 3).tolist()}, "
                  f"restatement differs in {int((m != mine).sum())} pixels")
            assert m.shape == (V, T, H, W) and m.dtype == bool and np.array_equal(m, mine)
            out[f"{name}_static_{i}"] = np.packbits(m.reshape(-1))
        if frames.dtype == np.uint8:
            got = [prefix_fn(torch.from_numpy(frames), thr, int(mx)) for thr, mx in PREFIX_RULES]
            diffs = R.boundary_mean_diff(frames)
            print(f"{name} boundary mean diffs {np.round(diffs, 4).tolist()} static prefix per rule {got}")
            assert got == [R.static_prefix(diffs, T, thr, int(mx)) for thr, mx in PREFIX_RULES]
            for j, g in enumerate(got):
                out[f"{name}_prefix_{j}"] = np.array(g, np.int64)
    assert out["prefix_prefix_0"].tolist() == [0, 1, 2, 3]
    path = os.path.join(HERE, "motion_mask.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 256 * 1024


if __name__ == "__main__":
    main()
