"""Writes tests/golden/overlay.npz: what the track-overlay tests take from outside the project, generated in the build container
(matplotlib is there; the reference is at the path tests/golden/_ref_import.py names).

    python tests/golden/make_golden_overlay.py

  lut            (256, 3) uint8: matplotlib's gist_rainbow, 256 entries, each channel rint(lut * 255) (the distance of the nearest
                 channel to a tie is printed)
  color_y_hp     (n, 2) int64 rows (y, Hp) with y from -5 to Hp + 4, and color_rgb (n, 3) uint8: rint(cmap(Normalize(0, Hp)(y)) * 255),
                 what the reference's draw_tracks_on_video picks for a track whose query-frame row is y
  proj_*         3 cameras x 5 frames x 64 points with camera z >= 0.5: tracks (5, 64, 3), intrs (3, 5, 3, 3), extrs (3, 5, 3, 4),
                 proj_ref (3, 5, 64, 3) fp32 = the reference's world_space_to_pixel_xy_and_camera_z per view (pixel x, pixel y,
                 camera z), proj_f64 (3, 5, 64, 3) = the same projection evaluated in fp64 from the fp32 inputs
Data only."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..")]
from _ref_import import import_reference  # noqa: E402


def main():
    import matplotlib.pyplot as plt
    from matplotlib import colormaps
    cmap = colormaps["gist_rainbow"]
    lut = cmap(np.arange(256))[:, :3] * 255.0
    print("nearest distance of a channel to a tie:", float(np.abs(lut - np.floor(lut) - 0.5).min()))
    out = {"lut": np.rint(lut).astype(np.uint8)}
    rows, rgb = [], []
    for Hp in (72, 40, 104, 513):
        norm = plt.Normalize(0, Hp)
        for y in range(-5, Hp + 5):
            rows.append((y, Hp))
            rgb.append(np.rint(np.array(cmap(norm(y))[:3]) * 255.0))
    out["color_y_hp"], out["color_rgb"] = np.array(rows, np.int64), np.array(rgb).astype(np.uint8)

    ref = import_reference()
    rng = np.random.default_rng(7)
    Vn, Tn, Nn = 3, 5, 64
    K = np.zeros((Vn, Tn, 3, 3), np.float32)
    E = np.zeros((Vn, Tn, 3, 4), np.float32)
    for v in range(Vn):
        for t in range(Tn):
            ax = rng.normal(size=3)
            ax /= np.linalg.norm(ax)
            ang = rng.uniform(-0.6, 0.6)
            Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
            Rm = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
            E[v, t, :, :3], E[v, t, :, 3] = Rm, rng.uniform(-0.5, 0.5, 3) + np.array([0, 0, 3.0])
            K[v, t] = np.array([[rng.uniform(200, 600), rng.uniform(-1, 1), rng.uniform(100, 300)], [0, rng.uniform(200, 600), rng.uniform(100, 300)], [0, 0, 1]])
    tracks = rng.uniform(-1.2, 1.2, (Tn, Nn, 3)).astype(np.float32)
    got = np.zeros((Vn, Tn, Nn, 3), np.float32)
    for v in range(Vn):
        xy, z = ref.mu.world_space_to_pixel_xy_and_camera_z(torch.from_numpy(tracks), torch.from_numpy(K[v]), torch.from_numpy(E[v]))
        got[v] = torch.cat([xy, z], -1).numpy()
    t64, K64, E64 = tracks.astype(np.float64), K.astype(np.float64), E.astype(np.float64)
    cam = np.einsum("vtij,tnj->vtni", E64[..., :3], t64) + E64[:, :, None, :, 3]
    hom = np.einsum("vtij,vtnj->vtni", K64, cam)
    f64 = np.concatenate([hom[..., :2] / hom[..., 2:], cam[..., 2:]], -1)
    assert cam[..., 2].min() >= 0.5, cam[..., 2].min()
    print("camera z in", float(cam[..., 2].min()), float(cam[..., 2].max()), "reference fp32 max |error| vs fp64:", float(np.abs(got - f64).max()))
    out.update(proj_tracks=tracks, proj_intrs=K, proj_extrs=E, proj_ref=got, proj_f64=f64)
    path = os.path.join(HERE, "overlay.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 256 * 1024


if __name__ == "__main__":
    main()
