"""Generate tests/golden/e2e_backward.npz: the REFERENCE MVTracker (imported from the read-only reference checkout, CPU, exact-distance
kNN as for e2e_two_windows) on a seeded clip and on its time-flip, and the backward-tracking merge of the two runs.

    python tests/golden/make_golden_backward.py [seed [output.npz]]

Semantics pinned here ("Backward tracking"): F = the reference on the clip, B' = the reference on the clip reversed
along T with query times T-1-qt, B[t] = B'[T-1-t];  merged[t, n] = B[t, n] if t < qt[n] and the reversed run reached track n, else
F[t, n].  Visibility LOGITS are the per-window outputs of the reference's forward_iteration laid out over (T, N) by the window list
(the reference itself only returns their sigmoid).

The clip is synth.make_clip(seed, V=2, T=18, H=128, W=128); the 12 query points are placed here, on the rendered surfaces at chosen
query frames: frame 0, frames below S/2 = 6 (no reversed window reaches them), mid-clip frames, and frames >= T - S/2 = 12 (no forward
window reaches them).  With max qt = 14 the reversed pass runs the windows 3 and 9 in reversed time; the second one runs past frame 0
(repeat-first-frame padding).  Only data goes into the .npz: the seed, the query points and the reference's outputs.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from _ref_import import import_reference  # noqa: E402
from mvtracker_amd import synth  # noqa: E402
from mvtracker_amd.backward import window_prefixes  # noqa: E402

QUERY_FRAMES = (0, 0, 3, 3, 5, 7, 7, 9, 10, 12, 14, 14)
CLIP = dict(V=2, T=18, H=128, W=128)


def make_queries(clip, seed):
    """(1, N, 4) query points (t, x, y, z): a random pixel with valid depth of a random view at the query's frame, unprojected."""
    rng = np.random.default_rng(1000 + seed)
    depths, intrs, extrs = clip["depths"][0], clip["intrs"][0], clip["extrs"][0]
    V, H, W = CLIP["V"], CLIP["H"], CLIP["W"]
    q = np.zeros((len(QUERY_FRAMES), 4), np.float64)
    for n, tq in enumerate(QUERY_FRAMES):
        for _ in range(64):
            v = int(rng.integers(V))
            px, py = int(rng.integers(W // 16, W - W // 16)), int(rng.integers(H // 16, H - H // 16))
            d = float(depths[v, tq, 0, py, px])
            if d > 0:
                break
        K, E = intrs[v, tq].astype(np.float64), extrs[v, tq].astype(np.float64)
        cam = np.linalg.inv(K) @ np.array([px, py, 1.0]) * d
        q[n] = [tq, *(E[:, :3].T @ (cam - E[:, 3]))]
    return q[None].astype(np.float32)


def flip_clip(args):
    """(rgbs, depths, query_points, intrs, extrs) of the time-reversed clip, query times T-1-qt."""
    rgbs, depths, q, intrs, extrs = args
    T = rgbs.shape[2]
    qf = q.clone()
    qf[0, :, 0] = (T - 1) - q[0, :, 0].long().float()
    return [rgbs.flip(2), depths.flip(2), qf, intrs.flip(2), extrs.flip(2)]


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 71
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "e2e_backward.npz")
    R = import_reference()
    torch.manual_seed(0)
    torch.set_num_threads(8)

    def knn_exact(k, xyz_ref, xyz_query):
        d = torch.cdist(xyz_query, xyz_ref, p=2, compute_mode="donot_use_mm_for_euclid_dist")
        return torch.topk(d, k, dim=-1, largest=False, sorted=True)

    R.mvt.knn = knn_exact
    model = R.mvt.MVTracker(hidden_size=256).eval()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(shapes, 0).items()}, strict=True)
    S = model.S
    clip = synth.make_clip(seed=seed, N=1, **CLIP)
    T = CLIP["T"]
    q = make_queries(clip, seed)
    args = [torch.from_numpy(clip[k]) for k in ("rgbs", "depths")] + [torch.from_numpy(q)] + \
           [torch.from_numpy(clip[k]) for k in ("intrs", "extrs")]

    def run(a):
        """The reference's result plus the (T, N) visibility logits and the window list."""
        logits = []
        orig = model.forward_iteration

        def spy(*aa, **k):
            o = orig(*aa, **k)
            logits.append(o[1].clone())
            return o

        model.forward_iteration = spy
        try:
            with torch.no_grad():
                r = model(*a, iters=4)
        finally:
            model.forward_iteration = orig
        qt = a[2][0, :, 0].long().numpy()
        order = np.argsort(qt, kind="stable")
        wins = window_prefixes(qt[order], S, T)
        assert len(wins) == len(logits), (wins, len(logits))
        lg = np.zeros((T, len(qt)), np.float32)
        written = np.zeros((T, len(qt)), bool)
        for (w, p1), v in zip(wins, logits):
            v = v.reshape(v.shape[1], -1).numpy()  # (S, p1)
            assert v.shape == (S, p1), v.shape
            n_loc = min(S, T - w)
            lg[w:w + n_loc, order[:p1]] = v[:n_loc]
            written[w:w + n_loc, order[:p1]] = True
        vis = r["vis_e"][0].numpy()
        # the layout above is the reference's (entries no window writes stay zero on both sides)
        assert np.abs(np.where(written, 1 / (1 + np.exp(-lg.astype(np.float64))), 0.0) - vis).max() < 1e-6
        return r["traj_e"][0].numpy(), vis, lg, r["feat_init"].numpy(), wins

    traj_f, vis_f, lg_f, feat_f, wins_f = run(args)
    traj_r, vis_r, lg_r, feat_r, wins_r = run(flip_clip(args))
    traj_b, vis_b, lg_b = traj_r[::-1].copy(), vis_r[::-1].copy(), lg_r[::-1].copy()
    qt = q[0, :, 0].astype(np.int64)
    reached = np.zeros(len(qt), bool)
    if wins_r:
        reached[np.argsort(T - 1 - qt, kind="stable")[:wins_r[-1][1]]] = True
    take_b = (np.arange(T)[:, None] < qt[None, :]) & reached[None, :]
    np.savez_compressed(
        out, seed=seed, **{k: np.asarray(v) for k, v in CLIP.items()}, query_points=q,
        traj_forward=traj_f[None], vis_forward=vis_f[None], logits_forward=lg_f[None], feat_init_forward=feat_f,
        traj_backward=traj_b[None], vis_backward=vis_b[None], logits_backward=lg_b[None], feat_init_reversed=feat_r,
        traj_merged=np.where(take_b[..., None], traj_b, traj_f)[None], vis_merged=np.where(take_b, vis_b, vis_f)[None],
        logits_merged=np.where(take_b, lg_b, lg_f)[None],
        windows_forward=np.asarray(wins_f, np.int64).reshape(-1, 2), windows_backward=np.asarray(wins_r, np.int64).reshape(-1, 2))
    print(f"{out}: {os.path.getsize(out) / 1024:.1f} KiB, forward windows {wins_f}, reversed windows {wins_r}")


if __name__ == "__main__":
    main()
