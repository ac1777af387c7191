"""fp64 restatement of the region clustering rules (mvtracker_amd/cluster.py, csrc/cloud_cluster.hip): DBSCAN as a function of the
cloud alone, the oriented-box crop and the largest-cluster choice with the reference's two fallbacks.  numpy / scipy only.

With adj(i, j) = d2(i, j) <= r2 (a point is its own neighbour): core(i) = |{j: adj(i, j)}| >= min_samples; clusters are the connected
components of the core points under adj, numbered in ascending order of their lowest core index; a non-core point with a core
neighbour takes the lowest cluster number among its core neighbours; every other point is -1.  Rows that are not finite take no
part (-1).  Brute force up to BRUTE points, scipy's cKDTree (candidates, then the same exact test) above."""
import numpy as np

BRUTE = 2048
FEW, NONE, EMPTY = 1, 2, 3
STATE_FIELDS = ("candidates", "core", "clusters", "chosen", "chosen_size", "noise", "fallback", "status")


def valid_rows(x):
    return np.isfinite(np.asarray(x)[:, :3]).all(1)


def r2_of(eps):
    """The device's threshold: fp32(eps * eps), rounded once."""
    return float(np.float32(float(eps) ** 2))


def neighbour_pairs(x, r2):
    """(i, j) of every ordered pair with d2 <= r2, self pairs included; x (n, 3) fp64."""
    n = len(x)
    if n <= BRUTE:
        d = x[:, None, :] - x[None, :, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        return np.nonzero(d2 <= r2)
    from scipy.spatial import cKDTree
    pr = cKDTree(x).query_pairs(np.sqrt(r2) * (1.0 + 1e-6) + 1e-12, output_type="ndarray")
    d = x[pr[:, 0]] - x[pr[:, 1]]
    pr = pr[d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2] <= r2]
    s = np.arange(n)
    return np.concatenate([pr[:, 0], pr[:, 1], s]), np.concatenate([pr[:, 1], pr[:, 0], s])


def min_pair_gap(x, eps):
    """min over pairs of |d2 - eps^2| / eps^2 in fp64 (inf without a pair): the fixture's margin condition."""
    x = np.asarray(x, np.float64)[:, :3]
    x = x[valid_rows(x)]
    e2 = float(eps) ** 2
    best = np.inf
    for a in range(0, len(x), 512):
        d = x[a:a + 512, None, :] - x[None, :, :]
        d2 = (d * d).sum(-1)
        d2[np.arange(len(d2)), a + np.arange(len(d2))] = np.inf
        best = min(best, float(np.abs(d2 - e2).min()) / e2) if d2.size else best
    return best


def dbscan(points, eps, min_samples, r2=None):
    """labels (M,) int32 and core (M,) bool of points (M, >= 3)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    p = np.asarray(points)
    M = len(p)
    labels = np.full(M, -1, np.int32)
    core = np.zeros(M, bool)
    ok = valid_rows(p) if M else np.zeros(0, bool)
    idx = np.nonzero(ok)[0]
    if len(idx) == 0:
        return {"labels": labels, "core": core}
    x = p[idx, :3].astype(np.float64)
    r2 = r2_of(eps) if r2 is None else float(r2)
    i, j = neighbour_pairs(x, r2)
    n = len(x)
    cnt = np.bincount(i, minlength=n)
    c = cnt >= int(min_samples)
    lab = np.full(n, -1, np.int64)
    if c.any():
        cc = c[i] & c[j]
        g = coo_matrix((np.ones(int(cc.sum()), np.int8), (i[cc], j[cc])), shape=(n, n))
        comp = connected_components(g, directed=False)[1]
        ci = np.nonzero(c)[0]
        first = np.full(comp.max() + 1, n, np.int64)
        np.minimum.at(first, comp[ci], ci)  # the lowest core index of every component that holds a core point
        order = np.argsort(first[np.unique(comp[ci])])
        ids = np.full(comp.max() + 1, -1, np.int64)
        ids[np.unique(comp[ci])[order]] = np.arange(len(order))
        lab[ci] = ids[comp[ci]]
        b = (~c[i]) & c[j]  # non-core i with a core neighbour j
        bl = np.full(n, np.iinfo(np.int64).max, np.int64)
        np.minimum.at(bl, i[b], lab[j[b]])
        has = bl < np.iinfo(np.int64).max
        lab[has & ~c] = bl[has & ~c]
    labels[idx] = lab
    core[idx] = c
    return {"labels": labels, "core": core}


def region_T_world(pose):
    """The host's crop matrix: the fp64 inverse of world_T_region (4, 4), rows 0..2 rounded once to fp32."""
    return np.linalg.inv(np.asarray(pose, np.float64))[:3].astype(np.float32)


def region_coords(points, pose):
    """Coordinates of points (M, >= 3) in the region's frame, fp64 arithmetic on the rounded matrix."""
    m = region_T_world(pose).astype(np.float64)
    p = np.asarray(points)[:, :3].astype(np.float64)
    return p @ m[:, :3].T + m[:, 3]


def face_margin(points, pose, box):
    """The smallest distance of a finite point's region coordinates from a face plane of the box (inf without a point)."""
    c = region_coords(points, pose)[valid_rows(points)]
    b = np.asarray(box, np.float64)
    return float(min(np.abs(c - b[:, 0]).min(), np.abs(c - b[:, 1]).min())) if len(c) else np.inf


def crop(points, pose, box):
    """Rows kept by the crop: finite and strictly inside the box (lo < c < hi on all three axes)."""
    if box is None:
        return valid_rows(points)
    c = region_coords(points, pose)
    b = np.asarray(box, np.float64)
    with np.errstate(invalid="ignore"):
        return valid_rows(points) & ((c > b[:, 0]) & (c < b[:, 1])).all(1)


def select(points, pose, box, eps, min_samples):
    """classify_gripper_points on the untransformed points: dict(select, labels, core, state); state as the device's row."""
    p = np.asarray(points)
    keep = crop(p, pose, box)
    x = np.where(keep[:, None], p[:, :3].astype(np.float64), np.nan)
    r = dbscan(x, eps, min_samples)
    lab = r["labels"]
    n_cand, n_clusters = int(keep.sum()), int(lab.max()) + 1 if len(lab) else 0
    chosen, size, fb = -1, 0, 0
    if n_clusters > 0:
        counts = np.bincount(lab[lab >= 0])
        chosen = int(np.argmax(counts))
        size = int(counts[chosen])
    if n_cand == 0:
        fb, sel = EMPTY, np.zeros(len(p), bool)
    elif n_cand < int(min_samples):
        fb, sel = FEW, keep.copy()
    elif n_clusters == 0:
        fb, sel = NONE, keep.copy()
    else:
        sel = lab == chosen
    state = dict(candidates=n_cand, core=int(r["core"].sum()), clusters=n_clusters, chosen=chosen, chosen_size=size,
                 noise=int((keep & (lab < 0)).sum()), fallback=fb, status=0)
    return {"select": sel, "labels": lab, "core": r["core"], "state": state}
