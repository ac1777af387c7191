"""fp64 restatement of cloud preparation (include/mvtracker_hip.h, "Cloud preparation") with numpy and
scipy.spatial.cKDTree, brute force for the exact cases: the yardstick of tests/test_gpu_cloud_prep.py and the engine of the mock
tests/hip_mock_prep.py.  Open3D is not a dependency of either project's tests; these are its rules.

Normals (EstimateNormals with KDTreeSearchParamHybrid): the neighbours of point i are, of the finite points of its cloud with
d2 < fl(fl(r) fl(r)) (strict, i itself included), the max_nn smallest by (d2, index); e_j = p_j - p_i in fp64, S1 and S2 summed in
ascending key order, C = S2 / n - (S1 / n)(S1 / n)^T, the normal a unit eigenvector of the smallest eigenvalue.  NaN where n < 3 or
lambda_mid <= 1e-12 lambda_max (the one deviation: Open3D leaves (0, 0, 1)).
Voxels (VoxelDownSample): origin = min - voxel / 2, cell = floor((p - origin) / voxel), the mean of every cell's points; rows in
ascending order of the first input index of the cell."""
import numpy as np

try:
    from scipy.spatial import cKDTree
except ImportError:  # pragma: no cover
    cKDTree = None

import camera_align_ref as A

MAX_NN = 64
RANGE, FULL = 1, 2


def valid_rows(x):
    return np.isfinite(np.asarray(x)[:, :3]).all(1)


def radius_sq(radius):
    r = np.float32(radius)
    with np.errstate(over="ignore"):
        return float(np.float32(r * r))


def d2_f32(q, pts):
    """The kernels' d2 = fma(dz,dz,fma(dy,dy,dx*dx)) in fp32: q (3,) or (m,1,3) against pts (n,3), float32 in, float64 out holding
    fp32 values.  The fused steps are taken in fp64 (a product of two fp32 numbers is exact there) and rounded to fp32."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = (np.asarray(pts, np.float32) - np.asarray(q, np.float32)).astype(np.float64)
        t = (d[..., 0] * d[..., 0]).astype(np.float32).astype(np.float64)
        t = (d[..., 1] * d[..., 1] + t).astype(np.float32).astype(np.float64)
        return (d[..., 2] * d[..., 2] + t).astype(np.float32).astype(np.float64)


def neighbours_brute(xyz, radius, max_nn):
    """idx (P, max_nn) int32 in ascending (d2, index) order, padded with -1; cnt (P,) int32, -1 for a row that takes no part;
    d2 (P, max_nn) of the kept ones (NaN padding).  The fp32 d2 of the kernels: exact rule, ties by index."""
    xyz = np.asarray(xyz, np.float32)[:, :3]
    P, r2 = len(xyz), radius_sq(radius)
    ok = valid_rows(xyz)
    rows = np.flatnonzero(ok)
    pts = xyz[rows]
    idx, cnt, d2o = np.full((P, max_nn), -1, np.int32), np.where(ok, 0, -1).astype(np.int32), np.full((P, max_nn), np.nan)
    k = min(max_nn, len(rows))
    col = np.arange(len(rows), dtype=np.uint64)
    for i0 in range(0, len(rows), 256):
        dd = d2_f32(pts[i0:i0 + 256, None, :], pts[None, :, :])
        dd[~(dd < r2)] = np.inf
        # the key (d2, index) as one integer: the bits of a non-negative fp32 number order as the number does
        key = (dd.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | col
        order = np.argpartition(key, k - 1, axis=1)[:, :k]
        order = np.take_along_axis(order, np.argsort(np.take_along_axis(key, order, 1), axis=1), 1)
        ds = np.take_along_axis(dd, order, 1)
        keep = np.isfinite(ds)
        k = order.shape[1]
        idx[rows[i0:i0 + 256], :k] = np.where(keep, rows[order], -1)
        d2o[rows[i0:i0 + 256], :k] = np.where(keep, ds, np.nan)
        cnt[rows[i0:i0 + 256]] = keep.sum(1)
    return idx, cnt, d2o


def cut(idx, cnt, d2, max_nn, radius):
    """The lists for a smaller max_nn and radius from sorted lists taken with larger ones: knnSearch(max_nn), then the cut at r^2."""
    keep = (idx[:, :max_nn] >= 0) & (d2[:, :max_nn] < radius_sq(radius))  # (a prefix: the lists are ascending)
    return np.where(keep, idx[:, :max_nn], -1).astype(np.int32), np.where(cnt < 0, -1, keep.sum(1)).astype(np.int32)


def neighbours_tree(xyz, radius, max_nn):
    """The same through a cKDTree in fp64 (large or rendered clouds: a tie at the last place or at r^2 may fall either way against
    the kernels' fp32 d2).  d2 is the fp64 one."""
    xyz = np.asarray(xyz, np.float32)[:, :3]
    P, r2 = len(xyz), radius_sq(radius)
    ok = valid_rows(xyz)
    rows = np.flatnonzero(ok)
    pts = xyz[rows].astype(np.float64)
    idx, cnt, d2o = np.full((P, max_nn), -1, np.int32), np.where(ok, 0, -1).astype(np.int32), np.full((P, max_nn), np.nan)
    if len(rows) == 0:
        return idx, cnt, d2o
    k = min(max_nn, len(rows))
    _, nn = cKDTree(pts).query(pts, k=k)
    nn = nn.reshape(len(rows), k)
    dd = ((pts[nn] - pts[:, None, :]) ** 2).sum(-1)
    dd[~(dd < r2)] = np.inf
    key = np.lexsort((rows[nn], dd), axis=1)
    nn, dd = np.take_along_axis(nn, key, 1), np.take_along_axis(dd, key, 1)
    keep = np.isfinite(dd)
    idx[rows, :k] = np.where(keep, rows[nn], -1)
    d2o[rows, :k] = np.where(keep, dd, np.nan)
    cnt[rows] = keep.sum(1)
    return idx, cnt, d2o


def covariance(xyz, idx, cnt):
    """cov (P, 6) = (xx, xy, xz, yy, yz, zz) of C = S2 / n - (S1 / n)(S1 / n)^T, the sums taken neighbour by neighbour in the order of
    idx, every product and sum rounded on its own (fp64); NaN for a row that takes no part."""
    p = np.asarray(xyz, np.float32)[:, :3].astype(np.float64)
    P = len(p)
    s1, s2 = np.zeros((P, 3)), np.zeros((P, 6))
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    for r in range(idx.shape[1]):
        m = idx[:, r] >= 0
        e = p[idx[m, r]] - p[m]
        s1[m] += e
        for k, (a, b) in enumerate(pairs):
            s2[m, k] += e[:, a] * e[:, b]
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.where(cnt > 0, cnt, 0).astype(np.float64)[:, None]
        mean = s1 / n
        cov = np.stack([s2[:, k] / n[:, 0] - mean[:, a] * mean[:, b] for k, (a, b) in enumerate(pairs)], 1)
    cov[cnt < 0] = np.nan
    return cov


def sym(cov):
    c = np.asarray(cov)
    return np.stack([c[..., [0, 1, 2]], c[..., [1, 3, 4]], c[..., [2, 4, 5]]], -2)


def normals_of(xyz, cov, cnt, viewpoint=None):
    """(P, 3) fp64 unit normals by numpy.linalg.eigh, NaN where cnt < 3 or lambda_mid <= 1e-12 lambda_max; eig (P, 3) ascending."""
    P = len(cov)
    out, eig = np.full((P, 3), np.nan), np.full((P, 3), np.nan)
    m = cnt >= 3
    if m.any():
        w, v = np.linalg.eigh(sym(cov[m]))
        n = v[:, :, 0]
        n = n / np.linalg.norm(n, axis=1, keepdims=True)
        n[~(w[:, 1] > 1e-12 * w[:, 2])] = np.nan
        if viewpoint is not None:
            p = np.asarray(xyz, np.float32)[m, :3].astype(np.float64)
            flip = (n * (np.asarray(viewpoint, np.float32).astype(np.float64) - p)).sum(1) < 0
            n[flip] = -n[flip]
        out[m], eig[m] = n, w
    return out, eig


def estimate(xyz, radius, max_nn, viewpoint=None, brute=None):
    """One cloud (P, >= 3) float32 -> dict(idx, cnt, d2, cov, nrm, eig)."""
    if brute is None:
        brute = cKDTree is None
    idx, cnt, d2 = (neighbours_brute if brute else neighbours_tree)(xyz, radius, max_nn)
    cov = covariance(xyz, idx, cnt)
    nrm, eig = normals_of(xyz, cov, cnt, viewpoint)
    return dict(idx=idx, cnt=cnt, d2=d2, cov=cov, nrm=nrm, eig=eig)


def pca_normals(xyz, radius, max_nn):
    return estimate(xyz, radius, max_nn)["nrm"]


def align_views_pca(clouds0, gw, gh, cap, radius, max_nn, max_iterations=30, sweeps=2, anchor=0, sample_stride=1):
    """camera_align_ref.align_views with PCA normals: the same sweep, the same ICP."""
    V, F = len(clouds0), len(clouds0[0])
    D = np.stack([np.eye(4)] * V)
    cur = [[c[:, :3].copy() for c in row] for row in clouds0]
    nrm = [[pca_normals(c, radius, max_nn) for c in row] for row in cur]
    info = dict(fitness=np.zeros(V), rmse=np.zeros(V), iterations=np.zeros(V, int), status=np.zeros(V, int), order=[])
    for _ in range(sweeps):
        for v in range(V):
            if v == anchor:
                continue
            others = [u for u in range(V) if u != v]
            info["order"].append((v, tuple(others)))
            r = A.icp([A.sample(clouds0[v][f], gw, gh, sample_stride) for f in range(F)], [[(cur[u][f], nrm[u][f]) for u in others] for f in range(F)],
                      cap, max_iterations, D[v])
            D[v] = r["D"]
            for k in ("fitness", "rmse", "iterations", "status"):
                info[k][v] = r[k]
            for f in range(F):
                cur[v][f] = A.transform(D[v], clouds0[v][f])
                nrm[v][f] = pca_normals(cur[v][f], radius, max_nn)
    info["D"] = D
    return info


# ------------------------------------------------------------------------------------------------------------------ voxels
def voxel(xyz, voxel_size):
    """One cloud (P, >= 3) float32 -> dict(points (Mv, 3) float32 from the fixed-point sums, mean64 (Mv, 3) the fp64 mean of the
    members, fixed64 (Mv, 3) the fixed-point mean before rounding, counts, first, labels (P,), origin (3,), cells (Mv, 3), status)."""
    x = np.asarray(xyz, np.float32)[:, :3]
    P, vs = len(x), float(voxel_size)
    ok = valid_rows(x)
    empty = dict(points=np.zeros((0, 3), np.float32), mean64=np.zeros((0, 3)), fixed64=np.zeros((0, 3)), counts=np.zeros(0, np.int32),
                 first=np.zeros(0, np.int32), labels=np.full(P, -1, np.int32), origin=np.full(3, np.inf), cells=np.zeros((0, 3), np.int64), status=0)
    if not ok.any():
        return empty
    rows = np.flatnonzero(ok)
    p = x[rows].astype(np.float64)
    origin = p.min(0) - vs * 0.5
    with np.errstate(over="ignore", invalid="ignore"):
        u = (p - origin) / vs
    cell = np.floor(u)
    if not ((cell >= 0) & (cell < 2 ** 21)).all():
        return dict(empty, origin=origin, status=RANGE)
    ci = cell.astype(np.int64)
    key = ci[:, 0] | (ci[:, 1] << 21) | (ci[:, 2] << 42)
    uniq, inv = np.unique(key, return_inverse=True)
    first = np.full(len(uniq), np.iinfo(np.int64).max)
    np.minimum.at(first, inv, rows)
    order = np.argsort(first)
    rank = np.empty(len(uniq), np.int64)
    rank[order] = np.arange(len(uniq))
    lab = rank[inv]  # output row of every valid point
    Mv = len(uniq)
    counts = np.bincount(lab, minlength=Mv)
    fixed = np.rint((u - cell) * 2.0 ** 32).astype(np.uint64)
    sums = np.zeros((Mv, 3), np.uint64)
    msum = np.zeros((Mv, 3))
    cells = np.zeros((Mv, 3), np.int64)
    for c in range(3):
        np.add.at(sums[:, c], lab, fixed[:, c])
        np.add.at(msum[:, c], lab, p[:, c])
    cells[lab] = ci
    fixed64 = origin + (cells.astype(np.float64) + sums.astype(np.float64) / (counts[:, None].astype(np.float64) * 2.0 ** 32)) * vs
    labels = np.full(P, -1, np.int32)
    labels[rows] = lab
    return dict(points=fixed64.astype(np.float32), mean64=msum / counts[:, None], fixed64=fixed64, counts=counts.astype(np.int32),
                first=first[order].astype(np.int32), labels=labels, origin=origin, cells=cells, status=0)
