"""fp64 restatement of camera alignment (numpy + scipy.spatial.cKDTree), the yardstick of tests/test_gpu_camera_align.py and the
engine of the mock tests/hip_mock_align.py.  Open3D is not a dependency of either project's tests; these are its documented rules
(registration_icp with TransformationEstimationPointToPlane): the nearest target point strictly inside the cap, r = (p - q) . n,
J = [p x n | n], J^T J x = -J^T r, T(x) = Rz Ry Rx | t, fitness = correspondences / source points, rmse = sqrt(sum d2 / correspondences),
stop when both change by less than 1e-6.  Inputs are the fp32 points; all arithmetic here is fp64."""
import numpy as np

try:
    from scipy.spatial import cKDTree
except ImportError:  # pragma: no cover
    cKDTree = None

ROW = 30
FEW, SINGULAR = 1, 2


def valid_rows(x):
    return np.isfinite(x[:, :3]).all(1)


def cap_squared(cap):
    c = np.float32(cap)
    return float(np.float32(c * c))


def normals(xyz, gw, gh, max_edge):
    """xyz (gh*gw, >=3) float32 organised cloud -> (gh*gw, 3) fp64 normals, NaN rows where there is none."""
    p = xyz[:, :3].astype(np.float64).reshape(gh, gw, 3)
    me2 = cap_squared(max_edge)
    out = np.full((gh, gw, 3), np.nan)
    c, l, r, u, d = p[1:-1, 1:-1], p[1:-1, :-2], p[1:-1, 2:], p[:-2, 1:-1], p[2:, 1:-1]
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = np.isfinite(c).all(-1)
        for nb in (l, r, u, d):
            ok &= np.isfinite(nb).all(-1) & (((nb - c) ** 2).sum(-1) <= me2)
        cr = np.cross(r - l, d - u)
        ln = np.sqrt((cr ** 2).sum(-1))
        ok &= ln > 0
        out[1:-1, 1:-1] = np.where(ok[..., None], cr / ln[..., None], np.nan)
    return out.reshape(-1, 3)


def transform(D, xyz0):
    """D (3,4) or (4,4) fp64, xyz0 (n, >=3) float32 -> (n, 3) float32: fp64, rounded once; NaN rows stay NaN."""
    D = np.asarray(D, np.float64)
    with np.errstate(invalid="ignore"):
        out = (xyz0[:, :3].astype(np.float64) @ D[:3, :3].T + D[:3, 3]).astype(np.float32)
    out[~np.isfinite(out).all(1)] = np.nan
    return out


def target_union(targets):
    """targets: list of (xyz (N, >=3) float32, nrm (N, 3)) -> the candidates (points with a valid normal): points (K,3) fp64,
    normals (K,3) fp64, global index (K,)."""
    pts, nrm, gid, off = [], [], [], 0
    for xyz, n in targets:
        ok = valid_rows(xyz) & ~np.isnan(np.asarray(n)[:, 0])
        pts.append(xyz[ok, :3].astype(np.float64))
        nrm.append(np.asarray(n, np.float64)[ok, :3])
        gid.append(off + np.flatnonzero(ok))
        off += len(xyz)
    return np.concatenate(pts), np.concatenate(nrm), np.concatenate(gid)


def correspond(q, union, cap2, brute=False, tree=None):
    """q (M,3) float32 queries (NaN rows take no part) -> dict(idx (M,) global target index or -1, pos (M,) row of the union,
    d2 (M,) fp64, near (M,) bool: the best two candidates -- the cap counts as one -- differ by less than 1e-6 relative)."""
    pts, _, gid = union
    M = len(q)
    idx, pos, d2 = np.full(M, -1, np.int64), np.full(M, -1, np.int64), np.full(M, np.nan)
    near = np.zeros(M, bool)
    ok = np.isfinite(q).all(1)
    qq = q[ok].astype(np.float64)
    if len(pts) == 0 or len(qq) == 0:
        return dict(idx=idx, pos=pos, d2=d2, near=near)
    if brute or cKDTree is None:
        dd = ((qq[:, None, :] - pts[None, :, :]) ** 2).sum(-1)
        order = np.argsort(dd, axis=1, kind="stable")[:, :2]  # (ties: the lower global index, the union is in that order)
        b = order[:, 0]
        d_b = dd[np.arange(len(qq)), b]
        d_s = dd[np.arange(len(qq)), order[:, 1]] if dd.shape[1] > 1 else np.full(len(qq), np.inf)
    else:
        tree = tree or cKDTree(pts)
        dist, nn = tree.query(qq, k=2) if len(pts) > 1 else (lambda a, b: (a[:, None], b[:, None]))(*tree.query(qq, k=1))
        b = nn[:, 0]
        d_b = ((qq - pts[b]) ** 2).sum(-1)
        d_s = ((qq - pts[np.minimum(nn[:, 1], len(pts) - 1)]) ** 2).sum(-1) if dist.shape[1] > 1 else np.full(len(qq), np.inf)
        d_s = np.where(np.isfinite(dist[:, -1]), d_s, np.inf)
    hit = d_b < cap2
    second = np.where(hit, np.minimum(d_s, cap2), d_b)  # (no hit: the runner-up of "none" is the best candidate itself)
    first = np.where(hit, d_b, cap2)
    nr = np.abs(second - first) <= 1e-6 * np.maximum(second, first)
    rows = np.flatnonzero(ok)
    idx[rows[hit]], pos[rows[hit]], d2[rows[hit]] = gid[b[hit]], b[hit], d_b[hit]
    near[rows] = nr
    return dict(idx=idx, pos=pos, d2=d2, near=near)


def normal_equations(q, corr, union):
    """The 30 sums of the matched queries: 21 upper entries of J^T J (row-major), 6 of J^T r, count, sum r^2, sum d2."""
    pts, nrm, _ = union
    m = corr["pos"] >= 0
    p = q[m].astype(np.float64)
    t, n = pts[corr["pos"][m]], nrm[corr["pos"][m]]
    r = ((p - t) * n).sum(1)
    J = np.concatenate([np.cross(p, n), n], 1)
    A, b = J.T @ J, J.T @ r
    return np.concatenate([A[np.triu_indices(6)], b, [float(m.sum()), (r * r).sum(), corr["d2"][m].sum()]])


def unpack(sums):
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = sums[:21]
    return A + np.triu(A, 1).T, np.asarray(sums[21:27])


def solve(sums):
    """x of J^T J x = -J^T r, or None with the status bit (fewer than 6 correspondences; a pivot of LDL^T <= 1e-12 max diagonal)."""
    A, b = unpack(sums)
    if sums[27] < 6:
        return None, FEW
    maxd = A.diagonal().max()
    L, dd = np.eye(6), np.zeros(6)
    for j in range(6):
        d = A[j, j] - (L[j, :j] ** 2 * dd[:j]).sum()
        if not d > 1e-12 * maxd:
            return None, SINGULAR
        dd[j] = d
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j] * dd[:j]).sum()) / d
    return np.linalg.solve(A, -b), 0


def transform_of(x):
    """Open3D's TransformVector6dToMatrix4d: Rz(x2) Ry(x1) Rx(x0), translation x3..5."""
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rz @ Ry @ Rx, x[3:6]
    return T


def evaluate(src0_frames, D, unions, cap2, brute=False, trees=None):
    """One evaluation at D: the sums over the frames, the per-frame queries and correspondences."""
    qs = [transform(D, s) for s in src0_frames]
    corrs = [correspond(q, u, cap2, brute, None if trees is None else trees[f]) for f, (q, u) in enumerate(zip(qs, unions))]
    sums = sum(normal_equations(q, c, u) for q, c, u in zip(qs, corrs, unions))
    return sums, qs, corrs


def figures(sums, n_queries):
    count = sums[27]
    return (count / n_queries if n_queries > 0 else 0.0), (np.sqrt(sums[29] / count) if count > 0 else 0.0)


def icp(src0_frames, targets_frames, cap, max_iterations, D0=None, brute=False):
    """registration_icp's loop.  src0_frames: list over frames of (n, >=3) float32 queries (NaN rows: no part; already sampled);
    targets_frames: list over frames of lists of (xyz, nrm).  Returns dict(D (4,4), fitness, rmse, iterations, status, hist)."""
    cap2 = cap_squared(cap)
    D = np.eye(4) if D0 is None else np.array(D0, np.float64)
    unions = [target_union(t) for t in targets_frames]
    trees = None if (brute or cKDTree is None) else [cKDTree(u[0]) if len(u[0]) else None for u in unions]
    nq = sum(int(valid_rows(s).sum()) for s in src0_frames)
    it, status, hist = 0, 0, []
    sums, _, _ = evaluate(src0_frames, D, unions, cap2, brute, trees)
    fit, rmse = figures(sums, nq)
    hist.append((sums[27], fit, rmse))
    for _ in range(max_iterations):
        x, st = solve(sums)
        if x is None:
            status |= st
            break
        D = transform_of(x) @ D
        it += 1
        sums, _, _ = evaluate(src0_frames, D, unions, cap2, brute, trees)
        f2, r2 = figures(sums, nq)
        hist.append((sums[27], f2, r2))
        conv = abs(f2 - fit) < 1e-6 and abs(r2 - rmse) < 1e-6
        fit, rmse = f2, r2
        if conv:
            break
    return dict(D=D, fitness=fit, rmse=rmse, iterations=it, status=status, hist=hist)


def sample(cloud, gw, gh, s):
    """The queries of an organised cloud at sample_stride s (raster order of the samples)."""
    return cloud.reshape(gh, gw, -1)[::s, ::s].reshape(-1, cloud.shape[-1])


def align_views(clouds0, gw, gh, cap, max_edge, max_iterations=30, sweeps=2, anchor=0, sample_stride=1):
    """The sweep loop of align_cameras.  clouds0 [V][F]: (gh*gw, >=3) float32 organised clouds before any correction.
    Returns dict(D (V,4,4), fitness, rmse, iterations, status (V,), order: the (view, targets) pairs in the order they ran)."""
    V, F = len(clouds0), len(clouds0[0])
    D = np.stack([np.eye(4)] * V)
    cur = [[c[:, :3].copy() for c in row] for row in clouds0]
    nrm = [[normals(c, gw, gh, max_edge) for c in row] for row in cur]
    info = dict(fitness=np.zeros(V), rmse=np.zeros(V), iterations=np.zeros(V, int), status=np.zeros(V, int), order=[])
    for _ in range(sweeps):
        for v in range(V):
            if v == anchor:
                continue
            others = [u for u in range(V) if u != v]
            info["order"].append((v, tuple(others)))
            r = icp([sample(clouds0[v][f], gw, gh, sample_stride) for f in range(F)], [[(cur[u][f], nrm[u][f]) for u in others] for f in range(F)],
                    cap, max_iterations, D[v])
            D[v] = r["D"]
            for k in ("fitness", "rmse", "iterations", "status"):
                info[k][v] = r[k]
            for f in range(F):
                cur[v][f] = transform(D[v], clouds0[v][f])
                nrm[v][f] = normals(cur[v][f], gw, gh, max_edge)
    info["D"] = D
    return info
