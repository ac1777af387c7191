"""CPU restatement of the depth cleaning semantics (include/mvtracker_hip.h, "Depth cleaning") in fp64 with numpy and
scipy.spatial.cKDTree -- a brute-force numpy search stands in where scipy is missing (small clouds only).

It restates Open3D's RemoveStatisticalOutliers / RemoveRadiusOutliers as the reference's demo calls them: the kNN and radius searches
include the query point itself, the sample deviation divides by (valid - 1), the radius test is strict.  Open3D itself is not a
dependency, so no recorded output of the reference exists for this feature; this file is the yardstick.

The ``include_self`` / ``drop_last`` / ``divisor`` switches build the DEFECTS the tests must be able to see; the defaults are the rule.
"""
import numpy as np

try:
    from scipy.spatial import cKDTree
except ImportError:  # pragma: no cover
    cKDTree = None

BRUTE_FORCE_LIMIT = 8192


def _sorted_knn_distances(pts, k):
    """(M, k) Euclidean distances from every point to its k nearest points of the same cloud, itself included, ascending."""
    M = len(pts)
    if cKDTree is not None:
        d, _ = cKDTree(pts).query(pts, k=k)
        return d.reshape(M, k)
    assert M <= BRUTE_FORCE_LIMIT, "scipy is missing and the cloud is too large for the brute-force search"
    out = np.empty((M, k))
    for i0 in range(0, M, 256):
        diff = pts[i0:i0 + 256, None, :] - pts[None, :, :]
        out[i0:i0 + 256] = np.sort(np.sqrt((diff * diff).sum(-1)), axis=1)[:, :k]
    return out


def mean_knn_distance(pts, k, include_self=True, drop_last=False):
    """a_i: the mean distance from point i to its k' = min(k, M) nearest points, itself included at distance 0; the divisor is k'.
    Defects: include_self=False averages the k' nearest OTHER points; drop_last=True uses k - 1 neighbours."""
    pts = np.asarray(pts, np.float64)
    M = len(pts)
    if M == 0:
        return np.zeros(0)
    if drop_last:
        k = max(1, k - 1)
    if include_self:
        kk = min(k, M)
        return _sorted_knn_distances(pts, kk).sum(1) / kk
    kk = min(k + 1, M)
    d = _sorted_knn_distances(pts, kk)[:, 1:]
    return d.sum(1) / max(1, d.shape[1])


def statistics(a, std_ratio, divisor="M"):
    """M, mu, sigma, thr and the keep mask from the mean distances of the M valid points (fp64).  The divisor of mu and sigma is M,
    every valid point; the defect divisor="positive" uses the number of a > 0."""
    a = np.asarray(a, np.float64)
    M = len(a)
    pos = a > 0
    n = M if divisor == "M" else int(pos.sum())
    if M <= 1 or n <= 1:
        return dict(M=M, mu=0.0, sigma=0.0, thr=0.0, keep=np.zeros(M, bool))
    mu = a[pos].sum() / n
    sigma = np.sqrt(((a[pos] - mu) ** 2).sum() / (n - 1))
    thr = mu + std_ratio * sigma
    return dict(M=M, mu=mu, sigma=sigma, thr=thr, keep=pos & (a < thr))


def radius_sq(radius):
    """r^2 as the kernel takes it: float(radius) * float(radius), rounded to fp32."""
    r = np.float32(radius)
    return float(np.float32(r * r))


def radius_counts(pts, radius, r2=None):
    """c_i = #{j : |p_i - p_j|^2 < r^2}, self included (fp64 distances)."""
    pts = np.asarray(pts, np.float64)
    r2 = radius_sq(radius) if r2 is None else r2
    M = len(pts)
    if M == 0:
        return np.zeros(0, np.int64)
    if cKDTree is not None:
        t = cKDTree(pts)
        nb = t.query_ball_point(pts, np.sqrt(r2) * (1 + 1e-9) + 1e-12)  # a superset; the strict test is applied below
        out = np.empty(M, np.int64)
        for i, js in enumerate(nb):
            d = pts[js] - pts[i]
            out[i] = int(((d * d).sum(1) < r2).sum())
        return out
    assert M <= BRUTE_FORCE_LIMIT
    out = np.empty(M, np.int64)
    for i0 in range(0, M, 256):
        diff = pts[i0:i0 + 256, None, :] - pts[None, :, :]
        out[i0:i0 + 256] = ((diff * diff).sum(-1) < r2).sum(1)
    return out


def valid_rows(xyz):
    """Rows of a cloud (P, >= 3) that take part: three finite coordinates."""
    return np.isfinite(np.asarray(xyz)[:, :3]).all(1)


def clean_cloud(xyz, method="statistical", nb_neighbors=20, std_ratio=2.0, radius=0.05, min_points=5, include_self=True, drop_last=False,
                divisor="M", r2=None):
    """One cloud (P, 3 or 4), NaN rows taking no part.  Returns full-size arrays: ``keep`` (P,) bool and, statistical: ``a`` (P,) fp64
    (NaN where not valid), ``a32`` its fp32 rounding, M, mu, sigma, thr; radius: ``c`` (P,) int64 (-1 where not valid), M."""
    xyz = np.asarray(xyz)
    ok = valid_rows(xyz)
    pts = xyz[ok, :3].astype(np.float64)
    P = len(xyz)
    keep = np.zeros(P, bool)
    if method == "statistical":
        a = mean_knn_distance(pts, nb_neighbors, include_self, drop_last)
        st = statistics(a.astype(np.float32).astype(np.float64), std_ratio, divisor)  # (the statistics are taken over the fp32 a_i)
        full = np.full(P, np.nan)
        full[ok] = a
        keep[ok] = st["keep"]
        return dict(a=full, a32=full.astype(np.float32), keep=keep, M=st["M"], mu=st["mu"], sigma=st["sigma"], thr=st["thr"])
    if method == "radius":
        c = radius_counts(pts, radius, r2)
        full = np.full(P, -1, np.int64)
        full[ok] = c
        keep[ok] = c > min_points
        return dict(c=full, keep=keep, M=int(ok.sum()))
    raise ValueError(method)


def sphere_inside(xyz, centre, radius, margin=0.0):
    """The sphere crop: |X - centre|^2 < fl(r r) with fp32 differences (the kernel's), the squares summed in fp64.  With ``margin``
    also returns which points lie within margin * r^2 of the surface, where the kernel's fp32 d2 may decide either way."""
    p = np.asarray(xyz, np.float32)[..., :3]
    d = (p - np.asarray(centre, np.float32)).astype(np.float64)
    s = (d * d).sum(-1)
    r2 = radius_sq(radius)
    with np.errstate(invalid="ignore"):
        inside = s < r2
        return (inside, np.abs(s - r2) <= margin * r2) if margin else inside


def valid_pixels(depth, conf=None, conf_thresh=None):
    """Pixels of a depth map that enter the cloud before the sphere crop: finite depth > 0 and (both given) conf > conf_thresh."""
    d = np.asarray(depth, np.float32)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(d) & (d > 0)
        if conf is not None and conf_thresh is not None:
            ok &= np.asarray(conf, np.float32) > np.float32(conf_thresh)
    return ok
