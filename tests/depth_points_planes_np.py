"""The plane fit of include/dmi.h (dmi_fit_point_planes, dmi_views_fit_point_planes), restated in numpy straight from
the definition: brute force over all pairs, no grid.  Every floating-point operation is an f64 numpy operation of its own, so each is
rounded once and nothing is contracted; the moments are int64 sums."""
import numpy as np

MOVE, NORMALS = 1, 2
MAX_MEMBERS = 1 << 22
SWEEPS = 6
REPORT_NAMES = ("points_in", "fitted", "unsupported", "crowded", "max_neighbors", "neighbor_sum")   # the rest is the device's or a float
ROWS = 512        # queries per block of the pair matrix, at most
PAIRS = 1 << 18   # pairs per block, about


def lattice(radius):
    """(s, inv_s) of step 2."""
    radius = np.float64(radius)
    with np.errstate(over="ignore", under="ignore"):
        r2 = radius * radius
    if not (radius > 0 and np.isfinite(r2) and r2 >= np.finfo(np.float64).tiny):
        raise ValueError("radius")
    e = int(np.frexp(radius)[1])
    with np.errstate(over="ignore", under="ignore"):
        s, inv_s = np.ldexp(np.float64(1.0), 15 - e), np.ldexp(np.float64(1.0), e - 15)
    tiny = np.finfo(np.float64).tiny
    if not (np.isfinite(s) and np.isfinite(inv_s) and s >= tiny and inv_s >= tiny):
        raise ValueError("radius")
    return s, inv_s


def moments(xyz, radius):
    """(m int64 [P], S int64 [P, 3], T int64 [P, 6]) of steps 1 to 3.  The membership test runs over the whole pair matrix, in
    blocks of queries small enough to stay in the cache; the offsets are then rounded and summed for the member pairs alone."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    if not np.isfinite(xyz).all():
        raise ValueError("non-finite coordinate")
    s, _ = lattice(radius)
    radius = np.float64(radius)
    r2 = radius * radius
    p = len(xyz)
    m, S, T = np.zeros(p, dtype=np.int64), np.zeros((p, 3), dtype=np.int64), np.zeros((p, 6), dtype=np.int64)
    rows = max(1, min(ROWS, PAIRS // max(p, 1)))
    planes = [np.ascontiguousarray(xyz[:, k]) for k in range(3)]
    with np.errstate(over="ignore"):
        for first in range(0, p, rows):
            q = xyz[first:first + rows]
            d0 = planes[0][None, :] - q[:, None, 0]
            d1 = planes[1][None, :] - q[:, None, 1]
            d2 = planes[2][None, :] - q[:, None, 2]
            member = ((d0 * d0 + d1 * d1) + d2 * d2) <= r2
            i, j = np.nonzero(member)            # by query, then by index; every query has a member: itself
            count = member.sum(axis=1)
            starts = np.concatenate([[0], np.cumsum(count)[:-1]])
            u = [np.rint((xyz[j, k] - q[i, k]) * s).astype(np.int64) for k in range(3)]
            m[first:first + rows] = count
            for k in range(3):
                S[first:first + rows, k] = np.add.reduceat(u[k], starts)
            for col, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                T[first:first + rows, col] = np.add.reduceat(u[a] * u[b], starts)
    return m, S, T


def _rotate(A, V, p, q, r):
    """One Jacobi rotation of step 4 on every row of the stacks A [K, 3, 3] and V [K, 3, 3], skipped where A_pq == 0."""
    a = A[:, p, q].copy()
    go = a != 0.0
    safe = np.where(go, a, 1.0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        theta = (A[:, q, q] - A[:, p, p]) / (2.0 * safe)
        t = np.where(theta < 0.0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
        sigma = t * c
        ta = t * safe
        app, aqq = A[:, p, p] - ta, A[:, q, q] + ta
        rp, rq = A[:, r, p].copy(), A[:, r, q].copy()
        new_rp, new_rq = c * rp - sigma * rq, sigma * rp + c * rq
        vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
        new_vp, new_vq = c[:, None] * vp - sigma[:, None] * vq, sigma[:, None] * vp + c[:, None] * vq
    A[:, p, p], A[:, q, q] = np.where(go, app, A[:, p, p]), np.where(go, aqq, A[:, q, q])
    A[:, p, q] = A[:, q, p] = np.where(go, 0.0, A[:, p, q])
    A[:, r, p] = A[:, p, r] = np.where(go, new_rp, rp)
    A[:, r, q] = A[:, q, r] = np.where(go, new_rq, rq)
    V[:, :, p], V[:, :, q] = np.where(go[:, None], new_vp, vp), np.where(go[:, None], new_vq, vq)


def fit_from_moments(m, S, T):
    """(c [K, 3], n [K, 3] not yet oriented, lambda_min [K]) of step 4 for K balls (m >= 1 each)."""
    count = np.asarray(m, dtype=np.int64).astype(np.float64)
    S, T = np.asarray(S, dtype=np.int64).astype(np.float64), np.asarray(T, dtype=np.int64).astype(np.float64)
    c = S / count[:, None]
    A = np.empty((len(count), 3, 3))
    for col, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        A[:, a, b] = A[:, b, a] = T[:, col] / count - c[:, a] * c[:, b]
    V = np.tile(np.eye(3), (len(count), 1, 1))
    for _ in range(SWEEPS):
        _rotate(A, V, 0, 1, 2)
        _rotate(A, V, 0, 2, 1)
        _rotate(A, V, 1, 2, 0)
    lam = A[:, 0, 0].copy()
    n = V[:, :, 0].copy()
    for k in (1, 2):
        better = A[:, k, k] < lam
        lam = np.where(better, A[:, k, k], lam)
        n = np.where(better[:, None], V[:, :, k], n)
    length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    return c, n / length[:, None], lam


def orient(n, old):
    """Step 5 on [K, 3] normals and the old normals widened to f64."""
    g = (n[:, 0] * old[:, 0] + n[:, 1] * old[:, 1]) + n[:, 2] * old[:, 2]
    most = n[:, 0].copy()
    for k in (1, 2):
        most = np.where(np.abs(n[:, k]) > np.abs(most), n[:, k], most)
    negate = np.where(g == 0.0, most < 0.0, g < 0.0)
    return np.where(negate[:, None], -n, n)


def results_from_moments(m, S, T, inv_s, old):
    """(t [K], n [K, 3] oriented, plane_rms f32 [K]) of steps 4 to 6."""
    c, n, lam = fit_from_moments(m, S, T)
    n = orient(n, np.asarray(old, dtype=np.float64))
    rms = (np.sqrt(np.where(lam > 0.0, lam, 0.0)) * inv_s).astype(np.float32)
    t = ((c[:, 0] * n[:, 0] + c[:, 1] * n[:, 1]) + c[:, 2] * n[:, 2]) * inv_s
    return t, n, rms


def fit_planes(xyz, normal, radius, min_neighbors, flags):
    """(dict of xyz f64 [P, 3], normal f32 [P, 3], plane_rms f32 [P], neighbors u32 [P]; report).  normal may be None: zeros."""
    if min_neighbors < 2:
        raise ValueError("min_neighbors")
    if flags not in (1, 2, 3):
        raise ValueError("flags")
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    p = len(xyz)
    normal = np.zeros((p, 3), dtype=np.float32) if normal is None else np.ascontiguousarray(normal, dtype=np.float32).reshape(-1, 3)
    _, inv_s = lattice(radius)
    m, S, T = moments(xyz, radius)
    crowded = m > MAX_MEMBERS
    fit = ~crowded & (m - 1 >= min_neighbors)
    out_xyz, out_normal = xyz.copy(), normal.copy()
    rms = np.full(p, -1.0, dtype=np.float32)
    max_shift = 0.0
    if fit.any():
        t, n, rms[fit] = results_from_moments(m[fit], S[fit], T[fit], inv_s, normal[fit])
        if flags & MOVE:
            out_xyz[fit] = xyz[fit] + t[:, None] * n
            max_shift = float(np.abs(t).max())
        if flags & NORMALS:
            out_normal[fit] = n.astype(np.float32)
    neighbors = (m - 1).astype(np.uint32)
    report = dict(points_in=p, fitted=int(fit.sum()), unsupported=int((~fit & ~crowded).sum()), crowded=int(crowded.sum()),
                  max_neighbors=int(neighbors.max()) if p else 0, neighbor_sum=int(neighbors.astype(np.uint64).sum()), max_shift=max_shift)
    return dict(xyz=out_xyz, normal=out_normal, plane_rms=rms, neighbors=neighbors), report
