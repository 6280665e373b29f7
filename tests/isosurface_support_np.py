"""CPU restatement of dmi_filter_isosurface_support (include/dmi.h states the definition), vectorised numpy, written
from the definition and not from the kernels: plain f64 operations in the definition's order (numpy rounds every elementwise
operation and contracts nothing), one view at a time over all vertices; the filter from the counts by boolean masks and
cumulative sums.  Depths are [n, H, W] in vtk point order (row 0 = the bottom image row), as the views hold them, already
thresholded (-1 where the best cost exceeded the threshold) and, for an f32 store, already rounded to f32."""
import numpy as np

from coloration_depth_np import round_half_away


def pair_terms(points, K4, RT4):
    """(c [3][V], px, py, inside) of every vertex in one view: the camera coordinates, the rounded pixel (int64, -1 where there
    is none) and whether the pixel exists at all (finite quotients of magnitude below 2^31); the image bounds are the caller's."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    R = np.asarray(RT4, dtype=np.float64).reshape(-1)
    K = np.asarray(K4, dtype=np.float64).reshape(-1)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        c = [((R[4 * r] * x + R[4 * r + 1] * y) + R[4 * r + 2] * z) + R[4 * r + 3] for r in range(3)]
        h = [((K[4 * r] * c[0] + K[4 * r + 1] * c[1]) + K[4 * r + 2] * c[2]) + K[4 * r + 3] for r in range(3)]
        ru, rv = round_half_away(h[0] / h[2]), round_half_away(h[1] / h[2])
        ok = np.isfinite(ru) & np.isfinite(rv) & (np.abs(ru) < 2.0 ** 31) & (np.abs(rv) < 2.0 ** 31)
    px = np.where(ok, ru, -1).astype(np.int64)
    py = np.where(ok, rv, -1).astype(np.int64)
    return c, px, py, ok


def facing_s(normals, RT4, c):
    """s [V]: the normal, rotated into the camera's frame, dotted with the camera coordinates (every operation rounded)."""
    n = np.asarray(normals, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    R = np.asarray(RT4, dtype=np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        m = [(R[4 * r] * n[:, 0] + R[4 * r + 1] * n[:, 1]) + R[4 * r + 2] * n[:, 2] for r in range(3)]
        return (m[0] * c[0] + m[1] * c[1]) + m[2] * c[2]


def pair_table(points, normals, depths, K4, RT4, tolerance, facing=True):
    """(supports [n, V] bool, gap [n, V] f64: the rounded fabs(c_2 - d) where a pixel and a depth > 0 exist, NaN elsewhere,
    s [n, V] f64 or None)."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    dep = np.asarray(depths, dtype=np.float64)
    n, H, W = dep.shape
    supports = np.zeros((n, len(pts)), dtype=bool)
    gap = np.full((n, len(pts)), np.nan)
    s_all = np.full((n, len(pts)), np.nan) if facing else None
    for m in range(n):
        c, px, py, ok = pair_terms(pts, K4[m], RT4[m])
        with np.errstate(invalid="ignore"):
            ok = ok & (c[2] > 0.0) & (px >= 0) & (px < W) & (py >= 0) & (py < H)
            d = dep[m, np.where(ok, H - 1 - py, 0), np.where(ok, px, 0)]
            g = np.abs(c[2] - d)
            ok = ok & (d > 0.0)
            gap[m] = np.where(ok, g, np.nan)
            ok = ok & (g <= tolerance)
            if facing:
                s_all[m] = facing_s(normals, RT4[m], c)
                ok = ok & (s_all[m] < 0.0)
        supports[m] = ok
    return supports, gap, s_all


def support(points, normals, depths, K4, RT4, tolerance, facing=True):
    """support [V] int32: the number of views that support each vertex."""
    return pair_table(points, normals, depths, K4, RT4, tolerance, facing)[0].sum(axis=0).astype(np.int32)


def filter_mesh(points, triangles, normals, counts, min_views):
    """(vertices, triangles, normals or None) after the filter with the counts `counts`: a triangle survives iff its three ids are
    below V and each has at least min_views supporting views, a vertex iff a surviving triangle names it; order kept, ids
    renumbered.  min_views 0 changes nothing."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    nrm = None if normals is None else np.asarray(normals, dtype=np.float32).reshape(-1, 3)
    if min_views == 0:
        return pts.copy(), tri.copy(), None if nrm is None else nrm.copy()
    V = len(pts)
    valid = ((tri >= 0) & (tri < V)).all(axis=1)
    enough = np.asarray(counts) >= min_views
    keep_t = valid & enough[np.where(valid[:, None], tri, 0)].all(axis=1)
    keep_v = np.zeros(V, dtype=bool)
    keep_v[tri[keep_t].reshape(-1)] = True
    vmap = np.cumsum(keep_v) - keep_v
    return pts[keep_v], vmap[tri[keep_t]].astype(np.int64).reshape(-1, 3), None if nrm is None else nrm[keep_v]
