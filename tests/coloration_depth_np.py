"""Numpy restatement of the depth-tested colouring (include/dmi.h: dmi_color_set_depth_test): the projection,
bounds test and integer arithmetic of oracle_np.color_mesh_np with the visibility test added, in plain f64 operations in the
definition's order (numpy rounds every elementwise operation and contracts nothing).  Vectorised over the vertices, one view
at a time."""
import numpy as np


def round_half_away(u):
    """std::round: half away from zero, exact (the fractional part u - trunc(u) is exact)."""
    t = np.trunc(u)
    return t + np.where(np.abs(u - t) >= 0.5, np.sign(u), 0.0)


def camera_z(points, RT):
    """cz = ((RT[8]*x + RT[9]*y) + RT[10]*z) + RT[11]: TransformPoint's camera z (RD.cxx:173)."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    R = np.asarray(RT, dtype=np.float64).reshape(4, 4)
    return ((R[2, 0] * p[:, 0] + R[2, 1] * p[:, 1]) + R[2, 2] * p[:, 2]) + R[2, 3]


def pixels(points, K4, RT4):
    """(px, py, ok) of every vertex in one view: RT as a point transform, K as a vector transform, divide, std::round
    (RD.cxx:169-182); ok False where the quotient is not finite or beyond the int range.  The bounds test is the caller's."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    R = np.asarray(RT4, dtype=np.float64).reshape(4, 4)
    K = np.asarray(K4, dtype=np.float64).reshape(4, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    c = [((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z) + R[r, 3] for r in range(3)]
    d = [(K[r, 0] * c[0] + K[r, 1] * c[1]) + K[r, 2] * c[2] for r in range(3)]
    with np.errstate(all="ignore"):
        ru, rv = round_half_away(d[0] / d[2]), round_half_away(d[1] / d[2])
        ok = np.isfinite(ru) & np.isfinite(rv) & (np.abs(ru) < 2.0 ** 31) & (np.abs(rv) < 2.0 ** 31)
    px = np.where(ok, ru, -1).astype(np.int64)
    py = np.where(ok, rv, -1).astype(np.int64)
    return px, py, ok


def color_mesh_depth_np(points, colors, depths, K4, RT4, tol=None):
    """(mean u8 [n, 3], median u8 [n, 3], count i32 [n]).  colors [v, H, W, 3] u8 and depths [v, H, W] f64 in vtk point order
    (row 0 = the bottom image row).  tol None: no test (the reference's colouring, as color_mesh_np); else a pair counts iff the
    bounds test passes, cz > 0, d > 0 and fabs(cz - d) <= tol."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    col = np.asarray(colors, dtype=np.uint8)
    n, H, W, _ = col.shape
    dep = None if tol is None else np.asarray(depths, dtype=np.float64).reshape(n, H, W)
    nv = pts.shape[0]
    vals = np.full((n, nv, 3), 1000, dtype=np.int64)   # 1000: no value (sorts after every u8)
    valid = np.zeros((n, nv), dtype=bool)
    for m in range(n):
        px, py, ok = pixels(pts, K4[m], RT4[m])
        ok &= (px >= 0) & (py >= 0) & (px < W) & (py < H)
        row = np.where(ok, H - 1 - py, 0)
        colx = np.where(ok, px, 0)
        if tol is not None:
            cz = camera_z(pts, RT4[m])
            d = dep[m, row, colx]
            with np.errstate(invalid="ignore"):
                ok &= (cz > 0.0) & (d > 0.0) & (np.abs(cz - d) <= tol)
        valid[m] = ok
        vals[m][ok] = col[m, row[ok], colx[ok]]
    count = valid.sum(axis=0).astype(np.int32)
    mean = np.zeros((nv, 3), dtype=np.uint8)
    median = np.zeros((nv, 3), dtype=np.uint8)
    seen = count > 0
    sums = np.where(valid[:, :, None], vals, 0).sum(axis=0)
    k = count[seen].astype(np.int64)
    mean[seen] = (sums[seen] // k[:, None]).astype(np.uint8)          # int(sum / k): exact at these magnitudes
    srt = np.sort(vals, axis=0)[:, seen]                               # [view, vertex, channel]
    hi = np.take_along_axis(srt, np.repeat((k // 2)[None, :, None], 3, axis=2), axis=0)[0]
    lo = np.take_along_axis(srt, np.repeat(np.where(k % 2 == 0, k // 2 - 1, k // 2)[None, :, None], 3, axis=2), axis=0)[0]
    median[seen] = ((hi + lo) // 2).astype(np.uint8)                  # (a + b) / 2 truncated; a == b for odd counts
    return mean, median, count
