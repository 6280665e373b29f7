"""CPU restatement of dmi_filter_depth_consistency (include/dmi.h states the definition), vectorised numpy, written
from the definition and not from the kernel: plain f64 operations in the definition's order (numpy rounds every elementwise
operation and contracts nothing), one (source, target) pair of views at a time over all pixels of the source.  Depths are
[n, H, W] in vtk point order (row 0 = the bottom image row), as the views hold them."""
import numpy as np

from coloration_depth_np import round_half_away


def thresholded(depth, best_cost=None, threshold=None):
    """Step 1: D = the depths with -1 wherever the best cost exceeds the threshold (a NaN cost does not)."""
    D = np.array(depth, dtype=np.float64, copy=True)
    if best_cost is not None and threshold is not None:
        with np.errstate(invalid="ignore"):
            D[np.asarray(best_cost, dtype=np.float64) > threshold] = -1.0
    return D


def valid_pixels(D):
    """valid iff D > 0 and D < +inf: false for NaN, -1, 0 and negatives."""
    with np.errstate(invalid="ignore"):
        return (D > 0.0) & (D < np.inf)


def world_points(D_s, K4, RT4):
    """Step 2: (w_0, w_1, w_2), each [H, W] in vtk row order, of every pixel of one view (garbage where the pixel is not valid)."""
    H, W = D_s.shape
    K = np.asarray(K4, dtype=np.float64).reshape(4, 4)
    RT = np.asarray(RT4, dtype=np.float64).reshape(4, 4)
    px = np.arange(W, dtype=np.float64)[None, :]
    py = (H - 1 - np.arange(H)).astype(np.float64)[:, None]  # vtk row r holds image row H-1-r
    with np.errstate(all="ignore"):
        yn = (py - K[1, 2]) / K[1, 1]
        xn = ((px - K[0, 2]) - K[0, 1] * yn) / K[0, 0]
        c = (xn * D_s, yn * D_s, D_s)
        q = [c[i] - RT[i, 3] for i in range(3)]
        return [(RT[0, j] * q[0] + RT[1, j] * q[1]) + RT[2, j] * q[2] for j in range(3)]


def pair_agrees(w, D_t, K4, RT4, abs_tol, rel_tol):
    """Step 3 for one target view: bool [H, W] over the source's pixels."""
    H, W = D_t.shape
    K = np.asarray(K4, dtype=np.float64).reshape(4, 4)
    RT = np.asarray(RT4, dtype=np.float64).reshape(4, 4)
    with np.errstate(all="ignore"):
        c = [((RT[i, 0] * w[0] + RT[i, 1] * w[1]) + RT[i, 2] * w[2]) + RT[i, 3] for i in range(3)]
        h = [((K[i, 0] * c[0] + K[i, 1] * c[1]) + K[i, 2] * c[2]) + K[i, 3] for i in range(3)]
        ok = (c[2] > 0.0) & ~(h[2] < 0.0)
        ru, rv = round_half_away(h[0] / h[2]), round_half_away(h[1] / h[2])
        ok = ok & (ru >= 0.0) & (rv >= 0.0) & (ru < float(W)) & (rv < float(H))  # false for NaN and infinities
        ix = np.where(ok, ru, 0.0).astype(np.int64)
        iy = np.where(ok, rv, 0.0).astype(np.int64)
        d = D_t[H - 1 - iy, ix]
        bound = abs_tol + rel_tol * c[2]
        return ok & (d > 0.0) & (np.abs(c[2] - d) <= bound)


def filter_depth_consistency(depth, K4, RT4, min_views, abs_tolerance=0.0, rel_tolerance=0.0, best_cost=None, threshold=None):
    """(out_depth [n, H, W] f64, count [n, H, W] int32) of the definition."""
    D = thresholded(depth, best_cost, threshold)
    n = D.shape[0]
    valid = valid_pixels(D)
    count = np.zeros(D.shape, dtype=np.int32)
    for s in range(n):
        w = world_points(D[s], K4[s], RT4[s])
        for t in range(n):
            if t != s:
                count[s] += pair_agrees(w, D[t], K4[t], RT4[t], float(abs_tolerance), float(rel_tolerance)) & valid[s]
    out = np.where(valid & (count >= int(min_views)), D, -1.0)
    return out, count
