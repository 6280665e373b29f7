"""CPU restatement of dmi_estimate_scene_bounds (include/dmi.h states the definition), vectorised numpy, written from
the definition and not from the kernel: plain f64 operations in the definition's order (numpy rounds every elementwise operation and
contracts nothing), validity and back-projection taken from the restatement of 8g, the ranks by np.sort on the keys.  Depths are
[n, H, W] in vtk point order (row 0 = the bottom image row), as the views hold them."""
import numpy as np

from depth_consistency_np import thresholded, valid_pixels, world_points

SIGN = np.uint64(1) << np.uint64(63)
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def keys_of(values):
    """bits ^ (bits >> 63 ? ~0 : 1 << 63): ascending key order is numeric order, -0.0 before +0.0."""
    bits = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)
    return bits ^ np.where(bits >> np.uint64(63) != 0, ALL, SIGN)


def values_of(keys):
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    return (keys ^ np.where(keys >> np.uint64(63) != 0, SIGN, ALL)).view(np.float64)


def trim_rank(trim_fraction, N):
    """k = min((uint64_t)(trim_fraction * (double)N), (N - 1) / 2)."""
    return min(int(np.float64(trim_fraction) * np.float64(N)), (N - 1) // 2)


def taking_part(n, H, W, pixel_step):
    """bool [H, W] in vtk row order: image pixel (px, py) with px % step == 0 and py % step == 0; vtk row r is image row H-1-r."""
    px = np.arange(W)[None, :]
    py = (H - 1 - np.arange(H))[:, None]
    return (px % pixel_step == 0) & (py % pixel_step == 0)


def counted_coordinates(depth, K4, RT4, axes=None, pixel_step=1, best_cost=None, threshold=None):
    """[3, N] f64: s_a of every counted point (steps 1 to 3), in view, vtk row, column order."""
    D = thresholded(depth, best_cost, threshold)
    n, H, W = D.shape
    A = np.eye(3) if axes is None else np.asarray(axes, dtype=np.float64).reshape(3, 3)
    part = taking_part(n, H, W, int(pixel_step))
    out = [[], [], []]
    for m in range(n):
        take = valid_pixels(D[m]) & part
        w = [c[take] for c in world_points(D[m], K4[m], RT4[m])]
        with np.errstate(all="ignore"):
            s = [(A[a, 0] * w[0] + A[a, 1] * w[1]) + A[a, 2] * w[2] for a in range(3)]
        counted = np.isfinite(s[0]) & np.isfinite(s[1]) & np.isfinite(s[2])
        for a in range(3):
            out[a].append(s[a][counted])
    return np.stack([np.concatenate(o) for o in out])


def bounds_of(s, trim_fraction=0.0):
    """(lo [3], hi [3], N) of steps 4 and 5 from the counted coordinates [3, N]."""
    N = s.shape[1]
    if N == 0:
        return np.full(3, np.nan), np.full(3, np.nan), 0
    k = trim_rank(trim_fraction, N)
    lo, hi = np.empty(3), np.empty(3)
    for a in range(3):
        ordered = values_of(np.sort(keys_of(s[a])))
        lo[a], hi[a] = ordered[k], ordered[N - 1 - k]
    return lo, hi, N


def estimate_scene_bounds(depth, K4, RT4, trim_fraction=0.0, pixel_step=1, axes=None, best_cost=None, threshold=None):
    """(lo [3] f64, hi [3] f64, N) of the definition."""
    return bounds_of(counted_coordinates(depth, K4, RT4, axes, pixel_step, best_cost, threshold), trim_fraction)
