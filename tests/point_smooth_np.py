"""CPU restatement of the point smoothing (include/dmi.h: dmi_set_point_smoothing) in numpy: three passes, x then y
then z, each over the full f64 result of the one before; on the pass's axis, with N points, radius r and weights k_0..k_r,

    v(t) = value at clamp(t, 0, N-1);  acc = k_0 * v(q);  for i = 1..r ascending: acc = acc + k_i * (v(q-i) + v(q+i)),

every operation a rounded f64 operation of its own (numpy neither fuses nor reorders them).  The weights are passed in: the library
is the authority on them (capi.point_smoothing_weights)."""
import numpy as np


def radius(sigma, truncate=3.0):
    return int(np.ceil(truncate * sigma))


def weights_np(sigma, truncate=3.0):
    """The weights by the formula of the definition with numpy's exp: what the library's must be within a few ulp of."""
    r = radius(sigma, truncate)
    w = [1.0] + [float(np.exp(-float(i * i) / (2 * sigma * sigma))) for i in range(1, r + 1)]
    side = 0.0
    for i in range(1, r + 1):
        side = w[1] if i == 1 else side + w[i]
    S = w[0] + 2 * side
    return np.array([x / S for x in w], dtype=np.float64)


def smooth_axis(P, k, axis):
    """One pass along `axis` of P with the weights k_0..k_r; a single weight (r = 0: the axis is skipped) returns P's own bits."""
    k = np.asarray(k, dtype=np.float64)
    if len(k) == 1:
        return P.copy()
    n = P.shape[axis]
    q = np.arange(n)
    with np.errstate(all="ignore"):
        acc = k[0] * P
        for i in range(1, len(k)):
            lo = np.take(P, np.clip(q - i, 0, n - 1), axis=axis)
            hi = np.take(P, np.clip(q + i, 0, n - 1), axis=axis)
            acc = acc + k[i] * (lo + hi)
    return acc


def smooth(points, weights_xyz):
    """points [nz+1, ny+1, nx+1] f64 (x fastest) -> the smoothed lattice; weights_xyz = (k of x, k of y, k of z)."""
    P = np.ascontiguousarray(points, dtype=np.float64)
    kx, ky, kz = weights_xyz
    P = smooth_axis(P, kx, 2)
    P = smooth_axis(P, ky, 1)
    return smooth_axis(P, kz, 0)


def same_bits(a, b):
    """Every element the same 64 bits, or a NaN in both."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))
