"""CPU restatement of dmi_smooth_depths (include/dmi.h states the definition), vectorised numpy, written from the
definition and not from the kernel: plain f64 operations in the definition's order (numpy rounds every elementwise operation and
contracts nothing).  One tap offset (dy, dx) at a time for all centres at once, dy outer and dx inner, so every centre meets its
taps in the definition's order; a tap that is not valid or lies outside the image is a NaN, for which `u < T` is false.  Tiles,
halos and runs do not occur in it.  Depths are [n, H, W] as the views hold them.  The spatial weights s[0..r] are an argument: the
tests pass the library's (capi.depth_smoothing_weights), so that nothing hangs on numpy's exp agreeing with libm's to the last ulp;
spatial_weights restates the rule itself."""
import math

import numpy as np

from depth_speckle_np import thresholded, valid_pixels

MAX_RADIUS = 8


def spatial_weights(sigma, truncate=2.0):
    """r = (int)ceil(truncate * sigma); s[0] = 1, s[i] = exp(-(double)(i*i) / (2*sigma*sigma)): not normalised."""
    r = int(math.ceil(truncate * sigma))
    return np.array([1.0] + [math.exp(-float(i * i) / (2 * sigma * sigma)) for i in range(1, r + 1)], dtype=np.float64)


def smooth_once(D, s, abs_tolerance, rel_tolerance):
    """One iteration on D [n, H, W] (invalid pixels in any form) -> (out f64 [n, H, W], count int32 [n, H, W])."""
    D = np.asarray(D, dtype=np.float64)
    s = np.asarray(s, dtype=np.float64)
    r = len(s) - 1
    n, H, W = D.shape
    valid = valid_pixels(D)
    C = np.where(valid, D, np.nan)
    padded = np.full((n, H + 2 * r, W + 2 * r), np.nan)
    padded[:, r:r + H, r:r + W] = C
    with np.errstate(all="ignore"):
        tau = np.float64(abs_tolerance) + np.float64(rel_tolerance) * C
        T = tau * tau
        num, den = np.zeros_like(C), np.zeros_like(C)
        count = np.zeros(C.shape, dtype=np.int32)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                q = padded[:, r + dy:r + dy + H, r + dx:r + dx + W]
                delta = q - C
                u = delta * delta
                take = u < T  # strict; false for a NaN
                g = T - u
                w = (s[abs(dy)] * s[abs(dx)]) * (g * g)
                num = np.where(take, num + w * delta, num)
                den = np.where(take, den + w, den)
                count += take
        out = C + num / den
        keep = (den > 0.0) & (den < np.inf) & (out > 0.0) & (out < np.inf)
        out = np.where(keep, out, C)
    return np.where(valid, out, -1.0), np.where(valid, count, 0).astype(np.int32)


def smooth_depths(depth, s, abs_tolerance=0.0, rel_tolerance=0.0, iterations=1, best_cost=None, threshold=None):
    """dmi_smooth_depths: the threshold once, then `iterations` passes, each on the complete output of the one before; the counts
    are the last pass's."""
    D = thresholded(depth, best_cost, threshold)
    count = None
    for _ in range(int(iterations)):
        D, count = smooth_once(D, s, abs_tolerance, rel_tolerance)
    return D, count
