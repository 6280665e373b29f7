"""CPU restatement of dmi_filter_depth_speckles (include/dmi.h states the definition), vectorised numpy, written
from the definition and not from the kernels: plain f64 operations in the definition's order (numpy rounds every elementwise
operation and contracts nothing).  The labelling is a minimum-label union over the link list -- hook the larger of a link's two
labels to the smaller, then point every pixel at its label's label until nothing moves -- repeated until every link joins equal
labels: tiles, runs and borders do not occur in it.  Depths are [n, H, W] as the views hold them."""
import numpy as np


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


def linked(a, b, abs_tolerance, rel_tolerance):
    """Step 2 for arrays of neighbouring depths: the product, then the sum, then the difference, each rounded on its own."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        product = np.float64(rel_tolerance) * np.fmin(a, b)
        bound = np.float64(abs_tolerance) + product
        return valid_pixels(a) & valid_pixels(b) & (np.abs(a - b) <= bound)


def segment_labels(D, abs_tolerance, rel_tolerance):
    """One view [H, W] -> int64 [H, W]: the smallest index y * W + x of the pixel's segment, -1 at a pixel that is not valid."""
    H, W = D.shape
    index = np.arange(H * W, dtype=np.int64).reshape(H, W)
    right = linked(D[:, :-1], D[:, 1:], abs_tolerance, rel_tolerance)
    down = linked(D[:-1, :], D[1:, :], abs_tolerance, rel_tolerance)
    a = np.concatenate([index[:, :-1][right], index[:-1, :][down]])
    b = np.concatenate([index[:, 1:][right], index[1:, :][down]])
    label = index.reshape(-1).copy()
    while True:
        la, lb = label[a], label[b]
        if np.array_equal(la, lb):
            break
        np.minimum.at(label, np.maximum(la, lb), np.minimum(la, lb))
        while True:
            jumped = label[label]
            if np.array_equal(jumped, label):
                break
            label = jumped
    label = label.reshape(H, W)
    return np.where(valid_pixels(D), label, -1)


def filter_depth_speckles(depth, min_pixels, abs_tolerance=0.0, rel_tolerance=0.0, best_cost=None, threshold=None):
    """(out_depth [n, H, W] f64, size [n, H, W] int32) of the definition."""
    D = thresholded(depth, best_cost, threshold)
    size = np.zeros(D.shape, dtype=np.int32)
    for m in range(D.shape[0]):
        label = segment_labels(D[m], float(abs_tolerance), float(rel_tolerance))
        valid = label >= 0
        counts = np.bincount(label[valid], minlength=label.size)
        size[m][valid] = counts[label[valid]]
    out = np.where(valid_pixels(D) & (size >= int(min_pixels)), D, -1.0)
    return out, size
