"""CPU restatement of dmi_fill_depth_holes (include/dmi.h states the definition), vectorised numpy, written from the
definition and not from the kernels: plain f64 operations in the definition's order (numpy rounds every elementwise operation and
contracts nothing).  The labelling is depth_speckle_np's minimum-label union, over the pairs of neighbouring pixels that are both
NOT valid; the rim bounds are minima and maxima over the (hole pixel, valid neighbour) pairs; step 5 finds the nearest valid
column and row of every pixel by running maxima and minima of the valid pixels' coordinates.  Tiles, runs and borders do not occur
in it.  Depths are [n, H, W] as the views hold them."""
import numpy as np

from depth_speckle_np import thresholded, valid_pixels


def hole_labels(D):
    """One view [H, W] -> int64 [H, W]: the smallest index y * W + x of the pixel's hole, -1 at a valid pixel."""
    H, W = D.shape
    hole = ~valid_pixels(D)
    index = np.arange(H * W, dtype=np.int64).reshape(H, W)
    right = hole[:, :-1] & hole[:, 1:]
    down = hole[:-1, :] & hole[1:, :]
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
    return np.where(hole, label.reshape(H, W), -1)


def hole_records(D, label):
    """Steps 2 and 3 for one view: (size, touches_border, lo, hi), each indexed by a hole's label (arrays of H * W entries; lo is
    +inf and hi is -inf for a hole without a rim, which is the whole view)."""
    H, W = D.shape
    hole = label >= 0
    size = np.bincount(label[hole], minlength=H * W)
    edge = np.zeros((H, W), dtype=bool)
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
    touches = np.zeros(H * W, dtype=bool)
    touches[label[hole & edge]] = True
    lo, hi = np.full(H * W, np.inf), np.full(H * W, -np.inf)
    valid = ~hole
    # (hole pixel, valid 4-neighbour) pairs: the hole's side first
    for h_sel, v_sel in (((slice(None), slice(0, -1)), (slice(None), slice(1, None))), ((slice(None), slice(1, None)), (slice(None), slice(0, -1))),
                         ((slice(0, -1), slice(None)), (slice(1, None), slice(None))), ((slice(1, None), slice(None)), (slice(0, -1), slice(None)))):
        pair = hole[h_sel] & valid[v_sel]
        np.minimum.at(lo, label[h_sel][pair], D[v_sel][pair])
        np.maximum.at(hi, label[h_sel][pair], D[v_sel][pair])
    return size, touches, lo, hi


def fillable_holes(size, touches, lo, hi, max_pixels, abs_tolerance, rel_tolerance):
    """Step 4 per label: the product, then the sum, then the difference, each rounded on its own."""
    with np.errstate(all="ignore"):
        product = np.float64(rel_tolerance) * lo
        bound = np.float64(abs_tolerance) + product
        return (size > 0) & (size <= int(max_pixels)) & ~touches & (hi - lo <= bound)


def interpolated(D, ys, xs):
    """Step 5 for the pixels (ys, xs) of fillable holes of one view."""
    H, W = D.shape
    valid = valid_pixels(D)
    cols, rows = np.arange(W)[None, :], np.arange(H)[:, None]
    xl = np.maximum.accumulate(np.where(valid, cols, -1), axis=1)[ys, xs]
    xr = np.minimum.accumulate(np.where(valid, cols, W)[:, ::-1], axis=1)[:, ::-1][ys, xs]
    yu = np.maximum.accumulate(np.where(valid, rows, -1), axis=0)[ys, xs]
    yd = np.minimum.accumulate(np.where(valid, rows, H)[::-1, :], axis=0)[::-1, :][ys, xs]
    assert (xl >= 0).all() and (xr < W).all() and (yu >= 0).all() and (yd < H).all()      # the hole does not touch the border
    f = lambda a: a.astype(np.float64)                                                    # the integer spans, exactly
    with np.errstate(all="ignore"):
        h = (D[ys, xl] * f(xr - xs) + D[ys, xr] * f(xs - xl)) / f(xr - xl)
        v = (D[yu, xs] * f(yd - ys) + D[yd, xs] * f(ys - yu)) / f(yd - yu)
        return (h * f(yd - yu) + v * f(xr - xl)) / (f(yd - yu) + f(xr - xl))


def fill_depth_holes(depth, max_pixels, abs_tolerance=0.0, rel_tolerance=0.0, best_cost=None, threshold=None):
    """(out_depth [n, H, W] f64, size [n, H, W] int32) of the definition."""
    D = thresholded(depth, best_cost, threshold)
    out = np.where(valid_pixels(D), D, -1.0)
    size = np.zeros(D.shape, dtype=np.int32)
    for m in range(D.shape[0]):
        label = hole_labels(D[m])
        hole = label >= 0
        sizes, touches, lo, hi = hole_records(D[m], label)
        size[m][hole] = sizes[label[hole]]
        fillable = fillable_holes(sizes, touches, lo, hi, max_pixels, float(abs_tolerance), float(rel_tolerance))
        ys, xs = np.nonzero(hole & fillable[np.where(hole, label, 0)])
        if len(ys):
            out[m][ys, xs] = interpolated(D[m], ys, xs)
    return out, size


def hole_counts(depth, out_depth, size):
    """(holes, holes filled, pixels filled) over all views, as the command line's summary counts them."""
    holes = filled = pixels = 0
    for m in range(depth.shape[0]):
        label = hole_labels(np.asarray(depth[m], dtype=np.float64))
        roots = np.unique(label[label >= 0])
        holes += len(roots)
        got = out_depth[m].reshape(-1)[roots] != -1.0
        filled += int(got.sum())
        pixels += int(size[m].reshape(-1)[roots][got].sum())
    return holes, filled, pixels
