"""CPU restatement of dmi_thin_point_cloud / dmi_views_thin_points (include/dmi.h states the definition), numpy,
written from the definition and not from the kernels: bins by one rounded subtraction and one rounded division, cells by a stable
argsort of the keys, every sum added member by member in ascending input index by a plain loop over the member ranks, the first
member starting it.  numpy adds, divides and takes square roots in f64 one correctly rounded operation at a time: no FMA.  Raises
ValueError where the ABI refuses."""
import numpy as np

MAX_BINS = 1 << 21
MAX_POINTS = (1 << 32) - 1
REPORT_NAMES = ("points_in", "cells", "cells_kept", "multi_view_cells", "largest_cell", "with_normal")
ARRAY_NAMES = ("xyz", "normal", "view", "pixel", "count", "members")


def check_parameters(cell_size, min_points, n_points=0):
    h = float(cell_size)
    if not (np.isfinite(h) and h > 0.0):
        raise ValueError("cell_size is not a finite number > 0")
    if int(min_points) < 1:
        raise ValueError("min_points >= 1 required")
    if n_points > MAX_POINTS:
        raise ValueError("P must stay below 2^32")


def min_cell_size(p):
    """The smallest cell size the definition accepts for positions p: the quotient of the longest extent, as rounded, stays
    below 2^21."""
    extent = float((p.max(axis=0) - p.min(axis=0)).max())
    least = extent / MAX_BINS
    while not np.floor(extent / least) < MAX_BINS:
        least = float(np.nextafter(least, np.inf))
    return least


def bins(p, cell_size):
    """(b [P, 3] int64, n [3] int) of positions p; ValueError for what step 1 refuses."""
    h = float(cell_size)
    if not np.isfinite(p).all():
        raise ValueError("the cloud has a non-finite coordinate")
    lo, hi = p.min(axis=0), p.max(axis=0)
    with np.errstate(all="ignore"):
        top = np.floor((hi - lo) / h)
        if not (top < MAX_BINS).all():
            raise ValueError(f"more than 2^21 bins on an axis; the smallest acceptable cell size for this cloud is {min_cell_size(p)!r}")
        b = np.floor((p - lo) / h).astype(np.int64)
    return b, [int(t) + 1 for t in top]


def keys(p, cell_size):
    b, n = bins(p, cell_size)
    return (b[:, 2] * n[1] + b[:, 1]) * n[0] + b[:, 0]           # < 2^63: python ints would agree


def _empty():
    arrays = dict(xyz=np.zeros((0, 3), np.float64), normal=np.zeros((0, 3), np.float32), view=np.zeros(0, np.int32),
                  pixel=np.zeros(0, np.int32), count=np.zeros(0, np.int32), members=np.zeros(0, np.uint32))
    return arrays, dict.fromkeys(REPORT_NAMES, 0)


def thin(xyz, normal=None, view=None, pixel=None, count=None, *, cell_size, min_points=1):
    """(arrays, report): the six output arrays in cell order and the report's counts."""
    p = np.array(xyz, dtype=np.float64).reshape(-1, 3)
    n_points = len(p)
    check_parameters(cell_size, min_points, n_points)
    if n_points == 0:
        return _empty()
    nrm = np.zeros((n_points, 3), np.float32) if normal is None else np.array(normal, dtype=np.float32).reshape(-1, 3)
    ints = [np.zeros(n_points, np.int32) if a is None else np.array(a, dtype=np.int32).reshape(-1) for a in (view, pixel, count)]
    view, pixel, count = ints
    key = keys(p, cell_size)
    order = np.argsort(key, kind="stable")                        # by cell, ascending input index within one
    sorted_key = key[order]
    head = np.concatenate([[True], sorted_key[1:] != sorted_key[:-1]])
    first = np.flatnonzero(head)
    size = np.diff(np.concatenate([first, [n_points]])).astype(np.int64)
    cells = len(first)
    s = p[order[first]].copy()                                    # the first member starts the sums: no 0.0 + x
    t = nrm[order[first]].astype(np.float64)
    most = count[order[first]].copy()
    for r in range(1, int(size.max())):                           # the r-th member of every cell that has one
        more = size > r
        member = order[first[more] + r]
        s[more] = s[more] + p[member]
        t[more] = t[more] + nrm[member].astype(np.float64)
        most[more] = np.maximum(most[more], count[member])
    out_xyz = s / size.astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        length = np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2])
        has = np.isfinite(length) & (length > 0.0)
        merged = np.zeros((cells, 3), np.float32)
        merged[has] = (t[has] / length[has][:, None]).astype(np.float32)
    single = size == 1
    merged[single] = nrm[order[first[single]]]
    last = first + size - 1
    keep = size >= int(min_points)
    arrays = dict(xyz=out_xyz[keep], normal=merged[keep], view=view[order[first]][keep], pixel=pixel[order[first]][keep],
                  count=most[keep].astype(np.int32), members=size[keep].astype(np.uint32))
    report = dict(points_in=n_points, cells=cells, cells_kept=int(keep.sum()),
                  multi_view_cells=int((view[order[first]] != view[order[last]])[keep].sum()), largest_cell=int(size.max()),
                  with_normal=int((arrays["normal"] != 0).any(axis=1).sum()))
    return arrays, report
