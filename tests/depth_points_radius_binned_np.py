"""The radius neighbour count of include/dmi.h (dmi_count_point_neighbors, dmi_views_filter_points_radius) restated in
numpy for clouds of a million points, where depth_points_radius_np.py's all-pairs matrix is out of reach.  The counts are those of
the definition and of the brute force, bit for bit (tests/test_depth_points_radius_binned_np.py): only the set of pairs that are
tested is smaller.  It is written from the definition, not from the kernels: another cell size than the device's (1.25 radius, not
radius (1 + 2^-10)), another key (a ring of empty border cells, so the 27 neighbour keys are plain offsets), the pairs of a cell
with half its stencil counted for both ends, not every query against nine runs.

The pairs that are tested are a superset of the neighbour pairs.  Let i, j be neighbours: fl(fl(fl(d0 d0) + fl(d1 d1)) +
fl(d2 d2)) <= r2 with d = fl(x_i - x_j) and r2 = fl(radius radius).  Every term is >= 0 and rounding is monotone, so fl(a + b) >= a
for a representable a and b >= 0: fl(d_k d_k) <= r2 on every axis k.  A product that underflows belongs to |d_k| < 2^-537, below
any accepted radius (r2 is a normal number: radius >= 2^-511); otherwise d_k^2 <= r2 (1 + 2^-52) <= radius^2 (1 + 2^-52)^2, and
with the rounding of the subtraction |x_i - x_j| <= radius (1 + 2^-50) on every axis.  The cell of a coordinate is
floor(fl(fl(x - lo) / c)) with c >= 1.25 radius; both roundings are monotone and each is off by at most 2^-53 of its value, so the
two quotients, each below 2^40 (a wider axis is refused), differ by at most 0.8 (1 + 2^-50) + 2 * 2^40 * 2^-52 < 1 and their
floors by at most 1.  Neighbours therefore lie in the same cell or in cells adjacent on every axis: the 27 cells of the stencil.
An unordered pair of points in different cells is met exactly once, from the cell with the lower key (13 of the 26 offsets are
positive); a pair within one cell once, from its member of the lower sorted position.  The test of a pair is symmetric -- fl(a - b)
= -fl(b - a) and the squares do not see the sign -- so one evaluation counts for both ends.  A point never meets itself: the pairs
of a cell are taken over sorted positions i < j, which is by index."""
import numpy as np

CELL_FACTOR = 1.25          # cell side / radius; anything from 1 + 2^-40 on would do for the argument above
MAX_AXIS_CELLS = 1 << 40    # the argument's bound on a quotient
MAX_KEY = 1 << 62           # int64 keys, with room for the offsets
PAIRS = 1 << 21             # pairs tested at a time


def _pairs(lo, hi):
    """(owner, candidate) for every owner q and every candidate in [lo[q], hi[q])."""
    size = hi - lo
    total = int(size.sum())
    owner = np.repeat(np.arange(len(lo), dtype=np.int64), size)
    first = np.cumsum(size) - size                       # the first pair of every owner
    candidate = np.arange(total, dtype=np.int64) - np.repeat(first - lo, size)
    return owner, candidate


def count_neighbors(xyz, radius):
    """neighbors uint32 [P]: steps 1 to 4 of the definition.  ValueError where the ABI refuses, and for a cloud too wide for the
    keys of this restatement (which the ABI accepts)."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    if not np.isfinite(xyz).all():
        raise ValueError("non-finite coordinate")
    radius = np.float64(radius)
    with np.errstate(over="ignore", under="ignore"):
        r2 = radius * radius
    if not (radius > 0 and np.isfinite(r2) and r2 >= np.finfo(np.float64).tiny):
        raise ValueError("radius")
    p = len(xyz)
    out = np.zeros(p, dtype=np.int64)
    if p < 2:
        return out.astype(np.uint32)
    c = np.float64(CELL_FACTOR) * radius
    lo = xyz.min(axis=0)
    with np.errstate(over="ignore"):
        q = np.floor((xyz - lo) / c)
    if not (np.isfinite(q).all() and q.max() < MAX_AXIS_CELLS - 2):
        raise ValueError("the cloud is too wide for the binned restatement")
    b = q.astype(np.int64) + 1                           # one ring of empty cells round the grid
    n = [int(b[:, d].max()) + 2 for d in range(3)]
    if n[0] * n[1] * n[2] >= MAX_KEY:
        raise ValueError("the cloud is too wide for the binned restatement")
    key = (b[:, 2] * n[1] + b[:, 1]) * n[0] + b[:, 0]
    order = np.argsort(key, kind="stable")
    key = key[order]
    x0, x1, x2 = (np.ascontiguousarray(xyz[order, d]) for d in range(3))
    # offset 0 first (a cell with itself: the sorted positions behind each member, to the end of its cell), then the 13 positive
    # offsets of the 26
    offsets = [0] + sorted((e2 * n[1] + e1) * n[0] + e0 for e2 in (-1, 0, 1) for e1 in (-1, 0, 1) for e0 in (-1, 0, 1)
                           if (e2 * n[1] + e1) * n[0] + e0 > 0)
    assert len(offsets) == 14
    for offset in offsets:
        if offset == 0:
            first, last = np.arange(1, p + 1, dtype=np.int64), np.searchsorted(key, key, side="right")
        else:
            first, last = np.searchsorted(key, key + offset, side="left"), np.searchsorted(key, key + offset, side="right")
        ends = np.cumsum(last - first)
        at = 0
        while at < p:                                    # owners [at, to): about PAIRS pairs, at least one owner
            to = max(int(np.searchsorted(ends, (ends[at - 1] if at else 0) + PAIRS, side="right")), at + 1)
            i, j = _pairs(first[at:to], last[at:to])
            i += at
            with np.errstate(over="ignore", under="ignore"):
                d0 = x0[j] - x0[i]
                d1 = x1[j] - x1[i]
                d2 = x2[j] - x2[i]
                near = ((d0 * d0 + d1 * d1) + d2 * d2) <= r2
            out += np.bincount(i[near], minlength=p)
            out += np.bincount(j[near], minlength=p)
            at = to
    neighbors = np.zeros(p, dtype=np.uint32)
    neighbors[order] = out
    return neighbors
