"""CPU restatement of dmi_decimate_isosurface (include/dmi.h states the definition), numpy, written from the
definition and not from the kernels: bins by one rounded subtraction and one rounded division, clusters by np.unique over the
(b_2, b_1, b_0) triples, every representative's sum added member by member in ascending old id by a plain loop over the member
ranks, duplicates by the sorted triple with the first occurrence kept.  numpy adds and divides in f64 one rounded operation at a
time: no FMA.  Raises ValueError where the ABI refuses."""
import numpy as np

import isosurface_smooth_np as S

MAX_BINS = 1 << 21


def bins(p, cell_size):
    """(b [V, 3] int64, n [3] int) of positions p for the cell size; ValueError for what the call refuses."""
    h = float(cell_size)
    if not (np.isfinite(h) and h > 0.0):
        raise ValueError("dmi_decimate_isosurface: cell_size is not a finite number > 0")
    if not np.isfinite(p).all():
        raise ValueError("dmi_decimate_isosurface: the mesh has a non-finite vertex coordinate")
    lo, hi = p.min(axis=0), p.max(axis=0)
    with np.errstate(all="ignore"):
        top = np.floor((hi - lo) / h)
        if not (top < MAX_BINS).all():
            raise ValueError(f"dmi_decimate_isosurface: more than 2^21 bins on an axis; the smallest acceptable cell size for this "
                             f"mesh is {min_cell_size(p)!r}")
        b = np.floor((p - lo) / h).astype(np.int64)
    return b, [int(t) + 1 for t in top]


def min_cell_size(p):
    """The smallest cell size the definition accepts for positions p: the quotient of the longest extent, as rounded, stays
    below 2^21."""
    extent = float((p.max(axis=0) - p.min(axis=0)).max())
    least = extent / MAX_BINS
    while not np.floor(extent / least) < MAX_BINS:
        least = float(np.nextafter(least, np.inf))
    return least


def clusters(p, cell_size):
    """(cluster [V] int64: each vertex's cluster, numbered by ascending (b_2, b_1, b_0); count: how many there are)."""
    b, _ = bins(p, cell_size)
    if len(b) == 0:
        return np.zeros(0, np.int64), 0
    triples, cluster = np.unique(b[:, ::-1], axis=0, return_inverse=True)      # rows compared from b_2 down to b_0
    return cluster.reshape(-1).astype(np.int64), len(triples)


def representatives(p, cluster, count):
    """[count, 3] f64: per cluster the members' positions added left to right in ascending old id, divided by their number."""
    order = np.argsort(cluster, kind="stable")                                # by cluster, ascending id within one
    size = np.bincount(cluster, minlength=count).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int64)
    s = p[order[first]].copy()
    for r in range(1, int(size.max()) if count else 0):                       # the r-th member of every cluster that has one
        more = size > r
        s[more] = s[more] + p[order[first[more] + r]]
    return s / size.astype(np.float64)[:, None]


def decimate(verts, tris, cell_size, normals=None):
    """(vertices [V', 3] f64, triangles [T', 3] int64, normals [V', 3] f32 or None) of the decimated mesh."""
    p = np.array(verts, dtype=np.float64).reshape(-1, 3)
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    nv = len(p)
    if nv == 0:                                                               # an empty mesh stays empty (its cell size is checked)
        bins(np.zeros((1, 3)), cell_size)
        return p, np.zeros((0, 3), np.int64), normals
    cluster, count = clusters(p, cell_size)
    named = ((tris >= 0) & (tris < nv)).all(axis=1)                           # a triangle naming an id >= V is dropped
    new = np.zeros_like(tris)
    new[named] = cluster[tris[named]]
    keep = named & (new[:, 0] != new[:, 1]) & (new[:, 1] != new[:, 2]) & (new[:, 2] != new[:, 0])
    index = np.flatnonzero(keep)
    if len(index):                                                           # of each set of three ids the lowest index stays
        _, first = np.unique(np.sort(new[index], axis=1), axis=0, return_index=True)
        keep = np.zeros(len(tris), dtype=bool)
        keep[index[first]] = True
    used = np.zeros(count, dtype=bool)
    used[new[keep].reshape(-1)] = True
    number = np.cumsum(used) - used                                           # the referenced clusters, in cluster order
    out_v = representatives(p, cluster, count)[used]
    out_t = number[new[keep]].astype(np.int64).reshape(-1, 3)
    return out_v, out_t, (None if normals is None else S.geometric_normals(out_v, out_t))
