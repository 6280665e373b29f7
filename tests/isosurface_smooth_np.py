"""CPU restatement of dmi_smooth_isosurface (include/dmi.h states the definition), vectorised numpy, written from
the definition and not from the kernels: the neighbour lists (and the triangle lists of the normals) are padded to the largest
valence and summed rank by rank, so every sum is added left to right in ascending id as the definition says.  numpy adds,
multiplies, divides and takes square roots in f64 one rounded operation at a time: no FMA."""
import numpy as np


def _padded_rows(row, value, n_rows):
    """(table [n_rows, widest] of `value` grouped by `row` in the given order, padded with 0; count [n_rows]).  `row` ascending."""
    count = np.bincount(row, minlength=n_rows).astype(np.int64) if n_rows else np.zeros(0, np.int64)
    widest = int(count.max()) if len(row) else 0
    start = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64) if n_rows else np.zeros(0, np.int64)
    table = np.zeros((n_rows, widest), dtype=np.int64)
    table[row, np.arange(len(row), dtype=np.int64) - start[row]] = value
    return table, count


def adjacency(n_vertices, tris):
    """(neighbours [V, widest] int64: N(v) in ascending id, padded; valence [V]; fixed [V] bool).  N(v): the distinct ids u != v
    that share a triangle with v.  fixed: the endpoints of the undirected edges {a, b}, a != b, that exactly one triangle names
    (a triangle naming an edge twice, (a, b, a), is one triangle)."""
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    a = np.concatenate([tris[:, 0], tris[:, 1], tris[:, 2]])
    b = np.concatenate([tris[:, 1], tris[:, 2], tris[:, 0]])
    t = np.tile(np.arange(len(tris), dtype=np.int64), 3)
    real = a != b
    lo, hi, t = np.minimum(a, b)[real], np.maximum(a, b)[real], t[real]
    per_triangle = np.unique(np.stack([lo, hi, t], -1), axis=0) if len(t) else np.zeros((0, 3), np.int64)
    edges, named_by = (np.unique(per_triangle[:, :2], axis=0, return_counts=True) if len(per_triangle)
                       else (np.zeros((0, 2), np.int64), np.zeros(0, np.int64)))
    fixed = np.zeros(n_vertices, dtype=bool)
    fixed[edges[named_by == 1].reshape(-1)] = True
    pairs = np.concatenate([edges, edges[:, ::-1]])
    pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]             # by vertex, then by ascending neighbour id
    nbr, valence = _padded_rows(pairs[:, 0], pairs[:, 1], n_vertices)
    return nbr, valence, fixed


def step(p, nbr, valence, moves, f):
    """One Jacobi step with factor f over positions p [V, 3]: a new array."""
    out = p.copy()
    if nbr.shape[1] == 0:
        return out
    s = p[nbr[:, 0]].copy()
    for r in range(1, nbr.shape[1]):
        more = valence > r
        s[more] = s[more] + p[nbr[more, r]]
    with np.errstate(all="ignore"):
        m = s[moves] / valence[moves].astype(np.float64)[:, None]
        out[moves] = p[moves] + f * (m - p[moves])
    return out


def geometric_normals(p, tris):
    """[V, 3] f32: per vertex the area-weighted cross products (p[b] - p[a]) x (p[c] - p[a]) of the triangles (a, b, c) that name
    it, added in ascending triangle index, normalised unless the length is 0, rounded to f32."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    n = len(p)
    a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
    with np.errstate(all="ignore"):
        e, g = p[b] - p[a], p[c] - p[a]
        x = np.stack([e[:, 1] * g[:, 2] - e[:, 2] * g[:, 1], e[:, 2] * g[:, 0] - e[:, 0] * g[:, 2],
                      e[:, 0] * g[:, 1] - e[:, 1] * g[:, 0]], -1)
        tid = np.arange(len(tris), dtype=np.int64)
        named = np.unique(np.stack([tris.reshape(-1), np.repeat(tid, 3)], -1), axis=0) if len(tris) else np.zeros((0, 2), np.int64)
        table, count = _padded_rows(named[:, 0], named[:, 1], n)     # a triangle naming a vertex twice is listed once
        w = np.zeros((n, 3))
        if table.shape[1]:
            has = count > 0
            w[has] = x[table[has, 0]]
            for r in range(1, table.shape[1]):
                more = count > r
                w[more] = w[more] + x[table[more, r]]
        length = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
        unit = length != 0                                          # a NaN length is included
        w[unit] = w[unit] / length[unit][:, None]
        return w.astype(np.float32)


def smooth(verts, tris, iterations, lam, mu, normals=None):
    """(vertices, normals or None) after `iterations` Taubin iterations: a step with lam, then, if mu != 0, one with mu."""
    p = np.array(verts, dtype=np.float64).reshape(-1, 3)
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    if iterations == 0:
        return p, normals
    nbr, valence, fixed = adjacency(len(p), tris)
    moves = ~fixed & (valence >= 1)
    for _ in range(iterations):
        p = step(p, nbr, valence, moves, lam)
        if mu != 0:
            p = step(p, nbr, valence, moves, mu)
    return p, (None if normals is None else geometric_normals(p, tris))
