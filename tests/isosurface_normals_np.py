"""CPU restatement of the normals of dmi_extract_isosurface_normals, vectorised numpy, written from the
definition and not from the kernel: minus the lattice gradient (one-sided at the borders, central inside) at both ends of a
vertex's edge, interpolated at the vertex's t, through the cofactor matrix of the grid matrix, normalised, rounded to f32.
Vertices and triangles are tests/isosurface_np.py's."""
import numpy as np

import isosurface_np as R


def normal_matrix(matrix):
    """Nm [3, 3] f64: the cofactors C of the grid matrix's upper-left 3 x 3 A (indices mod 3), negated when det A < 0."""
    A = np.asarray(matrix, dtype=np.float64).reshape(4, 4)[:3, :3]
    C = np.empty((3, 3))
    for r in range(3):
        for c in range(3):
            C[r, c] = A[(r + 1) % 3, (c + 1) % 3] * A[(r + 2) % 3, (c + 2) % 3] - A[(r + 1) % 3, (c + 2) % 3] * A[(r + 2) % 3, (c + 1) % 3]
    det = A[0, 0] * C[0, 0] + A[0, 1] * C[0, 1] + A[0, 2] * C[0, 2]
    return -C if det < 0 else C


def neg_gradient(P, pts, spacing):
    """G [n, 3] f64 (x, y, z) at the lattice points pts [n, 3] (k, j, i) of P [nz+1, ny+1, nx+1]."""
    pts = np.asarray(pts, dtype=np.int64).reshape(-1, 3)
    k, j, i = pts[:, 0], pts[:, 1], pts[:, 2]
    n_cells = (P.shape[2] - 1, P.shape[1] - 1, P.shape[0] - 1)
    c = P[k, j, i]
    G = np.zeros((len(pts), 3))
    for e in range(3):
        N, h = n_cells[e], float(spacing[e])
        if N == 0:
            continue                                # G_e = 0 (no context has such an axis: cell_dims >= 1)
        idx = [i, j, k]
        q = idx[e]

        def at(off):
            moved = list(idx)
            moved[e] = np.clip(q + off, 0, N)
            return P[moved[2], moved[1], moved[0]]
        below, above = at(-1), at(1)
        with np.errstate(invalid="ignore", over="ignore"):
            G[:, e] = np.where(q == 0, (c - above) / h, np.where(q == N, (below - c) / h, (0.5 * (below - above)) / h))
    return G


def vertex_normals(P, iso, pts, axis, spacing, matrix):
    """[n, 3] f32 normals of the vertices on the edges owned by lattice points pts [n, 3] (k, j, i) along `axis` [n]."""
    P = np.asarray(P, dtype=np.float64)
    pts = np.asarray(pts, dtype=np.int64).reshape(-1, 3)
    axis = np.asarray(axis, dtype=np.int64)
    step = np.stack([(axis == 2), (axis == 1), (axis == 0)], -1).astype(np.int64)
    pb = pts + step
    va, vb = P[pts[:, 0], pts[:, 1], pts[:, 2]], P[pb[:, 0], pb[:, 1], pb[:, 2]]
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (iso - va) / (vb - va)
    t = np.where(np.isnan(va) | np.isnan(vb), np.where(va >= iso, 0.0, 1.0), t)
    Ga, Gb = neg_gradient(P, pts, spacing), neg_gradient(P, pb, spacing)
    Nm = normal_matrix(matrix)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g = Ga + t[:, None] * (Gb - Ga)
        w = np.empty_like(g)
        for r in range(3):
            w[:, r] = Nm[r, 0] * g[:, 0] + Nm[r, 1] * g[:, 1] + Nm[r, 2] * g[:, 2]
        L = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
        n = np.where((L != 0)[:, None], w / L[:, None], w)   # a NaN L divides too
    return n.astype(np.float32)


def vertex_edges(P, iso):
    """(pts [n, 3] (k, j, i), axis [n]) of every vertex, in vertex id order."""
    _, m = R.crossed_masks(np.asarray(P, dtype=np.float64), iso)
    where = np.nonzero(m.reshape(-1))[0]
    return np.stack(np.unravel_index(where // 3, m.shape[:3]), -1), where % 3


def extract_with_normals(P, iso, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), matrix=None):
    """(vertices [n, 3] f64, triangles [m, 3] int64, normals [n, 3] f32) of the point lattice P at `iso`."""
    P = np.ascontiguousarray(P, dtype=np.float64)
    if matrix is None:
        matrix = np.eye(4)
    verts, tris = R.extract(P, iso, origin, spacing, matrix)
    pts, axis = vertex_edges(P, iso)
    return verts, tris, vertex_normals(P, iso, pts, axis, spacing, matrix)


def edges_of_vertex_ids(P, iso, ids):
    """(pts [n, 3] (k, j, i), axis [n]) of the global vertex ids `ids`, without a global per-edge id array: a row's first id
    from the per-row counts, then the point within the row and the axis within the point (as sampled_cells numbers them)."""
    P = np.asarray(P, dtype=np.float64)
    _, m = R.crossed_masks(P, iso)
    per_point = m.sum(-1, dtype=np.uint8)
    row_base = np.concatenate([[0], np.cumsum(per_point.sum(-1, dtype=np.int64).reshape(-1))])
    ny1 = P.shape[1]
    ids = np.asarray(ids, dtype=np.int64)
    pts = np.empty((len(ids), 3), dtype=np.int64)
    axis = np.empty(len(ids), dtype=np.int64)
    rows = np.searchsorted(row_base, ids, side="right") - 1
    for n, (v, row) in enumerate(zip(ids, rows)):
        k, j = divmod(int(row), ny1)
        within = int(v - row_base[row])
        cum = np.cumsum(per_point[k, j], dtype=np.int64)
        i = int(np.searchsorted(cum, within, side="right"))
        r = within - int(cum[i] - per_point[k, j, i])
        axis[n] = np.nonzero(m[k, j, i])[0][r]
        pts[n] = (k, j, i)
    return pts, axis


def sampled_normals(P, iso, ids, spacing, matrix):
    """[len(ids), 3] f32 normals of the vertices with the global ids `ids` (e.g. those sampled_cells returns)."""
    pts, axis = edges_of_vertex_ids(P, iso, ids)
    if len(ids) == 0:
        return np.zeros((0, 3), dtype=np.float32)
    return vertex_normals(P, iso, pts, axis, spacing, matrix)
