"""CPU restatement of dmi_extract_isosurface, vectorised numpy, written from the definition and not from the
kernel: crossed-edge masks, a cumulative sum for the vertex ids, the generated case table for the triangles."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_table_module():
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(ROOT, "tools", "gen_mc_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = load_table_module()
EDGE_AXIS = np.array([d for d, _ in T.EDGES], dtype=np.int64)
EDGE_OFF = np.array([off for _, off in T.EDGES], dtype=np.int64)          # (x, y, z) of the edge's lower corner
TRI_COUNT = np.array(T.TRI_COUNT, dtype=np.int64)
TRI_EDGES = np.zeros((256, T.MAX_TRIS, 3), dtype=np.int64)
for _c in range(256):
    for _t, _tri in enumerate(T.TRIS[_c]):
        TRI_EDGES[_c, _t] = _tri


def crossed_masks(P, iso):
    """[nz+1, ny+1, nx+1, 3] bool: the lattice edge owned by each point along x, y, z is crossed."""
    inside = P >= iso                       # a NaN compares False: outside
    m = np.zeros(P.shape + (3,), dtype=bool)
    m[:, :, :-1, 0] = inside[:, :, :-1] != inside[:, :, 1:]
    m[:, :-1, :, 1] = inside[:, :-1, :] != inside[:, 1:, :]
    m[:-1, :, :, 2] = inside[:-1, :, :] != inside[1:, :, :]
    return inside, m


def cell_cases(inside):
    """[nz, ny, nx] case index of every cell, corner c = x + 2y + 4z."""
    case = np.zeros(tuple(s - 1 for s in inside.shape), dtype=np.uint8)
    for c in range(8):
        x, y, z = c & 1, (c >> 1) & 1, c >> 2
        case |= inside[z:z + case.shape[0], y:y + case.shape[1], x:x + case.shape[2]].astype(np.uint8) << np.uint8(c)
    return case


def vertex_positions(P, iso, pts, axis, origin, spacing, matrix):
    """World positions of the vertices on the edges owned by lattice points pts [n, 3] (k, j, i) along `axis` [n]."""
    k, j, i = pts[:, 0], pts[:, 1], pts[:, 2]
    step = np.stack([(axis == 2), (axis == 1), (axis == 0)], -1).astype(np.int64)
    kb, jb, ib = k + step[:, 0], j + step[:, 1], i + step[:, 2]
    va, vb = P[k, j, i], P[kb, jb, ib]
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (iso - va) / (vb - va)
    nan = np.isnan(va) | np.isnan(vb)
    t = np.where(nan, np.where(va >= iso, 0.0, 1.0), t)
    idx_a = np.stack([i, j, k], -1).astype(np.float64)
    idx_b = np.stack([ib, jb, kb], -1).astype(np.float64)
    origin = np.asarray(origin, dtype=np.float64)
    spacing = np.asarray(spacing, dtype=np.float64)
    ca = origin + idx_a * spacing
    cb = origin + idx_b * spacing
    x = ca.copy()
    rows = np.arange(len(axis))
    x[rows, axis] = ca[rows, axis] + t * (cb[rows, axis] - ca[rows, axis])
    M = np.asarray(matrix, dtype=np.float64).reshape(4, 4)
    w = np.empty_like(x)
    for r in range(3):
        w[:, r] = M[r, 0] * x[:, 0] + M[r, 1] * x[:, 1] + M[r, 2] * x[:, 2] + M[r, 3]
    return w


def extract(P, iso, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), matrix=None):
    """(vertices [n, 3] f64, triangles [m, 3] int64) of the point lattice P [nz+1, ny+1, nx+1] at `iso`."""
    P = np.ascontiguousarray(P, dtype=np.float64)
    if matrix is None:
        matrix = np.eye(4)
    inside, m = crossed_masks(P, iso)
    flat = m.reshape(-1)
    vid = (np.cumsum(flat, dtype=np.int64) - 1).reshape(m.shape)
    where = np.nonzero(flat)[0]
    pid, axis = where // 3, where % 3
    pts = np.stack(np.unravel_index(pid, P.shape), -1)
    verts = vertex_positions(P, iso, pts, axis, origin, spacing, matrix)
    tris = cell_triangles(inside, vid)
    return verts, tris


def cell_triangles(inside, vid, cells=None):
    """Triangles of the cells (all, or the linear ids `cells`, ascending) from the vertex id lattice vid [.., 3]."""
    case = cell_cases(inside)
    nz, ny, nx = case.shape
    if cells is None:
        cells = np.arange(case.size, dtype=np.int64)
    cells = np.asarray(cells, dtype=np.int64)
    cc = case.reshape(-1)[cells]
    keep = TRI_COUNT[cc] > 0
    cells, cc = cells[keep], cc[keep]
    k, rem = np.divmod(cells, nx * ny)
    j, i = np.divmod(rem, nx)
    e = TRI_EDGES[cc]                                   # [n, 5, 3]
    ids = vid[k[:, None, None] + EDGE_OFF[e, 2], j[:, None, None] + EDGE_OFF[e, 1], i[:, None, None] + EDGE_OFF[e, 0], EDGE_AXIS[e]]
    valid = np.arange(T.MAX_TRIS)[None, :] < TRI_COUNT[cc][:, None]
    return ids[valid].reshape(-1, 3).astype(np.int64)


def counts(P, iso):
    """(vertices, triangles) of the mesh, without building it."""
    inside, m = crossed_masks(np.asarray(P, dtype=np.float64), iso)
    return int(m.sum()), int(np.bincount(cell_cases(inside).reshape(-1), minlength=256) @ TRI_COUNT)


def emitting_cells(P, iso):
    inside, _ = crossed_masks(np.asarray(P, dtype=np.float64), iso)
    return np.nonzero(TRI_COUNT[cell_cases(inside).reshape(-1)] > 0)[0].astype(np.int64)


def sampled_cells(P, iso, cells, origin, spacing, matrix):
    """For the ascending cell ids `cells`: their triangles' global vertex ids and the positions of those vertices, without
    a global per-edge id array (the vertex id of an edge = crossed edges owned by earlier points + lower axes)."""
    P = np.asarray(P, dtype=np.float64)
    inside, m = crossed_masks(P, iso)
    per_point = m.sum(-1, dtype=np.uint8)
    row_base = np.concatenate([[0], np.cumsum(per_point.sum(-1, dtype=np.int64).reshape(-1))])
    nz, ny, nx = (s - 1 for s in P.shape)
    cells = np.asarray(cells, dtype=np.int64)
    k, rem = np.divmod(cells, nx * ny)
    j, i = np.divmod(rem, nx)
    # vid of every edge of the 2x2 rows around each sampled cell, from that row's prefix
    vid = {}
    out_tris = []
    case = np.zeros(len(cells), dtype=np.int64)
    for c in range(8):
        case |= inside[k + (c >> 2), j + ((c >> 1) & 1), i + (c & 1)].astype(np.int64) << c
    for n in range(len(cells)):
        cc = case[n]
        for t in range(TRI_COUNT[cc]):
            tri = []
            for e in TRI_EDGES[cc, t]:
                kk, jj, ii, d = k[n] + EDGE_OFF[e, 2], j[n] + EDGE_OFF[e, 1], i[n] + EDGE_OFF[e, 0], EDGE_AXIS[e]
                row = kk * (ny + 1) + jj
                before = int(per_point[kk, jj, :ii].sum(dtype=np.int64))
                v = int(row_base[row]) + before + int(m[kk, jj, ii, :d].sum())
                vid[v] = (kk, jj, ii, d)
                tri.append(v)
            out_tris.append(tri)
    tris = np.array(out_tris, dtype=np.int64).reshape(-1, 3)
    ids = np.array(sorted(vid), dtype=np.int64)
    pts = np.array([vid[v][:3] for v in ids], dtype=np.int64).reshape(-1, 3)
    axis = np.array([vid[v][3] for v in ids], dtype=np.int64)
    verts = vertex_positions(P, iso, pts, axis, origin, spacing, matrix) if len(ids) else np.zeros((0, 3))
    return tris, ids, verts
