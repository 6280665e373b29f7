"""CPU restatement of dmi_fill_isosurface_holes (include/dmi.h states the definition), numpy and plain loops,
written from the definition and not from the kernels: the boundary half-edges from a count of the undirected edges, the loops by
following next() from the smallest vertex of each, the centroid added left to right in walk order.  numpy adds and divides in
f64 one rounded operation at a time: no FMA."""
import numpy as np

import isosurface_smooth_np as S


def boundary(n_vertices, tris):
    """(half [B, 2] int64: the boundary half-edges start -> end, ascending in (min, max) of their ends; simple [V] bool;
    complex_ [V] bool; nxt [V] int64: next(a) of a simple vertex, -1 elsewhere).  Only triangles that name three distinct ids
    below V name half-edges; an undirected edge exactly one of them names is a boundary edge."""
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
    ok = (a != b) & (b != c) & (c != a) & (tris >= 0).all(1) & (tris < n_vertices).all(1)
    t = tris[ok]
    start = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    end = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    lo, hi = np.minimum(start, end), np.maximum(start, end)
    order = np.lexsort((hi, lo))
    start, end, lo, hi = start[order], end[order], lo[order], hi[order]
    first = np.ones(len(lo), dtype=bool)
    first[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    run = np.cumsum(first) - 1
    named_by = np.bincount(run) if len(run) else np.zeros(0, np.int64)
    single = named_by[run] == 1 if len(run) else np.zeros(0, bool)
    half = np.stack([start[single], end[single]], -1).astype(np.int64)
    out_deg = np.bincount(half[:, 0], minlength=n_vertices)
    in_deg = np.bincount(half[:, 1], minlength=n_vertices)
    simple = (out_deg == 1) & (in_deg == 1)
    complex_ = ((out_deg > 0) | (in_deg > 0)) & ~simple
    nxt = np.full(n_vertices, -1, dtype=np.int64)
    from_simple = simple[half[:, 0]]
    nxt[half[from_simple, 0]] = half[from_simple, 1]
    return half, simple, complex_, nxt


def loops(n_vertices, tris):
    """The loops, each an int64 array h_0 .. h_{L-1} in walk order with h_0 its smallest id, ordered by ascending h_0.  A chain
    that reaches a complex vertex is no loop."""
    _, simple, _, nxt = boundary(n_vertices, tris)
    seen = np.zeros(n_vertices, dtype=bool)
    found = []
    for v in np.flatnonzero(simple):
        if seen[v]:
            continue
        walk, cur, closed = [], int(v), False
        while simple[cur] and not seen[cur]:
            seen[cur] = True
            walk.append(cur)
            cur = int(nxt[cur])
            if cur == v:
                closed = True
                break
        # (v is the smallest unseen simple id: a walk that comes back to it has it as its smallest.  One that does not has met a
        # complex vertex, or a chain seen before, which had met one: a simple vertex has one half-edge in, so chains do not merge)
        if closed:
            found.append(np.array(walk, dtype=np.int64))
    return found


def fill(verts, tris, max_edges, normals=None):
    """dict(vertices, triangles, normals (None without), n_filled, boundary_edges_left, loop_sizes (all loops, in loop order),
    filled (the filled loops)) of the mesh after dmi_fill_isosurface_holes(max_edges)."""
    p = np.array(verts, dtype=np.float64).reshape(-1, 3)
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    n = len(p)
    half = boundary(n, tris)[0]
    all_loops = loops(n, tris)
    new_p, new_t, filled = [], [], []
    for h in all_loops:
        L = len(h)
        if not 3 <= L <= max_edges:
            continue
        filled.append(h)
        if L == 3:
            new_t.append([h[0], h[2], h[1]])
            continue
        with np.errstate(all="ignore"):
            s = p[h[0]].copy()
            for i in range(1, L):
                s = s + p[h[i]]
            c = s / np.float64(L)
        cid = n + len(new_p)
        new_p.append(c)
        for i in range(L):
            new_t.append([h[(i + 1) % L], h[i], cid])
    out_p = np.concatenate([p, np.array(new_p, dtype=np.float64).reshape(-1, 3)])
    out_t = np.concatenate([tris, np.array(new_t, dtype=np.int64).reshape(-1, 3)])
    out_n = None
    if normals is not None:
        normals = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
        # a new vertex is named by its L new triangles only, in ascending index: the geometric normals of those alone
        geometric = S.geometric_normals(out_p, out_t[len(tris):]) if len(new_p) else np.zeros((len(out_p), 3), np.float32)
        out_n = np.concatenate([normals, geometric[n:]])
    return {"vertices": out_p, "triangles": out_t, "normals": out_n, "n_filled": len(filled),
            "boundary_edges_left": len(half) - sum(len(h) for h in filled), "loop_sizes": [len(h) for h in all_loops],
            "filled": filled}
