"""CPU restatement of dmi_filter_isosurface_components (include/dmi.h states the definition), vectorised numpy,
written from the definition and not from the kernels: a Shiloach-Vishkin style hooking of flat trees for the labels, bincount for
the sizes, cumulative sums for the renumbering."""
import numpy as np

MIN_TRIANGLES, LARGEST = "min_triangles", "largest"


def labels(n_vertices, tris):
    """label[v] = the smallest vertex id of v's connected component (connectivity by id, through the triangles)."""
    parent = np.arange(n_vertices, dtype=np.int64)
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    if len(tris) == 0:
        return parent
    a = np.concatenate([tris[:, 0], tris[:, 0]])
    b = np.concatenate([tris[:, 1], tris[:, 2]])
    while True:
        while True:                      # flatten: every vertex points at its tree's root
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
        ra, rb = parent[a], parent[b]
        cross = ra != rb
        if not cross.any():
            return parent                # parents are never larger than their children: a root is its tree's smallest id
        hi, lo = np.maximum(ra, rb)[cross], np.minimum(ra, rb)[cross]
        parent[hi] = lo                  # any smaller root of the same component will do (the last one written stays)
        a, b = a[cross], b[cross]        # an edge inside one tree stays inside it


def components(n_vertices, tris):
    """(label [V], size [V]: size[l] = triangles of the component labelled l, 0 elsewhere)."""
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    lab = labels(n_vertices, tris)
    size = np.bincount(lab[tris[:, 0]], minlength=n_vertices).astype(np.int64) if n_vertices else np.zeros(0, np.int64)
    return lab, size


def filter_mesh(verts, tris, normals=None, mode=MIN_TRIANGLES, min_triangles=0):
    """The filtered mesh as a dict: vertices, triangles, normals (or None), region_id [V'], region_size [kept],
    counts = (V', T', components found, components kept)."""
    verts = np.asarray(verts).reshape(-1, 3)
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    nv = len(verts)
    lab, size = components(nv, tris)
    ids = np.arange(nv, dtype=np.int64)
    is_root = lab == ids
    if mode == MIN_TRIANGLES:
        keep_root = is_root & (size >= min_triangles)
    elif mode == LARGEST:
        keep_root = np.zeros(nv, dtype=bool)
        roots = ids[is_root]
        if len(roots):
            keep_root[roots[np.argmax(size[roots])]] = True      # the first maximum: the smallest label among ties
    else:
        raise ValueError(mode)
    keep_v = keep_root[lab]
    keep_t = keep_v[tris[:, 0]]
    vmap = np.cumsum(keep_v) - keep_v
    rmap = np.cumsum(keep_root) - keep_root
    out = {
        "vertices": verts[keep_v],
        "triangles": vmap[tris[keep_t]].astype(np.int64).reshape(-1, 3),
        "normals": None if normals is None else np.asarray(normals).reshape(-1, 3)[keep_v],
        "region_id": rmap[lab[keep_v]].astype(np.int64),
        "region_size": size[keep_root],
    }
    out["counts"] = (int(keep_v.sum()), int(keep_t.sum()), int(is_root.sum()), int(keep_root.sum()))
    return out
