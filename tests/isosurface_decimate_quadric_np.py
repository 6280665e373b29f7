"""CPU restatement of dmi_decimate_isosurface_placed with DMI_DECIMATE_QUADRIC (include/dmi.h states the
definition), numpy, written from the definition and not from the kernels.  Bins, clusters, means and triangles are
isosurface_decimate_np's; only the representatives differ: per cluster the plane quadrics of its corners about the mean, added
corner by corner in ascending corner index by a plain loop over the corner ranks (as representatives() adds the members), the
regularised 3x3 system solved by cofactors as the definition writes them (nothing from np.linalg), the result clamped to the
cluster's cell.  numpy multiplies, adds and divides in f64 one rounded operation at a time: no FMA.  Raises ValueError where the
ABI refuses."""
import numpy as np

import isosurface_decimate_np as D
import isosurface_smooth_np as S

MEAN, QUADRIC = 0, 1                                                          # DMI_DECIMATE_MEAN, DMI_DECIMATE_QUADRIC


def corner_sums(p, tris, cluster, count, mean):
    """(A [count, 6], g [count, 3], corners [count]): per cluster the sums of its corners' (n0n0, n0n1, n0n2, n1n1, n1n2, n2n2)
    and (n0 d, n1 d, n2 d), left to right in ascending corner index 3t + e, and how many corners it has (zeros where none)."""
    nv = len(p)
    named = np.flatnonzero(((tris >= 0) & (tris < nv)).all(axis=1))           # only these triangles have corners
    a, b, c = (p[tris[named, e]] for e in range(3))
    u, v = b - a, c - a
    n = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
    # corner 3t + e, ascending: (t, e) row-major
    owner = cluster[tris[named]].reshape(-1)                                  # the cluster of vertex tris[t][e]
    n = np.repeat(n, 3, axis=0)
    q = np.repeat(a, 3, axis=0) - mean[owner]
    d = -((n[:, 0] * q[:, 0] + n[:, 1] * q[:, 1]) + n[:, 2] * q[:, 2])
    term = np.stack([n[:, 0] * n[:, 0], n[:, 0] * n[:, 1], n[:, 0] * n[:, 2], n[:, 1] * n[:, 1], n[:, 1] * n[:, 2], n[:, 2] * n[:, 2],
                     n[:, 0] * d, n[:, 1] * d, n[:, 2] * d], axis=1)
    order = np.argsort(owner, kind="stable")                                  # by cluster, ascending corner index within one
    size = np.bincount(owner, minlength=count).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int64)
    s = np.zeros((count, 9))
    has = size > 0
    s[has] = term[order[first[has]]]                                          # the first contribution starts the sum
    for r in range(1, int(size.max()) if count else 0):                       # the r-th corner of every cluster that has one
        more = size > r
        s[more] = s[more] + term[order[first[more] + r]]
    return s[:, :6], s[:, 6:], size


def solve(A, g):
    """(x [count, 3], ok [count]): x_r = -(((c_r0 g0 + c_r1 g1) + c_r2 g2) / det) of M = A + 2^-10 tr I by its cofactors; ok
    where tr and det are finite numbers > 0."""
    with np.errstate(all="ignore"):
        tr = (A[:, 0] + A[:, 3]) + A[:, 5]
        mu = 0.0009765625 * tr
        m00, m01, m02, m11, m12, m22 = A[:, 0] + mu, A[:, 1], A[:, 2], A[:, 3] + mu, A[:, 4], A[:, 5] + mu
        c00 = m11 * m22 - m12 * m12
        c01 = m02 * m12 - m01 * m22
        c02 = m01 * m12 - m02 * m11
        c11 = m00 * m22 - m02 * m02
        c12 = m01 * m02 - m00 * m12
        c22 = m00 * m11 - m01 * m01
        det = (m00 * c00 + m01 * c01) + m02 * c02
        x = np.stack([-(((c00 * g[:, 0] + c01 * g[:, 1]) + c02 * g[:, 2]) / det),
                      -(((c01 * g[:, 0] + c11 * g[:, 1]) + c12 * g[:, 2]) / det),
                      -(((c02 * g[:, 0] + c12 * g[:, 1]) + c22 * g[:, 2]) / det)], axis=1)
        ok = np.isfinite(tr) & (tr > 0.0) & np.isfinite(det) & (det > 0.0)
    return x, ok


def cells(p, cluster, count, cell_size):
    """(L [count, 3], U [count, 3]): every cluster's cell, lo_d + (double)b_d h and lo_d + (double)(b_d + 1) h."""
    b, _ = D.bins(p, cell_size)
    of = np.zeros((count, 3), np.int64)
    of[cluster] = b                                                           # (all members of a cluster have the same bins)
    lo, h = p.min(axis=0), float(cell_size)
    return lo + of.astype(np.float64) * h, lo + (of + 1).astype(np.float64) * h


def representatives(p, tris, cluster, count, cell_size, details=None):
    """[count, 3] f64: every cluster's quadric representative.  `details`, a dict, receives the mean, the unclamped y, the cells
    and which clusters were solved and which clamped."""
    mean = D.representatives(p, cluster, count)
    A, g, corners = corner_sums(p, tris, cluster, count, mean)
    x, ok = solve(A, g)
    L, U = cells(p, cluster, count, cell_size)
    with np.errstate(all="ignore"):
        y = mean + x
        ok = ok & (corners > 0) & ~np.isnan(y).any(axis=1)
        z = np.where(y < L, L, y)
        z = np.where(z > U, U, z)
    out = np.where(ok[:, None], z, mean)
    if details is not None:
        details.update(mean=mean, y=y, lower=L, upper=U, solved=ok, clamped=ok & (z != y).any(axis=1), corners=corners)
    return out


def decimate(verts, tris, cell_size, normals=None, placement=QUADRIC, details=None):
    """(vertices [V', 3] f64, triangles [T', 3] int64, normals [V', 3] f32 or None) of the decimated mesh."""
    if placement not in (MEAN, QUADRIC):
        raise ValueError(f"dmi_decimate_isosurface_placed: placement {placement} is neither DMI_DECIMATE_MEAN nor DMI_DECIMATE_QUADRIC")
    if placement == QUADRIC and 3 * (np.size(tris) // 3) >= 1 << 32:
        raise ValueError("dmi_decimate_isosurface_placed: mesh too large for 32-bit corner indices (3 T >= 2^32)")
    if placement == MEAN:
        return D.decimate(verts, tris, cell_size, normals)
    mean_v, out_t, _ = D.decimate(verts, tris, cell_size, None)              # refuses what the call refuses
    if len(mean_v) == 0:                                                      # nothing to place
        return D.decimate(verts, tris, cell_size, normals)
    p = np.array(verts, dtype=np.float64).reshape(-1, 3)
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    cluster, count = D.clusters(p, cell_size)
    # the output's clusters: those a surviving triangle names, i.e. those any non-degenerate triangle names (the duplicates of a
    # survivor name the survivor's clusters)
    named = ((tris >= 0) & (tris < len(p))).all(axis=1)
    new = cluster[tris[named]]
    proper = (new[:, 0] != new[:, 1]) & (new[:, 1] != new[:, 2]) & (new[:, 2] != new[:, 0])
    used = np.zeros(count, dtype=bool)
    used[new[proper].reshape(-1)] = True
    inner = {}
    reps = representatives(p, tris, cluster, count, cell_size, inner)
    assert used.sum() == len(mean_v) and inner["mean"][used].tobytes() == mean_v.tobytes()
    if details is not None:
        details.update({k: v[used] for k, v in inner.items()})
    out_v = reps[used]
    return out_v, out_t, (None if normals is None else S.geometric_normals(out_v, out_t))
