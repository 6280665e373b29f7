"""Numpy restatement of the rendered depth planes (include/dmi.h: dmi_color_render_depths; DESIGN.md 8b''): a triangle mesh
rasterised into one z-buffer per view, in plain f64 operations in the definition's order (numpy rounds every elementwise operation
and contracts nothing; its division is correctly rounded).  Small triangles are taken all at once, one pixel offset of their
ranges at a time; large ones one by one over their whole range.  The plane is a minimum, so none of that order matters."""
import numpy as np


def project(points, K4, RT4):
    """(u, v, cz, ok) of every vertex in one view: TransformPoint by [R|T] left to right, the 3x3 K without translation, two
    divisions; ok iff cz > 0, dz > 0 and u, v finite."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    R = np.asarray(RT4, dtype=np.float64).reshape(4, 4)
    K = np.asarray(K4, dtype=np.float64).reshape(4, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    c = [((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z) + R[r, 3] for r in range(3)]
    d = [(K[r, 0] * c[0] + K[r, 1] * c[1]) + K[r, 2] * c[2] for r in range(3)]
    with np.errstate(all="ignore"):
        u, v = d[0] / d[2], d[1] / d[2]
        ok = (c[2] > 0.0) & (d[2] > 0.0) & np.isfinite(u) & np.isfinite(v)
    return u, v, c[2], ok


def pixel_ranges(u, v, W, H):
    """(x0, x1, y0, y1) as f64 of triangles with vertex coordinates u, v [t, 3]: [max(0, ceil(min)), min(W-1, floor(max))]."""
    x0 = np.maximum(0.0, np.ceil(u.min(axis=1)))
    x1 = np.minimum(float(W - 1), np.floor(u.max(axis=1)))
    y0 = np.maximum(0.0, np.ceil(v.min(axis=1)))
    y1 = np.minimum(float(H - 1), np.floor(v.max(axis=1)))
    return x0, x1, y0, y1


def shade(u, v, cz, x, y):
    """(covered and kept, d) at pixel centres (x, y) (f64 arrays that broadcast against the triangles' u, v, cz [..., 3])."""
    u0, u1, u2 = u[..., 0], u[..., 1], u[..., 2]
    v0, v1, v2 = v[..., 0], v[..., 1], v[..., 2]
    e0 = (u2 - u1) * (y - v1) - (v2 - v1) * (x - u1)
    e1 = (u0 - u2) * (y - v2) - (v0 - v2) * (x - u2)
    e2 = (u1 - u0) * (y - v0) - (v1 - v0) * (x - u0)
    covered = ((e0 >= 0.0) & (e1 >= 0.0) & (e2 >= 0.0)) | ((e0 <= 0.0) & (e1 <= 0.0) & (e2 <= 0.0))
    s = (e0 + e1) + e2
    with np.errstate(all="ignore"):
        q = (e0 / cz[..., 0] + e1 / cz[..., 1]) + e2 / cz[..., 2]
        d = s / q
        keep = covered & (s != 0.0) & np.isfinite(d) & (d > 0.0)
    return keep, d


def render_view_np(points, triangles, K4, RT4, W, H, small=6):
    """The plane of one view: [H, W] f64 with row y = image row y (TOP row first, the pixel coordinates of the colouring), +inf
    where nothing covers."""
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    plane = np.full((H, W), np.inf, dtype=np.float64)
    if tri.shape[0] == 0:
        return plane
    pu, pv, pcz, pok = project(points, K4, RT4)
    ok = pok[tri].all(axis=1)
    u, v, cz = pu[tri][ok], pv[tri][ok], pcz[tri][ok]
    x0, x1, y0, y1 = pixel_ranges(u, v, W, H)
    some = (x0 <= x1) & (y0 <= y1)
    u, v, cz, x0, x1, y0, y1 = u[some], v[some], cz[some], x0[some], x1[some], y0[some], y1[some]
    is_small = (x1 - x0 < small) & (y1 - y0 < small)
    s = is_small
    for oy in range(small):
        for ox in range(small):
            x, y = x0[s] + ox, y0[s] + oy
            inside = (x <= x1[s]) & (y <= y1[s])
            keep, d = shade(u[s], v[s], cz[s], x, y)
            keep &= inside
            np.minimum.at(plane, (y[keep].astype(np.int64), x[keep].astype(np.int64)), d[keep])
    for t in np.nonzero(~is_small)[0]:
        xs = np.arange(int(x0[t]), int(x1[t]) + 1, dtype=np.float64)[None, :]
        ys = np.arange(int(y0[t]), int(y1[t]) + 1, dtype=np.float64)[:, None]
        keep, d = shade(u[t], v[t], cz[t], xs, ys)
        sub = plane[int(y0[t]):int(y1[t]) + 1, int(x0[t]):int(x1[t]) + 1]
        np.minimum(sub, np.where(keep, d, np.inf), out=sub)
    return plane


def render_depths_np(points, triangles, K4, RT4, W, H):
    """[n, H, W] planes (top row first, +inf = empty) of the views K4 / RT4 [n, 4, 4]."""
    K = np.asarray(K4, dtype=np.float64).reshape(-1, 4, 4)
    R = np.asarray(RT4, dtype=np.float64).reshape(-1, 4, 4)
    return np.stack([render_view_np(points, triangles, K[m], R[m], W, H) for m in range(K.shape[0])])


def to_vtk_depths(planes):
    """What dmi_color_download_depths returns for such planes: vtk point order (row 0 = the bottom image row), -1 for +inf."""
    p = np.asarray(planes, dtype=np.float64)
    return np.where(np.isinf(p), -1.0, p)[..., ::-1, :].copy()
