"""CPU restatement of dmi_views_build_points (include/dmi.h states the definition), vectorised numpy, written from the
definition and not from the kernel: plain f64 operations in the definition's order (numpy rounds every elementwise operation and
contracts nothing).  Depths come in as the views hold them, [n, H, W] in vtk point order (row 0 = the bottom image row); inside,
every plane is in image row order, so that an index [view, py, px] is the definition's and np.nonzero's order is the output's."""
import numpy as np

from coloration_depth_np import round_half_away
from depth_consistency_np import thresholded, valid_pixels, world_points


def _matrices(K4, RT4):
    return np.asarray(K4, dtype=np.float64).reshape(4, 4), np.asarray(RT4, dtype=np.float64).reshape(4, 4)


def pair_target(w, D_t, K4, RT4, abs_tol, rel_tol):
    """Step 3 of the consistency definition for one target view, in image row order: (agrees bool [H, W] over the source's pixels,
    iy, ix int [H, W]: the pixel of the target the source pixel lands on; 0 where it lands on none)."""
    H, W = D_t.shape
    K, RT = _matrices(K4, RT4)
    with np.errstate(all="ignore"):
        c = [((RT[i, 0] * w[0] + RT[i, 1] * w[1]) + RT[i, 2] * w[2]) + RT[i, 3] for i in range(3)]
        h = [((K[i, 0] * c[0] + K[i, 1] * c[1]) + K[i, 2] * c[2]) + K[i, 3] for i in range(3)]
        ok = (c[2] > 0.0) & ~(h[2] < 0.0)
        ru, rv = round_half_away(h[0] / h[2]), round_half_away(h[1] / h[2])
        ok = ok & (ru >= 0.0) & (rv >= 0.0) & (ru < float(W)) & (rv < float(H))
        ix = np.where(ok, ru, 0.0).astype(np.int64)
        iy = np.where(ok, rv, 0.0).astype(np.int64)
        d = D_t[iy, ix]
        bound = abs_tol + rel_tol * c[2]
        return ok & (d > 0.0) & (np.abs(c[2] - d) <= bound), iy, ix


def camera_points(D_s, K4):
    """Step 2's camera-space point c = (xn*d, yn*d, d) of every pixel with its own depth; D_s [H, W] in image row order."""
    H, W = D_s.shape
    K, _ = _matrices(K4, np.eye(4))
    px = np.arange(W, dtype=np.float64)[None, :]
    py = np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        yn = (py - K[1, 2]) / K[1, 1]
        xn = ((px - K[0, 2]) - K[0, 1] * yn) / K[0, 0]
        return [xn * D_s, yn * D_s, D_s]


def _shifted(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx] inside the image, `fill` outside."""
    H, W = a.shape
    b = np.full((H, W), fill, dtype=a.dtype)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    if (H - abs(dy)) > 0 and (W - abs(dx)) > 0:
        b[yd, xd] = a[ys, xs]
    return b


def _tangent(c, usable_plus, usable_minus, dy, dx):
    """(exists bool [H, W], t: three f64 [H, W], one_sided bool [H, W]) along one image axis."""
    exists = usable_plus | usable_minus
    both = usable_plus & usable_minus
    t = []
    with np.errstate(all="ignore"):
        for j in range(3):
            plus, minus = _shifted(c[j], dy, dx, np.nan), _shifted(c[j], -dy, -dx, np.nan)
            hi = np.where(usable_plus, plus, c[j])
            lo = np.where(usable_minus, minus, c[j])
            t.append(hi - lo)
    return exists, t, exists & ~both


def normals(D_s, K4, RT4, normal_abs_tol, normal_rel_tol):
    """Step 5 for every pixel of one view (image row order): (n f32 [H, W, 3], has bool [H, W], one_sided bool [H, W]: a normal
    that used a one-sided tangent).  Garbage-free: n is 0 wherever there is no normal, pixels that are not valid included."""
    H, W = D_s.shape
    _, RT = _matrices(K4, RT4)
    valid = valid_pixels(D_s)
    c = camera_points(D_s, K4)
    with np.errstate(all="ignore"):
        bound = normal_abs_tol + normal_rel_tol * D_s

        def usable(dy, dx):
            d2, v2 = _shifted(D_s, dy, dx, -1.0), _shifted(valid, dy, dx, False)
            return v2 & (np.abs(d2 - D_s) <= bound)

        ex, tx, onex = _tangent(c, usable(0, 1), usable(0, -1), 0, 1)
        ey, ty, oney = _tangent(c, usable(1, 0), usable(-1, 0), 1, 0)
        m = [tx[1] * ty[2] - tx[2] * ty[1], tx[2] * ty[0] - tx[0] * ty[2], tx[0] * ty[1] - tx[1] * ty[0]]
        s = (m[0] * c[0] + m[1] * c[1]) + m[2] * c[2]
        m = [np.where(s > 0.0, -mj, mj) for mj in m]
        g = [(RT[0, j] * m[0] + RT[1, j] * m[1]) + RT[2, j] * m[2] for j in range(3)]
        L = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
        has = valid & ex & ey & np.isfinite(L) & (L > 0.0)
        n = np.stack([np.where(has, gj / L, 0.0) for gj in g], axis=-1).astype(np.float32)
    return n, has, has & (onex | oney)


def consistency_counts(Dimg, K4, RT4, abs_tol, rel_tol):
    """Step 1: out_count of the consistency definition, [n, H, W] int32 in image row order; w of every view beside it."""
    n = Dimg.shape[0]
    valid = valid_pixels(Dimg)
    count = np.zeros(Dimg.shape, dtype=np.int32)
    ws = []
    for s in range(n):
        w = [x[::-1] for x in world_points(Dimg[s, ::-1], K4[s], RT4[s])]  # the helper speaks vtk row order
        ws.append(w)
        for t in range(n):
            if t != s:
                count[s] += pair_target(w, Dimg[t], K4[t], RT4[t], abs_tol, rel_tol)[0] & valid[s]
    return count, ws


def build_points(depth, K4, RT4, abs_tolerance, rel_tolerance, normal_abs_tolerance=None, normal_rel_tolerance=None, min_views=1,
                 pixel_step=1, dedupe=True, best_cost=None, threshold=None):
    """(arrays, report) of the definition.  arrays: xyz f64 [P, 3], normal f32 [P, 3], view i32 [P], pixel i32 [P], count i32 [P];
    report: valid, candidates, owned, points, with_normal; and one_sided, the emitted normals that used a one-sided tangent."""
    abs_tol, rel_tol = float(abs_tolerance), float(rel_tolerance)
    nabs = abs_tol if normal_abs_tolerance is None else float(normal_abs_tolerance)
    nrel = rel_tol if normal_rel_tolerance is None else float(normal_rel_tolerance)
    K4, RT4 = np.asarray(K4, dtype=np.float64), np.asarray(RT4, dtype=np.float64)
    Dimg = np.ascontiguousarray(thresholded(depth, best_cost, threshold)[:, ::-1, :])
    n, H, W = Dimg.shape
    valid = valid_pixels(Dimg)
    count, ws = consistency_counts(Dimg, K4, RT4, abs_tol, rel_tol)
    px, py = np.arange(W)[None, :], np.arange(H)[:, None]
    candidate = valid & (px % int(pixel_step) == 0) & (py % int(pixel_step) == 0) & (count >= int(min_views))
    owned = np.zeros_like(candidate)
    if dedupe:
        for s in range(n):
            for t in range(s):
                agrees, iy, ix = pair_target(ws[s], Dimg[t], K4[t], RT4[t], abs_tol, rel_tol)
                owned[s] |= candidate[s] & agrees & candidate[t][iy, ix]
    emitted = candidate & ~owned
    view, iy, ix = np.nonzero(emitted)  # ascending (view, py, px)
    xyz = np.zeros((view.size, 3), dtype=np.float64)
    normal = np.zeros((view.size, 3), dtype=np.float32)
    with_normal = one_sided = 0
    for s in range(n):
        sel = view == s
        if not sel.any():
            continue
        for j in range(3):
            xyz[sel, j] = ws[s][j][iy[sel], ix[sel]]
        nrm, has, one = normals(Dimg[s], K4[s], RT4[s], nabs, nrel)
        normal[sel] = nrm[iy[sel], ix[sel]]
        with_normal += int(has[iy[sel], ix[sel]].sum())
        one_sided += int(one[iy[sel], ix[sel]].sum())
    arrays = dict(xyz=xyz, normal=normal, view=view.astype(np.int32), pixel=(iy * W + ix).astype(np.int32),
                  count=count[view, iy, ix].astype(np.int32))
    report = dict(valid=int(valid.sum()), candidates=int(candidate.sum()), owned=int(owned.sum()), points=int(view.size),
                  with_normal=with_normal, one_sided=one_sided)
    return arrays, report
