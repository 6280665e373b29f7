"""Scenes for tests/test_coloration_edges.py: cases in which the test, not chance, decides what the colouring meets.

  * the PIXEL-GRID scene: n identical views with RT = I and K = I and one vertex (x z, y z, z) per pixel.  The reference's
    expression gives pixel (x, y) without a rounding anywhere, so vertex i = y W + x sees colors[m, H-1-y, x] as its m-th
    value: the test writes any multiset per vertex and channel, and the expectation is a sort;
  * named multisets for the medians (all equal, middle pairs across a nibble-bin boundary, empty bins between them, ...);
  * coordinate images, whose colour IS the pixel, and vertices bisected to the reference's own tie boundaries;
  * a restatement of the host's choice between the two view loops, so that a test can say which one a vertex order takes.

Helpers only; every expectation here is plain numpy."""
import functools

import numpy as np

from cudadepthmapintegration_amd import scene
from coloration_depth_np import pixels


# ---- the pixel-grid scene --------------------------------------------------------------------------------------------------------
def pixel_grid_scene(W, H, n, z=None):
    """(points [W H, 3], K4 [n, 4, 4], RT4 [n, 4, 4]).  z None: every vertex at z = 1; else z [W H] with x z and y z exact
    (then the quotient is exactly x, y and the camera z of vertex i is exactly z[i])."""
    yy, xx = np.mgrid[0:H, 0:W]
    zz = np.ones(W * H) if z is None else np.asarray(z, dtype=np.float64)
    pts = np.stack([xx.ravel() * zz, yy.ravel() * zz, zz], axis=1)
    eye = np.tile(np.eye(4), (n, 1, 1))
    return pts, eye.copy(), eye.copy()


def planes_from_values(vals, W, H):
    """vals [n, W H, ...] (the m-th value of vertex i = y W + x) -> [n, H, W, ...] in vtk row order (row 0 = bottom)."""
    v = np.asarray(vals)
    return np.ascontiguousarray(v.reshape((v.shape[0], H, W) + v.shape[2:])[:, ::-1])


def depths_from_mask(mask, W, H):
    """mask [n, W H] bool -> depth planes: 1.0 where the pair is to count (cz is exactly 1, tolerance 0), -1.0 where not."""
    return planes_from_values(np.where(mask, 1.0, -1.0), W, H)


def expected_from_values(vals, mask=None):
    """(mean, median, count) of the multisets: vals [n, nv, 3] u8, mask [n, nv] bool (None: every pair counts).  sorted,
    sum // cnt, (s[cnt//2] + s[cnt//2 - 1]) // 2 for even counts, s[cnt//2] for odd ones; zeros where the count is 0."""
    v = np.ascontiguousarray(np.asarray(vals).transpose(1, 2, 0)).astype(np.int16)     # [nv, 3, n]
    n = v.shape[2]
    ok = np.ones(v.shape[::2], dtype=bool) if mask is None else np.asarray(mask, dtype=bool).T   # [nv, n]
    cnt = ok.sum(axis=1).astype(np.int64)
    sums = np.where(ok[:, None, :], v, 0).sum(axis=2, dtype=np.int64)
    s = np.sort(np.where(ok[:, None, :], v, np.int16(1000)), axis=2)                    # the invalid ones sort last
    seen = cnt > 0
    k = np.where(seen, cnt, 1)
    hi = np.take_along_axis(s, np.broadcast_to((k // 2)[:, None, None], (len(k), 3, 1)), axis=2)[:, :, 0].astype(np.int64)
    lo_rank = np.where(k % 2 == 0, k // 2 - 1, k // 2)
    lo = np.take_along_axis(s, np.broadcast_to(lo_rank[:, None, None], (len(k), 3, 1)), axis=2)[:, :, 0].astype(np.int64)
    mean = np.where(seen[:, None], sums // k[:, None], 0).astype(np.uint8)
    median = np.where(seen[:, None], (hi + lo) // 2, 0).astype(np.uint8)
    assert n >= cnt.max()
    return mean, median, cnt.astype(np.int32)


def expected_by_python_sort(vals, mask=None):
    """The same, one vertex at a time with sorted(): what expected_from_values is checked against on small scenes."""
    vals = np.asarray(vals)
    n, nv, _ = vals.shape
    mean, median, count = np.zeros((nv, 3), np.uint8), np.zeros((nv, 3), np.uint8), np.zeros(nv, np.int32)
    for i in range(nv):
        keep = [m for m in range(n) if mask is None or mask[m, i]]
        cnt = count[i] = len(keep)
        for ch in range(3):
            if cnt:
                s = sorted(int(vals[m, i, ch]) for m in keep)
                mean[i, ch] = sum(s) // cnt
                median[i, ch] = (s[cnt // 2] + s[cnt // 2 - 1]) // 2 if cnt % 2 == 0 else s[cnt // 2]
    return mean, median, count


# ---- named multisets ---------------------------------------------------------------------------------------------------------------
def _halves(lo_max, hi_min):
    """k values whose lower half is <= lo_max and contains it, whose upper half is >= hi_min and contains it: for an even k
    the middle pair is (lo_max, hi_min)."""
    def make(rng, k):
        a, b = k // 2, k - k // 2
        low = rng.integers(0, lo_max + 1, size=a)
        high = rng.integers(hi_min, 256, size=b)
        if a:
            low[0] = lo_max
        high[0] = hi_min
        return np.concatenate([low, high])
    return make


def _all_equal(v):
    return lambda rng, k: np.full(k, v)


def _many_duplicates(rng, k):
    out = rng.integers(0, 256, size=k)
    out[rng.random(k) < 0.6] = 0x9C
    return out


NAMED_MULTISETS = [
    ("equal 0x00", _all_equal(0x00)), ("equal 0x0F", _all_equal(0x0F)), ("equal 0x10", _all_equal(0x10)),
    ("equal 0x7F", _all_equal(0x7F)), ("equal 0x80", _all_equal(0x80)), ("equal 0xFF", _all_equal(0xFF)),
    ("middle pair 0x0F 0x10", _halves(0x0F, 0x10)),                 # neighbouring bins
    ("middle pair 0x2F 0x90", _halves(0x2F, 0x90)),                 # empty bins in between
    ("middle pair 0x53 0x5A", _halves(0x53, 0x5A)),                 # one bin, different low nibbles
    ("middle pair 0x57 0x57", _halves(0x57, 0x57)),                 # one bin, equal low nibbles
    ("many duplicates", _many_duplicates),
    ("extremes", lambda rng, k: rng.choice(np.array([0x00, 0xFF]), size=k)),
    ("random", lambda rng, k: rng.integers(0, 256, size=k)),
]
# what only a very large count can break: every value in one counter of the 16-bit histograms (a carry would leave bins 0..7
# for bins 8..15 of the same word)
HEAVY_MULTISETS = NAMED_MULTISETS + [
    ("upper nibble 3", lambda rng, k: 0x30 | rng.integers(0, 16, size=k)),
    ("upper nibble 0", lambda rng, k: rng.integers(0, 16, size=k)),
    ("upper nibble 7", lambda rng, k: 0x70 | rng.integers(0, 16, size=k)),
    ("lower nibble 5", lambda rng, k: (rng.integers(0, 16, size=k) << 4) | 5),
    ("equal 0x35", _all_equal(0x35)),
    ("middle pair 0x4F 0x50", _halves(0x4F, 0x50)),
]


def case_counts(n):
    """The counts a masked scene cycles through: 0, 1, 2, 3, n - 1 and n (those that exist for n views)."""
    out = []
    for k in (n, 0, 1, n - 1, 2, 3):
        if 0 <= k <= n and k not in out:
            out.append(k)
    return out


def case_values(n, nv, masked, seed, cases=None):
    """(vals [n, nv, 3] u8, mask [n, nv] bool or None, names [nv][3]).  Vertex i, channel ch holds the named multiset number
    (i + 4 ch) mod len(cases) -- neighbouring lanes and the three channels of a vertex differ -- in a random order over the
    views that count for it.  masked: the count of vertex i cycles through case_counts(n) (the two cycle lengths are coprime,
    so every case meets every count) and the views that do not count carry random values, which nothing may look at."""
    cases = NAMED_MULTISETS if cases is None else cases
    rng = np.random.default_rng(seed)
    vals = rng.integers(0, 256, size=(n, nv, 3), dtype=np.uint8)
    mask = None
    counts = np.full(nv, n)
    if masked:
        cyc = case_counts(n)
        assert np.gcd(len(cyc), len(cases)) == 1
        counts = np.array([cyc[i % len(cyc)] for i in range(nv)])
        # vertex i counts the views whose place in one shuffled order, turned by i's own offset, is below its count
        place = (rng.permutation(n)[:, None] + rng.integers(0, n, size=nv)[None, :]) % n
        mask = place < counts[None, :]
    names = []
    for i in range(nv):
        k = int(counts[i])
        where = slice(None) if mask is None else mask[:, i]
        names.append([cases[(i + 4 * ch) % len(cases)][0] for ch in range(3)])
        if k == 0:
            continue
        for ch in range(3):
            vals[where, i, ch] = rng.permutation(cases[(i + 4 * ch) % len(cases)][1](rng, k)).astype(np.uint8)
    return vals, mask, names


# ---- which view loop a vertex order takes --------------------------------------------------------------------------------------
def in_coherent_order(points):
    """The host's test (dmi_color_process): fewer than 64 vertices, or the median squared step between consecutive vertices
    under a hundredth of that between vertices half the array apart -> the pipelined view loop; else the plain one."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    if n < 64:
        return True
    samples = min(512, n // 2)
    i = np.arange(samples) * ((n - 1) // samples)

    def upper_median(a, b):
        d = ((p[a] - p[b]) ** 2).sum(axis=1)
        d = np.where(np.isfinite(d), d, 1.0e300)
        return np.sort(d)[len(d) // 2]
    return bool(upper_median(i, i + 1) < 0.01 * upper_median(i, (i + n // 2) % n))


# ---- coordinate images and tie boundaries ----------------------------------------------------------------------------------------
def coordinate_image(W, H):
    """[1, H, W, 3] u8, vtk row order: image pixel (px, py) holds R = px & 255, G = py & 255, B = (px >> 8) | ((py >> 8) << 4)."""
    py, px = np.mgrid[0:H, 0:W]
    img = np.stack([px & 255, py & 255, (px >> 8) | ((py >> 8) << 4)], axis=-1).astype(np.uint8)
    return np.ascontiguousarray(img[::-1])[None]


def decode_pixel(mean):
    """(px, py) from the mean of ONE view of a coordinate image."""
    m = np.asarray(mean).astype(np.int64)
    return m[:, 0] | ((m[:, 2] & 15) << 8), m[:, 1] | ((m[:, 2] >> 4) << 8)


def unproject(K4, RT4, u, v, cz):
    """World points whose real projection is (u, v) at camera z cz (cz < 0: behind the camera, where the reference still
    projects)."""
    K3, R, t = np.asarray(K4)[:3, :3], np.asarray(RT4)[:3, :3], np.asarray(RT4)[:3, 3]
    q = np.linalg.solve(K3, np.stack([u, v, np.ones_like(u)]))          # K3 c = s (u, v, 1)
    c = q * (cz / q[2])
    return (R.T @ (c - t[:, None])).T


def ulp_shift(x, s):
    """x moved by s units in the last place (s < 0: towards -inf), through the ordered integers of the doubles."""
    b = np.asarray(x, dtype=np.float64).view(np.int64)
    o = np.where(b < 0, np.int64(-2 ** 63) - b, b) + np.asarray(s, dtype=np.int64)
    return np.where(o < 0, np.int64(-2 ** 63) - o, o).view(np.float64)


ULP_STEPS = [0, 1, 2, 3, 2 ** 8, 2 ** 16, 2 ** 24, 2 ** 30]
BOUNDARIES = ("interior", "low", "high")   # between two pixels inside the image / pixel -1 | 0 / pixel size-1 | size


def tie_boundaries(K4, RT4, W, H, axis, boundary, count, rng, cz_range, signed_cz=False):
    """Vertices at the reference's own tie boundary of pixel axis `axis` (0: x, 1: y).  For `count` vertices that start inside
    the pixel next to the boundary, the world coordinate that moves that pixel coordinate most is bisected, vectorised over
    coloration_depth_np.pixels, until two adjacent doubles select different pixels.  Returns (points [count', 15, 3], pair):
    points[:, j] is the boundary double moved by STEPS[j] ulps towards (+) or away from (-) its neighbour on the other side;
    pair = (index of step 0, index of step +1) along axis 1."""
    size = (W, H)[axis]
    other = (H, W)[axis]
    if boundary == "interior":
        target = rng.integers(1, size - 2, size=count) + rng.uniform(-0.3, 0.3, size=count)
        direction = rng.choice([-1.0, 1.0], size=count)
    elif boundary == "low":
        target, direction = rng.uniform(-0.4, 0.4, size=count), -np.ones(count)
    else:
        target, direction = size - 1 + rng.uniform(-0.4, 0.4, size=count), np.ones(count)
    cross = rng.uniform(1.0, other - 2.0, size=count)                  # the other pixel coordinate: well inside
    cz = rng.uniform(*cz_range, size=count)
    if signed_cz:
        cz *= rng.choice([-1.0, 1.0], size=count)
    u, v = (target, cross) if axis == 0 else (cross, target)
    lo = unproject(K4, RT4, u, v, cz)

    def selected(p):
        px, py, ok = pixels(p, K4, RT4)
        return np.where(ok, (px, py)[axis], np.int64(-2 ** 40))
    start = selected(lo)
    if boundary == "interior":
        same_side = lambda p: selected(p) == start
    elif boundary == "low":
        same_side = lambda p: selected(p) >= 0
    else:
        same_side = lambda p: (selected(p) <= size - 1) & (selected(p) > -2 ** 40)
    # d(pixel coordinate) / d(world coordinate c) = (P[axis][c] - t P[2][c]) / dz with P = K3 [R|T]
    P = np.asarray(K4)[:3, :3] @ np.asarray(RT4)[:3, :4]
    dz = P[2, :3] @ lo.T + P[2, 3]
    grad = (P[axis, :3][None, :] - target[:, None] * P[2, :3][None, :]) / dz[:, None]
    c = np.argmax(np.abs(grad), axis=1)
    rows = np.arange(count)
    hi = lo.copy()
    hi[rows, c] += direction * 1.1 / grad[rows, c]                      # about 1.1 pixels further: the next pixel
    keep = same_side(lo) & ~same_side(hi)
    lo, hi, c, rows = lo[keep], hi[keep], c[keep], np.arange(int(keep.sum()))
    a, b = lo[rows, c].copy(), hi[rows, c].copy()                       # a: this side, b: the other side
    for _ in range(80):
        mid = a + (b - a) / 2
        done = (mid == a) | (mid == b)
        if done.all():
            break
        p = lo.copy()
        p[rows, c] = mid
        side = same_side(p)
        a = np.where(side & ~done, mid, a)
        b = np.where(~side & ~done, mid, b)
    towards = np.where(b > a, 1, -1)
    keep = ulp_shift(a, towards) == b                                   # adjacent doubles (a coordinate next to 0 may not get there)
    lo, c, a, b, towards, rows = lo[keep], c[keep], a[keep], b[keep], towards[keep], np.arange(int(keep.sum()))
    steps = np.array(ULP_STEPS + [-s for s in ULP_STEPS[1:]], dtype=np.int64)
    pts = np.repeat(lo[:, None, :], len(steps), axis=1)
    pts[rows, :, c] = ulp_shift(a[:, None], towards[:, None] * steps[None, :])
    return pts, (0, 1)


def geo_offset_view(RT4, offset):
    """The same camera for vertices moved by `offset`: R (p + o) + (T - R o) = R p + T."""
    out = np.array(RT4, dtype=np.float64)
    out[:3, 3] = out[:3, 3] - out[:3, :3] @ np.asarray(offset, dtype=np.float64)
    return out


GEO_OFFSET = np.array([5.0e6, 4.0e6, 1.0e3])


def _exact_camera(W, H):
    K4, RT4 = np.eye(4), np.eye(4)
    K4[0, 0], K4[1, 1], K4[0, 2], K4[1, 2] = 64.0, 32.0, float(W // 2), float(H // 2)
    return K4, RT4


def _sphere_views(n, W, H, radius, seed):
    v = scene.make_views(n, 8, 8, seed=seed, radius=radius)             # the poses; the intrinsics for this image size:
    K4 = v.K4.copy()
    K4[:, 0, 0] = K4[:, 1, 1] = 0.9 * W
    K4[:, 0, 2], K4[:, 1, 2] = W / 2.0, H / 2.0
    return K4, v.RT4


@functools.lru_cache(maxsize=None)
def pixel_selection_sets():
    """{view kind: [call, ...]}; a call is a dict of ONE view (K4, RT4 [1, 4, 4], W, H), the vertices `points` [nv, 3] (rows of
    15 ulp steps per boundary vertex, flattened), `first` / `second` (indices of the two sides of every boundary pair) and
    `border` (bool per pair: an image border, where the count goes from 1 to 0)."""
    rng = np.random.default_rng(2024)
    cams = {"exact": [], "sphere": [], "geo": [], "general_k": [], "large": []}
    W, H = 96, 72
    cams["exact"].append((*_exact_camera(W, H), W, H, (0.5, 4.0), False, None))
    for radius, cz_range, signed in ((3.0, (2.4, 3.6), False), (0.8, (0.15, 1.4), True)):   # 0.8: inside the mesh, dz of both signs
        K4, RT4 = _sphere_views(2, W, H, radius, seed=5)
        for m in range(2):
            cams["sphere"].append((K4[m], RT4[m], W, H, cz_range, signed, None))
            cams["geo"].append((K4[m], RT4[m], W, H, cz_range, signed, GEO_OFFSET))
    K4, RT4 = _sphere_views(1, W, H, 3.0, seed=6)
    Kg = K4[0].copy()
    Kg[2, :3] = [0.05, -0.03, 0.9]                                       # a general third row: dz mixes cx, cy, cz
    cams["general_k"].append((Kg, RT4[0], W, H, (2.4, 3.6), False, None))
    K4, RT4 = _sphere_views(1, 4096, 3000, 3.0, seed=7)
    cams["large"].append((K4[0], RT4[0], 4096, 3000, (2.4, 3.6), False, None))
    out = {}
    for kind, views in cams.items():
        per_class = 60 // len(views)                                    # 6 classes x 60: 360 boundary vertices per kind
        calls = []
        for K4, RT4, W, H, cz_range, signed, offset in views:
            if offset is not None:
                RT4 = geo_offset_view(RT4, offset)
            blocks, border = [], []
            for axis in (0, 1):
                for boundary in BOUNDARIES:
                    pts, _ = tie_boundaries(K4, RT4, W, H, axis, boundary, per_class, rng, cz_range, signed)
                    blocks.append(pts)
                    border.append(np.full(len(pts), boundary != "interior"))
            pts = np.concatenate(blocks)
            steps = pts.shape[1]
            first = np.arange(len(pts)) * steps
            calls.append({"K4": K4[None], "RT4": RT4[None], "W": W, "H": H, "points": pts.reshape(-1, 3).copy(),
                          "first": first, "second": first + 1, "border": np.concatenate(border)})
        out[kind] = calls
    return out


def guard_vertices():
    """(K4 [1, 4, 4], RT4 [1, 4, 4], W, H, finite [a, 3], non_finite [b, 3]): vertices at the guards of the pixel shortcut, for
    the exact camera (u = 64 x / z + 48, v = 32 y / z + 36).  The finite ones have moderate coordinates, so a chunk that holds
    only them keeps small margins."""
    W, H = 96, 72
    K4, RT4 = _exact_camera(W, H)
    fx, fy, cx, cy = 64.0, 32.0, 48.0, 36.0
    den = 5e-324
    pts = []

    def at(u, v, z=1.0):
        pts.append([(u - cx) * z / fx, (v - cy) * z / fy, z])
    for size, along_x in ((W, True), (H, False)):                      # exact halves round away from zero; (-0.5, 0) is pixel 0
        for t in (-0.5, 0.5, 1.5, 2.5, size - 1.5, size - 0.5, -0.25, -0.49999999999999994, np.nextafter(-0.5, -1.0),
                  np.nextafter(size - 0.5, 0.0)):
            for z in (1.0, 0.75, -2.0):
                at(t, 10.0, z) if along_x else at(10.0, t, z)
    for big in (65536.0, 2.0 ** 31, 2.0 ** 31 + 4096.0, 2.0 ** 40):     # |u| or |v| around the 65 536 guard, at and beyond 2^31
        for s in (-1.0, 1.0):
            for d in (np.nextafter(big, 0.0), big, np.nextafter(big, np.inf)):
                pts.append([s * d / 64.0 / 1024.0, 0.0, 1.0 / 1024.0])   # u = s d + 48, v = 36
                pts.append([0.0, s * d / 32.0 / 1024.0, 1.0 / 1024.0])   # u = 48, v = s d + 36
                if big < 2.0 ** 32:
                    pts.append([s * d / 64.0 - 0.75, 0.0, 1.0])          # u = s d exactly
    for z in (0.0, -0.0, den, -den, 3 * den, 2.0 ** -1030):             # dz exactly 0, -0.0, +- a denormal: 0/dz, x/dz
        for xy in ((0.0, 0.0), (0.25, -0.125), (-0.0, 0.0)):
            pts.append([xy[0], xy[1], z])
    for xy in ((1.0, 1.0), (0.0, 0.0), (-3.0, 0.5)):                     # on the camera plane z = 0 (identity pose)
        pts.append([xy[0], xy[1], 0.0])
    finite = np.array(pts, dtype=np.float64)
    bad = []
    for v in (np.inf, -np.inf, np.nan):
        for a in range(3):
            p = [0.1, -0.2, 1.5]
            p[a] = v
            bad.append(p)
    bad.append([np.inf, np.inf, np.inf])
    bad.append([-np.inf, 0.0, -np.inf])
    return K4[None], RT4[None], W, H, finite, np.array(bad, dtype=np.float64)


DEGENERATE = np.array([[1e9, -1e9, 1e9], [np.nan, 0.0, 0.0]])          # the vertices that switch the shortcut off for a chunk
