"""The coloration pass at its edges (kernels: csrc/coloration_kernels.hip; context and host driver: csrc/dmi_capi_color.hip): pixel ties where the shortcut of the pixel selection runs
and where it must not, medians of multisets the test names, both median kernels at 65 535 / 65 536 views, tiled planes with
partial tiles checked texel by texel, and the view counts around the rounds of the pipelined view loop.  Scenes and
expectations: tests/coloration_cases.py.  Every output is an integer: every comparison is np.array_equal."""
import functools

import numpy as np
import pytest

from cudadepthmapintegration_amd import capi, scene
import coloration_cases as cases
from coloration_depth_np import color_mesh_depth_np
from oracle import oracle, oracle_np

NAMES = ("mean", "median", "count")


def _same(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        bad = np.flatnonzero((np.asarray(g) != np.asarray(w)).reshape(len(w), -1).any(axis=1))
        assert bad.size == 0, f"{name} {what}: {bad.size} vertices differ, first {bad[:5]}: got {g[bad[:5]].tolist()} want {w[bad[:5]].tolist()}"


# ---- CPU: the scenes against the oracles -------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,n", [(13, 7, 9), (7, 3, 4), (1, 1, 1)])
def test_pixel_grid_expectation_is_the_oracles(W, H, n):
    pts, K4, RT4 = cases.pixel_grid_scene(W, H, n)
    vals, _, _ = cases.case_values(n, W * H, False, seed=1)
    colors = cases.planes_from_values(vals, W, H)
    want = cases.expected_from_values(vals)
    _same(cases.expected_by_python_sort(vals), want, "python sort")
    _same(oracle.color_mesh(pts, colors, K4, RT4), want, "C oracle")
    _same(oracle_np.color_mesh_np(pts, colors, K4, RT4), want, "numpy oracle")
    vals, mask, names = cases.case_values(n, W * H, True, seed=2)
    colors = cases.planes_from_values(vals, W, H)
    want = cases.expected_from_values(vals, mask)
    _same(cases.expected_by_python_sort(vals, mask), want, "python sort, masked")
    _same(color_mesh_depth_np(pts, colors, cases.depths_from_mask(mask, W, H), K4, RT4, 0.0), want, "depth restatement")
    assert sorted(set(want[2].tolist())) == sorted(cases.case_counts(n)[:W * H])
    if W * H >= len(cases.NAMED_MULTISETS):
        assert {nm for row in names for nm in row} == {c[0] for c in cases.NAMED_MULTISETS}


def test_pixel_grid_with_a_depth_per_vertex_is_exact():
    """Vertices (x z, y z, z) with z = 1 + i / 4096: still pixel (x, y) and camera z exactly z, so a depth plane that holds z
    at every texel passes the test at tolerance 0 everywhere, and one that holds it anywhere else fails."""
    W, H = 13, 7
    z = 1.0 + np.arange(W * H) / 4096.0
    pts, K4, RT4 = cases.pixel_grid_scene(W, H, 1, z=z)
    vals, _, _ = cases.case_values(1, W * H, False, seed=3)
    colors = cases.planes_from_values(vals, W, H)
    depths = cases.planes_from_values(z[None], W, H)
    got = color_mesh_depth_np(pts, colors, depths, K4, RT4, 0.0)
    assert np.array_equal(got[2], np.ones(W * H, np.int32)) and np.array_equal(got[0], vals[0])
    assert color_mesh_depth_np(pts, colors, np.roll(depths, 1, axis=2), K4, RT4, 0.0)[2].sum() == 0


def test_named_multisets_are_what_their_names_say():
    rng = np.random.default_rng(4)
    for k in (2, 4, 24, 65534):
        for name, make in cases.HEAVY_MULTISETS:
            s = np.sort(make(rng, k))
            assert len(s) == k and s.min() >= 0 and s.max() <= 255
            if name.startswith("middle pair"):
                lo, hi = (int(t, 16) for t in name.split()[2:])
                assert (s[k // 2 - 1], s[k // 2]) == (lo, hi)


def test_vertex_orders_take_the_loops_they_are_meant_to():
    pts, _, _ = cases.pixel_grid_scene(*VIEW_COUNT_GRID, 1)
    assert cases.in_coherent_order(pts) and cases.in_coherent_order(pts[:61])
    assert not cases.in_coherent_order(pts[np.random.default_rng(5).permutation(len(pts))])


@functools.lru_cache(maxsize=None)
def _selection_reference():
    """oracle.color_mesh on every call of every view kind: {kind: [(mean, median, count), ...]}"""
    out = {}
    for kind, calls in cases.pixel_selection_sets().items():
        out[kind] = [oracle.color_mesh(c["points"], cases.coordinate_image(c["W"], c["H"]), c["K4"], c["RT4"]) for c in calls]
    return out


def test_tie_boundary_sets_are_not_vacuous_and_the_oracles_agree():
    """On the oracle's output alone: in every view kind at least 50 boundary pairs select different pixels on their two sides
    and at least 20 border pairs have count 1 on one side and 0 on the other.  And the numpy restatement of the reference
    agrees with the C oracle on exactly these vertices."""
    ref = _selection_reference()
    for kind, calls in cases.pixel_selection_sets().items():
        differ = borders = pairs = 0
        for c, (mean, median, count) in zip(calls, ref[kind]):
            px, py = cases.decode_pixel(mean)
            a, b = c["first"], c["second"]
            pairs += len(a)
            inside = (count[a] == 1) & (count[b] == 1)
            differ += int((inside & ((px[a] != px[b]) | (py[a] != py[b]))).sum())
            borders += int((c["border"] & (count[a] + count[b] == 1)).sum())
            assert np.array_equal(mean, median)                        # one view
            _same(oracle_np.color_mesh_np(c["points"], cases.coordinate_image(c["W"], c["H"]), c["K4"], c["RT4"]),
                  (mean, median, count), f"numpy oracle, {kind}")
        assert differ >= 50 and borders >= 20 and pairs >= 300, (kind, differ, borders, pairs)


def test_guard_vertices_meet_the_guards():
    K4, RT4, W, H, finite, bad = cases.guard_vertices()
    img = cases.coordinate_image(W, H)
    mean, _, count = oracle.color_mesh(finite, img, K4, RT4)
    _same(oracle_np.color_mesh_np(finite, img, K4, RT4), oracle.color_mesh(finite, img, K4, RT4), "numpy oracle, guards")
    px, py = cases.decode_pixel(mean)
    with np.errstate(all="ignore"):
        u = (64.0 * finite[:, 0] + 48.0 * finite[:, 2]) / finite[:, 2]
    assert ((u > -0.5) & (u < 0) & (count == 1) & (px == 0)).any()       # (-0.5, 0) is pixel 0
    assert ((u == -0.5) & (count == 0)).any() and ((u == W - 0.5) & (count == 0)).any()   # halves go away from zero
    assert ((u == 0.5) & (px == 1) & (count == 1)).any() and ((u == 2.5) & (px == 3)).any()
    for lo, hi in ((65535.0, 65536.0), (65536.0, 65538.0), (2.0 ** 31 - 1, np.inf)):
        assert ((np.abs(u) >= lo) & (np.abs(u) < hi)).any()
    assert (np.abs(finite[:, 2]) == 5e-324).any() and (count[np.abs(finite[:, 2]) == 5e-324] == 1).any()
    assert np.abs(finite).max() < 1e8
    assert not oracle.color_mesh(bad, img, K4, RT4)[2].any()


# ---- GPU: named medians, view counts, vertex orders ----------------------------------------------------------------------------
VIEW_COUNT_GRID = (21, 46)     # 966 vertices: four workgroups, the last partial; 21 % 8 and 46 % 4 leave partial tiles...
# ... and rows 23 apart are far enough for the host to call the row order coherent (test_vertex_orders_take_the_loops_...)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 9, 15, 16, 17, 24, 25])
def test_gpu_named_medians_at_every_view_count_and_order(n):
    """Named multisets per vertex and channel, counts 0 / 1 / 2 / 3 / n-1 / n by depth masks, for the view counts around the
    rounds of the pipelined loop (prologue 8, rounds of 8, epilogue, tail): fewer than 64 vertices and the grid in row order
    take the pipelined loop, a random permutation the plain one, the device's reordering the pipelined one through perm."""
    W, H = VIEW_COUNT_GRID
    pts, K4, RT4 = cases.pixel_grid_scene(W, H, n)
    shuffle = np.random.default_rng(n).permutation(len(pts))
    orders = {"61 vertices": np.arange(61), "row order": np.arange(len(pts)), "shuffled": shuffle}
    with capi.ColorContext() as c:
        for masked in (False, True):
            vals, mask, _ = cases.case_values(n, W * H, masked, seed=100 + n)
            want = cases.expected_from_values(vals, mask)
            c.clear_views()
            if masked:
                c.add_views(cases.planes_from_values(vals, W, H), K4, RT4, depths=cases.depths_from_mask(mask, W, H))
            else:
                c.add_views(cases.planes_from_values(vals, W, H), K4, RT4)
            c.set_depth_test(masked, 0.0)
            for reorder in (False, True):
                c.set_vertex_reorder(reorder)
                for name, sel in orders.items():
                    _same(c.process(pts[sel]), tuple(w[sel] for w in want), f"{n} views, {name}, masked {masked}, reorder {reorder}")


# ---- GPU: the tiled planes, texel by texel ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(1, 1), (7, 3), (9, 5), (13, 7), (33, 18), (64, 48)])
def test_gpu_every_texel_of_partial_tiles(W, H):
    """One vertex per pixel, colours that name (view, x, y), a depth plane with a value of its own at every texel: one view at a
    time the mean IS the texel, and at tolerance 0 the count is 1 only if the depth gathered is that texel's.  A wrong tile
    index or row flip in pack_color_kernel, pack_depth_kernel or texel_index moves some texel and fails."""
    n, nv = 3, W * H
    i = np.arange(nv)
    x, y = i % W, i // W
    vals = np.stack([np.stack([x, y, (37 * m + x * y) % 256], axis=-1) for m in range(n)]).astype(np.uint8)
    z = 1.0 + (np.arange(n)[:, None] * nv + i[None, :]) / 16384.0         # [n, nv]: distinct over views and texels, x z exact
    colors, depths = cases.planes_from_values(vals, W, H), np.stack([cases.planes_from_values(z[m][None], W, H)[0] for m in range(n)])
    with capi.ColorContext() as c:
        for m in range(n):
            pts, K4, RT4 = cases.pixel_grid_scene(W, H, 1, z=z[m])
            c.clear_views()
            c.add_views(colors[m:m + 1], K4, RT4, depths=depths[m:m + 1])
            for test in (False, True):
                c.set_depth_test(test, 0.0)
                _same(c.process(pts), (vals[m], vals[m], np.ones(nv, np.int32)), f"view {m}, depth test {test}")
            # the same vertices against the NEXT view's z: no depth matches, whatever texel is read
            other, _, _ = cases.pixel_grid_scene(W, H, 1, z=z[(m + 1) % n])
            assert not c.process(other)[2].any()
        # all views at once, the depth 1.0 everywhere but at one texel per view: the count pins those texels
        holes = sorted({(0, 0), (W - 1, H - 1), (W - 1, 0), (0, H - 1), (min(8, W - 1), min(4, H - 1)), (7 % W, 3 % H), (W // 2, H // 2)})
        mask = np.ones((len(holes), nv), dtype=bool)
        for m, (hx, hy) in enumerate(holes):
            mask[m, hy * W + hx] = False
        hv = np.stack([np.stack([x, y, (37 * m + x * y) % 256], axis=-1) for m in range(len(holes))]).astype(np.uint8)
        pts, K4, RT4 = cases.pixel_grid_scene(W, H, len(holes))
        c.clear_views()
        c.add_views(cases.planes_from_values(hv, W, H), K4, RT4, depths=cases.depths_from_mask(mask, W, H))
        c.set_depth_test(True, 0.0)
        want = cases.expected_from_values(hv, mask)
        assert want[2].min() == len(holes) - (1 if nv > 1 else len(holes)) and want[2].sum() == len(holes) * (nv - 1)
        _same(c.process(pts), want, "holes")


# ---- GPU: batches and chunks -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_batches_that_grow_the_stage_buffer_and_chunks_that_reuse_both_buffer_sets():
    """41 x 25 = 1025 vertices in chunks of 256: five chunks, both buffer sets used twice and once more, ONE vertex in the last.
    Views in two batches: colours only first (which sizes the stage buffer), then a batch with depths (which needs a bigger
    one)."""
    W, H, n1, n2 = 41, 25, 5, 4
    n = n1 + n2
    pts, K4, RT4 = cases.pixel_grid_scene(W, H, n)
    assert len(pts) == 4 * 256 + 1 and n2 * 8 > n1 * 3
    vals, mask, _ = cases.case_values(n, W * H, True, seed=7)
    colors, depths = cases.planes_from_values(vals, W, H), cases.depths_from_mask(mask, W, H)
    plain, masked = cases.expected_from_values(vals), cases.expected_from_values(vals, mask)
    shuffle = np.random.default_rng(8).permutation(len(pts))
    with capi.ColorContext() as c:
        c.set_scratch_budget(n * 4 * 256)
        c.add_views(colors[:n1], K4[:n1], RT4[:n1])
        c.add_views(colors[n1:], K4[n1:], RT4[n1:], depths=depths[n1:])
        for reorder in (False, True):
            c.set_vertex_reorder(reorder)
            _same(c.process(pts), plain, f"plain, reorder {reorder}")
            _same(c.process(pts[shuffle]), tuple(w[shuffle] for w in plain), f"plain, shuffled, reorder {reorder}")
        c.clear_views()
        c.add_views(colors[:n1], K4[:n1], RT4[:n1], depths=depths[:n1])
        c.add_views(colors[n1:], K4[n1:], RT4[n1:], depths=depths[n1:])
        c.set_depth_test(True, 0.0)
        for reorder in (True, False):
            c.set_vertex_reorder(reorder)
            _same(c.process(pts), masked, f"masked, reorder {reorder}")
            _same(c.process(pts[shuffle]), tuple(w[shuffle] for w in masked), f"masked, shuffled, reorder {reorder}")
        c.set_scratch_budget(1 << 30)
        _same(c.process(pts), masked, "masked, one chunk")


# ---- GPU: 65 535 views (the last count of the histogram medians) and beyond (the bit-by-bit kernel) --------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [65535, 65536, 65543])
def test_gpu_medians_at_the_16_bit_limit_of_the_histograms(n):
    """19 x 14 = 266 vertices (two workgroups, the second partial; partial tiles both ways) against n views added in two batches.
    65 535: every value of a vertex in ONE 16-bit counter (all equal; one upper nibble; one lower nibble), the MedianSeed's
    16-bit ranks at their largest, an even count of 65 534 by masks with the middle pair across a bin boundary.  65 536 and
    65 543: median_kernel and the projection kernel's instantiations without histograms, with and without the depth test, in
    the caller's order and through the device's reordering."""
    W, H = 19, 14
    pts, _, _ = cases.pixel_grid_scene(W, H, 1)
    eye = np.broadcast_to(np.eye(4), (n, 4, 4))
    vals, mask, names = cases.case_values(n, W * H, True, seed=n, cases=cases.HEAVY_MULTISETS)
    plain, masked = cases.expected_from_values(vals), cases.expected_from_values(vals, mask)
    assert {n, n - 1, 0, 1, 2, 3} == set(masked[2].tolist())
    # an even count of 65 534 or more whose middle pair lies across a bin boundary (at 65 535 views: made by a mask)
    assert any(masked[2][i] > 3 and masked[2][i] % 2 == 0 and "middle pair 0x4F 0x50" in names[i] for i in range(W * H))
    colors, depths = cases.planes_from_values(vals, W, H), cases.depths_from_mask(mask, W, H)
    first = 40000
    with capi.ColorContext() as c:
        c.add_views(colors[:first], eye[:first], eye[:first], depths=depths[:first])
        c.add_views(colors[first:], eye[first:], eye[first:], depths=depths[first:])
        for reorder in (False, True):
            c.set_vertex_reorder(reorder)
            c.set_depth_test(False, 0.0)
            _same(c.process(pts), plain, f"{n} views, reorder {reorder}")
            c.set_depth_test(True, 0.0)
            _same(c.process(pts), masked, f"{n} views, masked, reorder {reorder}")


# ---- GPU: the pixel selection against the C oracle -------------------------------------------------------------------------------
def _pad_to_chunks(points, chunk=256):
    """points repeated up to a whole number of chunks: what follows starts a chunk of its own"""
    extra = (-len(points)) % chunk
    return np.concatenate([points, points[:extra]]) if extra else points


def _three_arrangements(c, points, want, what, colors, K4, RT4):
    """alone (small margins: the shortcut decides most pairs); with the 1e9 vertex and the NaN vertex in the same chunk (useless
    margins: every pair takes the reference's expression); in chunks of 256 with those two in a chunk of their own"""
    nv = len(points)
    tail = oracle.color_mesh(cases.DEGENERATE, colors, K4, RT4)       # (the 1e9 vertex may well be inside a view)
    c.set_scratch_budget(1 << 30)
    _same(c.process(points), want, f"{what}, alone")
    got = c.process(np.concatenate([points, cases.DEGENERATE]))
    _same(tuple(g[:nv] for g in got), want, f"{what}, with degenerate vertices")
    _same(tuple(g[nv:] for g in got), tail, f"{what}, the degenerate vertices")
    padded = _pad_to_chunks(points)
    c.set_scratch_budget(4 * 256)
    got = c.process(np.concatenate([padded, cases.DEGENERATE]))
    _same(tuple(g[:nv] for g in got), want, f"{what}, degenerate vertices in their own chunk")
    _same(tuple(g[len(padded):] for g in got), tail, f"{what}, the degenerate vertices in their own chunk")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["exact", "sphere", "geo", "general_k", "large"])
def test_gpu_pixel_selection_at_the_references_tie_boundaries(kind):
    """Every vertex of the tie-boundary sets (the boundary double and 14 neighbours up to 2^30 ulps away, interior pixels and the
    four image borders, in x and in y) selects the oracle's pixel: the coordinate image makes the mean the pixel itself."""
    ref = _selection_reference()[kind]
    with capi.ColorContext() as c:
        for j, (call, want) in enumerate(zip(cases.pixel_selection_sets()[kind], ref)):
            c.clear_views()
            img = cases.coordinate_image(call["W"], call["H"])
            c.add_views(img, call["K4"], call["RT4"])
            _three_arrangements(c, call["points"], want, f"{kind} view {j}", img, call["K4"], call["RT4"])


@pytest.mark.gpu
def test_gpu_pixel_selection_at_the_guards():
    K4, RT4, W, H, finite, bad = cases.guard_vertices()
    img = cases.coordinate_image(W, H)
    with capi.ColorContext() as c:
        c.add_views(img, K4, RT4)
        _three_arrangements(c, finite, oracle.color_mesh(finite, img, K4, RT4), "finite guards", img, K4, RT4)
        c.set_scratch_budget(1 << 30)
        both = np.concatenate([finite, bad])
        _same(c.process(both), oracle.color_mesh(both, img, K4, RT4), "all guards")
        # on a camera plane of a general pose: the centre itself and points of the plane through it
        views = scene.make_views(3, W, H, seed=9, radius=3.0)
        R, t = views.RT4[0, :3, :3], views.RT4[0, :3, 3]
        centre = -R.T @ t
        plane = np.array([centre + a * R[0] + b * R[1] for a, b in ((0, 0), (1, 0), (0, 1), (0.3, -0.7), (1e-9, 0), (-2, 5))])
        colors = scene.make_colors(3, W, H, seed=10)
        c.clear_views()
        c.add_views(colors, views.K4, views.RT4)
        _three_arrangements(c, plane, oracle.color_mesh(plane, colors, views.K4, views.RT4), "camera plane", colors, views.K4, views.RT4)


@pytest.mark.gpu
@pytest.mark.parametrize("n_views,wh,nv,radius", [(5, (64, 48), 1000, 3.0), (33, (160, 120), 20000, 3.0), (8, (96, 72), 5000, 0.8)])
def test_gpu_color_mesh_bit_exact_without_degenerate_vertices(n_views, wh, nv, radius):
    """test_coloration.py's test_gpu_color_mesh_bit_exact with the same scenes and no 1e9 / NaN vertex: there those two make
    every margin infinite and no pair takes the shortcut; here the shortcut decides nearly all of them."""
    views = scene.make_views(n_views, wh[0], wh[1], seed=11, radius=radius)
    colors = scene.make_colors(n_views, wh[0], wh[1], seed=12)
    pts = scene.make_mesh_points(nv, seed=12)
    want = oracle.color_mesh(pts, colors, views.K4, views.RT4)
    _same(capi.color_mesh(pts, colors, views.K4, views.RT4), want, "shortcut on")
    assert want[2].max() >= min(n_views, 4)
