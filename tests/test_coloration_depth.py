"""The opt-in visibility test of the colouring (include/dmi.h: dmi_color_add_views_with_depth, dmi_color_set_depth_test;
DESIGN.md 8b): known answers and the restatement (tests/coloration_depth_np.py) on the CPU; on the GPU every output bit for
bit against the restatement -- occlusion, vertices behind cameras, special depths, tolerance boundaries, chunking, vertex
order -- and the plain pass untouched with the test off."""
import numpy as np
import pytest

from cudadepthmapintegration_amd import capi, scene
from coloration_depth_np import camera_z, color_mesh_depth_np, pixels
from oracle import oracle, oracle_np


def _three_view_scene():
    """One vertex (0, 0, 1) and three views of 8 x 6 that all select image pixel (3, 2) for it: view 0 sees it (depth 1 there),
    view 1 has an occluder's depth (0.5) there, view 2 has it behind the camera (RT = -I: cz = -1, the pixel is the same)."""
    W, H, n = 8, 6, 3
    K4 = np.tile(np.eye(4), (n, 1, 1))
    K4[:, 0, 0] = K4[:, 1, 1] = 10.0
    K4[:, 0, 2], K4[:, 1, 2] = 3.0, 2.0
    RT4 = np.tile(np.eye(4), (n, 1, 1))
    RT4[2, :3, :3] = -np.eye(3)
    colors = np.zeros((n, H, W, 3), dtype=np.uint8)
    depths = np.full((n, H, W), 7.0)
    for m, (rgb, d) in enumerate([((200, 10, 30), 1.0), ((20, 220, 40), 0.5), ((90, 90, 250), 1.0)]):
        colors[m, H - 1 - 2, 3] = rgb
        depths[m, H - 1 - 2, 3] = d
    return np.array([[0.0, 0.0, 1.0]]), colors, depths, K4, RT4


def test_known_answers_three_views():
    pts, colors, depths, K4, RT4 = _three_view_scene()
    mean, median, count = color_mesh_depth_np(pts, colors, depths, K4, RT4, 0.1)
    assert count[0] == 1 and list(mean[0]) == [200, 10, 30] and list(median[0]) == [200, 10, 30]
    # without the test all three count (the reference: no z-sign, no depth test)
    plain = oracle.color_mesh(pts, colors, K4, RT4)
    assert plain[2][0] == 3 and list(plain[0][0]) == [(200 + 20 + 90) // 3, (10 + 220 + 90) // 3, (30 + 40 + 250) // 3]
    for g, w in zip(color_mesh_depth_np(pts, colors, depths, K4, RT4, None), plain):
        assert np.array_equal(g, w)
    # a tolerance that reaches the occluder lets view 1 in; the view from behind stays out whatever the tolerance
    assert color_mesh_depth_np(pts, colors, depths, K4, RT4, 0.5)[2][0] == 2
    assert color_mesh_depth_np(pts, colors, depths, K4, RT4, 1e300)[2][0] == 2
    # special depths reject the pair
    for bad in (-1.0, np.nan, np.inf, 0.0):
        d = depths.copy()
        d[0, 6 - 1 - 2, 3] = bad
        assert color_mesh_depth_np(pts, colors, d, K4, RT4, 1e300)[2][0] == 1       # view 1 only (huge tolerance)


def test_restatement_with_a_huge_tolerance_is_the_reference_where_cz_and_d_are_positive():
    views = scene.make_views(9, 40, 30, seed=5)
    colors = scene.make_colors(9, 40, 30, seed=6)
    rng = np.random.default_rng(7)
    depths = rng.uniform(0.1, 9.0, size=(9, 30, 40))
    pts = scene.make_mesh_points(600, seed=8, radius=0.6) * 0.8       # inside the cameras' sphere: cz > 0 in every view
    for m in range(views.n):
        assert np.all(camera_z(pts, views.RT4[m]) > 0)
    got = color_mesh_depth_np(pts, colors, depths, views.K4, views.RT4, 1.7e308)
    want = oracle_np.color_mesh_np(pts, colors, views.K4, views.RT4)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert want[2].max() >= 5


def test_depth_context_without_gpu_fails_loudly():
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(capi.DmiError):
        capi.ColorContext()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
SPHERES = [((0.0, 0.0, 0.0), 0.5), ((0.55, 0.35, 0.25), 0.3)]   # the second in front of the first from some cameras


def _two_sphere_depth(K, RT, W, H):
    """Camera-z depth of the nearer of the two spheres at each pixel centre, f64, vtk row order; -1 where neither is hit."""
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    dx = ((np.arange(W) - cx) / fx)[None, :]
    dy = ((np.arange(H) - cy) / fy)[:, None]
    best = np.full((H, W), np.inf)
    for center, r in SPHERES:
        c = RT[:3, :3] @ np.asarray(center) + RT[:3, 3]
        a = dx * dx + dy * dy + 1.0
        b = dx * c[0] + dy * c[1] + c[2]
        disc = b * b - a * (c @ c - r * r)
        t = (b - np.sqrt(np.maximum(disc, 0.0))) / a
        best = np.where((disc >= 0) & (t > 0) & (t < best), t, best)
    return np.where(np.isfinite(best), best, -1.0)[::-1].copy()


def _two_sphere_scene(n_views=13, W=64, H=48, nv=6000, seed=3):
    views = scene.make_views(n_views, 8, 8, seed=seed, radius=2.2)
    K4 = views.K4.copy()
    K4[:, 0, 0] = K4[:, 1, 1] = 0.9 * W
    K4[:, 0, 2], K4[:, 1, 2] = W / 2.0, H / 2.0
    depths = np.stack([_two_sphere_depth(K4[m, :3, :3], views.RT4[m], W, H) for m in range(n_views)])
    rng = np.random.default_rng(seed)
    # special depths: "no depth", NaN, +inf scattered over every map
    for val in (-1.0, np.nan, np.inf):
        idx = rng.random(depths.shape) < 0.03
        depths[idx] = val
    colors = scene.make_colors(n_views, W, H, seed=seed + 1)
    d = rng.standard_normal((nv, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    k = nv // 3
    pts = np.empty((nv, 3))
    pts[:k] = np.asarray(SPHERES[0][0]) + SPHERES[0][1] * d[:k]                    # on the big sphere (partly hidden)
    pts[k:2 * k] = np.asarray(SPHERES[1][0]) + SPHERES[1][1] * d[k:2 * k]          # on the small one
    pts[2 * k:] = rng.uniform(-3.5, 3.5, size=(nv - 2 * k, 3))                    # elsewhere, many behind some camera
    return pts, colors, depths, K4, views.RT4


def _engineer_boundaries(pts, depths, K4, RT4, tol, n_each=6):
    """Depths set so that fabs(cz - d) is exactly tol, one ulp above and one ulp below it, for pairs of view 0.  Returns the
    counts of each kind (pairs that the restatement must accept / reject)."""
    W, H = depths.shape[2], depths.shape[1]
    px, py, ok = pixels(pts, K4[0], RT4[0])
    cz = camera_z(pts, RT4[0])
    ok &= (px >= 0) & (py >= 0) & (px < W) & (py < H) & (cz > 2 * tol)
    used, kinds = set(), {"equal": 0, "above": 0, "below": 0}
    for i in np.flatnonzero(ok):
        key = (int(px[i]), int(py[i]))
        if key in used:
            continue
        kind = [k for k, v in kinds.items() if v < n_each]
        if not kind:
            break
        d = cz[i] - tol
        while abs(cz[i] - d) > tol:
            d = np.nextafter(d, np.inf)
        while abs(cz[i] - d) < tol:
            d = np.nextafter(d, -np.inf)
        if abs(cz[i] - d) != tol:
            continue
        if kind[0] == "above":       # one ulp further from the vertex: |cz - d| > tol
            while abs(cz[i] - d) <= tol:
                d = np.nextafter(d, -np.inf)
        elif kind[0] == "below":     # one ulp nearer: |cz - d| < tol
            while abs(cz[i] - d) >= tol:
                d = np.nextafter(d, np.inf)
        used.add(key)
        depths[0, H - 1 - key[1], key[0]] = d
        kinds[kind[0]] += 1
    return kinds


def _check(got, want, what=""):
    for name, g, w in zip(("mean", "median", "count"), got, want):
        assert np.array_equal(g, w), f"{name} {what}"


@pytest.mark.gpu
def test_gpu_two_sphere_occlusion_bit_exact():
    tol = 0.0390625                    # 5 / 128: cz - d can equal it exactly (a difference of two doubles near 2 is exact)
    pts, colors, depths, K4, RT4 = _two_sphere_scene()
    kinds = _engineer_boundaries(pts, depths, K4, RT4, tol)
    assert min(kinds.values()) >= 3, kinds
    want = color_mesh_depth_np(pts, colors, depths, K4, RT4, tol)
    plain = oracle.color_mesh(pts, colors, K4, RT4)
    assert want[2].sum() < 0.8 * plain[2].sum() and want[2].max() >= 4       # occlusion and specials reject, others stay
    order = scene.morton_order(pts)
    with capi.ColorContext() as c:
        c.add_views(colors, K4, RT4, depths=depths)
        _check(c.process(pts), plain, "test off")
        c.set_depth_test(True, tol)
        for budget in (1 << 30, 13 * 4 * 1024):                                  # one chunk / six chunks
            c.set_scratch_budget(budget)
            for reorder in (False, True):
                c.set_vertex_reorder(reorder)
                _check(c.process(pts), want, f"budget {budget} reorder {reorder}")
                got = c.process(pts[order])                                          # mesh order: the pipelined loop
                _check(got, tuple(w[order] for w in want), f"ordered, budget {budget} reorder {reorder}")
        c.set_vertex_reorder(False)
        c.set_scratch_budget(1 << 30)
        # the boundary: exactly tol counts, one ulp beyond does not -- and a tolerance one ulp smaller drops the "equal" pairs
        for t in (tol, np.nextafter(tol, 0.0), np.nextafter(tol, 1.0), 0.0):
            c.set_depth_test(True, t)
            _check(c.process(pts[order]), tuple(w[order] for w in color_mesh_depth_np(pts, colors, depths, K4, RT4, t)), f"tol {t}")
        # view counts that leave a tail of the pipelined loop, and fewer views than one round of it
        for n_v in (9, 8, 5, 1):
            c.clear_views()
            c.add_views(colors[:n_v], K4[:n_v], RT4[:n_v], depths=depths[:n_v])
            c.set_depth_test(True, tol)
            w = color_mesh_depth_np(pts, colors[:n_v], depths[:n_v], K4[:n_v], RT4[:n_v], tol)
            _check(c.process(pts[order]), tuple(x[order] for x in w), f"{n_v} views ordered")
            _check(c.process(pts), w, f"{n_v} views")


@pytest.mark.gpu
def test_gpu_views_without_depths_and_switching_the_test_off():
    pts, colors, depths, K4, RT4 = _two_sphere_scene(n_views=6, nv=3000, seed=9)
    with capi.ColorContext() as c:
        with pytest.raises(capi.DmiError) as e:
            c.set_depth_test(True, float("nan"))
        assert e.value.code == 1
        for bad in (-1e-9, float("inf")):
            with pytest.raises(capi.DmiError):
                c.set_depth_test(True, bad)
        c.add_views(colors[:3], K4[:3], RT4[:3], depths=depths[:3])
        c.add_views(colors[3:], K4[3:], RT4[3:])                         # no depths for these
        plain = c.process(pts)
        _check(plain, oracle.color_mesh(pts, colors, K4, RT4), "plain")
        c.set_depth_test(True, 0.05)
        with pytest.raises(capi.DmiError) as e:
            c.process(pts)
        assert e.value.code == 1 and "without depths" in str(e.value)
        c.set_depth_test(False, 0.05)
        _check(c.process(pts), plain, "test switched off")
        c.clear_views()                                                    # drops the depths as well
        c.add_views(colors, K4, RT4, depths=depths)
        c.set_depth_test(True, 0.05)
        _check(c.process(pts), color_mesh_depth_np(pts, colors, depths, K4, RT4, 0.05), "all with depths")
        c.clear_views()
        c.add_views(colors, K4, RT4)
        with pytest.raises(capi.DmiError):
            c.process(pts)


@pytest.mark.gpu
def test_gpu_host_mirror_with_depth_from_list_files(tmp_path):
    pts, colors, depths, K4, RT4 = _two_sphere_scene(n_views=4, W=40, H=30, nv=2000, seed=11)
    depths[~np.isfinite(depths)] = -1.0                                  # (the ascii writer's text is for finite values)
    views = scene.Views(depths, K4, RT4, None)
    lv, lk = scene.write_view_files(str(tmp_path), views, colors)
    got = capi.mesh_coloration_from_lists(pts, lv, lk, depth_tolerance=0.05)
    _check(got, color_mesh_depth_np(pts, colors, depths, K4, RT4, 0.05), "host mirror")
    _check(capi.mesh_coloration_from_lists(pts, lv, lk), oracle.color_mesh(pts, colors, K4, RT4), "host mirror, plain")


@pytest.mark.gpu
def test_gpu_depth_test_at_bench_shape_sample():
    """bench.py's coloration probe shape: 2 M mesh-ordered vertices x 64 views of 1280 x 720 with the sphere's depth maps; a
    sample of 4096 vertices spread over the whole range (every chunk) is checked against the restatement."""
    n, W, H, nv = 64, 1280, 720, 2_000_000
    views = scene.make_views(n, 8, 8, seed=77)
    K4 = views.K4.copy()
    K4[:, 0, 0] = K4[:, 1, 1] = 0.9 * W
    K4[:, 0, 2], K4[:, 1, 2] = W / 2.0, H / 2.0
    colors = np.empty((n, H, W, 3), dtype=np.uint8)
    colors[:] = (np.arange(H * W * 3, dtype=np.uint32) % 251).astype(np.uint8).reshape(1, H, W, 3)
    colors += (np.arange(n, dtype=np.uint8) * 7)[:, None, None, None]
    depths = np.stack([scene.render_sphere_depth(K4[m, :3, :3], views.RT4[m], W, H) for m in range(n)])
    pts = scene.make_mesh_points(nv, seed=78)
    pts = pts[scene.morton_order(pts)]
    with capi.ColorContext() as c:
        c.add_views(colors, K4, views.RT4, depths=depths)
        c.set_depth_test(True, 0.01)
        mean, median, count = c.process(pts)
    ids = np.unique(np.concatenate([np.linspace(0, nv - 1, 4094).astype(np.int64), [0, nv - 1]]))
    assert len(ids) >= 4000
    want = color_mesh_depth_np(pts[ids], colors, depths, K4, views.RT4, 0.01)
    _check((mean[ids], median[ids], count[ids]), want, "sample")
    assert want[2].max() >= 10 and (want[2] == 0).any()
