"""dmi_color_render_depths / dmi_color_render_isosurface_depths (DESIGN.md 8b''): the mesh's own z-buffer as the depth planes of
the colouring's visibility test, bit for bit against tests/mesh_depth_np.py.

Hand-made triangles on one view of 37 x 29 (no multiple of the 8 x 4 tile) whose camera makes u, v exact integers and halves, so
that edges pass through pixel centres; the lane cap and the queue of the large pass, its overflow included; tails of triangles
and views; the sphere of scene.py extracted at 32^3, rendered in place and from the downloaded mesh, and coloured with the
rendered planes; life cycle and refusals."""
import functools

import numpy as np
import pytest

import coloration_depth_np as CD
import mesh_depth_np as MD
from cudadepthmapintegration_amd import capi, scene

INVALID_ARGUMENT, STATE = 1, 4
W, H = 37, 29
GROUP, CAP = capi.RENDER_VIEW_GROUP, capi.RENDER_LANE_CAP


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the hand-made camera: u = (2 cx + cz) / cz, v = (2 cy + cz) / cz, [R|T] a translation by dyadic numbers --------------------
def _camera(n=1):
    K = np.eye(4)
    K[0, 0] = K[1, 1] = 2.0
    K[0, 2] = K[1, 2] = 1.0
    RT = np.eye(4)
    RT[:3, 3] = (0.5, -0.25, 1.0)
    K4, RT4 = np.repeat(K[None], n, axis=0), np.repeat(RT[None], n, axis=0)
    for m in range(n):  # later views: the same camera moved sideways by whole and half pixels' worth
        RT4[m, 0, 3] += 0.25 * m
    return K4, RT4


def _vertex(u, v, cz):
    """The world point that view 0 of _camera projects to exactly (u, v) at camera z cz (u, v halves, cz a power of two)."""
    return [(u - 1.0) * cz / 2.0 - 0.5, (v - 1.0) * cz / 2.0 + 0.25, cz - 1.0]


def _mesh(triangles_uvz):
    pts = np.array([_vertex(*p) for t in triangles_uvz for p in t], dtype=np.float64)
    tri = np.arange(len(pts), dtype=np.int64).reshape(-1, 3)
    return pts, tri


HAND_MADE = [
    # two triangles that share the edge (4, 3) - (12, 11), which passes through pixel centres; opposite windings
    [(4, 3, 4), (12, 3, 4), (12, 11, 4)],
    [(4, 3, 4), (4, 11, 4), (12, 11, 4)],
    # vertices at half pixels, edges through centres
    [(14.5, 2.5, 2), (20.5, 2.5, 4), (14.5, 8.5, 8)],
    [(20.5, 8.5, 2), (14.5, 8.5, 2), (20.5, 2.5, 2)],
    # a repeated vertex and a collinear triangle: s == 0, nothing covered
    [(22, 4, 4), (22, 4, 4), (30, 9, 4)],
    [(22, 12, 4), (26, 14, 4), (30, 16, 4)],
    # one over each image border, one wholly outside
    [(-5, 10, 4), (3, 12, 4), (-2, 18, 4)],
    [(33, 10, 4), (44, 12, 4), (35, 17, 4)],
    [(10, -6, 4), (15, 2, 4), (7, 1, 4)],
    [(10, 26, 4), (16, 33, 4), (6, 31, 4)],
    [(50, 50, 4), (60, 50, 4), (55, 60, 4)],
    # two overlapping triangles at different depths (the nearer one wins wherever both cover)
    [(3, 14, 8), (15, 14, 8), (9, 26, 8)],
    [(5, 15, 2), (13, 16, 2), (9, 22, 4)],
]


def _behind_camera_triangle():
    """One vertex with cz <= 0: the triangle is skipped although its other vertices project into the image."""
    return np.array([_vertex(20, 20, 4), _vertex(28, 20, 4), [0.0, 0.0, -1.5]], dtype=np.float64)


def _hand_made_mesh(order=slice(None)):
    pts, tri = _mesh(HAND_MADE)
    extra = _behind_camera_triangle()
    tri = np.concatenate([tri, [[len(pts), len(pts) + 1, len(pts) + 2]]])[order]
    return np.concatenate([pts, extra]), np.ascontiguousarray(tri)


def _colors(n, w=W, h=H, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _render(pts, tri, K4, RT4, w=W, h=H, queue=None, batches=None, stats=None):
    """The planes the GPU renders, downloaded: [n, h, w] in vtk order.  stats: a dict that receives the call's queued pairs and
    pass times."""
    with capi.ColorContext() as c:
        n = len(K4)
        for lo, hi in (batches or [(0, n)]):
            c.add_views(_colors(hi - lo, w, h), K4[lo:hi], RT4[lo:hi])
        if queue is not None:
            c.set_render_queue_capacity(queue)
        c.render_depths(pts, tri)
        if stats is not None:
            stats.update(queued=c.render_queued_pairs(), pass_ms=c.render_pass_ms(), kernel_ms=c.render_kernel_ms())
        return c.download_depths()


def _pairs_beyond_the_cap(pts, tri, K4, RT4, w=W, h=H):
    """How many (triangle, view) pairs have more than CAP pixels in their clipped range: what the large pass must be given."""
    n = 0
    for m in range(len(K4)):
        u, v, _, ok = MD.project(pts, K4[m], RT4[m])
        keep = ok[tri].all(axis=1)
        x0, x1, y0, y1 = MD.pixel_ranges(u[tri][keep], v[tri][keep], w, h)
        some = (x0 <= x1) & (y0 <= y1)
        n += int((((x1 - x0 + 1) * (y1 - y0 + 1))[some] > CAP).sum())
    return n


def _want(pts, tri, K4, RT4, w=W, h=H):
    return MD.to_vtk_depths(MD.render_depths_np(pts, tri, K4, RT4, w, h))


def test_hand_made_scene_is_what_it_claims_on_the_cpu():
    K4, RT4 = _camera()
    pts, tri = _mesh(HAND_MADE)
    u, v, cz, ok = MD.project(pts, K4[0], RT4[0])
    flat = np.array([p for t in HAND_MADE for p in t], dtype=np.float64)
    assert ok.all() and (u == flat[:, 0]).all() and (v == flat[:, 1]).all() and (cz == flat[:, 2]).all()
    assert not MD.project(_behind_camera_triangle(), K4[0], RT4[0])[3].all()
    plane = MD.render_view_np(*_hand_made_mesh(), K4[0], RT4[0], W, H)
    assert plane[3, 4] == 4.0 and plane[11, 12] == 4.0 and plane[7, 8] == 4.0       # shared edge and its ends: inclusive
    assert np.isinf(plane[4:17, 22:31]).all()                                         # degenerate triangles cover nothing
    assert np.isfinite(plane[:, 0]).any() and np.isfinite(plane[:, W - 1]).any() and np.isfinite(plane[0]).any() and np.isfinite(plane[H - 1]).any()
    assert np.isinf(plane[20:24, 20:29]).all()                                        # the triangle with a vertex behind the camera
    assert plane[18, 9] < 8.0 and plane[15, 4] == 8.0                                 # the nearer of two, and the farther alone


@pytest.mark.gpu
def test_hand_made_triangles_bit_for_bit_in_both_orders():
    K4, RT4 = _camera()
    pts, tri = _hand_made_mesh()
    want = _want(pts, tri, K4, RT4)
    got = _render(pts, tri, K4, RT4)
    assert (want > 0).sum() > 100 and (want == -1.0).sum() > 100
    assert _same_bits(got, want), int((got != want).sum())
    assert _same_bits(_render(*_hand_made_mesh(slice(None, None, -1)), K4, RT4), want)


def _cap_triangles():
    """Ranges of exactly CAP pixels (8 x 8), of one more (5 x 13) and the whole image."""
    assert CAP == 64
    exactly = [(2, 3, 4), (9, 3, 4), (2, 10, 2)]
    one_more = [(12, 3, 4), (16, 3, 2), (12, 15, 4)]
    whole = [(-10, -10, 8), (100, -10, 8), (-10, 100, 16)]
    return exactly, one_more, whole


@pytest.mark.gpu
def test_lane_cap_queue_and_queue_overflow():
    K4, RT4 = _camera(2)
    exactly, one_more, whole = _cap_triangles()
    for name, tris in (("cap", [exactly]), ("cap+1", [one_more]), ("whole image", [whole]), ("all", [exactly, one_more, whole, whole[::-1]])):
        pts, tri = _mesh(tris)
        u, v, _, _ = MD.project(pts, K4[0], RT4[0])
        x0, x1, y0, y1 = MD.pixel_ranges(u[tri], v[tri], W, H)
        sizes = ((x1 - x0 + 1) * (y1 - y0 + 1)).astype(int).tolist()
        print(name, "range sizes in view 0:", sizes)
        if name == "cap":
            assert sizes == [CAP]
        if name == "cap+1":
            assert sizes == [CAP + 1]
        if name == "whole image":
            assert sizes == [W * H]
        want = _want(pts, tri, K4, RT4)
        assert (want[0] > 0).any()
        stats, stats1 = {}, {}
        assert _same_bits(_render(pts, tri, K4, RT4, stats=stats), want), name
        assert _same_bits(_render(pts, tri, K4, RT4, queue=1, stats=stats1), want), name + ", queue of one entry"
        # the large pass took exactly the pairs beyond the cap, with or without the overflow's second run
        beyond = _pairs_beyond_the_cap(pts, tri, K4, RT4)
        print(name, "queued", stats["queued"], "pass ms", stats["pass_ms"], "with a queue of one", stats1["pass_ms"])
        assert stats["queued"] == stats1["queued"] == beyond
        assert beyond == {"cap": 0, "cap+1": 1, "whole image": 2, "all": 5}[name]
        assert all(x >= 0.0 for x in stats["pass_ms"].values()) and stats["pass_ms"]["small"] > 0.0 and stats["kernel_ms"] > 0.0
    assert (_want(*_mesh([whole]), K4, RT4) > 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n_triangles,n_views,batches", [(0, 1, None), (1, 1, None), (257, 1, None), (257, GROUP + 1, None),
                                                         (257, 3, [(0, 2), (2, 3)])])
def test_tails_of_triangles_views_and_batches(n_triangles, n_views, batches):
    rng = np.random.default_rng(n_triangles + n_views)
    K4, RT4 = _camera(n_views)
    tris = []
    for _ in range(n_triangles):
        cx, cy = rng.integers(0, 2 * W) / 2.0, rng.integers(0, 2 * H) / 2.0
        tris.append([(cx + dx / 2.0, cy + dy / 2.0, float(2 ** rng.integers(1, 4))) for dx, dy in rng.integers(-9, 10, (3, 2))])
    pts, tri = _mesh(tris) if tris else (np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64))
    want = _want(pts, tri, K4, RT4)
    if batches is None:
        got = _render(pts, tri, K4, RT4)
    else:
        # one batch with uploaded depths (replaced by the rendering), one without (gets its planes from it)
        with capi.ColorContext() as c:
            (a0, a1), (b0, b1) = batches
            c.add_views(_colors(a1 - a0), K4[a0:a1], RT4[a0:a1], depths=np.full((a1 - a0, H, W), 3.0))
            c.add_views(_colors(b1 - b0), K4[b0:b1], RT4[b0:b1])
            c.render_depths(pts, tri)
            got = c.download_depths()
            assert _same_bits(c.download_depths(first=b0, count=b1 - b0), want[b0:b1])
    assert got.shape == (n_views, H, W)
    assert (want > 0).any() == (n_triangles > 0)
    assert _same_bits(got, want), int((got != want).sum())


# ---- the extracted sphere ------------------------------------------------------------------------------------------------------
SW, SH, S_VIEWS = 80, 60, 4
TOLERANCE = 2.0 / 32   # one voxel


@functools.lru_cache(maxsize=None)
def _sphere_scene():
    grid = scene.default_grid(32)
    ray = scene.default_ray_potential(grid)
    views = scene.make_views(S_VIEWS, SW, SH, seed=3)
    colors = scene.make_colors(S_VIEWS, SW, SH, seed=5)
    for a in (views.depth, views.K4, views.RT4, colors):
        a.setflags(write=False)
    return grid, ray, views, colors


def _extracted():
    grid, ray, views, _ = _sphere_scene()
    ctx = capi.FusionContext(grid, ray)
    ctx.add_views(views)
    ctx.fuse()
    ctx.synchronize()
    v, t = ctx.extract_isosurface(0.0)[:2]
    assert len(v) > 1000 and len(t) > 1000
    return ctx, v, t


@functools.lru_cache(maxsize=None)
def _sphere_reference(v_bytes, t_bytes):
    """The restatement's planes of the extracted mesh (computed once; keyed by the mesh's bytes)."""
    _, _, views, _ = _sphere_scene()
    v = np.frombuffer(v_bytes, dtype=np.float64).reshape(-1, 3)
    t = np.frombuffer(t_bytes, dtype=np.int64).reshape(-1, 3)
    want = _want(v, t, views.K4, views.RT4, SW, SH)
    want.setflags(write=False)
    return want


@pytest.mark.gpu
def test_sphere_in_place_equals_downloaded_mesh_equals_restatement_and_round_trips():
    _, _, views, colors = _sphere_scene()
    ctx, v, t = _extracted()
    want = _sphere_reference(v.tobytes(), np.ascontiguousarray(t, dtype=np.int64).tobytes())
    with ctx, capi.ColorContext() as c, capi.ColorContext() as c2:
        c.add_views(colors, views.K4, views.RT4)
        ctx.render_isosurface_depths(c)
        in_place = c.download_depths()
        assert c.render_kernel_ms() > 0.0
        c.render_depths(v, t)
        from_host = c.download_depths()
        ctx.render_isosurface_depths(c)          # twice: nothing changes
        again = c.download_depths()
        print(f"{len(v)} vertices, {len(t)} triangles, {S_VIEWS} views of {SW} x {SH}: {c.render_kernel_ms():.3f} ms of kernels, "
              f"{int((want > 0).sum())} covered pixels")
        assert (want > 0).sum() > SW * SH // 4
        assert _same_bits(in_place, want), int((in_place != want).sum())
        assert _same_bits(from_host, want) and _same_bits(again, want)
        # download_depths round-trips through add_views(depths=...) to the same colours
        c.set_depth_test(True, TOLERANCE)
        rendered = c.process(v)
        c2.add_views(colors, views.K4, views.RT4, depths=in_place)
        c2.set_depth_test(True, TOLERANCE)
        uploaded = c2.process(v)
        for a, b in zip(rendered, uploaded):
            assert _same_bits(a, b)


@pytest.mark.gpu
def test_colouring_with_rendered_planes_is_the_restatement_fed_the_restatements_planes():
    _, _, views, colors = _sphere_scene()
    ctx, v, t = _extracted()
    planes = _sphere_reference(v.tobytes(), np.ascontiguousarray(t, dtype=np.int64).tobytes())
    want = CD.color_mesh_depth_np(v, colors, planes, views.K4, views.RT4, TOLERANCE)
    plain = CD.color_mesh_depth_np(v, colors, None, views.K4, views.RT4, None)
    with ctx, capi.ColorContext() as c:
        c.add_views(colors, views.K4, views.RT4)
        ctx.render_isosurface_depths(c)
        c.set_depth_test(True, TOLERANCE)
        through_process = c.process(v)
        assert ctx.color_isosurface(c) == len(v)
        in_place = ctx.download_isosurface_colors()
    for name, a, b, w in zip(("mean", "median", "count"), through_process, in_place, want):
        assert _same_bits(a, w), (name, "ColorContext.process")
        assert _same_bits(b, w), (name, "color_isosurface")
    print("counts with rendered planes", np.bincount(want[2], minlength=S_VIEWS + 1).tolist(), "plain", np.bincount(plain[2], minlength=S_VIEWS + 1).tolist())
    assert (want[2] > 0).any()
    assert (want[2] < plain[2]).any()   # a far-side vertex: inside the image of a view that does not see it


@pytest.mark.gpu
def test_life_cycle_and_refusals():
    K4, RT4 = _camera(2)
    pts, tri = _hand_made_mesh()
    want = _want(pts, tri, K4, RT4)
    with capi.ColorContext() as c:
        with pytest.raises(capi.DmiError) as e:                      # no views
            c.render_depths(pts, tri)
        assert e.value.code == STATE and "dmi_color_render_depths" in str(e.value)
        c.add_views(_colors(2), K4, RT4)
        with pytest.raises(capi.DmiError) as e:                      # download without planes
            c.download_depths()
        assert e.value.code == INVALID_ARGUMENT and "no depth plane" in str(e.value)
        c.render_depths(pts, tri)
        assert _same_bits(c.download_depths(), want)
        for bad in (len(pts), -1):                                   # out-of-range ids: refused, the planes stay as they were
            broken = tri.copy()
            broken[3, 1] = bad
            with pytest.raises(capi.DmiError) as e:
                c.render_depths(pts, broken)
            assert e.value.code == INVALID_ARGUMENT and "outside" in str(e.value)
            assert _same_bits(c.download_depths(), want)
        with pytest.raises(capi.DmiError) as e:
            c.download_depths(first=1, count=2)
        assert e.value.code == INVALID_ARGUMENT
        with pytest.raises(capi.DmiError):
            c.set_render_queue_capacity(0)
        c.render_depths(pts, tri[:0])                                # no triangles: a success, every plane empty
        assert (c.download_depths() == -1.0).all()
        c.clear_views()                                              # ... drops the planes
        c.add_views(_colors(2), K4, RT4)
        with pytest.raises(capi.DmiError) as e:
            c.download_depths()
        assert e.value.code == INVALID_ARGUMENT
        # a fusion context without an extraction is refused, as in color_isosurface
        grid = scene.default_grid(8)
        with capi.FusionContext(grid, scene.default_ray_potential(grid)) as ctx:
            with pytest.raises(capi.DmiError) as e:
                ctx.render_isosurface_depths(c)
            assert e.value.code == INVALID_ARGUMENT and "no mesh" in str(e.value)
            # ... with a mesh, a colour context without views is a state error, whose text comes through the fusion context
            ctx.add_views(scene.make_views(2, 16, 12, seed=1))
            ctx.fuse()
            ctx.extract_isosurface(0.0)
            with capi.ColorContext() as empty:
                with pytest.raises(capi.DmiError) as e:
                    ctx.render_isosurface_depths(empty)
                assert e.value.code == STATE and "dmi_color_render_isosurface_depths" in str(e.value) and "no views" in str(e.value)
            # ... and into a context that has views the mesh is rendered, whatever their size
            ctx.render_isosurface_depths(c)
            assert c.download_depths().shape == (2, H, W)
