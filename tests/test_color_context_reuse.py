"""One capi.ColorContext through a sequence in which the buffers of every group of its state (csrc/dmi_color_context.h) grow,
are reused while large enough, and are released -- twice over.  Every output must equal, bit for bit, what a FRESH context returns
for the same step, and the numpy restatements (coloration_cases, coloration_depth_np, mesh_depth_np).

Images of 41 x 25 (partial 8 x 4 tiles); the pixel-grid scene of coloration_cases, 1025 vertices:
  1. 5 views with colours only, then 4 with depths (the stage buffer grows from 3 to 8 bytes per pixel); a scratch budget of
     9 * 4 * 256 bytes cuts the vertices into five chunks (both buffer sets); vertex reorder off and on;
  2. 300 vertices with a budget of 1 GiB (every work buffer is kept), then the 1025 again (still large enough);
  3. clear; 17 views with depths (the view tables grow; one rasteriser group of 16 and a tail of one); the depth test; an
     octahedron rendered with a queue that starts with ONE entry (it grows inside the call); the planes downloaded; the depth test
     against the rendered planes (which now own every depth plane);
  4. clear (the rendered planes go with the views); 3 views without depths, rendered, planes 1 and 2 downloaded;
  5. the mesh of a 16^3 fusion context coloured in place with the fused test (the fused tables and the order-of-work sample are
     allocated) and without it.
Only results and return codes are asserted (a failing call raises)."""
import functools

import numpy as np
import pytest

import coloration_cases as C
import coloration_depth_np as CD
import mesh_depth_np as MD
from cudadepthmapintegration_amd import capi, scene

W, H = 41, 25
NV = W * H
SMALL_BUDGET = 9 * 4 * 256
THRESHOLD, FUSED_TOL, RENDER_TOL, ISO = 0.8, 0.3, 0.25, 0.0   # FUSED_TOL: 2.4 voxels of the 16^3 grid
# around the vertices' plane z = 1: its front faces are nearer than the vertices they cover, by less than RENDER_TOL near the rim
OCTAHEDRON = (np.array([[5.0, 12, 1], [35, 12, 1], [20, 2, 1], [20, 22, 1], [10, 6, 0.5], [30, 18, 1.5]]),
              np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]))


@functools.lru_cache(maxsize=None)
def _data():
    rng = np.random.default_rng(11)
    points, _, _ = C.pixel_grid_scene(W, H, 1)
    eye = np.tile(np.eye(4), (17, 1, 1))
    vals = rng.integers(0, 256, size=(17, NV, 3), dtype=np.uint8)
    mask = rng.random((17, NV)) < 0.6
    d = dict(points=points, eye=eye, vals=vals, mask=mask, colors=C.planes_from_values(vals, W, H), depths=C.depths_from_mask(mask, W, H))
    views = scene.make_views(4, W, H, seed=3, with_best_cost=True)
    d.update(views=views, fused_colors=scene.make_colors(4, W, H, seed=5), thresholded=np.where(views.best_cost > THRESHOLD, -1.0, views.depth))
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def _add(c, lo, hi, with_depth):
    d = _data()
    c.add_views(d["colors"][lo:hi], d["eye"][lo:hi], d["eye"][lo:hi], depths=d["depths"][lo:hi] if with_depth else None)


def _load_nine(c):
    c.clear_views()
    _add(c, 0, 5, False)
    _add(c, 5, 9, True)   # the stage buffer grows
    c.set_depth_test(False)


def step1(c, _mesh):
    d, out = _data(), {}
    _load_nine(c)
    c.set_scratch_budget(SMALL_BUDGET)
    for reorder in (False, True):
        c.set_vertex_reorder(reorder)
        out["1 five chunks, reorder " + str(reorder)] = c.process(d["points"])
    c.set_vertex_reorder(False)
    return out


def step2(c, _mesh, fresh=False):
    d = _data()
    if fresh:
        _load_nine(c)
    c.set_scratch_budget(1 << 30)
    return {"2 300 vertices": c.process(d["points"][:300]), "2 all vertices again": c.process(d["points"])}


def step3(c, _mesh):
    d, out = _data(), {}
    c.clear_views()
    _add(c, 0, 17, True)
    c.set_depth_test(True, 0.0)
    out["3 uploaded depths"] = c.process(d["points"])
    c.set_render_queue_capacity(1)
    c.render_depths(*OCTAHEDRON)
    assert c.render_queued_pairs() > 1    # more large pairs than the queue started with: it grew inside the call
    out["3 rendered planes"] = (c.download_depths(),)
    c.set_depth_test(True, RENDER_TOL)
    out["3 rendered depths"] = c.process(d["points"])
    return out


def step4(c, _mesh):
    c.clear_views()
    _add(c, 0, 3, False)
    c.render_depths(*OCTAHEDRON)
    return {"4 planes 1 and 2": (c.download_depths(1, 2),)}


def step5(c, mesh):
    d, out = _data(), {}
    ctx, v = mesh
    c.clear_views()
    c.add_views(d["fused_colors"], d["views"].K4, d["views"].RT4)
    c.set_depth_test(False)
    for name, tol in (("5 fused test", FUSED_TOL), ("5 no test", None)):
        assert ctx.color_isosurface(c, fused_depth_tolerance=tol) == len(v)
        out[name] = ctx.download_isosurface_colors()
    return out


STEPS = (step1, step2, step3, step4, step5)


def _restatements(v):
    """label -> expected arrays, in plain numpy"""
    d = _data()
    nine = C.expected_from_values(d["vals"][:9])
    planes = MD.to_vtk_depths(MD.render_depths_np(*OCTAHEDRON, d["eye"], d["eye"], W, H))
    want = {"1 five chunks, reorder False": nine, "1 five chunks, reorder True": nine, "2 all vertices again": nine,
            "2 300 vertices": C.expected_from_values(d["vals"][:9, :300]),
            "3 uploaded depths": C.expected_from_values(d["vals"], d["mask"]),
            "3 rendered planes": (planes,),
            "3 rendered depths": CD.color_mesh_depth_np(d["points"], d["colors"], planes, d["eye"], d["eye"], RENDER_TOL),
            "4 planes 1 and 2": (planes[1:3],),
            "5 fused test": CD.color_mesh_depth_np(v, d["fused_colors"], d["thresholded"], d["views"].K4, d["views"].RT4, FUSED_TOL),
            "5 no test": CD.color_mesh_depth_np(v, d["fused_colors"], None, d["views"].K4, d["views"].RT4, None)}
    seen = want["3 rendered depths"][2]
    assert (seen > 0).any() and (seen == 0).any() and (planes > 0).any() and (planes == -1.0).any()   # not vacuous
    assert (want["5 fused test"][2] > 0).any() and (want["5 fused test"][2] < want["5 no test"][2]).any()
    return want


def _assert_same(got, want, what):
    assert len(got) == len(want), what
    for q, (a, b) in enumerate(zip(got, want)):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, q, int((a != b).sum()) if a.shape == b.shape else None)


@pytest.mark.gpu
def test_a_reused_context_returns_what_fresh_contexts_return():
    d = _data()
    grid = scene.default_grid(16)
    ctx = capi.FusionContext(grid, scene.default_ray_potential(grid))
    with ctx:
        ctx.add_views(d["views"], threshold=THRESHOLD)
        ctx.fuse()
        ctx.synchronize()
        v = ctx.extract_isosurface(ISO)[0]
        assert len(v) >= 64   # the in-place form takes its order-of-work sample
        mesh = (ctx, v)
        want = _restatements(v)
        fresh = {}
        for step in STEPS:
            with capi.ColorContext() as f:
                fresh.update(step(f, mesh, fresh=True) if step is step2 else step(f, mesh))
        assert sorted(fresh) == sorted(want)
        for label in want:
            _assert_same(fresh[label], want[label], ("fresh context against the restatement", label))
        with capi.ColorContext() as c:
            for round_ in (1, 2):
                for step in STEPS:
                    for label, got in step(c, mesh).items():
                        _assert_same(got, fresh[label], ("round", round_, "against a fresh context", label))
                        _assert_same(got, want[label], ("round", round_, "against the restatement", label))
