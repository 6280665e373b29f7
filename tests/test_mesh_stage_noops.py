"""The calls of the mesh stages that have nothing to do, on the device: a stage on an empty mesh, smooth_isosurface(0), a fill below
three edges and a fill of a closed mesh leave the stage's kernel time and every pass time at exactly 0.0 -- after a call that left
them above 0 -- and the mesh's regions, support counts and colours as the drop table of csrc/dmi_mesh_stage.h says, row by row; a
support call with min_views 0 has one pass, the other two are exactly 0.0.  The scene is that of tests/test_mesh_sequence_model.py:
an 8^3 grid, two views of 24 x 18."""
import numpy as np
import pytest

from cudadepthmapintegration_amd import capi, scene

pytestmark = pytest.mark.gpu

Z, Y, X = np.mgrid[0:8, 0:8, 0:8].astype(np.float64)
CLOSED = 2.6 - np.sqrt((X - 3.4) ** 2 + (Y - 3.6) ** 2 + (Z - 3.5) ** 2)   # a sphere inside the grid
OPEN = 6.6 - np.sqrt((X - 3.4) ** 2 + (Y - 3.6) ** 2 + (Z + 3.0) ** 2)     # a cap that leaves it: one rim
ABOVE = float(max(CLOSED.max(), OPEN.max())) + 1.0                         # an iso-value with an empty surface


@pytest.fixture(scope="module")
def contexts():
    grid = scene.default_grid(8)
    views = scene.make_views(2, 24, 18, seed=2, with_best_cost=True)
    with capi.FusionContext(grid, scene.default_ray_potential(grid)) as ctx, capi.ColorContext() as color:
        ctx.add_views(views, 0.8)
        color.add_views(scene.make_colors(2, 24, 18, seed=4), views.K4, views.RT4)
        yield ctx, color


def _everything(ctx, color):
    ctx.filter_isosurface_components("min_triangles", 0)
    ctx.filter_isosurface_support(0, 0.5, True)
    ctx.color_isosurface(color)
    assert _has(ctx) == (True, True, True)


def _has(ctx):
    """(regions, support counts, colours) are the mesh's: their downloads are not refused"""
    out = []
    for download in (ctx.download_isosurface_regions, ctx.download_isosurface_support, ctx.download_isosurface_colors):
        try:
            download()
            out.append(True)
        except capi.DmiError as e:
            assert e.code == 1, e
            out.append(False)
    return tuple(out)


def _snapshot(ctx):
    parts = ctx.download_isosurface() + (ctx.download_isosurface_normals(),) + ctx.download_isosurface_regions() + \
        (ctx.download_isosurface_support(),) + ctx.download_isosurface_colors()
    return [a.tobytes() for a in parts]


def _times_of(ctx, stage):
    return getattr(ctx, f"isosurface_{stage}_kernel_ms")(), getattr(ctx, f"isosurface_{stage}_pass_ms")()


def _exactly_zero(ctx, stage):
    ms, passes = _times_of(ctx, stage)
    bits = np.array([ms] + list(passes.values())).view(np.uint64)
    assert (bits == 0).all(), (stage, ms, passes)   # +0.0, every one


# stage -> (its getters' name, the call, what an empty mesh keeps of (regions, support counts, colours)): the rows kComponents,
# kSmoothing, nothing (iterations 0), kDecimation twice, nothing (the fill), nothing (the support call, whose counts are the result)
STAGES = {
    "components": ("filter", lambda c: c.filter_isosurface_components("min_triangles", 0), (True, False, False)),
    "smooth": ("smooth", lambda c: c.smooth_isosurface(2), (True, False, False)),
    "smooth 0": ("smooth", lambda c: c.smooth_isosurface(0), (True, True, True)),
    "decimate": ("decimate", lambda c: c.decimate_isosurface(0.3), (False, False, False)),
    "decimate quadric": ("decimate", lambda c: c.decimate_isosurface(0.3, "quadric"), (False, False, False)),
    "fill": ("holes", lambda c: c.fill_isosurface_holes(65536), (True, True, True)),
    "support": ("support", lambda c: c.filter_isosurface_support(1, 0.5, True), (True, True, True)),
    "support 0": ("support", lambda c: c.filter_isosurface_support(0, 0.5, True), (True, True, True)),
}


@pytest.mark.parametrize("name", list(STAGES))
def test_a_stage_on_an_empty_mesh_takes_no_time_and_drops_its_row(contexts, name):
    ctx, color = contexts
    getters, call, kept = STAGES[name]
    ctx.upload_grid(OPEN)
    assert ctx.extract_isosurface_with_normals(0.0)[0].shape[0] > 50
    (ctx.smooth_isosurface(2) if name == "smooth 0" else call(ctx))
    assert _times_of(ctx, getters)[0] > 0.0                      # a call that worked: the times are there to be zeroed
    assert ctx.extract_isosurface_with_normals(ABOVE)[0].shape[0] == 0
    _everything(ctx, color)
    call(ctx)
    _exactly_zero(ctx, getters)
    assert _has(ctx) == kept, name
    assert [len(a) for a in ctx.download_isosurface()] == [0, 0] and len(ctx.download_isosurface_normals()) == 0


def test_smoothing_zero_times_takes_no_time_and_keeps_everything(contexts):
    ctx, color = contexts
    ctx.upload_grid(CLOSED)
    ctx.extract_isosurface_with_normals(0.0)
    ctx.smooth_isosurface(2)
    assert ctx.isosurface_smooth_kernel_ms() > 0.0
    _everything(ctx, color)
    before = _snapshot(ctx)
    ctx.smooth_isosurface(0)
    _exactly_zero(ctx, "smooth")
    assert _has(ctx) == (True, True, True) and _snapshot(ctx) == before


@pytest.mark.parametrize("field, max_edges", [(OPEN, 2), (OPEN, 0), (CLOSED, 65536)], ids=["below three edges", "no edges", "a closed mesh"])
def test_a_fill_that_fills_nothing_takes_no_time_and_keeps_everything(contexts, field, max_edges):
    ctx, color = contexts
    ctx.upload_grid(OPEN)
    nv = ctx.extract_isosurface_with_normals(0.0)[0].shape[0]
    filled = ctx.fill_isosurface_holes(65536)
    assert (filled[0], filled[2]) == (nv + 1, 1) and ctx.isosurface_holes_kernel_ms() > 0.0
    ctx.upload_grid(field)
    verts, tris, _ = ctx.extract_isosurface_with_normals(0.0)
    _everything(ctx, color)
    before = _snapshot(ctx)
    got = ctx.fill_isosurface_holes(max_edges)
    assert got[:3] == (len(verts), len(tris), 0) and (got[3] > 4) == (field is OPEN)
    _exactly_zero(ctx, "holes")
    assert _has(ctx) == (True, True, True) and _snapshot(ctx) == before


def test_a_support_call_without_a_trim_has_one_pass(contexts):
    ctx, color = contexts
    ctx.upload_grid(CLOSED)
    nv = ctx.extract_isosurface_with_normals(0.0)[0].shape[0]
    assert 0 < ctx.filter_isosurface_support(1, 0.5, True)[0] < nv
    assert all(ms > 0.0 for ms in ctx.isosurface_support_pass_ms().values())
    left = ctx.download_isosurface()[0].shape[0]
    assert ctx.filter_isosurface_support(0, 0.5, True)[0] == left
    ms, passes = _times_of(ctx, "support")
    assert ms > 0.0 and passes["counts"] > 0.0
    assert np.array([passes["scans"], passes["compaction"]]).view(np.uint64).tolist() == [0, 0]
