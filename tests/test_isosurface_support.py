"""dmi_filter_isosurface_support: the mesh a fusion context holds, trimmed by view support where it is.

The scene is test_isosurface_coloration.py's: a 32^3-cell grid around the sphere of scene.py, 6 views of 96 x 72 with uniform best
costs of which the threshold 0.8 removes a scattered fifth.  The iso-value 0 gives the sphere's front, the back shell delta behind
it and the sheets where seen space meets unseen space (7044 vertices, more than half of them near no view's kept depth); the
iso-value 1 mostly the surface.

On the CPU: the ABI, the command line's usage errors, and the scene's conditions from the oracle's fusion, isosurface_normals_np and
isosurface_support_np, so that the GPU tests cannot pass vacuously.  On the GPU: counts and trimmed meshes against the restatement,
bit for bit, on f32 and f64 depth stores; a tolerance tie; 70 views (several view groups of the counting kernel); after the
component filter, the smoother and the decimation; the life cycle; the command line end to end."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import isosurface_normals_np as N
import isosurface_support_np as S
from cudadepthmapintegration_amd import capi, scene
from oracle import oracle_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT, STATE = 1, 4   # DMI_ERR_INVALID_ARGUMENT, DMI_ERR_STATE (include/dmi.h)
N_VIEWS, W, H = 6, 96, 72
THRESHOLD = 0.8                  # of the uniform best costs: a scattered fifth of the pixels goes
TOLERANCE = 0.1                  # 1.6 voxels of 2 / 32

NEW_SYMBOLS = ["dmi_filter_isosurface_support", "dmi_download_isosurface_support", "dmi_get_isosurface_support_kernel_ms",
               "dmi_get_isosurface_support_pass_ms"]


def test_abi_has_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "dmi.h")).read()
    assert "DMI_ERR_INVALID_ARGUMENT = 1," in header and "DMI_ERR_STATE = 4" in header
    lib = ctypes.CDLL(capi.load()._name)
    for name in NEW_SYMBOLS:
        assert name + "(" in header and name in capi.ABI_SYMBOLS and hasattr(lib, name), name
    assert lib.dmi_abi_version() == 5 and "#define DMI_ABI_VERSION 5 " in header
    for name in ("filter_isosurface_support", "download_isosurface_support", "isosurface_support_kernel_ms"):
        assert callable(getattr(capi.FusionContext, name)), name
    # null arguments are refused without a device, and the message names the entry point
    L = capi.load()
    n = ctypes.c_uint64(0)
    assert L.dmi_filter_isosurface_support(None, 1, 0.1, 0, ctypes.byref(n), ctypes.byref(n)) == INVALID_ARGUMENT
    assert "dmi_filter_isosurface_support" in L.dmi_last_error(None).decode()
    assert L.dmi_download_isosurface_support(None, None) == INVALID_ARGUMENT
    assert "dmi_download_isosurface_support" in L.dmi_last_error(None).decode()
    assert L.dmi_get_isosurface_support_kernel_ms(None, None) == INVALID_ARGUMENT
    assert "dmi_get_isosurface_support_kernel_ms" in L.dmi_last_error(None).decode()
    assert L.dmi_get_isosurface_support_pass_ms(None, None) == INVALID_ARGUMENT
    assert "dmi_get_isosurface_support_pass_ms" in L.dmi_last_error(None).decode()


@functools.lru_cache(maxsize=None)
def _scene(exact_f32=True):
    """(grid, ray, views, thresholded depths); exact_f32 False: one depth of view 0 is not an f32 (the store goes f64)."""
    grid = scene.default_grid(32)
    ray = scene.default_ray_potential(grid)
    views = scene.make_views(N_VIEWS, W, H, seed=3, with_best_cost=True)
    if not exact_f32:
        row, col = np.argwhere((views.depth[0] > 0) & (views.best_cost[0] <= THRESHOLD))[0]
        views.depth[0, row, col] += 2.0 ** -40
        assert np.float64(np.float32(views.depth[0, row, col])) != views.depth[0, row, col]
    thresholded = np.where(views.best_cost > THRESHOLD, -1.0, views.depth)
    for a in (views.depth, views.best_cost, views.K4, views.RT4, thresholded):
        a.setflags(write=False)
    return grid, ray, views, thresholded


@functools.lru_cache(maxsize=None)
def _cpu_mesh(iso):
    """(vertices, triangles, normals) of the scene's oracle fusion at `iso`, by the numpy restatements."""
    grid, ray, views, thresholded = _scene()
    cells, _, _ = oracle_np.fuse(grid.cell_dims, grid.origin, grid.spacing, grid.grid_matrix, ray.thickness, ray.rho, ray.eta, ray.delta,
                                 thresholded, views.K4, views.RT4)
    v, t, n = N.extract_with_normals(oracle_np.cell_to_point_np(cells), iso, grid.origin, grid.spacing, np.asarray(grid.grid_matrix))
    for a in (v, t, n):
        a.setflags(write=False)
    return v, t, n


def _counts(v, n, tol=TOLERANCE, facing=True, exact_f32=True, depths=None):
    _, _, views, thresholded = _scene(exact_f32)
    return S.support(v, n, thresholded if depths is None else depths, views.K4, views.RT4, tol, facing)


MANY_VIEWS, MANY_ISO = 70, 12.0   # 70 views sum to a field whose contour at 12 lies on the sphere (at 0 it is far outside it)


@functools.lru_cache(maxsize=None)
def _many_views_scene():
    """(grid, ray, views, thresholded depths): a 16^3 grid and 70 views of 48 x 36, for the view groups of the counting kernel."""
    grid = scene.default_grid(16)
    ray = scene.default_ray_potential(grid)
    views = scene.make_views(MANY_VIEWS, 48, 36, seed=11, with_best_cost=True)
    thresholded = np.where(views.best_cost > THRESHOLD, -1.0, views.depth)
    for a in (views.depth, views.best_cost, views.K4, views.RT4, thresholded):
        a.setflags(write=False)
    return grid, ray, views, thresholded


def test_many_views_scene_conditions_hold_on_the_cpu():
    grid, ray, views, thresholded = _many_views_scene()
    cells, _, _ = oracle_np.fuse(grid.cell_dims, grid.origin, grid.spacing, grid.grid_matrix, ray.thickness, ray.rho, ray.eta, ray.delta,
                                 thresholded, views.K4, views.RT4)
    v, t, n = N.extract_with_normals(oracle_np.cell_to_point_np(cells), MANY_ISO, grid.origin, grid.spacing, np.asarray(grid.grid_matrix))
    assert 256 < len(v) < 20000
    for facing in (True, False):
        supports = S.pair_table(v, n, thresholded, views.K4, views.RT4, TOLERANCE, facing)[0]
        counts = supports.sum(axis=0)
        assert counts.max() > 1 and (counts == 0).sum() > 100 and (counts > 0).sum() > 100
        seen = supports.any(axis=1)
        assert seen[:32].any() and seen[32:64].any() and seen[64:].any()
        assert len(set(np.nonzero(seen)[0] // 8)) == 9            # every group of eight views supports something


def test_scene_conditions_hold_on_the_cpu():
    _, _, views, thresholded = _scene()
    v0, t0, n0 = _cpu_mesh(0.0)
    v1, t1, n1 = _cpu_mesh(1.0)
    assert len(v0) == 7044 and len(v0) % 256 != 0
    s0 = _counts(v0, n0)
    s1 = _counts(v1, n1)
    assert (s0 == 0).sum() == 5797 > len(v0) / 2                  # iso 0: most of the contour is no surface anybody saw
    assert len(v1) == 1790 and (s1 == 0).sum() == 155 < len(v1) / 5   # iso 1: mostly the surface
    keep = (s0[t0] >= 1).all(axis=1)
    assert keep.any() and not keep.all()
    mixed = (s0[t0] >= 1).any(axis=1) & ~keep                     # triangles across the boundary of the support
    assert mixed.sum() == 1992
    named = np.zeros(len(v0), dtype=bool)
    named[t0[keep].reshape(-1)] = True
    assert ((s0 >= 1) & ~named).sum() == 61                       # supported, but named by no surviving triangle: they go too
    fv, ft, fn = S.filter_mesh(v0, t0, n0, s0, 1)
    assert len(fv) == named.sum() and len(ft) == keep.sum() and len(fn) == len(fv)
    assert (_counts(v1, n1, facing=False) != s1).any()            # the facing test rejects pairs the depth test accepts
    for v, n in ((v0, n0), (v1, n1)):
        supports, _, s = S.pair_table(v, n, thresholded, views.K4, views.RT4, TOLERANCE, True)
        assert supports.any() and not (s[supports] == 0).any()
        unfaced = S.pair_table(v, n, thresholded, views.K4, views.RT4, TOLERANCE, False)[0]
        assert not (s[unfaced] == 0).any()                        # no pair the other tests accept sits on the facing test's edge
    # the filter is idempotent: the counts depend only on position and normal
    again = _counts(fv, fn)
    assert np.array_equal(again, s0[named])
    v2, t2, _ = S.filter_mesh(fv, ft, fn, again, 1)
    assert v2.tobytes() == fv.tobytes() and np.array_equal(t2, ft)


BASE = ["--gridOrigin", "-2.29", "-2.24", "-2.2", "--gridEnd", "1.19", "1.67", "1.22", "--dataFolder", "data",
        "--outputGridFilename", "out.vts", "--outputMeshFilename", "mesh.vtp", "--rayThick", "0.1", "--gridDims", "10"]


def _usage_error(flags):
    r = subprocess.run([capi.cli_binary()] + BASE + flags, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, (flags, r.stderr)
    return r.stderr


def test_cli_support_flags():
    assert "--meshMinSupportViews needs --meshSupportDepthTolerance" in _usage_error(["--extractMesh", "--meshMinSupportViews", "1"])
    assert "--meshSupportArray needs --meshSupportDepthTolerance" in _usage_error(["--extractMesh", "--meshSupportArray"])
    assert "--meshMinSupportViews needs --extractMesh" in _usage_error(["--meshMinSupportViews", "1", "--meshSupportDepthTolerance", "0.1"])
    assert "--meshSupportArray needs --extractMesh" in _usage_error(["--meshSupportArray", "--meshSupportDepthTolerance", "0.1"])
    assert "--meshSupportDepthTolerance needs --meshMinSupportViews or --meshSupportArray" in \
        _usage_error(["--extractMesh", "--meshSupportDepthTolerance", "0.1"])
    assert "--meshSupportNoFacing needs --meshMinSupportViews or --meshSupportArray" in _usage_error(["--extractMesh", "--meshSupportNoFacing"])
    assert "takes one --device" in _usage_error(["--extractMesh", "--meshMinSupportViews", "1", "--meshSupportDepthTolerance", "0.1",
                                                 "--device", "0", "1"])
    for value in ("-1", "1.5", "x", ""):
        assert "Bad value for --meshMinSupportViews" in _usage_error(["--extractMesh", "--meshMinSupportViews", value])
    for value in ("-1", "nan", "inf", "x", ""):
        assert "Bad value for --meshSupportDepthTolerance" in _usage_error(["--extractMesh", "--meshSupportDepthTolerance", value])
    text = _usage_error(["--help"])
    for flag in ("--meshMinSupportViews v", "--meshSupportDepthTolerance v", "--meshSupportNoFacing\n", "--meshSupportArray\n"):
        assert flag in text and "not in the reference" in text.split(flag)[1].split("--help")[0], flag


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _fusion_context(iso=0.0, exact_f32=True, depth_storage="auto", normals=True):
    """The scene fused and its iso-surface extracted: (context, vertices, triangles, normals or None)."""
    grid, ray, views, _ = _scene(exact_f32)
    ctx = capi.FusionContext(grid, ray, depth_storage=depth_storage)
    ctx.add_views(views, threshold=THRESHOLD)
    ctx.fuse()
    ctx.synchronize()
    if normals:
        v, t, n = ctx.extract_isosurface_with_normals(iso)
    else:
        (v, t), n = ctx.extract_isosurface(iso), None
    return ctx, v, t, n


@pytest.mark.gpu
@pytest.mark.parametrize("store", ["f32", "f64"])
@pytest.mark.parametrize("facing", [True, False])
@pytest.mark.parametrize("iso", [0.0, 1.0])
def test_counts_are_the_restatement(iso, facing, store):
    exact = store == "f32"
    ctx, v, t, n = _fusion_context(iso, exact_f32=exact)
    with ctx:
        assert ctx.info().depth_storage_in_use == (capi.DMI_DEPTH_F32 if exact else capi.DMI_DEPTH_F64)
        cv, ct, cn = _cpu_mesh(iso)
        if exact:                                   # the mesh is the restatements' own (the scene's conditions are about it)
            assert _same_bits(v, cv) and _same_bits(t, ct) and _same_bits(n, cn)
        assert ctx.filter_isosurface_support(0, TOLERANCE, facing) == (len(v), len(t))
        got = ctx.download_isosurface_support()
        want = _counts(v, n, facing=facing, exact_f32=exact)
        print(f"iso {iso} facing {facing} {store}: {len(v)} vertices, counts {np.bincount(got, minlength=N_VIEWS + 1).tolist()}, "
              f"{ctx.isosurface_support_kernel_ms():.3f} ms")
        assert got.dtype == np.int32 and _same_bits(got, want), int((got != want).sum())
        assert (got > 0).any() and (got == 0).any() and ctx.isosurface_support_kernel_ms() > 0.0
        passes = ctx.isosurface_support_pass_ms()
        assert passes["counts"] > 0.0 and passes["scans"] == 0.0 and passes["compaction"] == 0.0
        v1, t1 = ctx.download_isosurface()          # min_views 0 leaves the mesh untouched
        assert _same_bits(v1, v) and _same_bits(t1, t) and _same_bits(ctx.download_isosurface_normals(), n)


@pytest.mark.gpu
def test_forced_f32_store_tests_against_the_rounded_depth():
    ctx, v, t, n = _fusion_context(0.0, exact_f32=False, depth_storage="f32")
    with ctx:
        assert ctx.info().depth_storage_in_use == capi.DMI_DEPTH_F32
        thresholded = _scene(False)[3]
        rounded = thresholded.astype(np.float32).astype(np.float64)
        assert (rounded != thresholded).sum() == 1
        ctx.filter_isosurface_support(0, TOLERANCE)
        assert _same_bits(ctx.download_isosurface_support(), _counts(v, n, exact_f32=False, depths=rounded))


@pytest.mark.gpu
@pytest.mark.parametrize("normals", [True, False])
@pytest.mark.parametrize("min_views", [0, 1, 2, 7])
def test_trimmed_mesh_is_the_restatement(min_views, normals):
    ctx, v, t, n = _fusion_context(0.0, normals=normals)
    with ctx:
        counts = _counts(v, n, facing=normals)
        wv, wt, wn = S.filter_mesh(v, t, n, counts, min_views)
        got = ctx.filter_isosurface_support(min_views, TOLERANCE, facing=normals)
        assert got == (len(wv), len(wt)), (got, len(wv), len(wt))
        gv, gt = ctx.download_isosurface()
        assert _same_bits(gv, wv) and _same_bits(gt, wt)
        if normals:
            assert _same_bits(ctx.download_isosurface_normals(), wn)
        print(f"min_views {min_views}: {len(v)} -> {len(gv)} vertices, {len(t)} -> {len(gt)} triangles, passes {ctx.isosurface_support_pass_ms()}")
        if min_views == 0:
            assert _same_bits(gv, v) and _same_bits(gt, t)
            assert _same_bits(ctx.download_isosurface_support(), counts)
        elif min_views == 7:                        # more than there are views
            assert got == (0, 0) and len(ctx.download_isosurface_support()) == 0
        else:
            assert 0 < len(gv) < len(v) and 0 < len(gt) < len(t)
            kept = np.zeros(len(v), dtype=bool)
            kept[t[(counts[t] >= min_views).all(axis=1)].reshape(-1)] = True
            assert _same_bits(ctx.download_isosurface_support(), counts[kept])   # the counts of the mesh as the call left it
            assert (ctx.download_isosurface_support() >= min_views).all()
            # a second identical call changes nothing
            assert ctx.filter_isosurface_support(min_views, TOLERANCE, facing=normals) == got
            v2, t2 = ctx.download_isosurface()
            assert _same_bits(v2, gv) and _same_bits(t2, gt) and _same_bits(ctx.download_isosurface_support(), counts[kept])


@pytest.mark.gpu
def test_tolerance_tie():
    ctx, v, t, n = _fusion_context(1.0)
    _, _, views, thresholded = _scene()
    with ctx:
        supports, gap, _ = S.pair_table(v, n, thresholded, views.K4, views.RT4, TOLERANCE, True)
        m, i = np.unravel_index(np.argmax(np.where(supports, gap, -1.0)), gap.shape)   # the supporting pair with the widest gap
        tie = float(gap[m, i])
        assert supports[m, i] and 0.0 < tie <= TOLERANCE
        below = float(np.nextafter(tie, 0.0))
        at, under = _counts(v, n, tol=tie), _counts(v, n, tol=below)
        assert at[i] == under[i] + 1                # the pair counts at its own gap and not a bit below
        ctx.filter_isosurface_support(0, tie)
        assert _same_bits(ctx.download_isosurface_support(), at)
        ctx.filter_isosurface_support(0, below)
        assert _same_bits(ctx.download_isosurface_support(), under)
        ctx.filter_isosurface_support(0, 0.0)       # a zero tolerance is accepted
        assert _same_bits(ctx.download_isosurface_support(), _counts(v, n, tol=0.0))


@pytest.mark.gpu
@pytest.mark.parametrize("facing", [True, False])
def test_seventy_views_cross_every_view_group(facing):
    grid, ray, views, thresholded = _many_views_scene()
    with capi.FusionContext(grid, ray) as ctx:
        ctx.add_views(views, threshold=THRESHOLD)
        ctx.fuse()
        ctx.synchronize()
        v, t, n = ctx.extract_isosurface_with_normals(MANY_ISO)
        assert 256 < len(v) < 20000                  # more than one block, far fewer than fill the chip: the views are split
        assert ctx.filter_isosurface_support(0, TOLERANCE, facing) == (len(v), len(t))
        got = ctx.download_isosurface_support()
        supports = S.pair_table(v, n, thresholded, views.K4, views.RT4, TOLERANCE, facing)[0]
        want = supports.sum(axis=0).astype(np.int32)
        print(f"70 views, facing {facing}: {len(v)} vertices, counts {np.bincount(got).tolist()}, {ctx.isosurface_support_kernel_ms():.3f} ms")
        assert _same_bits(got, want), int((got != want).sum())
        assert got.max() > 1 and (got == 0).any()
        seen = supports.any(axis=1)                  # views that support some vertex: below 32, between 32 and 64, and the tail
        assert seen[:32].any() and seen[32:64].any() and seen[64:].any()
        # the filter reads the counts the groups have added up
        wv, wt, wn = S.filter_mesh(v, t, n, want, 1)
        assert ctx.filter_isosurface_support(1, TOLERANCE, facing) == (len(wv), len(wt)) and 0 < len(wv) < len(v)
        gv, gt = ctx.download_isosurface()
        assert _same_bits(gv, wv) and _same_bits(gt, wt) and _same_bits(ctx.download_isosurface_normals(), wn)


@pytest.mark.gpu
def test_counts_after_filter_smoothing_and_decimation():
    ctx, v, t, n = _fusion_context(0.0)
    with ctx:
        def check(step):
            v1, t1 = ctx.download_isosurface()
            n1 = ctx.download_isosurface_normals()
            assert ctx.filter_isosurface_support(0, TOLERANCE) == (len(v1), len(t1))
            got = ctx.download_isosurface_support()
            assert _same_bits(got, _counts(v1, n1)), step
            assert (got > 0).any() and (got == 0).any(), step
            return v1
        nv = ctx.filter_isosurface_components("min_triangles", 50)[0]
        assert 0 < nv < len(v)
        check("filter")
        ctx.smooth_isosurface(3)
        assert len(check("smooth")) == nv
        nv2, _ = ctx.decimate_isosurface(1.5 * 2.0 / 32)             # its normals kernel is still queued when the counting starts
        assert 0 < nv2 == len(check("decimate")) < nv
        # ... and a trim of that mesh is the restatement's
        v1, t1 = ctx.download_isosurface()
        n1 = ctx.download_isosurface_normals()
        wv, wt, wn = S.filter_mesh(v1, t1, n1, _counts(v1, n1), 1)
        assert ctx.filter_isosurface_support(1, TOLERANCE) == (len(wv), len(wt))
        gv, gt = ctx.download_isosurface()
        assert _same_bits(gv, wv) and _same_bits(gt, wt) and _same_bits(ctx.download_isosurface_normals(), wn)


def _refused(call, text, code=INVALID_ARGUMENT):
    with pytest.raises(capi.DmiError) as e:
        call()
    assert e.value.code == code and text in str(e.value), str(e.value)


@pytest.mark.gpu
def test_life_cycle_of_the_counts():
    grid, ray, views, _ = _scene()
    with capi.FusionContext(grid, ray) as bare:
        _refused(lambda: bare.filter_isosurface_support(1, TOLERANCE, facing=False), "no mesh")
        bare.upload_grid(np.zeros(grid.cell_dims[::-1]))
        bare.extract_isosurface(0.5)
        _refused(lambda: bare.filter_isosurface_support(1, TOLERANCE, facing=False), "no views", STATE)
    ctx, v, t, n = _fusion_context(0.0)
    with ctx, capi.ColorContext() as c:
        c.add_views(scene.make_colors(N_VIEWS, W, H, seed=5), views.K4, views.RT4)
        _refused(ctx.download_isosurface_support, "dmi_download_isosurface_support")          # before any support call
        steps = {"extraction": lambda: ctx.extract_isosurface_with_normals(0.0),
                 "filter": lambda: ctx.filter_isosurface_components("min_triangles", 0),
                 "smooth": lambda: ctx.smooth_isosurface(1), "decimate": lambda: ctx.decimate_isosurface(2.0 / 32)}
        for name, step in steps.items():
            ctx.filter_isosurface_support(0, TOLERANCE)
            ctx.download_isosurface_support()
            step()
            _refused(ctx.download_isosurface_support, "dmi_download_isosurface_support")
        ctx.extract_isosurface_with_normals(0.0)
        ctx.filter_isosurface_support(0, TOLERANCE)
        counts = ctx.download_isosurface_support()
        ctx.smooth_isosurface(0)                                      # nothing to do: the counts stay
        assert _same_bits(ctx.download_isosurface_support(), counts)
        # a counts-only call keeps regions and colours; a trim that removes something drops both
        ctx.filter_isosurface_components("min_triangles", 0)
        ctx.color_isosurface(c)
        ctx.filter_isosurface_support(0, TOLERANCE)
        ctx.download_isosurface_regions()
        ctx.download_isosurface_colors()
        nv, nt = ctx.filter_isosurface_support(1, TOLERANCE)
        assert 0 < nv < len(v)
        _refused(ctx.download_isosurface_regions, "dmi_download_isosurface_regions")
        _refused(ctx.download_isosurface_colors, "dmi_download_isosurface_colors")
        ctx.filter_isosurface_components("min_triangles", 0)          # a component filter runs again: the regions are back
        assert len(ctx.download_isosurface_regions()[0]) == nv
        # an empty mesh is a success
        ev, et, en = ctx.extract_isosurface_with_normals(1e30)
        assert len(ev) == 0 and ctx.filter_isosurface_support(1, TOLERANCE) == (0, 0)
        assert len(ctx.download_isosurface_support()) == 0 and ctx.isosurface_support_kernel_ms() == 0.0


@pytest.mark.gpu
def test_refusals_leave_mesh_and_counts_as_they_were():
    L = capi.load()
    ctx, v, t, _ = _fusion_context(0.0, normals=False)
    n = ctypes.c_uint64(0)
    with ctx:
        ctx.filter_isosurface_support(0, TOLERANCE, facing=False)
        first = ctx.download_isosurface_support()

        def refused(call, text):
            _refused(call, text)
            v1, t1 = ctx.download_isosurface()
            assert _same_bits(v1, v) and _same_bits(t1, t) and _same_bits(ctx.download_isosurface_support(), first)

        refused(lambda: ctx.filter_isosurface_support(1, TOLERANCE, facing=True), "normals")    # the mesh has none
        for tol in (-1.0, float("nan"), float("inf")):
            refused(lambda: ctx.filter_isosurface_support(1, tol, facing=False), "tolerance")
        refused(lambda: ctx.filter_isosurface_support(-1, TOLERANCE, facing=False), "min_views")
        assert L.dmi_filter_isosurface_support(ctx._h, 1, TOLERANCE, 0, None, ctypes.byref(n)) == INVALID_ARGUMENT
        assert L.dmi_filter_isosurface_support(ctx._h, 1, TOLERANCE, 0, ctypes.byref(n), None) == INVALID_ARGUMENT
        assert L.dmi_download_isosurface_support(ctx._h, None) == INVALID_ARGUMENT
        assert _same_bits(ctx.download_isosurface_support(), first)
        ctx.clear_views()                                             # no resident views: a state error, the mesh stays
        _refused(lambda: ctx.filter_isosurface_support(1, TOLERANCE, facing=False), "no views", STATE)
        v1, t1 = ctx.download_isosurface()
        assert _same_bits(v1, v) and _same_bits(t1, t) and _same_bits(ctx.download_isosurface_support(), first)


# ---- the command line: --meshMinSupportViews, --meshSupportDepthTolerance, --meshSupportNoFacing, --meshSupportArray ---------------
def _reconstruct(tmp_path, lv, lk, name, extra):
    grid, ray, _, _ = _scene()
    end = [grid.origin[a] + (grid.cell_dims[a] + 1) * grid.spacing[a] for a in range(3)]
    args = [capi.cli_binary(), "--dataFolder", os.path.dirname(lv), "--depthMapFile", os.path.basename(lv), "--KRTFile", os.path.basename(lk),
            "--gridDims"] + [str(c + 1) for c in grid.cell_dims] + ["--gridOrigin"] + [repr(float(x)) for x in grid.origin] + \
           ["--gridEnd"] + [repr(float(x)) for x in end] + \
           ["--rayThick", repr(ray.thickness), "--rayRho", repr(ray.rho), "--rayEta", repr(ray.eta), "--rayDelta", repr(ray.delta),
            "--threshBestCost", repr(THRESHOLD), "--contour", "0.0", "--outputGridFilename", str(tmp_path / (name + ".vts")),
            "--outputMeshFilename", str(tmp_path / (name + ".vtp")), "--extractMesh"] + extra
    return subprocess.run(args, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)


@pytest.mark.gpu
def test_cli_trim_and_support_array_are_the_api_path(tmp_path):
    _, _, views, _ = _scene()
    data = tmp_path / "data"
    data.mkdir()
    lv, lk = scene.write_view_files(str(data), views)
    r = _reconstruct(tmp_path, lv, lk, "trimmed", ["--meshMinSupportViews", "1", "--meshSupportDepthTolerance", repr(TOLERANCE),
                                                    "--meshSupportArray"])
    assert r.returncode == 0, r.stderr + r.stdout
    mesh = capi.read_polydata(str(tmp_path / "trimmed.vtp"))
    ctx, v, t, _ = _fusion_context(0.0)
    with ctx:
        nv, nt = ctx.filter_isosurface_support(1, TOLERANCE)
        wv, wt = ctx.download_isosurface()
        ctx.filter_isosurface_support(0, TOLERANCE)
        counts = ctx.download_isosurface_support()
    assert 0 < nv < len(v) and _same_bits(mesh.points.reshape(-1, 3), wv)
    assert np.array_equal(np.asarray(mesh.connectivity).reshape(-1, 3), wt)
    assert list(mesh.point_data) == ["NbSupportingViews"]             # the normals served the facing test and are not written
    assert _same_bits(np.asarray(mesh.point_data["NbSupportingViews"]).reshape(-1), counts) and (counts >= 1).all()
    line = [x for x in r.stdout.splitlines() if x.startswith("mesh support:")]
    assert len(line) == 1 and f"at least 1 of {N_VIEWS} views" in line[0] and f"{len(v)} vertices" in line[0] and f"{nv} vertices" in line[0], r.stdout
    # the array alone, without the facing test: the whole mesh and its counts
    # (with the other arrays: behind RegionId)
    r = _reconstruct(tmp_path, lv, lk, "counted", ["--meshSupportDepthTolerance", repr(TOLERANCE), "--meshSupportArray", "--meshSupportNoFacing",
                                                    "--meshNormals", "--meshRegionIds"])
    assert r.returncode == 0 and "mesh support:" not in r.stdout, r.stderr + r.stdout
    whole = capi.read_polydata(str(tmp_path / "counted.vtp"))
    assert _same_bits(whole.points.reshape(-1, 3), v)
    assert list(whole.point_data) == ["Normals", "reconstruction_scalar", "RegionId", "NbSupportingViews"]
    ctx, v, t, n = _fusion_context(0.0)
    with ctx:
        ctx.filter_isosurface_support(0, TOLERANCE, facing=False)
        assert _same_bits(np.asarray(whole.point_data["NbSupportingViews"]).reshape(-1), ctx.download_isosurface_support())
    # omitting the tolerance is a usage error
    r = _reconstruct(tmp_path, lv, lk, "refused", ["--meshMinSupportViews", "1"])
    assert r.returncode != 0 and "--meshSupportDepthTolerance" in r.stderr and not os.path.exists(tmp_path / "refused.vtp")
