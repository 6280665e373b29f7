"""The value side of the fusion at exact threshold ties, on the device, bit for bit against the oracle.

The reference's strict compares (cu:105-120: |diff| > delta, |diff| > thick, diff > 0, diff != 0) are restated by the C++
column, the generated acc_potential_* asm of the ZF instantiations, fuse_kernel, the f32 and f64 depth instantiations, GENK and
ROT, class_from_bounds / border_class of the coarse and the fine pass, and the outward rounding of the f32 min/max pyramid.  The
scenes of tests/potential_tie_cases.py put diff exactly on 0, +-thick and +-delta on whole layers of voxels, at every alignment
to 8-bricks, 16-bricks, 32-boxes and the grid's ends (tests/test_potential_tie_cases.py proves that on the CPU, and that a `>=`
for a `>` changes the expected grids).  Every case here fuses such a scene through one form of the compares -- all views at
once, and group by group (a group's grid shows a one-ulp error that the sum of 76 views can round away) -- and names the form
in its assertion message; on a mismatch the views are fused one at a time and the first wrong voxel is reported as
(family, view, the view's depth layer, layer along the axis, voxel, expected, got)."""
import numpy as np
import pytest

import potential_tie_cases as tc
from cudadepthmapintegration_amd import capi
from helpers import bits_equal

pytestmark = pytest.mark.gpu

FX = capi.VARIANT_FIXED_TILE_SHAPE
TK8 = capi.VARIANT_TILE_SHAPE["tk8_w7_g8"]
# name -> (context arguments, fuse onto an uploaded grid)
PATHS = {
    "zero_grid": ({}, False),     # zero grid, no counters: the ZF instantiations and their acc_potential_*_f32 asm -- for pinhole
                                  # views and f32 depth tables; general K and f64 depth tables have no ZF instantiation
                                  # (launch_shape, fusion_tile.hip) and take the C++ column on this path too
    "counted": ({"count_hits": True}, False),                                # the C++ form of the column
    "uploaded_grid": ({}, True),                                             # the general non-ZF instantiations
    "uploaded_grid_counted": ({"count_hits": True}, True),
    "no_brick_classes": ({"kernel_variant": capi.VARIANT_NO_BRICK_CLASSES}, False),
    "general_kernel": ({"kernel_variant": capi.VARIANT_FORCE_GENERAL}, False),
    "general_kernel_counted": ({"kernel_variant": capi.VARIANT_FORCE_GENERAL, "count_hits": True}, True),
    "keep_behind_adds": ({"kernel_variant": capi.VARIANT_KEEP_BEHIND_ADDS}, False),
    "no_interior": ({"kernel_variant": capi.VARIANT_NO_INTERIOR}, False),
    "columns_16": ({"kernel_variant": FX}, False),
    "columns_8": ({"kernel_variant": TK8}, False),
    "columns_16_counted": ({"kernel_variant": FX, "count_hits": True}, False),
    "persistent_always": ({"kernel_variant": capi.VARIANT_PERSISTENT_ALWAYS}, False),
    "persistent_never": ({"kernel_variant": capi.VARIANT_PERSISTENT_NEVER}, False),
    "f64_depth": ({"depth_storage": "f64"}, False),
    "f64_depth_columns_16": ({"depth_storage": "f64", "kernel_variant": FX}, False),
    "f64_depth_uploaded_grid": ({"depth_storage": "f64"}, True),
    "windows_always": ({"kernel_variant": capi.VARIANT_WINDOWS_ALWAYS}, False),
    "windows_always_columns_16": ({"kernel_variant": capi.VARIANT_WINDOWS_ALWAYS | FX}, False),
    "no_windows": ({"kernel_variant": capi.VARIANT_NO_WINDOWS}, False),
}
FEW = ("zero_grid", "counted", "uploaded_grid", "no_brick_classes", "general_kernel", "columns_16", "f64_depth")
SCENES = [(f, g) for g in tc.GRIDS for f in tc.FAMILIES]


def _first_wrong_view(ctx, grid, rp, views, init, family, layers, path):
    """Fuses the views one at a time and describes the first voxel that differs from the oracle."""
    for m in range(views.n):
        ctx.upload_grid(init) if init is not None else ctx.reset_grid()
        ctx.fuse(m, 1)
        got = ctx.download_grid()
        want = tc.oracle_grid(grid, rp, views, m, 1, init=init, count_hits=False)[0]
        if not bits_equal(got, want):
            bad = ~((np.isnan(got) & np.isnan(want)) | (got.view(np.uint64) == want.view(np.uint64)))
            k, j, i = (int(x) for x in np.argwhere(bad)[0])
            return (f"path {path}, family {family}: view {m} (its depth lies in layer {layers[m] if layers else '?'}) is wrong in "
                    f"{np.count_nonzero(bad)} voxels, first at layer {(i, j, k)[tc.axis_of(family)]} along the axis, voxel (i, j, k) = "
                    f"{(i, j, k)}: expected {want[k, j, i]!r}, got {got[k, j, i]!r}")
    return f"path {path}, family {family}: every view alone equals the oracle; only their sum differs"


def _fuse_and_compare(family, grid, rp, views, want, path, layers=None, check=None):
    """One context of `path`: all views at once (grid, and hits when counted), then every group of tc.groups() alone when
    `want` has them.  `check(ctx)` runs after the fusion of all views."""
    kw, with_init = PATHS[path]
    init = tc.init_grid(grid.n_voxels) if with_init else None
    what = (path, family)
    with capi.FusionContext(grid, rp, **kw) as ctx:
        ctx.add_views(views)
        if init is not None:
            ctx.upload_grid(init)
        ctx.fuse()
        out = ctx.download_grid()
        if not bits_equal(out, want["all"][0]):
            pytest.fail(_first_wrong_view(ctx, grid, rp, views, init, family, layers, path))
        if kw.get("count_hits"):
            vh, mh = ctx.download_hits()
            assert np.array_equal(mh, want["all"][2]), what
            assert np.array_equal(vh, want["all"][1]), what
        if check is not None:
            check(ctx)
        for g, (first, count) in enumerate(tc.groups() if "groups" in want else ()):
            ctx.upload_grid(init) if init is not None else ctx.reset_grid()
            ctx.fuse(first, count)
            if not bits_equal(ctx.download_grid(), want["groups"][g]):
                pytest.fail(f"views {first}..{first + count - 1}: " + _first_wrong_view(ctx, grid, rp, views, init, family, layers, path))


def _tie_case(family, grid_kind, kind, param_set, path, check=None):
    grid, views = tc.tie_scene(family, grid_kind, kind)
    want = tc.expected(family, grid_kind, kind, param_set, with_init=PATHS[path][1])
    _fuse_and_compare(family, grid, tc.PARAM_SETS[param_set], views, want, path, tc.view_layers(), check)


# ---- the tie scenes through every form of the compares --------------------------------------------------------------------------
@pytest.mark.parametrize("family,grid_kind", SCENES)
def test_ties_on_every_path(family, grid_kind):
    """Main parameter set, constant and split depth maps, identity and permutation grid (ROT): the whole path matrix."""
    for kind in ("plain", "split"):
        for path in PATHS:
            _tie_case(family, grid_kind, kind, "main", path)


@pytest.mark.parametrize("grid_kind", tc.GRIDS)
@pytest.mark.parametrize("param_set", [p for p in tc.PARAM_SETS if p != "main"])
def test_ties_of_the_other_parameter_sets(param_set, grid_kind):
    """thick = 0 (NaN at diff == 0), delta = 0, delta == thick, delta < thick, rho < 0 with either sign of eta."""
    for family in tc.FAMILIES:
        for kind in ("plain", "split"):
            for path in FEW:
                _tie_case(family, grid_kind, kind, param_set, path)


@pytest.mark.parametrize("grid_kind", tc.GRIDS)
def test_ties_with_a_general_k(grid_kind):
    """K[2][2] = 2 on every view: h.z = 2 c.z exactly, the same pixels, the GENK instantiations."""
    for family in tc.FAMILIES:
        def genk(ctx):
            p = ctx.view_paths()
            assert p["tiled_general_k"] == ctx.info().n_views and ctx.info().tiled_kernel == 1, p
        for path in ("zero_grid", "counted", "uploaded_grid", "no_brick_classes", "no_interior", "f64_depth"):
            _tie_case(family, grid_kind, "general_k", "main", path, check=genk)
        _tie_case(family, grid_kind, "general_k", "main", "general_kernel")


@pytest.mark.parametrize("grid_kind", tc.GRIDS)
def test_f32_grid_is_the_rounded_expectation(grid_kind):
    for family in tc.FAMILIES:
        grid, views = tc.tie_scene(family, grid_kind)
        want = tc.expected(family, grid_kind, "plain", "main")
        for kw in ({}, {"count_hits": True}, {"kernel_variant": capi.VARIANT_FORCE_GENERAL}):
            with capi.FusionContext(grid, tc.PARAM_SETS["main"], grid_dtype="f32", **kw) as ctx:
                ctx.add_views(views)
                ctx.fuse()   # (a launch sums in f64 and rounds once)
                assert np.array_equal(ctx.download_grid(np.float32).view(np.uint32), want["all"][0].astype(np.float32).view(np.uint32)), (family, kw)
                for g, (first, count) in enumerate(tc.groups()):
                    ctx.reset_grid()
                    ctx.fuse(first, count)
                    assert np.array_equal(ctx.download_grid(np.float32).view(np.uint32),
                                          want["groups"][g].astype(np.float32).view(np.uint32)), (family, kw, g)


# ---- holes: MIXED_FREE_OR_NODEPTH (gathering and window FREE column), or skip ------------------------------------------------------
@pytest.mark.parametrize("family,grid_kind", SCENES)
def test_ties_with_a_tenth_of_the_pixels_missing(family, grid_kind):
    def windows(ctx):
        assert ctx.window_pair_count() > 0, (family, grid_kind)

    def free_or_no_depth(ctx):
        assert ctx.mixed_reason_histogram()["free_or_no_depth"] > 0, (family, grid_kind)
    for kind in ("holes", "split_holes"):
        for param_set in ("main", "rho_neg_eta_neg", "rho_neg_eta_pos"):   # the free-space constant's sign: free_column_exact
            for path in ("windows_always", "windows_always_columns_16"):
                _tie_case(family, grid_kind, kind, param_set, path, check=windows)
            _tie_case(family, grid_kind, kind, param_set, "no_windows", check=free_or_no_depth)
            for path in ("zero_grid", "counted", "uploaded_grid", "uploaded_grid_counted", "no_brick_classes", "keep_behind_adds",
                         "general_kernel", "f64_depth", "columns_16"):
                _tie_case(family, grid_kind, kind, param_set, path)


# ---- the picture leaves the image: border_class, map_serves true and false -------------------------------------------------------
@pytest.mark.parametrize("grid_kind", tc.GRIDS)
@pytest.mark.parametrize("kind", [k + h for k in tc.BORDER_PC for h in ("", "_holes")])
def test_ties_at_the_image_border(kind, grid_kind):
    for family in tc.FAMILIES:
        for path in ("zero_grid", "counted", "uploaded_grid", "no_brick_classes", "no_interior", "windows_always", "no_windows",
                     "columns_16", "f64_depth", "general_kernel"):
            _tie_case(family, grid_kind, kind, "main", path)


# ---- the classes really decide ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,grid_kind", SCENES)
def test_free_behind_and_mixed_bricks_all_occur(family, grid_kind):
    """Without these the class compares would not be under test."""
    for kind in ("plain", "split"):
        for path in ("zero_grid", "counted", "columns_16"):
            def classes(ctx):
                h = ctx.brick_class_histogram()
                assert h["free"] > 0 and h["behind"] > 0 and h["mixed"] > 0, (family, grid_kind, kind, path, h)
                assert ctx.mixed_reason_histogram()["near_surface"] > 0
            _tie_case(family, grid_kind, kind, "main", path, check=classes)


# ---- outward rounding of the f32 pyramid -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,grid_kind", SCENES)
def test_depths_between_two_f32_values_at_a_tie(family, grid_kind):
    """Depths 2^-45 (and 2^-29) off an f32 value, 2^-46 (2^-30) on the near side of a delta tie, at the outer layers of 8-bricks, 16-bricks,
    32-boxes and the grid: a pyramid rounded to nearest proves the brick free / behind, the reference gives -+rho.  Stored as
    f32 the depth IS the f32 value and the expectation is the oracle's on the narrowed table."""
    grid, views, sides, layers, _, e1s = tc.rounding_scene(family, grid_kind)
    rp = tc.PARAM_SETS["main"]
    narrow = tc.narrowed(views)
    want64 = {"all": tc.oracle_grid(grid, rp, views)}
    want32 = {"all": tc.oracle_grid(grid, rp, narrow)}
    assert not bits_equal(want64["all"][0], want32["all"][0])
    init = tc.init_grid(grid.n_voxels)
    for storage in ("auto", "f64", "f32"):
        want = want32 if storage == "f32" else want64
        for kw in ({}, {"count_hits": True}, {"kernel_variant": FX}, {"kernel_variant": TK8}, {"kernel_variant": capi.VARIANT_NO_BRICK_CLASSES},
                   {"kernel_variant": capi.VARIANT_FORCE_GENERAL}):
            what = (family, storage, kw)
            with capi.FusionContext(grid, rp, depth_storage=storage, **kw) as ctx:
                ctx.add_views(views)
                assert ctx.info().depth_storage_in_use == (capi.DMI_DEPTH_F32 if storage == "f32" else capi.DMI_DEPTH_F64), what
                ctx.fuse()
                assert bits_equal(ctx.download_grid(), want["all"][0]), what
                if kw.get("count_hits"):
                    vh, mh = ctx.download_hits()
                    assert np.array_equal(vh, want["all"][1]) and np.array_equal(mh, want["all"][2]), what
                src = narrow if storage == "f32" else views
                for m in range(views.n):       # view by view, onto an uploaded grid every other time
                    start = init if m % 2 else None
                    ctx.upload_grid(start) if start is not None else ctx.reset_grid()
                    ctx.fuse(m, 1)
                    one = tc.oracle_grid(grid, rp, src, m, 1, init=start, count_hits=False)[0]
                    assert bits_equal(ctx.download_grid(), one), what + (m, sides[m], layers[m], e1s[m])


# ---- depth values at the ends of the range -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["auto", "f64", "f32"])
def test_depths_at_the_ends_of_the_range(storage):
    """+-inf, +-0, a negative depth, subnormals, the two f64 neighbours of the sentinel (sentinels once narrowed), FLT_MAX and
    twice that: fused as the reference fuses them -- under f32 storage as it fuses the narrowed table."""
    grid, rp, views, _ = tc.range_ends_scene()
    src = tc.narrowed(views) if storage == "f32" else views
    want = tc.oracle_grid(grid, rp, src)
    init = tc.init_grid(grid.n_voxels)
    want_init = tc.oracle_grid(grid, rp, src, init=init)
    for kw in ({}, {"count_hits": True}, {"kernel_variant": capi.VARIANT_NO_BRICK_CLASSES}, {"kernel_variant": capi.VARIANT_FORCE_GENERAL},
               {"kernel_variant": FX}, {"kernel_variant": capi.VARIANT_WINDOWS_ALWAYS}):
        what = (storage, kw)
        with capi.FusionContext(grid, rp, depth_storage=storage, **kw) as ctx:
            ctx.add_views(views)
            assert ctx.info().depth_storage_in_use == (capi.DMI_DEPTH_F32 if storage == "f32" else capi.DMI_DEPTH_F64), what
            ctx.fuse()
            assert bits_equal(ctx.download_grid(), want[0]), what
            if kw.get("count_hits"):
                vh, mh = ctx.download_hits()
                assert np.array_equal(vh, want[1]) and np.array_equal(mh, want[2]), what
            ctx.upload_grid(init)
            ctx.fuse()
            assert bits_equal(ctx.download_grid(), want_init[0]), what
