"""A brick's window-pair entries (WinPair, csrc/fusion_kernels.h) reach the window column of fuse_tile_kernel through a per-wave
area in LDS that holds the entries of one GROUP of 256 views -- view v's at (v & 255) * 16 --, filled when the brick starts and
whenever the view loop enters another group (csrc/fusion_tile.hip).  What can go wrong there changes a sum: an entry taken from
the wrong place of the area, an area not refilled at a group boundary, a view range that starts inside a group, the tail of the
last group (beyond the resident views) reaching a column, a persistent workgroup reading the entries of the brick it fused before.

A launch with VARIANT_NO_WINDOWS never reads the pair table (the FREE column gathers from the validity maps): for each case below
the grid fused with windows must equal, bit for bit, the grid of the same context settings without them, and the launch must have
had window pairs at all.  One case is compared with the CPU oracle as well.  These properties hold for any route the entries take.

Small grids (64 x 64 x 48 and 72 x 40 x 33 cells), maps of 96 x 64 with 10 % of the pixels without a depth (scattered: pairs get
windows), 16- and 8-voxel columns:

* 31, 32, 33, 255, 256, 257 and 288 views: around a block of 32 and around the group; the last two refill the area;
* views [first, 288) with first = 5, 37 and 250: a range that starts inside a group, and one that crosses into the second group
  after six views; views [256, 288): the second group alone, which must have window pairs of its own;
* both launch forms, a slab launch whose brick numbers do not start at 0, a rotated grid;
* 192 x 192 x 128 cells (4608 bricks of 16 layers, 9216 of 8) in the persistent form: more bricks than the chip holds one-wave
  workgroups of this kernel (at most 256 CUs x 4 SIMDs x 5), so workgroups take one brick after another."""
import functools

import numpy as np
import pytest

from cudadepthmapintegration_amd import capi, scene
from oracle import oracle
from helpers import bits_equal, oracle_params_from_scene

BASE = capi.VARIANT_BRICK_CLASSES_ALWAYS | capi.VARIANT_WINDOWS_ALWAYS | capi.VARIANT_FIXED_TILE_SHAPE
TK8 = 224  # tile-shape bits 7: 8-voxel columns
SHAPES = {"tk16": 0, "tk8": TK8}
W, H = 96, 64
N_MAX = 288
DIMS_A = (64, 64, 48)
DIMS_B = (72, 40, 33)
DIMS_SLAB = (64, 64, 96)
DIMS_MANY = (192, 192, 128)
ORACLE_VIEWS = 33


@functools.lru_cache(maxsize=None)
def _views(n):
    # cameras on a ring around the grid, every one looking across the columns: each view has window pairs, the last ones of a
    # fusion too (near the poles of the sphere layout, looking along the columns, a view has none)
    views, thr = scene.make_scene_views("speckle", n, W, H, seed=40, layout="ring")
    assert views.best_cost is not None and thr is not None
    for a in (views.depth, views.K4, views.RT4, views.best_cost):
        a.setflags(write=False)
    return views, thr


@functools.lru_cache(maxsize=None)
def _oracle_grid():
    grid = scene.default_grid(DIMS_B)
    rp = scene.default_ray_potential(grid)
    views, thr = _views(ORACLE_VIEWS)
    d = oracle.apply_depth_threshold(views.depth, views.best_cost, thr).reshape(views.depth.shape)
    want, _, _ = oracle.fuse(oracle_params_from_scene(grid, rp, views), d, views.K4, views.RT4, n_threads=oracle.max_threads())
    want.setflags(write=False)
    return want


def _fuse(grid, n_views, variant, steps):
    """The grid after `steps` (a function of the context) and the window pairs of its last launch."""
    views, thr = _views(n_views)
    with capi.FusionContext(grid, scene.default_ray_potential(grid), kernel_variant=variant) as ctx:
        ctx.add_views(views, threshold=thr)
        steps(ctx)
        return ctx.download_grid(), ctx.window_pair_count()


def _with_and_without_windows(grid, n_views, variant, steps):
    out, n_win = _fuse(grid, n_views, BASE | variant, steps)
    ref, n_ref = _fuse(grid, n_views, BASE | variant | capi.VARIANT_NO_WINDOWS, steps)
    print(f"window pairs {n_win} (without windows: {n_ref}), voxels that differ: {int(np.count_nonzero(out.view(np.uint64) != ref.view(np.uint64)))}")
    assert n_ref == 0
    assert n_win > 0
    assert bits_equal(out, ref)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n_views", [31, 32, 33, 255, 256, 257, 288])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_view_counts_around_a_block_and_around_the_group(shape, n_views):
    _with_and_without_windows(scene.default_grid(DIMS_A), n_views, SHAPES[shape], lambda ctx: ctx.fuse())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_against_the_oracle(shape):
    out = _with_and_without_windows(scene.default_grid(DIMS_B), ORACLE_VIEWS, SHAPES[shape], lambda ctx: ctx.fuse())
    assert bits_equal(out, _oracle_grid())


@pytest.mark.gpu
@pytest.mark.parametrize("first", [5, 37, 250, 256])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_view_range_that_starts_inside_a_group(shape, first):
    _with_and_without_windows(scene.default_grid(DIMS_A), N_MAX, SHAPES[shape], lambda ctx: ctx.fuse(first, N_MAX - first))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["persistent", "one_per_brick"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_both_launch_forms_across_a_group_boundary(shape, form):
    bits = {"persistent": capi.VARIANT_PERSISTENT_ALWAYS, "one_per_brick": capi.VARIANT_PERSISTENT_NEVER}[form]
    _with_and_without_windows(scene.default_grid(DIMS_B), 257, SHAPES[shape] | bits, lambda ctx: ctx.fuse())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_slab_whose_bricks_do_not_start_at_zero(shape):
    _with_and_without_windows(scene.default_grid(DIMS_SLAB), 257, SHAPES[shape], lambda ctx: ctx.fuse_slab(32, 64))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_rotated_grid(shape):
    _with_and_without_windows(scene.default_grid(DIMS_B, rotated=True), 257, SHAPES[shape], lambda ctx: ctx.fuse())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_persistent_workgroups_that_take_brick_after_brick(shape):
    _with_and_without_windows(scene.default_grid(DIMS_MANY), 33, SHAPES[shape] | capi.VARIANT_PERSISTENT_ALWAYS, lambda ctx: ctx.fuse())
