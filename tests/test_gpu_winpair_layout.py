"""The window-pair table is laid out [block of 32 views][brick][32 views] (csrc/fusion_launch_rules.h: win_pair_index):
window_origin_kernel writes it, fuse_tile_kernel's window column reads it, and an entry that one of them puts or looks for in the
wrong place is a wrong window -- a wrong validity bit for some voxel, a changed sum.  A launch with VARIANT_NO_WINDOWS never reads
the table (the FREE column gathers from the validity maps): for each case below the grid with windows must equal, bit for bit, the
grid of the same context settings without them, and the launch must have window pairs at all.

The cases are the smallest shapes at which the index can go wrong, on the speckle scene (10 % of the pixels without a depth,
scattered: pairs get windows), with 16-voxel and with 8-voxel columns:

* 72 x 40 x 48 voxels x 70 views of 160 x 120: 9 x 5 bricks a layer -- 135 bricks with 16-voxel columns, no multiple of the 64 that
  a workgroup of the origin pass takes --, views in three blocks, the last one ragged; this case also against the CPU oracle;
* the same, fused as views 0-4 and then 5-44: a range that starts and ends inside a block, onto a grid that is not fresh;
* 64 x 64 x 96 voxels x 33 views, fused as three slabs of 32 layers: brick numbers counted over the whole grid in a slab launch;
* the first case on the rotated grid, and in both launch forms (persistent workgroups or one per brick)."""
import functools

import numpy as np
import pytest

from cudadepthmapintegration_amd import capi, scene
from oracle import oracle
from helpers import bits_equal, oracle_params_from_scene

BASE = capi.VARIANT_BRICK_CLASSES_ALWAYS | capi.VARIANT_WINDOWS_ALWAYS | capi.VARIANT_FIXED_TILE_SHAPE
TK8 = 224  # tile-shape bits 7: 8-voxel columns
SHAPES = {"tk16": 0, "tk8": TK8}
W, H = 160, 120
DIMS = (72, 40, 48)
SLAB_DIMS = (64, 64, 96)


@functools.lru_cache(maxsize=None)
def _views(n):
    views, thr = scene.make_scene_views("speckle", n, W, H, seed=38)
    assert views.best_cost is not None and thr is not None
    return views, thr


@functools.lru_cache(maxsize=None)
def _oracle_grid():
    grid = scene.default_grid(DIMS)
    rp = scene.default_ray_potential(grid)
    views, thr = _views(70)
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


def _with_and_without_windows(grid, n_views, variant, steps, expect_pairs=True):
    out, n_win = _fuse(grid, n_views, BASE | variant, steps)
    ref, n_ref = _fuse(grid, n_views, BASE | variant | capi.VARIANT_NO_WINDOWS, steps)
    print(f"window pairs {n_win} (without windows: {n_ref}), voxels that differ: {int(np.count_nonzero(out.view(np.uint64) != ref.view(np.uint64)))}")
    assert n_ref == 0
    assert bits_equal(out, ref)
    if expect_pairs:
        assert n_win > 0
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_ragged_bricks_and_view_blocks_against_no_windows_and_the_oracle(shape):
    out = _with_and_without_windows(scene.default_grid(DIMS), 70, SHAPES[shape], lambda ctx: ctx.fuse())
    assert bits_equal(out, _oracle_grid())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_view_range_inside_a_block_onto_a_fused_grid(shape):
    def steps(ctx):
        ctx.fuse(0, 5)
        ctx.fuse(5, 40)
    # (the second launch accumulates onto a grid that is not fresh: it runs without windows, so only the grids are compared)
    _with_and_without_windows(scene.default_grid(DIMS), 70, SHAPES[shape], steps, expect_pairs=False)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_slab_launches_number_their_bricks_over_the_whole_grid(shape):
    def steps(ctx):
        for z in (0, 32, 64):
            ctx.fuse_slab(z, 32)
    _with_and_without_windows(scene.default_grid(SLAB_DIMS), 33, SHAPES[shape], steps)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_rotated_grid(shape):
    _with_and_without_windows(scene.default_grid(DIMS, rotated=True), 70, SHAPES[shape], lambda ctx: ctx.fuse())


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["persistent", "one_per_brick"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_both_launch_forms(shape, form):
    bits = {"persistent": capi.VARIANT_PERSISTENT_ALWAYS, "one_per_brick": capi.VARIANT_PERSISTENT_NEVER}[form]
    _with_and_without_windows(scene.default_grid(DIMS), 70, SHAPES[shape] | bits, lambda ctx: ctx.fuse())
