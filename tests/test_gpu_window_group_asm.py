"""The window column of fuse_tile_kernel forms the candidates of four voxels -- the chains of the Newton reciprocals, the
verification, the look-ups' row addresses -- in ONE asm statement per group (win_group4, csrc/fusion_tile_acc.inc) in the 16-voxel
kernels, with its values in fixed registers that the statement reuses; after the column the voxels that some lane did not accept
are redone in fp64 from record fields loaded once per pair (csrc/fusion_tile.hip).  What can go wrong there changes a sum: a
register rewritten before its last reader, a reciprocal carried wrongly from one group to the next, the first group (the only
v_rcp_f32, operands instead of registers for the first voxel), a threshold or a row address taken from the wrong voxel, a field of
the record at the wrong offset in the redo.

A launch with VARIANT_NO_WINDOWS never enters the window column (the FREE column gathers from the validity maps): for each case
below the grid fused with windows must equal, bit for bit, the grid of the same settings without them, and the launch must have
had window pairs at all.  One case is compared with the CPU oracle as well.

Speckle maps of 96 x 64 (10 % of the pixels without a depth, scattered: pairs get windows), cameras on a ring.  The smallest grids
at which each piece runs.  The few-brick grids have the voxel size of the 64-cell ones (1/32) and stand on the z axis above the
scene's sphere (radius 0.6), from z = 1 up: every ring camera sees the background through them, pixels away from the sphere's
outline, and the bricks on the camera's side of the axis lie more than delta in front of it: free space with holes -- window
pairs -- in every view (as a cube of [-1, 1]^3 cut into so few cells, a brick would cover more pixels than a window holds and be
near the surface besides: no window pair at all).

* 16 x 16 x 32 cells with 1, 2 and 9 views (9 crosses a word of brick classes), 16-voxel columns: every group position of a
  column; 16 x 16 x 16 with 8-voxel columns (which keep the link-by-link form: two groups);
* 64 x 64 x 48 with 33 views, both column heights: hundreds of redone voxels (0.16 per pair) through the hoisted loads;
* a rotated grid (the ROT instantiations), both launch forms, and 24 x 16 x 33 cells: the top brick sticks out of the grid and
  takes the full-test column, the bricks below it have windows;
* 72 x 40 x 33 with 33 views against the oracle."""
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
DIMS_GROUPS = {"tk16": (16, 16, 32), "tk8": (16, 16, 16)}
DIMS_REDO = (64, 64, 48)
DIMS_TOP = (24, 16, 33)
DIMS_ORACLE = (72, 40, 33)
N_REDO = 33


@functools.lru_cache(maxsize=None)
def _views(n):
    views, thr = scene.make_scene_views("speckle", n, W, H, seed=40, layout="ring")
    assert views.best_cost is not None and thr is not None
    for a in (views.depth, views.K4, views.RT4, views.best_cost):
        a.setflags(write=False)
    return views, thr


@functools.lru_cache(maxsize=None)
def _oracle_grid():
    grid = scene.default_grid(DIMS_ORACLE)
    rp = scene.default_ray_potential(grid)
    views, thr = _views(N_REDO)
    d = oracle.apply_depth_threshold(views.depth, views.best_cost, thr).reshape(views.depth.shape)
    want, _, _ = oracle.fuse(oracle_params_from_scene(grid, rp, views), d, views.K4, views.RT4, n_threads=oracle.max_threads())
    want.setflags(write=False)
    return want


def _small_grid(dims):
    s = 1.0 / 32
    return scene.GridDesc(tuple(dims), (-0.5 * dims[0] * s, -0.5 * dims[1] * s, 1.0), (s, s, s), np.eye(4))


def _fuse(grid, n_views, variant):
    """The grid after one fusion and the window pairs of the launch."""
    views, thr = _views(n_views)
    with capi.FusionContext(grid, scene.default_ray_potential(grid), kernel_variant=variant) as ctx:
        ctx.add_views(views, threshold=thr)
        ctx.fuse()
        return ctx.download_grid(), ctx.window_pair_count()


def _with_and_without_windows(grid, n_views, variant):
    out, n_win = _fuse(grid, n_views, BASE | variant)
    ref, n_ref = _fuse(grid, n_views, BASE | variant | capi.VARIANT_NO_WINDOWS)
    print(f"window pairs {n_win} (without windows: {n_ref}), voxels that differ: {int(np.count_nonzero(out.view(np.uint64) != ref.view(np.uint64)))}")
    assert n_ref == 0
    assert n_win > 0
    assert bits_equal(out, ref)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n_views", [1, 2, 9])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_group_position_of_a_column(shape, n_views):
    _with_and_without_windows(_small_grid(DIMS_GROUPS[shape]), n_views, SHAPES[shape])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_redone_voxels_through_the_hoisted_loads(shape):
    _with_and_without_windows(scene.default_grid(DIMS_REDO), N_REDO, SHAPES[shape])


@pytest.mark.gpu
def test_rotated_grid():
    _with_and_without_windows(scene.default_grid(DIMS_ORACLE, rotated=True), 9, SHAPES["tk16"])


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["persistent", "one_per_brick"])
def test_both_launch_forms(form):
    bits = {"persistent": capi.VARIANT_PERSISTENT_ALWAYS, "one_per_brick": capi.VARIANT_PERSISTENT_NEVER}[form]
    _with_and_without_windows(_small_grid(DIMS_GROUPS["tk16"]), 9, SHAPES["tk16"] | bits)


@pytest.mark.gpu
def test_a_top_brick_that_sticks_out_of_the_grid():
    _with_and_without_windows(_small_grid(DIMS_TOP), 9, SHAPES["tk16"])


@pytest.mark.gpu
def test_against_the_oracle():
    out = _with_and_without_windows(scene.default_grid(DIMS_ORACLE), N_REDO, SHAPES["tk16"])
    assert bits_equal(out, _oracle_grid())
