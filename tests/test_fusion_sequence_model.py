"""tests/fusion_sequence_model.py against itself, on the CPU: the model is what tests/test_gpu_sequence_fuzz.py holds a fusion
context to, so it must first be the oracle where the oracle has an answer of its own.
  * one add_views + fuse is oracle.fuse (grid bit for bit, both hit counters), with and without a best-cost threshold;
  * slabs fused one after the other, and view ranges fused one after the other, are one fuse bit for bit, hits included;
  * an uploaded grid of -0.0 keeps its -0.0 exactly in the voxels no view reaches and loses it everywhere else, where a potential
    of +0.0 (far behind the surface) or a non-zero one was added -- with a negative eta no potential is -0.0;
  * an f32 model rounds once per call; a refused call changes nothing; clear_views withdraws the views' hit counts until a reset."""
import numpy as np
import pytest

from cudadepthmapintegration_amd import scene
from fusion_sequence_model import FusionSequenceModel, ModelRefusal, same_grid
from helpers import bits_equal, oracle_params_from_scene
from oracle import oracle

DIMS = (24, 24, 64)
W, H = 40, 24


def _scene(rotated=False):
    grid = scene.default_grid(DIMS, rotated=rotated)
    views = scene.make_views(7, W, H, seed=31, dense=True, with_best_cost=True)
    return grid, scene.default_ray_potential(grid), views


@pytest.mark.parametrize("threshold", [None, 0.8])
def test_one_step_is_the_oracle(threshold):
    grid, ray, views = _scene(rotated=True)
    depth = views.depth if threshold is None else oracle.apply_depth_threshold(views.depth, views.best_cost, threshold).reshape(views.depth.shape)
    want, vh, mh = oracle.fuse(oracle_params_from_scene(grid, ray, views), depth, views.K4, views.RT4)
    m = FusionSequenceModel(grid, ray, count_hits=True)
    m.add_views(views, threshold)
    m.fuse()
    assert m.n_views == 7 and bits_equal(m.grid, want) and np.array_equal(m.voxel_hits, vh) and np.array_equal(m.map_hits, mh)
    assert (threshold is None) == bits_equal(depth, views.depth)   # the threshold took depths away
    assert bits_equal(m.point_data(), oracle.cell_to_point(want))


def test_slabs_and_ranges_are_one_fuse():
    grid, ray, views = _scene()
    init = np.random.default_rng(5).standard_normal(DIMS[::-1])
    models = [FusionSequenceModel(grid, ray, count_hits=True) for _ in range(4)]
    for m in models:
        m.upload_grid(init)
        m.add_views(views)
    whole, slabs, ranges, streamed = models
    whole.fuse()
    slabs.fuse_slab(32, 32)
    assert bits_equal(slabs.grid[:32], init[:32]) and not slabs.voxel_hits[:32].any() and slabs.voxel_hits[32:].any()
    slabs.fuse_slab(0, 32)
    ranges.fuse(0, 3)
    ranges.fuse(3, 0)
    ranges.fuse(3, 4)
    assert bits_equal(streamed.fuse_download(0, 5), streamed.grid)
    streamed.fuse_download(5, 2)
    assert whole.voxel_hits.any() and whole.map_hits.all()
    for m in (slabs, ranges, streamed):
        assert bits_equal(m.grid, whole.grid) and np.array_equal(m.voxel_hits, whole.voxel_hits) and np.array_equal(m.map_hits, whole.map_hits)
        assert same_grid(m.grid, whole)


def test_negative_zero_survives_exactly_where_nothing_is_added():
    grid = scene.default_grid(DIMS)
    ray = scene.RayPotential(thickness=0.05, rho=0.8, eta=-0.2, delta=0.2)   # free space adds +0.16, far behind a surface adds +0.0
    views = scene.make_views(3, W, H, seed=23, dense=True)
    views.depth[np.random.default_rng(8).random(views.depth.shape) < 0.3] = -1.0
    m = FusionSequenceModel(grid, ray, count_hits=True)
    m.add_views(views)
    m.upload_grid(np.full(DIMS[::-1], -0.0))
    m.fuse()
    negative_zero = (m.grid == 0) & np.signbit(m.grid)
    positive_zero = (m.grid == 0) & ~np.signbit(m.grid)
    assert np.array_equal(negative_zero, m.voxel_hits == 0)       # missed by every view: untouched; reached by one: no longer -0.0
    assert negative_zero.any() and positive_zero.any() and (m.grid != 0).any()
    assert (m.voxel_hits[positive_zero] > 0).all()
    # ... and in two steps, the second starting from the first one's grid
    two = FusionSequenceModel(grid, ray, count_hits=True)
    two.add_views(views)
    two.upload_grid(np.full(DIMS[::-1], -0.0))
    two.fuse(0, 1)
    assert (((two.grid == 0) & np.signbit(two.grid)) == (two.voxel_hits == 0)).all()
    two.fuse(1, 2)
    assert bits_equal(two.grid, m.grid)


def test_f32_model_rounds_once_per_call():
    grid, ray, views = _scene()
    want = oracle.fuse(oracle_params_from_scene(grid, ray, views), views.depth, views.K4, views.RT4)[0]
    m = FusionSequenceModel(grid, ray, grid_dtype="f32")
    m.add_views(views)
    m.fuse()
    assert np.array_equal(m.grid, want.astype(np.float32).astype(np.float64)) and not np.array_equal(m.grid, want)
    assert same_grid(want.astype(np.float32), m) and not same_grid(np.nextafter(want.astype(np.float32), np.float32(9)), m)
    first = m.grid.copy()
    m.fuse(0, 2)   # a second call starts from the ROUNDED grid
    again = oracle.fuse(oracle_params_from_scene(grid, ray, views), views.depth[:2], views.K4[:2], views.RT4[:2], init_grid=first)[0]
    assert np.array_equal(m.grid, again.astype(np.float32).astype(np.float64))
    assert not m.voxel_hits.any()   # hits are not counted unless asked for


def test_refusals_and_cleared_views():
    grid, ray, views = _scene()
    m = FusionSequenceModel(grid, ray, count_hits=True)
    with pytest.raises(ModelRefusal):
        m.fuse()
    assert bits_equal(m.fuse_download(0, 0), np.zeros(DIMS[::-1]))   # a plain download needs no view
    m.add_views(views.subset(0, 4))
    m.fuse()
    before = (m.grid.copy(), m.voxel_hits.copy(), m.map_hits.copy())
    for refused in (lambda: m.fuse(2, 3), lambda: m.fuse(5, 0), lambda: m.fuse_slab(16, 16), lambda: m.fuse_slab(0, 40),
                    lambda: m.fuse_slab(32, 40), lambda: m.fuse_download(4, 1),
                    lambda: m.add_views(scene.make_views(1, 56, 32, seed=1, dense=True))):
        with pytest.raises(ModelRefusal):
            refused()
    assert bits_equal(m.grid, before[0]) and np.array_equal(m.voxel_hits, before[1]) and np.array_equal(m.map_hits, before[2])
    assert m.n_views == 4 and m.map_hits_known
    m.fuse(4, 0)   # an empty range at the end is no refusal
    m.clear_views()
    assert m.n_views == 0 and not m.map_hits_known and np.array_equal(m.voxel_hits, before[1])
    m.add_views(scene.make_views(2, 56, 32, seed=1, dense=True))   # another image size after a clear
    m.fuse()
    assert (m.voxel_hits >= before[1]).all() and not m.map_hits_known
    m.reset_grid()
    assert m.map_hits_known and not m.map_hits.any() and not m.voxel_hits.any() and not m.grid.any() and not np.signbit(m.grid).any()
