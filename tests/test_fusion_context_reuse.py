"""One capi.FusionContext through a sequence in which every buffer of the fusion groups of its state (csrc/dmi_context.h: views,
hits, volume, tables) is allocated, reused while large enough, grown and released -- twice over.  Every downloaded grid, hit
counter, brick_class_histogram(), mixed_reason_histogram(), window_pair_count() and view_paths() must equal, bit for bit, what a
FRESH context returns for the same step; one whole-grid result per depth type is also the numpy oracle's (oracle_np.fuse), compared
as tests/test_gpu_parity.py compares.  The library's shipped launch rules (helpers.shipped_defaults): 24 x 24 x 40 cells are 45
wave bricks, so a launch of fewer than 48 views fuses without brick classes.

Grid 24 x 24 x 40 (3 x 3 x 5 bricks of 8-voxel columns; 40 layers because dmi_fuse_slab takes layers in units of 32), images of
40 x 24, both grid types:
  1. 3 views, fuse: no classes, the zero row.  Up to 50 views, reset, fuse: classes on -- the class table, the order pair and the
     cz table are in use.  Up to 70 views, reset, fuse: the record arrays grow past 64 records, the class pitch doubles to 128.
  2. The 70 views, reset, fuse_slab(0, 32) and fuse_slab(32, 8): two more slot-permutation geometries, and the deferred zero
     fill is flushed.
  3. A context with count_hits: 3 views, fuse(0, 3), up to 70 views, fuse(3, 67): the views' hit counters keep their counts
     across their growth.
  4. 50 views of the speckle scene (a best-cost threshold leaves a tenth of the pixels without a depth, scattered: the fraction
     of tests/test_gpu_window_centre.py), every depth moved 4 units back so that, as there, the whole grid lies in free space
     (at 40 x 24 pixels the scene itself has next to no brick that sees only background): window_pair_count() > 0, on the fresh
     context too -- the windows instantiation runs and the class table carries the window pairs.
  5. clear_views(), the 70 views at 56 x 32 (staging and pyramids change size), fuse; one more view whose depths are no f32 values
     under AUTO storage: the store is promoted to f64; fuse.
info().device_bytes after step 5 is the same in both rounds, and greater than 0."""
import functools

import numpy as np
import pytest

from cudadepthmapintegration_amd import capi, scene
from helpers import bits_equal, shipped_defaults
from oracle import oracle_np

DIMS = (24, 24, 40)
SMALL, LARGE = (40, 24), (56, 32)


@functools.lru_cache(maxsize=None)
def _data():
    grid = scene.default_grid(DIMS)
    small = scene.make_views(70, *SMALL, seed=21, dense=True)
    large = scene.make_views(71, *LARGE, seed=22, dense=True)
    # the 71st view's depths, one ulp of f64 above an f32 value: AUTO storage must keep every bit
    inexact = large.subset(70, 71)
    inexact.depth[...] = np.where(inexact.depth > 0, np.nextafter(inexact.depth, np.inf), inexact.depth)
    speckle, threshold = scene.make_scene_views("speckle", 50, *SMALL, seed=23, speckle=0.1)
    speckle.depth[...] = np.where(speckle.depth > 0, (speckle.depth + 4.0).astype(np.float32), speckle.depth)   # (f32 values still)
    d = dict(grid=grid, ray=scene.default_ray_potential(grid), small=small, large=large.subset(0, 70), inexact=inexact, speckle=speckle,
             threshold=threshold)
    for v in (small, d["large"], inexact, speckle):
        for a in (v.depth, v.K4, v.RT4, v.best_cost):
            if a is not None:
                a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _oracle(which):
    """label -> (grid f64, voxel hits, map hits) of the numpy oracle, computed once"""
    d = _data()
    g, r = d["grid"], d["ray"]

    def fuse(depth, K4, RT4):
        return oracle_np.fuse(g.cell_dims, g.origin, g.spacing, g.grid_matrix, r.thickness, r.rho, r.eta, r.delta, depth, K4, RT4)
    if which == "small":
        return fuse(d["small"].depth, d["small"].K4, d["small"].RT4)
    if which == "speckle":
        v = d["speckle"]
        return fuse(np.where(v.best_cost > d["threshold"], -1.0, v.depth), v.K4, v.RT4)
    both = [np.concatenate([getattr(d["large"], a), getattr(d["inexact"], a)]) for a in ("depth", "K4", "RT4")]
    return fuse(*both)


def _observe(ctx):
    """everything a caller can read back after a fusion, as arrays"""
    grid = ctx.download_grid(np.float64 if ctx.grid_dtype == "f64" else np.float32)
    return (grid, np.array(list(ctx.brick_class_histogram().values())), np.array(list(ctx.mixed_reason_histogram().values())),
            np.array([ctx.window_pair_count()]), np.array(list(ctx.view_paths().values())))


def _start(ctx):
    ctx.clear_views()
    ctx.reset_grid()


def step1(ctx):
    small, out = _data()["small"], {}
    _start(ctx)
    ctx.add_views(small.subset(0, 3))
    ctx.fuse()
    out["1 three views"] = _observe(ctx)
    ctx.add_views(small.subset(3, 50))
    ctx.reset_grid()
    ctx.fuse()
    out["1 fifty views"] = _observe(ctx)
    ctx.add_views(small.subset(50, 70))
    ctx.reset_grid()
    ctx.fuse()
    out["1 seventy views"] = _observe(ctx)
    return out


def step2(ctx):
    _start(ctx)
    ctx.add_views(_data()["small"])
    ctx.fuse_slab(0, 32)
    ctx.fuse_slab(32, 8)
    return {"2 two slabs": _observe(ctx)}


def step3(ctx):
    small = _data()["small"]
    _start(ctx)
    ctx.add_views(small.subset(0, 3))
    ctx.fuse(0, 3)
    ctx.add_views(small.subset(3, 70))
    ctx.fuse(3, 67)
    return {"3 hits": _observe(ctx) + ctx.download_hits()}


def step4(ctx):
    d = _data()
    _start(ctx)
    ctx.add_views(d["speckle"], threshold=d["threshold"])
    ctx.fuse()
    return {"4 speckle": _observe(ctx)}


def step5(ctx):
    d, out = _data(), {}
    _start(ctx)
    ctx.add_views(d["large"])
    ctx.fuse()
    out["5 larger images"] = _observe(ctx)
    assert ctx.info().depth_storage_in_use == capi.DMI_DEPTH_F32
    ctx.add_views(d["inexact"])
    assert ctx.info().depth_storage_in_use == capi.DMI_DEPTH_F64
    ctx.reset_grid()
    ctx.fuse()
    out["5 promoted store"] = _observe(ctx)
    return out


def _assert_same(got, want, what):
    assert len(got) == len(want), what
    for q, (a, b) in enumerate(zip(got, want)):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, q, int((a != b).sum()) if a.shape == b.shape else None)


def _assert_oracle(got_grid, want, grid_dtype, what):
    if grid_dtype == "f64":
        assert bits_equal(got_grid, want), what
    else:
        assert np.array_equal(got_grid, want.astype(np.float32)), what   # exactly the f32 rounding of the f64 sum


def _fresh_and_reused(steps, check_fresh, **options):
    d = _data()
    fresh = {}
    for step in steps:
        with capi.FusionContext(d["grid"], d["ray"], **options) as f:
            fresh.update(step(f))
    check_fresh(fresh)
    with capi.FusionContext(d["grid"], d["ray"], **options) as ctx:
        held = []
        for round_ in (1, 2):
            for step in steps:
                for label, got in step(ctx).items():
                    _assert_same(got, fresh[label], ("round", round_, "against a fresh context", label))
            held.append(int(ctx.info().device_bytes))
        assert held[0] == held[1] and held[0] > 0, held


@pytest.mark.gpu
@pytest.mark.parametrize("grid_dtype", ["f64", "f32"])
def test_a_reused_context_returns_what_fresh_contexts_return(grid_dtype):
    def check_fresh(fresh):
        classes, windows = 1, 3   # positions in _observe's tuple
        assert fresh["1 three views"][classes].sum() == 0       # a launch without classes
        assert fresh["1 fifty views"][classes].sum() == 45 * 50 and fresh["1 seventy views"][classes].sum() == 45 * 70
        assert fresh["2 two slabs"][classes].sum() == 45 * 70   # (a slab's launch keeps the whole grid's rows)
        assert fresh["4 speckle"][windows][0] > 0               # the windows instantiation ran
        assert fresh["5 promoted store"][windows][0] == 0
        for label, which in (("1 seventy views", "small"), ("2 two slabs", "small"), ("4 speckle", "speckle"), ("5 promoted store", "large")):
            _assert_oracle(fresh[label][0], _oracle(which)[0], grid_dtype, label)

    with shipped_defaults():
        _fresh_and_reused((step1, step2, step4, step5), check_fresh, grid_dtype=grid_dtype)


@pytest.mark.gpu
def test_hit_counters_keep_their_counts_when_they_grow():
    def check_fresh(fresh):
        grid, voxel_hits, map_hits = fresh["3 hits"][0], fresh["3 hits"][-2], fresh["3 hits"][-1]
        want, want_voxel_hits, want_map_hits = _oracle("small")
        assert map_hits[:3].min() > 0   # counted before the growth, still there after it
        assert np.array_equal(map_hits, want_map_hits) and np.array_equal(voxel_hits, want_voxel_hits)
        assert bits_equal(grid, want)

    with shipped_defaults():
        _fresh_and_reused((step3,), check_fresh, count_hits=True)
