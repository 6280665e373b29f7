"""dmi_filter_depth_consistency on the GPU: the filtered depths, the counts and the in-place form against the numpy
restatement (depth_consistency_np.py), bit for bit, at the smallest shapes that can still go wrong: sizes that are no multiple of the
16 x 16 tile, a single view, a single pair, more views than any group the kernel may form, cameras inside the volume, a skewed
K, geo-referenced magnitudes, every kind of invalid depth, a best-cost plane, every combination of the parameters, pixel ties."""
import functools

import numpy as np
import pytest

import depth_consistency_np as C
from cudadepthmapintegration_amd import capi, scene

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT = 1


def _frozen(views):
    for a in (views.depth, views.K4, views.RT4) + (() if views.best_cost is None else (views.best_cost,)):
        a.setflags(write=False)
    return views


def _check(views, min_views=2, abs_tol=0.0, rel_tol=0.01, threshold=None):
    """One call against the restatement; returns (filtered depths, counts, valid mask of the input after the threshold)."""
    bc = views.best_cost if threshold is not None else None
    want_d, want_c = C.filter_depth_consistency(views.depth, views.K4, views.RT4, min_views, abs_tol, rel_tol, bc, threshold)
    got, counts, ms = capi.filter_depth_consistency(views, min_views=min_views, abs_tolerance=abs_tol, rel_tolerance=rel_tol,
                                                    threshold=threshold)
    assert got.best_cost is None and got.K4 is views.K4 and got.RT4 is views.RT4
    assert counts.dtype == np.int32 and got.depth.dtype == np.float64
    bad = np.argwhere(counts != want_c)
    assert len(bad) == 0, (len(bad), bad[:5], counts[tuple(bad[0])], want_c[tuple(bad[0])])
    assert got.depth.tobytes() == want_d.tobytes()
    assert ms > 0.0
    return got.depth, counts, C.valid_pixels(C.thresholded(views.depth, bc, threshold))


@functools.lru_cache(maxsize=None)
def _sphere(n, W=37, H=29, seed=1):
    return _frozen(scene.make_views(n, W, H, seed=seed))


@pytest.mark.parametrize("n", [1, 2, 3, 9])
def test_sizes_that_are_no_tile_multiple(n):
    views = _sphere(n)
    out, counts, valid = _check(views, min_views=1)
    assert valid.any() and not valid.all()
    if n == 1:
        assert (counts == 0).all() and (out == -1.0).all()
    if n == 9:
        assert counts.max() >= 3 and (out > 0).any() and ((out == -1.0) & valid).any()


def test_more_views_than_any_group():
    views = _frozen(scene.make_views(70, 16, 12, seed=11))
    out, counts, valid = _check(views, min_views=3)
    assert counts.max() > 8 and (out > 0).any()
    supported = [(counts[s][valid[s]] > 0).any() for s in range(70)]
    assert all(supported[:3]) and all(supported[-3:])


@functools.lru_cache(maxsize=None)
def _room(skewed=False):
    v = scene.make_room_views(8, 48, 36, seed=2)
    if skewed:
        v.K4[:, 0, 1] = 0.7
        v.K4[:, 1, 1] *= 1.1
        v.K4[:, 0, 2] += 1.3
    return _frozen(v)


@pytest.mark.parametrize("skewed", [False, True])
def test_cameras_inside_the_volume(skewed):
    views = _room(skewed)
    out, counts, valid = _check(views, min_views=1, rel_tol=0.02)
    assert valid.all() and counts.max() >= (1 if skewed else 2) and (counts == 0).any() and (out > 0).any() and (out == -1.0).any()


def test_geo_referenced_magnitudes():
    grid = scene.default_grid(8)
    _, _, views = scene.to_world_frame(grid, scene.default_ray_potential(grid), _sphere(9), 10.0, (5.0e6, -5.0e6, 5.0e6))
    out, counts, valid = _check(_frozen(views), min_views=2)
    assert np.abs(views.RT4[:, :3, 3]).max() > 1e6 and counts.max() >= 2 and (out > 0).any()


def test_every_kind_of_invalid_depth():
    base = _sphere(9)
    rng = np.random.default_rng(5)
    depth = base.depth.copy()
    pick = rng.random(depth.shape) < 0.2      # a fifth of all pixels: where sources sit and where targets sample
    depth[pick] = rng.choice([-1.0, 0.0, -3.0, np.nan, np.inf, -np.inf], size=int(pick.sum()))
    out, counts, valid = _check(_frozen(scene.Views(depth, base.K4, base.RT4)), min_views=1)
    assert not valid[pick].any() and (out[pick] == -1.0).all() and (counts[pick] == 0).all()
    plain = C.filter_depth_consistency(base.depth, base.K4, base.RT4, 1, 0.0, 0.01)[1]
    assert (counts < plain).any() and counts.max() >= 2   # targets did sample the seeded pixels


def test_best_cost_plane_with_a_threshold():
    views = _frozen(scene.make_views(6, 37, 29, seed=4, with_best_cost=True))
    out, counts, valid = _check(views, min_views=1, threshold=0.7)
    cut = views.best_cost > 0.7
    assert cut.any() and (out[cut] == -1.0).all() and (counts[cut] == 0).all() and (out > 0).any()
    # a threshold without costs, and costs without a threshold, change nothing
    _check(scene.Views(views.depth, views.K4, views.RT4), min_views=1, threshold=0.7)
    _check(views, min_views=1)


@pytest.mark.parametrize("abs_tol", [0.0, 0.01])
@pytest.mark.parametrize("rel_tol", [0.0, 0.01])
def test_every_combination_of_the_parameters(abs_tol, rel_tol):
    seen = []
    for min_views in (0, 1, 3):
        out, counts, valid = _check(_sphere(9), min_views=min_views, abs_tol=abs_tol, rel_tol=rel_tol)
        seen.append(int((out > 0).sum()))
    assert seen[0] == int(C.valid_pixels(_sphere(9).depth).sum()) and seen[0] >= seen[1] >= seen[2]
    if abs_tol or rel_tol:
        assert seen[1] > seen[2] > 0
    else:
        assert seen[1] < seen[0]


def test_duplicate_views_count_exactly_one_at_tolerance_zero():
    v = _sphere(3)
    idx = [0, 0, 1, 1, 2, 2]
    out, counts, valid = _check(_frozen(scene.Views(v.depth[idx], v.K4[idx], v.RT4[idx])), min_views=1, abs_tol=0.0, rel_tol=0.0)
    assert valid.sum() == 884 and (counts[valid] == 1).all()


def test_pixel_ties_go_through_the_exact_division():
    """Each view's twin has its principal point moved by half a pixel: every projection into the twin lands on a half-integer, up
    to rounding, which the checked reciprocal must leave to the exact division."""
    v = _sphere(3)
    idx = [0, 0, 1, 1, 2, 2]
    K = v.K4[idx].copy()
    K[1::2, 0, 2] += 0.5
    K[1::2, 1, 2] -= 0.5
    out, counts, valid = _check(_frozen(scene.Views(v.depth[idx], K, v.RT4[idx])), min_views=1, rel_tol=0.05)
    assert counts.max() >= 1


@pytest.mark.parametrize("seed", range(12))
def test_random_small_scenes(seed):
    rng = np.random.default_rng(1000 + seed)
    n, W, H = int(rng.integers(2, 7)), int(rng.integers(5, 41)), int(rng.integers(5, 41))
    views = scene.make_views(n, W, H, seed=seed, with_best_cost=True)
    depth = np.where(views.depth > 0, views.depth * (1.0 + 0.02 * rng.standard_normal(views.depth.shape)), views.depth)
    _check(_frozen(scene.Views(depth, views.K4, views.RT4, views.best_cost)), min_views=int(rng.integers(0, 3)),
           abs_tol=float(rng.choice([0.0, 0.02])), rel_tol=float(rng.choice([0.0, 0.01, 0.03])),
           threshold=float(rng.choice([0.5, 0.9])))


def test_two_runs_give_identical_bytes_and_the_in_place_form_works():
    views = _sphere(9)
    a, ca, ms = capi.filter_depth_consistency(views, min_views=2, rel_tolerance=0.01)
    b, cb, _ = capi.filter_depth_consistency(views, min_views=2, rel_tolerance=0.01)
    assert ms > 0.0 and a.depth.tobytes() == b.depth.tobytes() and ca.tobytes() == cb.tobytes()
    depth = views.depth.copy()
    inplace = scene.Views(depth, views.K4, views.RT4)
    c, cc, _ = capi.filter_depth_consistency(inplace, min_views=2, rel_tolerance=0.01, out=depth)
    assert c.depth is depth and depth.tobytes() == a.depth.tobytes() and cc.tobytes() == ca.tobytes()
    assert depth.tobytes() != views.depth.tobytes()


def test_a_refused_call_leaves_the_output_untouched():
    views = _sphere(3)
    K = views.K4.copy()
    K[2, 1, 0] = 0.25
    out = np.full(views.depth.shape, 7.0)
    with pytest.raises(capi.DmiError) as e:
        capi.filter_depth_consistency(scene.Views(views.depth, K, views.RT4), min_views=1, out=out)
    assert e.value.code == INVALID_ARGUMENT and "view 2" in str(e.value) and (out == 7.0).all()
    with pytest.raises(capi.DmiError) as e:
        capi.filter_depth_consistency(views, min_views=1, device=1 << 20, out=out)
    assert e.value.code == INVALID_ARGUMENT and "device" in str(e.value) and (out == 7.0).all()
