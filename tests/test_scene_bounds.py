"""dmi_estimate_scene_bounds on the GPU: lo, hi and the number of points against the numpy restatement
(scene_bounds_np.py), bit for bit and without a tolerance, at the smallest shapes that can still go wrong: sizes that are no
multiple of a chunk, one view, more chunks than one workgroup visits, every trim and pixel step up to 2^31 - 1, rotated axes, coordinates of both
signs, equal coordinates, signed zeros, keys that differ in the last digit only, geo-referenced magnitudes, every kind of invalid
depth, coordinates that overflow, no point at all, every refused argument."""
import ctypes
import functools

import numpy as np
import pytest

import scene_bounds_np as B
from cudadepthmapintegration_amd import capi, scene

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT = 1
ALL_TRIMS = (0.0, "1/N", 0.01, 0.25, 0.5)


def _frozen(views):
    for a in (views.depth, views.K4, views.RT4) + (() if views.best_cost is None else (views.best_cost,)):
        a.setflags(write=False)
    return views


def _check(views, trims=(0.0, 0.01), pixel_step=1, axes=None, threshold=None):
    """One call per trim against the restatement; returns the counted coordinates [3, N] and the last (lo, hi)."""
    bc = views.best_cost if threshold is not None else None
    s = B.counted_coordinates(views.depth, views.K4, views.RT4, axes, pixel_step, bc, threshold)
    lo = hi = None
    for trim in trims:
        trim = 1.0 / max(s.shape[1], 1) if trim == "1/N" else trim
        want_lo, want_hi, want_n = B.bounds_of(s, trim)
        lo, hi, n_points, ms = capi.estimate_scene_bounds(views, trim_fraction=trim, pixel_step=pixel_step, axes=axes, threshold=threshold)
        assert n_points == want_n, (trim, n_points, want_n)
        assert lo.dtype == np.float64 and hi.dtype == np.float64 and ms > 0.0
        if want_n == 0:
            assert np.isnan(lo).all() and np.isnan(hi).all()
        else:
            assert lo.tobytes() == want_lo.tobytes() and hi.tobytes() == want_hi.tobytes(), (trim, lo, want_lo, hi, want_hi)
    return s, lo, hi


@functools.lru_cache(maxsize=None)
def _sphere(n, W=37, H=29, seed=1):
    return _frozen(scene.make_views(n, W, H, seed=seed))


@functools.lru_cache(maxsize=None)
def _room():
    return _frozen(scene.make_room_views(8, 48, 36, seed=2))


def _plane_views(depth, W=37, H=29):
    """One camera with the identity rotation at the origin: w_2 of a pixel is its depth itself."""
    K = np.eye(4)
    K[0, 0] = K[1, 1] = 0.9 * W
    K[0, 2], K[1, 2] = W / 2.0, H / 2.0
    return _frozen(scene.Views(np.ascontiguousarray(np.broadcast_to(depth, (1, H, W)), dtype=np.float64), K[None].copy(), np.eye(4)[None].copy()))


@pytest.mark.parametrize("pixel_step", [1, 2, 5])
@pytest.mark.parametrize("n", [1, 2, 9])
def test_sizes_that_are_no_chunk_multiple(n, pixel_step):
    s, lo, hi = _check(_sphere(n), trims=ALL_TRIMS, pixel_step=pixel_step)
    assert 0 < s.shape[1] < n * 37 * 29 and (lo <= hi).all()
    if pixel_step > 1:
        assert s.shape[1] < B.counted_coordinates(_sphere(n).depth, _sphere(n).K4, _sphere(n).RT4).shape[1]


@pytest.mark.parametrize("pixel_step", [29, 30, 37, 40, 2**31 - 1])
def test_a_step_beyond_the_image_leaves_pixel_0_0_of_every_view(pixel_step):
    """Steps around and above W = 37 and H = 29 up to the largest the call admits: only image pixel (0, 0) -- vtk row H-1, column 0
    -- of every view takes part once the step exceeds both, and N is the number of views whose corner holds a depth."""
    base = scene.make_views(5, 37, 29, seed=2, dense=True)
    depth = base.depth.copy()
    depth[3, 28, 0] = -1.0                      # one view without a depth in its corner
    depth[:, 0, 0] = np.nan                     # the other end of column 0 must not be mistaken for it
    s, lo, hi = _check(_frozen(scene.Views(depth, base.K4, base.RT4)), trims=ALL_TRIMS, pixel_step=pixel_step)
    if pixel_step >= 37:
        assert s.shape[1] == 4
    else:
        assert s.shape[1] > 4


def test_many_views_of_a_small_image():
    s, lo, hi = _check(_frozen(scene.make_views(70, 16, 12, seed=11)), trims=ALL_TRIMS)
    assert s.shape[1] > 70 and (lo <= hi).all()


def test_more_chunks_than_workgroups_so_that_a_workgroup_visits_several():
    views = _frozen(scene.make_views(300, 96, 80, seed=3, dense=True))   # 8 chunks a view: 2400 chunks
    s, lo, hi = _check(views, trims=(0.005,))
    assert s.shape[1] == 300 * 96 * 80


def test_rotated_axes_that_are_no_unit_vectors():
    R = scene.default_grid(8, rotated=True).grid_matrix[:3, :3]
    axes = R * np.array([[0.5], [3.0], [1.0 / 7.0]])
    s, lo, hi = _check(_sphere(9), trims=ALL_TRIMS, axes=axes)
    plain = B.counted_coordinates(_sphere(9).depth, _sphere(9).K4, _sphere(9).RT4)
    assert s.shape == plain.shape and not np.array_equal(s, plain)


def test_room_cameras_give_coordinates_of_both_signs():
    s, lo, hi = _check(_room(), trims=ALL_TRIMS[:4])
    assert (s.min(axis=1) < 0).all() and (s.max(axis=1) > 0).all()
    _check(_room(), trims=(0.0, 0.5), pixel_step=5)


def test_a_plane_facing_the_camera_has_one_coordinate():
    s, lo, hi = _check(_plane_views(2.5), trims=ALL_TRIMS)
    assert lo[2] == 2.5 and hi[2] == 2.5 and (s[2] == 2.5).all()
    lo, hi, _, _ = capi.estimate_scene_bounds(_plane_views(2.5), trim_fraction=0.25)
    assert lo[2] == 2.5 and hi[2] == 2.5 and lo[0] < hi[0] and lo[1] < hi[1]


def test_signed_zeros_are_ordered_by_their_sign():
    """An all-zero first row of the axes: s_0 = (0*w_0 + 0*w_1) + 0*w_2 is -0.0 where all of w are negative and +0.0 elsewhere."""
    axes = np.array([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    s, lo, hi = _check(_room(), trims=ALL_TRIMS, axes=axes)
    negative = int(np.signbit(s[0]).sum())
    assert (s[0] == 0.0).all() and 0 < negative < s.shape[1]
    lo, hi, _, _ = capi.estimate_scene_bounds(_room(), trim_fraction=0.0, axes=axes)
    assert lo[0] == 0.0 and np.signbit(lo[0]) and hi[0] == 0.0 and not np.signbit(hi[0])


def test_keys_that_differ_in_the_last_digit_only():
    near = 2.0
    far = np.float64(near).view(np.uint64) + np.uint64(200)
    depth = np.full((29, 37), near)
    depth.reshape(-1)[1::2] = np.array([far], dtype=np.uint64).view(np.float64)[0]
    s, lo, hi = _check(_plane_views(depth), trims=ALL_TRIMS)
    values = np.unique(s[2])
    assert len(values) == 2 and np.all(B.keys_of(values) >> np.uint64(8) == B.keys_of(values)[0] >> np.uint64(8))
    lo, hi, n_points, _ = capi.estimate_scene_bounds(_plane_views(depth), trim_fraction=0.25)
    assert lo[2] == values[0] and hi[2] == values[1] and n_points == 29 * 37


def test_geo_referenced_magnitudes():
    grid = scene.default_grid(8)
    _, _, views = scene.to_world_frame(grid, scene.default_ray_potential(grid), _sphere(9), 10.0, (5.0e6, -5.0e6, 5.0e6))
    s, lo, hi = _check(_frozen(views), trims=ALL_TRIMS)
    assert np.abs(lo).min() > 1e6 and (lo <= hi).all() and (s.min(axis=1) < s.max(axis=1)).all()


def test_every_kind_of_invalid_depth_and_a_best_cost_plane():
    base = scene.make_views(6, 37, 29, seed=4, with_best_cost=True)
    rng = np.random.default_rng(5)
    depth = base.depth.copy()
    pick = rng.random(depth.shape) < 0.2
    depth[pick] = rng.choice([-1.0, 0.0, -3.0, np.nan, np.inf, -np.inf], size=int(pick.sum()))
    views = _frozen(scene.Views(depth, base.K4, base.RT4, base.best_cost))
    s, _, _ = _check(views, trims=ALL_TRIMS)
    cut, _, _ = _check(views, trims=ALL_TRIMS, threshold=0.7)
    assert 0 < cut.shape[1] < s.shape[1] < B.counted_coordinates(base.depth, base.K4, base.RT4).shape[1]
    # a threshold without costs changes nothing
    same, _, _ = _check(scene.Views(views.depth, views.K4, views.RT4), threshold=0.7)
    assert same.shape == s.shape


def test_points_whose_coordinates_overflow_leave_all_three_axes():
    axes = np.array([[1.7e308, 1.7e308, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    s, lo, hi = _check(_room(), trims=ALL_TRIMS, axes=axes)
    assert 0 < s.shape[1] < B.counted_coordinates(_room().depth, _room().K4, _room().RT4).shape[1]
    assert np.isfinite(lo).all() and np.isfinite(hi).all()


def test_no_point_at_all_gives_nan_and_ok():
    v = _sphere(2)
    for depth in (np.full(v.depth.shape, -1.0), np.full(v.depth.shape, np.nan)):
        lo, hi, n_points, ms = capi.estimate_scene_bounds(scene.Views(depth, v.K4, v.RT4), trim_fraction=0.01)
        assert n_points == 0 and np.isnan(lo).all() and np.isnan(hi).all()
    _check(scene.Views(np.full(v.depth.shape, -1.0), v.K4, v.RT4), trims=(0.0, 0.01, 0.25, 0.5))


def test_two_runs_give_identical_output():
    a = capi.estimate_scene_bounds(_sphere(9), trim_fraction=0.01)
    b = capi.estimate_scene_bounds(_sphere(9), trim_fraction=0.01)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and a[2] > 0


def _raw(views, **change):
    """The C call itself with one argument changed: (status, message, lo, hi, n_points) with the outputs preset to 7."""
    L = capi.load()
    dp = ctypes.POINTER(ctypes.c_double)
    ptr = lambda a: a.ctypes.data_as(dp)
    d = np.ascontiguousarray(views.depth)
    n, H, W = d.shape
    k, rt = np.ascontiguousarray(views.K4).reshape(-1), np.ascontiguousarray(views.RT4).reshape(-1)
    lo, hi, count = np.full(3, 7.0), np.full(3, 7.0), ctypes.c_uint64(7)
    args = dict(depth=ptr(d), best_cost=None, threshold=0.0, K4=ptr(k), RT4=ptr(rt), n=n, W=W, H=H, axes9=None, trim_fraction=0.01,
                pixel_step=1, device=0, lo=ptr(lo), hi=ptr(hi), n_points=ctypes.byref(count), kernel_ms=None)
    keep = [v for v in change.values() if isinstance(v, np.ndarray)]
    args.update({name: ptr(v) if isinstance(v, np.ndarray) else v for name, v in change.items()})
    rc = L.dmi_estimate_scene_bounds(*args.values())
    del keep
    return rc, L.dmi_last_error(None).decode(), lo, hi, count.value


REFUSED = [
    ("depth", dict(depth=None)), ("K4", dict(K4=None)), ("RT4", dict(RT4=None)), ("lo", dict(lo=None)), ("hi", dict(hi=None)),
    ("n_points", dict(n_points=None)), ("n ", dict(n=0)), ("W ", dict(W=0)), ("W ", dict(W=32769)), ("H ", dict(H=0)),
    ("H ", dict(H=40000)), ("trim_fraction", dict(trim_fraction=float("nan"))), ("trim_fraction", dict(trim_fraction=-0.01)),
    ("trim_fraction", dict(trim_fraction=0.5000001)), ("pixel_step", dict(pixel_step=0)), ("pixel_step", dict(pixel_step=-3)),
    ("axes9", dict(axes9=np.array([1.0, 0, 0, 0, np.inf, 0, 0, 0, 1.0]))), ("axes9", dict(axes9=np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, np.nan]))),
    ("threshold", dict(best_cost=np.zeros((3, 29, 37)), threshold=float("nan"))),
    ("n * W * H", dict(n=2**31 - 1, W=32768, H=32768)), ("device", dict(device=1 << 20)),
]


@pytest.mark.parametrize("named,change", REFUSED, ids=[f"{i}-{r[0].strip()}" for i, r in enumerate(REFUSED)])
def test_a_refused_argument_leaves_the_outputs_untouched(named, change):
    rc, message, lo, hi, count = _raw(_sphere(3), **change)
    assert rc == INVALID_ARGUMENT and "dmi_estimate_scene_bounds" in message and named in message, message
    assert (lo == 7.0).all() and (hi == 7.0).all() and count == 7


def test_a_refused_k_names_its_view():
    views = _sphere(3)
    K = views.K4.copy()
    K[2, 1, 0] = 0.25
    rc, message, lo, hi, count = _raw(scene.Views(views.depth, K, views.RT4))
    assert rc == INVALID_ARGUMENT and "view 2" in message and (lo == 7.0).all() and (hi == 7.0).all() and count == 7
    with pytest.raises(capi.DmiError) as e:
        capi.estimate_scene_bounds(views, trim_fraction=0.7)
    assert e.value.code == INVALID_ARGUMENT and "trim_fraction" in str(e.value)
