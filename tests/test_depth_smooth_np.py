"""dmi_smooth_depths without a GPU: what the definition does, on its numpy restatement (depth_smooth_np.py) against
closed forms, so that the GPU tests compare against something that is known to stop at edges, to settle ties and to keep what is
not valid; what the smoothing is for, on the `noisy` scene; the argument refusals of the C ABI, which come before the device is
touched."""
import ctypes
import os

import numpy as np
import pytest

import depth_smooth_np as S
from cudadepthmapintegration_amd import capi, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT, DEVICE = 1, 2   # DMI_ERR_INVALID_ARGUMENT, DMI_ERR_DEVICE (include/dmi.h)
INVALID_KINDS = (0.0, -3.0, np.nan, np.inf, -np.inf, -1.0, -0.0)


def weights(sigma, truncate=2.0):
    return capi.depth_smoothing_weights(sigma, truncate)


def noisy_scene():
    """The scene of the quality condition: (noisy depths, noise-free depths, one voxel's spacing)."""
    spacing = float(scene.default_grid(64).spacing[0])
    noisy, _ = scene.make_scene_views("noisy", 3, 320, 240, seed=1, holes=3, noise_sigma=spacing)
    clean, _ = scene.make_scene_views("noisy", 3, 320, 240, seed=1, holes=3, noise_sigma=0.0)
    return noisy.depth, clean.depth, spacing


def test_library_weights_follow_the_rule():
    for sigma, truncate, r in ((1.5, 2.0, 3), (4.0, 2.0, 8), (0.5, 2.0, 1), (0.0, 2.0, 0), (1.0, 3.0, 3), (2.0, 4.0, 8)):
        s, mine = weights(sigma, truncate), S.spatial_weights(sigma, truncate)
        assert len(s) == r + 1 and s[0] == 1.0
        assert np.all(np.abs(s - mine) <= np.spacing(mine))  # libm's exp and Python's within an ulp
    for sigma, truncate in ((-1.0, 2.0), (np.nan, 2.0), (np.inf, 2.0), (1.0, 0.0), (1.0, 4.5), (1.0, np.nan), (4.01, 2.0), (2.01, 4.0)):
        with pytest.raises(capi.DmiError) as e:
            weights(sigma, truncate)
        assert e.value.code == INVALID_ARGUMENT and "dmi_depth_smoothing_weights" in str(e.value), (sigma, truncate)


def test_plateaus_on_both_sides_of_a_step_come_out_bit_identical():
    d = np.full((1, 12, 20), 2.0)
    d[:, :, 9:] = 3.0
    out, count = S.smooth_depths(d, weights(1.5), abs_tolerance=0.5, iterations=3)
    assert out.tobytes() == d.tobytes()
    assert count[0, 6, 3] == 49 and count[0, 6, 8] == 7 * 4 and count[0, 6, 9] == 7 * 4 and count[0, 0, 0] == 16


def test_the_tie_is_not_taken_and_one_ulp_more_is():
    d = np.full((1, 5, 5), 2.0)
    d[0, 2, 3] = 2.5                                   # |delta| == tau exactly at the centre (2, 2) and its seven other neighbours
    out, count = S.smooth_depths(d, weights(0.5), abs_tolerance=0.5)
    assert count[0, 2, 2] == 8 and count[0, 2, 3] == 1 and out.tobytes() == d.tobytes()
    more = np.nextafter(0.5, 1.0)
    out, count = S.smooth_depths(d, weights(0.5), abs_tolerance=more)
    assert count[0, 2, 2] == 9 and count[0, 2, 3] == 9
    # the tap is taken with g = T - u of an ulp of T: its weight is 1e-32 of the centre's and moves nothing
    assert out[0, 2, 2] == 2.0 and out[0, 2, 3] == 2.5


def test_a_taken_tap_whose_weight_underflows_counts_and_adds_nothing():
    c, step = 2.0 ** -240, 2.0 ** -250
    d = np.full((1, 3, 3), c)
    d[0, 1, 2] = c + step
    out, count = S.smooth_depths(d, weights(0.5), abs_tolerance=np.nextafter(step, 1.0))
    g = np.nextafter(step, 1.0) ** 2 - step * step
    assert g > 0.0 and g * g == 0.0                     # (T - u)^2 underflows to zero ...
    assert count[0, 1, 1] == 9 and out.tobytes() == d.tobytes()   # ... the tap is counted all the same


def test_the_interior_of_a_linear_slope_is_reproduced():
    yy, xx = np.mgrid[0:24, 0:30]
    d = (5.0 + 0.013 * xx - 0.007 * yy)[None]
    out, count = S.smooth_depths(d, weights(1.5), abs_tolerance=1.0, iterations=2)
    inner = (slice(None), slice(6, -6), slice(6, -6))
    assert (count[inner] == 49).all()
    assert np.max(np.abs(out[inner] - d[inner]) / d[inner]) <= 1e-12
    assert np.max(np.abs(out - d)) > 1e-4               # the border rows do move: their windows are one-sided


def test_radius_zero_and_zero_tolerances_are_the_identity():
    rng = np.random.default_rng(5)
    d = rng.uniform(1.0, 9.0, (2, 9, 11))
    d[rng.random(d.shape) < 0.2] = -1.0
    out, count = S.smooth_depths(d, weights(0.0), abs_tolerance=0.5, rel_tolerance=0.1, iterations=2)
    assert out.tobytes() == d.tobytes() and np.array_equal(count, (d > 0).astype(np.int32))
    out, count = S.smooth_depths(d, weights(1.5), abs_tolerance=0.0, rel_tolerance=0.0)
    assert out.tobytes() == d.tobytes() and (count == 0).all()


def test_every_kind_of_invalid_depth_comes_out_as_minus_one():
    d = np.full((1, 4, len(INVALID_KINDS) + 2), 2.0)
    for i, bad in enumerate(INVALID_KINDS):
        d[0, 1, 1 + i] = bad
    out, count = S.smooth_depths(d, weights(1.0), abs_tolerance=0.5)
    assert (out[0, 1, 1:-1] == -1.0).all() and not np.signbit(out[0, 0]).any() and (count[0, 1, 1:-1] == 0).all()
    keep = S.valid_pixels(d)
    assert (out[keep] == 2.0).all() and (count[keep] > 0).all()


def test_best_cost_above_the_threshold_only():
    d = np.full((1, 5, 5), 2.0)
    cost = np.zeros((1, 5, 5))
    cost[0, 2, 2] = 0.75                   # above: the pixel has no depth
    cost[0, 1, 1] = 0.5                    # equal: it stays
    cost[0, 3, 3] = np.nan                 # a NaN cost does not exceed the threshold
    out, count = S.smooth_depths(d, weights(0.5), abs_tolerance=0.5, best_cost=cost, threshold=0.5)
    assert out[0, 2, 2] == -1.0 and count[0, 2, 2] == 0 and (out == -1.0).sum() == 1
    assert count[0, 1, 1] == 8 and count[0, 3, 3] == 8 and count[0, 0, 4] == 4


def test_taps_cross_neither_row_ends_nor_view_seams():
    d = np.full((2, 4, 5), 2.0)
    d[0, 1, 4] = 2.25                      # the end of row 1: row 2's first pixel is its successor in memory
    d[0, 3, 2] = 2.25                      # the last row of view 0: view 1's first row follows it in memory
    out, count = S.smooth_depths(d, weights(0.5), abs_tolerance=0.5)
    assert out[0, 2, 0] == 2.0 and out[0, 1, 0] == 2.0 and (out[0, :, 0] == 2.0).all()
    assert (out[1] == 2.0).all()
    assert count[0, 0, 0] == 4 and count[0, 2, 0] == 6 and count[1, 0, 2] == 6 and count[0, 1, 1] == 9
    assert out[0, 1, 3] > 2.0 and out[0, 2, 2] > 2.0
    both, _ = S.smooth_depths(d, weights(0.5), abs_tolerance=0.5)
    for m in range(2):
        alone, _ = S.smooth_depths(d[m:m + 1], weights(0.5), abs_tolerance=0.5)
        assert alone.tobytes() == both[m:m + 1].tobytes()


def test_no_pixel_moves_further_than_its_tolerance():
    rng = np.random.default_rng(11)
    d = rng.uniform(2.0, 3.0, (2, 40, 50))
    d[rng.random(d.shape) < 0.1] = -1.0
    a, rel = 0.2, 0.05
    out, _ = S.smooth_depths(d, weights(1.5), abs_tolerance=a, rel_tolerance=rel)
    keep = d > 0
    tau = a + rel * d[keep]
    assert (np.abs(out[keep] - d[keep]) <= tau * (1 + 1e-12)).all() and np.abs(out[keep] - d[keep]).max() > 0.05
    assert np.array_equal(out == -1.0, ~keep)


def test_two_iterations_are_two_single_calls():
    rng = np.random.default_rng(12)
    d = rng.uniform(2.0, 2.4, (1, 30, 33))
    d[rng.random(d.shape) < 0.1] = -1.0
    s = weights(1.0)
    twice, count = S.smooth_depths(d, s, abs_tolerance=0.3, iterations=2)
    first, _ = S.smooth_depths(d, s, abs_tolerance=0.3)
    second, count2 = S.smooth_depths(first, s, abs_tolerance=0.3)
    assert twice.tobytes() == second.tobytes() and np.array_equal(count, count2) and twice.tobytes() != first.tobytes()


def test_quality_on_the_noisy_scene():
    """sigma 1.5, truncate 2, a = 3 x spacing, rel 0 on 3 views of 320 x 240 with noise of one voxel spacing: RMS against the
    noise-free scene 0.03122 unsmoothed, 0.01653 (0.53) after one iteration, 0.00758 (0.24) after two."""
    noisy, clean, spacing = noisy_scene()
    keep = S.valid_pixels(noisy)
    rms = lambda D: float(np.sqrt(np.mean((D[keep] - clean[keep]) ** 2)))
    s = weights(1.5, 2.0)
    base = rms(noisy)
    one, _ = S.smooth_depths(noisy, s, abs_tolerance=3 * spacing)
    two, _ = S.smooth_depths(noisy, s, abs_tolerance=3 * spacing, iterations=2)
    print("rms", base, rms(one), rms(one) / base, rms(two), rms(two) / base)
    assert rms(one) <= 0.6 * base
    assert rms(two) <= 0.3 * base
    assert np.array_equal(S.valid_pixels(one), keep) and np.array_equal(S.valid_pixels(two), keep)
    assert (np.abs(one[keep] - noisy[keep]) <= 3 * spacing * (1 + 1e-12)).all()


# ---- the C ABI's refusals: all before the device is touched --------------------------------------------------------------------
def _call(depth, *, best_cost=None, threshold=0.0, n=None, W=None, H=None, sigma=1.0, truncate=2.0, abs_tol=0.5, rel_tol=0.0,
          iterations=1, null=()):
    L = capi.load()
    d = np.ascontiguousarray(depth, dtype=np.float64)
    out = np.full(d.shape, 7.0)
    count = np.full(d.shape, 7, dtype=np.int32)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    bc = None if best_cost is None else np.ascontiguousarray(best_cost, dtype=np.float64)
    rc = L.dmi_smooth_depths(None if "depth" in null else dp(d), None if bc is None else dp(bc), threshold,
                             d.shape[0] if n is None else n, d.shape[2] if W is None else W, d.shape[1] if H is None else H,
                             sigma, truncate, abs_tol, rel_tol, iterations, 0, None if "out_depth" in null else dp(out),
                             count.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None)
    assert (out == 7.0).all() and (count == 7).all()          # a refused call leaves out_depth and out_count untouched
    return rc, L.dmi_last_error(None).decode()


def check_argument_refusals():
    d = np.full((2, 6, 8), 2.0)
    for name in ("depth", "out_depth"):
        rc, text = _call(d, null=(name,))
        assert rc == INVALID_ARGUMENT and "dmi_smooth_depths" in text and name in text, text
    for kwargs, name in (({"n": 0}, "n >= 1"), ({"n": -1}, "n >= 1"), ({"W": 0}, "W must"), ({"W": 32769}, "W must"), ({"H": 0}, "H must"),
                         ({"H": 32769}, "H must"),
                         ({"sigma": -1.0}, "sigma"), ({"sigma": np.nan}, "sigma"), ({"sigma": np.inf}, "sigma"),
                         ({"truncate": 0.0}, "truncate"), ({"truncate": -1.0}, "truncate"), ({"truncate": 4.5}, "truncate"),
                         ({"truncate": np.nan}, "truncate"), ({"truncate": np.inf}, "truncate"),
                         ({"sigma": 4.01, "truncate": 2.0}, "radius"), ({"sigma": 9.0, "truncate": 1.0}, "radius"),
                         ({"abs_tol": -1.0}, "abs_tolerance"), ({"abs_tol": np.nan}, "abs_tolerance"), ({"abs_tol": np.inf}, "abs_tolerance"),
                         ({"rel_tol": -0.5}, "rel_tolerance"), ({"rel_tol": np.nan}, "rel_tolerance"), ({"rel_tol": np.inf}, "rel_tolerance"),
                         ({"iterations": 0}, "iterations"), ({"iterations": -2}, "iterations"), ({"iterations": 17}, "iterations"),
                         ({"best_cost": np.zeros_like(d), "threshold": np.nan}, "threshold")):
        rc, text = _call(d, **kwargs)
        assert rc == INVALID_ARGUMENT and name in text, (kwargs, text)


def test_argument_refusals_name_the_argument():
    check_argument_refusals()


def test_header_symbol_list_and_library_agree():
    header = open(os.path.join(ROOT, "include", "dmi.h")).read()
    L = capi.load()
    for symbol in ("dmi_smooth_depths", "dmi_depth_smoothing_weights"):
        assert f"int {symbol}(" in header and symbol in capi.ABI_SYMBOLS and hasattr(L, symbol)
    assert L.dmi_abi_version() == 5
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for words in ("tau = abs_tolerance + rel_tolerance * c;   T = tau * tau;   num = 0;  den = 0;  count = 0",
                  "delta = q - c;  u = delta * delta", "w = (s[|dy|] * s[|dx|]) * (g * g)",
                  "num = num + w * delta;  den = den + w;  count += 1", "out = c + num / den",
                  "if !(den > 0 && den < inf && out > 0 && out < inf): out = c", "r = (int)ceil(truncate * sigma)",
                  "s[i] = exp(-(double)(i*i) / (2*sigma*sigma))"):
        assert words in header and words in design, words


def test_python_binding_raises_with_the_code():
    v = scene.make_views(2, 8, 6, seed=0)
    with pytest.raises(capi.DmiError) as e:
        capi.smooth_depths(v, sigma=-1.0)
    assert e.value.code == INVALID_ARGUMENT and "sigma" in str(e.value)
    with pytest.raises(capi.DmiError) as e:
        capi.smooth_depths(v, sigma=1.0, iterations=17)
    assert e.value.code == INVALID_ARGUMENT and "iterations" in str(e.value)


def test_without_a_device_a_valid_call_fails_loudly():
    """Only after every argument has passed is the device looked for: where there is none, that is the error."""
    v = scene.make_views(2, 8, 6, seed=0)
    if capi.device_count() > 0:
        out, counts, ms = capi.smooth_depths(v, sigma=0.0, abs_tolerance=1.0)
        assert out.depth.tobytes() == np.where(S.valid_pixels(v.depth), v.depth, -1.0).tobytes() and ms > 0
        return
    with pytest.raises(capi.DmiError) as e:
        capi.smooth_depths(v, sigma=1.0, abs_tolerance=1.0)
    assert e.value.code == DEVICE and "dmi_smooth_depths" in str(e.value)
