"""dmi_filter_depth_speckles without a GPU: what the definition does, on its numpy restatement
(depth_speckle_np.py), so that the GPU tests compare against something that is known to label and to filter; the ties of the
LINKED relation; the argument refusals of the C ABI, which come before the device is touched; the command line's three flags."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

import depth_speckle_np as S
from depth_speckle_cases import FMA_PAIR, TIE_PAIRS, random_levels
from test_depth_consistency_np import outlier_scene
from cudadepthmapintegration_amd import capi, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT, DEVICE = 1, 2   # DMI_ERR_INVALID_ARGUMENT, DMI_ERR_DEVICE (include/dmi.h)


def flood_fill_sizes(D, abs_tolerance, rel_tolerance):
    """The definition once more, in plain Python and one pixel at a time: a stack-based flood fill over the 4-neighbours."""
    H, W = len(D), len(D[0])
    valid = lambda v: v > 0.0 and v < float("inf")
    size = [[0] * W for _ in range(H)]
    seen = [[False] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            if seen[y][x] or not valid(D[y][x]):
                continue
            seen[y][x] = True
            stack, members = [(y, x)], []
            while stack:
                cy, cx = stack.pop()
                members.append((cy, cx))
                a = D[cy][cx]
                for ny, nx in ((cy, cx + 1), (cy, cx - 1), (cy + 1, cx), (cy - 1, cx)):
                    if 0 <= ny < H and 0 <= nx < W and not seen[ny][nx] and valid(D[ny][nx]):
                        b = D[ny][nx]
                        product = rel_tolerance * min(a, b)
                        bound = abs_tolerance + product
                        if abs(a - b) <= bound:
                            seen[ny][nx] = True
                            stack.append((ny, nx))
            for cy, cx in members:
                size[cy][cx] = len(members)
    return np.array(size, dtype=np.int32)


def test_restatement_agrees_with_a_flood_fill():
    rng = np.random.default_rng(11)
    for case in range(12):
        if case % 2:
            d = random_levels(rng, 1, 30, 40)[0]
            abs_tol, rel_tol = 0.0, 0.0
        else:                                   # a noisy slope: the links depend on the tolerance
            d = 3.0 + 0.02 * np.arange(40)[None, :] + 0.05 * rng.random((30, 40))
            d[rng.random(d.shape) < 0.15] = -1.0
            abs_tol, rel_tol = 0.01, 0.008
        want = flood_fill_sizes(d.tolist(), abs_tol, rel_tol)
        for min_pixels in (0, 5):
            out, size = S.filter_depth_speckles(d[None], min_pixels, abs_tol, rel_tol)
            assert np.array_equal(size[0], want), case
            keep = (want >= min_pixels) & (d > 0)
            assert np.array_equal(out[0], np.where(keep, d, -1.0)), case
        assert len(np.unique(want)) > 3, case   # (the case has segments of several sizes)


def test_outliers_go_and_the_surface_stays():
    views, valid, sel = outlier_scene()
    out, size = S.filter_depth_speckles(views.depth, 20, 0.0, 0.05)
    kept = out > 0
    clean = valid & ~sel
    print(f"untouched kept {(kept & clean).sum()} of {clean.sum()}, outliers kept {(kept & sel).sum()} of {sel.sum()}")
    assert clean.sum() > 10000 and sel.sum() > 300
    assert (kept & clean).sum() >= 0.95 * clean.sum()
    assert (kept & sel).sum() <= 0.05 * sel.sum()
    assert np.array_equal(out[kept], views.depth[kept]) and (out[~kept] == -1.0).all()
    assert (size[~valid] == 0).all() and np.array_equal(kept, valid & (size >= 20))


def test_ties_of_the_linked_relation():
    for a, b, abs_tol, rel_tol, want in TIE_PAIRS:
        for pair in ((a, b), (b, a)):                            # the relation is symmetric
            for image in (np.array([[pair]]), np.array([[pair]]).transpose(0, 2, 1)):   # side by side, and one above the other
                out, size = S.filter_depth_speckles(image, 2, abs_tol, rel_tol)
                assert (size == (2 if want else 1)).all(), (a, b, abs_tol, rel_tol)
                assert (out == (image if want else -1.0)).all()
    # fmin, not fmax: with the larger depth the fourth pair would link
    a, b, _, rel_tol, _ = TIE_PAIRS[3]
    assert abs(a - b) <= rel_tol * max(a, b) and not abs(a - b) <= rel_tol * min(a, b)
    # the searched pair in exact arithmetic: product and sum rounded separately reach the difference, one rounding does not
    a, b, abs_tol, rel_tol, want = FMA_PAIR
    separately = float(np.float64(abs_tol) + np.float64(rel_tol) * np.float64(a))
    contracted = float(Fraction(abs_tol) + Fraction(rel_tol) * Fraction(a))   # (Fraction -> float rounds correctly, once)
    difference = float(np.float64(b) - np.float64(a))
    assert Fraction(b) - Fraction(a) == Fraction(difference)
    assert want and difference <= separately and not difference <= contracted


def test_a_segment_of_exactly_min_pixels_stays():
    d = np.full((1, 9, 11), -1.0)
    d[0, 2, 1:8] = 3.0              # 7 in a row
    d[0, 3:6, 7] = 3.0              # and 3 below its end: 10 pixels
    d[0, 7, 0:4] = 3.0              # 4 elsewhere
    for n, kept in ((4, 14), (5, 10), (10, 10), (11, 0)):
        out, size = S.filter_depth_speckles(d, n)
        assert int((out > 0).sum()) == kept, n
        assert sorted(np.unique(size).tolist()) == [0, 4, 10]
    assert (size[0, 2, 1:8] == 10).all() and (size[0, 7, 0:4] == 4).all()


def test_min_pixels_zero_normalises_every_invalid_kind():
    d = np.full((2, 5, 6), 2.0)
    d[0, 0, :6] = [0.0, -3.0, np.nan, np.inf, -np.inf, -1.0]
    out, size = S.filter_depth_speckles(d, 0)
    assert (out[0, 0] == -1.0).all() and (size[0, 0] == 0).all()
    assert (out[0, 1:] == 2.0).all() and (size[0, 1:] == 24).all() and (out[1] == 2.0).all() and (size[1] == 30).all()


def test_best_cost_threshold_comes_first():
    d = np.full((1, 4, 5), 2.0)
    cost = np.full((1, 4, 5), 0.5)
    cost[0, :, 2] = [0.7, np.nan, 0.7000000000000001, 0.9]      # equal to the threshold stays, NaN stays, above goes
    out, size = S.filter_depth_speckles(d, 0, best_cost=cost, threshold=0.7)
    assert out[0, :, 2].tolist() == [2.0, 2.0, -1.0, -1.0] and size[0, :, 2].tolist() == [18, 18, 0, 0]
    assert (size[0][out[0] > 0] == 18).all()
    a, sa = S.filter_depth_speckles(d, 10, best_cost=cost, threshold=0.7)
    b, sb = S.filter_depth_speckles(np.where(cost > 0.7, -1.0, d), 10)
    assert a.tobytes() == b.tobytes() and np.array_equal(sa, sb)


# ---- the C ABI's refusals: all before the device is touched --------------------------------------------------------------------
def _call(depth, *, best_cost=None, threshold=0.0, n=None, W=None, H=None, abs_tol=0.0, rel_tol=0.0, min_pixels=1, null=()):
    L = capi.load()
    d = np.ascontiguousarray(depth, dtype=np.float64)
    out = np.full(d.shape, 7.0)
    size = np.full(d.shape, 7, dtype=np.int32)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    bc = None if best_cost is None else np.ascontiguousarray(best_cost, dtype=np.float64)
    rc = L.dmi_filter_depth_speckles(None if "depth" in null else dp(d), None if bc is None else dp(bc), threshold,
                                     d.shape[0] if n is None else n, d.shape[2] if W is None else W, d.shape[1] if H is None else H,
                                     abs_tol, rel_tol, min_pixels, 0, None if "out_depth" in null else dp(out),
                                     size.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None)
    assert (out == 7.0).all() and (size == 7).all()           # a refused call leaves out_depth and out_size untouched
    return rc, L.dmi_last_error(None).decode()


def test_header_symbol_list_and_library_agree():
    header = open(os.path.join(ROOT, "include", "dmi.h")).read()
    assert "int dmi_filter_depth_speckles(" in header and "dmi_filter_depth_speckles" in capi.ABI_SYMBOLS
    L = capi.load()
    assert hasattr(L, "dmi_filter_depth_speckles") and L.dmi_abi_version() == 5
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for words in ("fabs(Da - Db) <= abs_tolerance + rel_tolerance * fmin(Da, Db)", "A pixel is VALID iff D > 0 and D < +inf"):
        assert words in header and words in design, words


def test_argument_refusals_name_the_argument():
    d = np.full((2, 6, 8), 2.0)
    for name in ("depth", "out_depth"):
        rc, text = _call(d, null=(name,))
        assert rc == INVALID_ARGUMENT and "dmi_filter_depth_speckles" in text and name in text, text
    for kwargs, name in (({"n": 0}, "n >= 1"), ({"n": -1}, "n >= 1"), ({"W": 0}, "W must"), ({"W": 32769}, "W must"), ({"H": 0}, "H must"),
                         ({"H": 32769}, "H must"), ({"min_pixels": -1}, "min_pixels"),
                         ({"abs_tol": -1.0}, "abs_tolerance"), ({"abs_tol": np.nan}, "abs_tolerance"), ({"abs_tol": np.inf}, "abs_tolerance"),
                         ({"rel_tol": -0.5}, "rel_tolerance"), ({"rel_tol": np.nan}, "rel_tolerance"), ({"rel_tol": np.inf}, "rel_tolerance"),
                         ({"best_cost": np.zeros_like(d), "threshold": np.nan}, "threshold")):
        rc, text = _call(d, **kwargs)
        assert rc == INVALID_ARGUMENT and name in text, (kwargs, text)


def test_python_binding_raises_with_the_code():
    v = scene.make_views(2, 8, 6, seed=0)
    with pytest.raises(capi.DmiError) as e:
        capi.filter_depth_speckles(v, min_pixels=-1)
    assert e.value.code == INVALID_ARGUMENT and "min_pixels" in str(e.value)
    with pytest.raises(capi.DmiError) as e:
        capi.filter_depth_speckles(v, min_pixels=1, rel_tolerance=float("nan"))
    assert e.value.code == INVALID_ARGUMENT and "rel_tolerance" in str(e.value)
    b = scene.make_views(2, 8, 6, seed=0, with_best_cost=True)
    with pytest.raises(capi.DmiError) as e:
        capi.filter_depth_speckles(b, min_pixels=1, threshold=float("nan"))
    assert e.value.code == INVALID_ARGUMENT and "threshold" in str(e.value)


def test_without_a_device_a_valid_call_fails_loudly():
    """Only after every argument has passed is the device looked for: where there is none, that is the error."""
    v = scene.make_views(2, 8, 6, seed=0)
    if capi.device_count() > 0:
        out, sizes, ms = capi.filter_depth_speckles(v, min_pixels=0)
        assert out.depth.tobytes() == v.depth.tobytes() and ms > 0
        return
    with pytest.raises(capi.DmiError) as e:
        capi.filter_depth_speckles(v, min_pixels=1)
    assert e.value.code == DEVICE and "dmi_filter_depth_speckles" in str(e.value)


# ---- the command line ------------------------------------------------------------------------------------------------------------
BASE = ["prog", "--gridOrigin", "-2.29", "-2.24", "-2.2", "--gridEnd", "1.19", "1.67", "1.22", "--dataFolder", "data",
        "--outputGridFilename", "out.vts", "--outputMeshFilename", "mesh.vtp", "--rayThick", "0.1", "--gridDims", "10"]


def test_cli_reads_the_three_flags():
    o, text = capi.cli_read_arguments(BASE)
    assert o is not None and o.depth_speckle_min_pixels == -1, text
    assert (o.depth_speckle_tolerance, o.depth_speckle_rel_tolerance) == (0.0, 0.01)
    o, text = capi.cli_read_arguments(BASE + ["--depthSpeckleMinPixels", "50"])
    assert o is not None and o.depth_speckle_min_pixels == 50 and o.depth_consistency_min_views == -1, text
    assert (o.depth_speckle_tolerance, o.depth_speckle_rel_tolerance) == (0.0, 0.01)
    o, text = capi.cli_read_arguments(BASE + ["--depthSpeckleMinPixels", "0", "--depthSpeckleTolerance", "0.25",
                                              "--depthSpeckleRelTolerance", "0", "--depthConsistencyMinViews", "2"])
    assert o is not None and o.depth_speckle_min_pixels == 0 and o.depth_consistency_min_views == 2, text
    assert (o.depth_speckle_tolerance, o.depth_speckle_rel_tolerance) == (0.25, 0.0)


def test_cli_refuses_dependent_and_out_of_range_forms():
    for flag in ("--depthSpeckleTolerance", "--depthSpeckleRelTolerance"):
        o, text = capi.cli_read_arguments(BASE + [flag, "0.1"])
        assert o is None and text.startswith(f"Error : {flag} needs --depthSpeckleMinPixels"), text
        for value in ("-1", "nan", "inf", "-inf", "x", ""):
            o, text = capi.cli_read_arguments(BASE + ["--depthSpeckleMinPixels", "1", flag, value])
            assert o is None and text.startswith(f"Bad value for {flag}"), (value, text)
    for value in ("-1", "1.5", "x", ""):
        o, text = capi.cli_read_arguments(BASE + ["--depthSpeckleMinPixels", value])
        assert o is None and text.startswith("Bad value for --depthSpeckleMinPixels"), (value, text)
    o, text = capi.cli_read_arguments(BASE + ["--help"])
    assert o is None
    for flag in ("--depthSpeckleMinPixels v", "--depthSpeckleTolerance v", "--depthSpeckleRelTolerance v"):
        assert flag in text and "not in the reference" in text.split(flag)[1].split("--help")[0], flag
    assert "image resolution" in text.split("--depthSpeckleRelTolerance v")[1].split("--gridAutoBounds")[0]
