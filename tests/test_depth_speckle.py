"""dmi_filter_depth_speckles on the GPU against its numpy restatement (depth_speckle_np.py), bit for bit in
out_depth and out_size, or against closed forms where the case has one: image sizes around the 64 x 32 tile, segments that cross
every tile border, segments made of many tile-local roots, the ties of the LINKED relation placed on tile borders, view borders
and row ends, and more than one staged piece.  Every case is milliseconds of kernels."""
import ctypes
import functools

import numpy as np
import pytest

import depth_speckle_np as S
from depth_speckle_cases import TIE_PAIRS, random_blobs, random_levels
from cudadepthmapintegration_amd import capi, scene

pytestmark = pytest.mark.gpu


def _views(depth, best_cost=None):
    eye = np.tile(np.eye(4), (depth.shape[0], 1, 1))
    return scene.Views(depth, eye, eye, best_cost)


def _gpu(depth, min_pixels, abs_tolerance=0.0, rel_tolerance=0.0, best_cost=None, threshold=None, **kwargs):
    out, size, ms = capi.filter_depth_speckles(_views(depth, best_cost), min_pixels=min_pixels, abs_tolerance=abs_tolerance,
                                               rel_tolerance=rel_tolerance, threshold=threshold, **kwargs)
    assert ms > 0 and out.best_cost is None
    return out.depth, size


def _same_as_restatement(depth, min_pixels, abs_tolerance=0.0, rel_tolerance=0.0, best_cost=None, threshold=None):
    out, size = _gpu(depth, min_pixels, abs_tolerance, rel_tolerance, best_cost, threshold)
    want, want_size = S.filter_depth_speckles(depth, min_pixels, abs_tolerance, rel_tolerance, best_cost, threshold)
    assert size.dtype == np.int32 and np.array_equal(size, want_size)
    assert out.tobytes() == want.tobytes()
    return out, size


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("W,H", [(1, 1), (70, 1), (1, 70), (63, 31), (64, 32), (65, 33), (129, 67)])
def test_sizes_around_the_tile(W, H, n):
    d = random_levels(np.random.default_rng(1000 * W + 10 * H + n), n, H, W)
    for min_pixels in (0, 3):
        out, size = _same_as_restatement(d, min_pixels)
    if W * H > 1000:
        assert 0 < (out > 0).sum() < (d > 0).sum() and size.max() > 3


@functools.lru_cache(maxsize=None)
def _serpentine():
    """(valid mask [150, 200] of a one-pixel-wide path through every even row, its length): row y runs left to right for y / 2
    even and right to left otherwise, and a pixel on the odd row below its last column leads on to the next."""
    W, H = 200, 150
    valid = np.zeros((H, W), dtype=bool)
    valid[0::2, :] = True
    for y in range(0, H - 2, 2):
        valid[y + 1, W - 1 if (y // 2) % 2 == 0 else 0] = True
    valid.setflags(write=False)
    return valid, 75 * W + 74


def test_serpentine_is_one_segment():
    valid, length = _serpentine()
    assert int(valid.sum()) == length == 15074
    d = np.where(valid, 2.0, -1.0)[None]
    out, size = _same_as_restatement(d, length)
    assert (size[0][valid] == length).all() and (size[0][~valid] == 0).all() and out.tobytes() == d.tobytes()
    assert (_gpu(d, length + 1)[0] == -1.0).all()


def test_serpentine_cut_by_one_depth_step():
    """Row 74 runs right to left (74 / 2 is odd): the step between columns 150 and 149 leaves 37 rows, 37 connecting pixels and
    columns 199..150 before it."""
    valid, length = _serpentine()
    first = np.zeros_like(valid)
    first[:74] = valid[:74]
    first[74, 150:] = True
    a, b = 37 * 200 + 37 + 50, length - (37 * 200 + 37 + 50)
    assert int(first.sum()) == a == 7487 and b == 7587
    d = np.where(valid, np.where(first, 2.0, 3.0), -1.0)[None]
    out, size = _same_as_restatement(d, 7500, abs_tolerance=0.5)
    assert (size[0][first] == a).all() and (size[0][valid & ~first] == b).all()
    assert np.array_equal(out[0] > 0, valid & ~first)
    assert ((_gpu(d, 7500, abs_tolerance=1.0)[1][0] == length) == valid).all()       # the step within the tolerance: one segment again


def test_checkerboard_has_no_diagonal_links():
    yy, xx = np.mgrid[0:50, 0:70]
    d = np.where((xx + yy) % 2 == 0, 2.0, -1.0)[None]
    for min_pixels in (0, 1):
        out, size = _same_as_restatement(d, min_pixels)
        assert out.tobytes() == d.tobytes() and np.array_equal(size[0], (d[0] > 0).astype(np.int32))
    assert (_gpu(d, 2)[0] == -1.0).all()


def test_comb_joined_in_the_tile_below():
    """A hundred teeth on every second column of the first row of tiles, joined only by a bar in the first row of the tiles below:
    32 tile-local roots per tile become one segment through the border pass, and its size is a sum over a hundred adds."""
    d = np.full((1, 40, 200), -1.0)
    d[0, :32, 0::2] = 2.0
    d[0, 32, :] = 2.0
    total = 100 * 32 + 200
    out, size = _same_as_restatement(d, total)
    assert (size[0][d[0] > 0] == total).all() and out.tobytes() == d.tobytes()
    d[0, 32, 101] = -1.0          # the bar cut under a gap: 51 teeth and 101 of the bar, 49 teeth and 98
    out, size = _same_as_restatement(d, 51 * 32 + 101)
    assert sorted(np.unique(size).tolist()) == [0, 49 * 32 + 98, 51 * 32 + 101]
    assert int((out > 0).sum()) == 51 * 32 + 101


@pytest.mark.parametrize("pair", range(len(TIE_PAIRS)))
def test_ties_on_tile_borders_view_borders_and_row_ends(pair):
    a, b, abs_tol, rel_tol, linked = TIE_PAIRS[pair]
    W, H = 130, 70
    d = np.full((2, H, W), -1.0)
    d[0, 5, 63], d[0, 5, 64] = a, b                    # across a vertical tile border
    d[0, 31, 10], d[0, 32, 10] = b, a                  # across a horizontal one
    d[0, 31, 63], d[0, 31, 64], d[0, 32, 63], d[0, 32, 64] = a, b, b, a     # round a tile corner
    d[0, H - 1, 7], d[1, 0, 7] = a, a                  # the last row of view 0 above the first of view 1: never neighbours
    d[1, 10, W - 1], d[1, 11, 0] = a, a                # the end of a row and the start of the next: never neighbours
    out, size = _same_as_restatement(d, 2, abs_tol, rel_tol)
    two, four = (2, 4) if linked else (1, 1)
    assert size[0, 5, 63:65].tolist() == [two, two] and size[0, 31:33, 10].tolist() == [two, two]
    assert size[0, 31:33, 63:65].reshape(-1).tolist() == [four] * 4
    assert size[0, H - 1, 7] == 1 and size[1, 0, 7] == 1 and size[1, 10, W - 1] == 1 and size[1, 11, 0] == 1
    assert int((out > 0).sum()) == (8 if linked else 0)


@pytest.mark.parametrize("n", [1, 3])
def test_one_segment_covers_the_view(n):
    d = np.full((n, 200, 300), 2.0)
    out, size = _gpu(d, 60000)
    assert (size == 60000).all() and out.tobytes() == d.tobytes()
    out, size = _gpu(d, 60001)                        # min_pixels above W * H
    assert (size == 60000).all() and (out == -1.0).all()
    out, size = _gpu(d, 1 << 40)
    assert (size == 60000).all() and (out == -1.0).all()


def test_every_kind_of_invalid_depth():
    d = np.full((2, 40, 70), 2.0)
    d[0, 3, :6] = [0.0, -3.0, np.nan, np.inf, -np.inf, -1.0]
    d[1, 35, 64:70] = [np.nan, -0.0, np.inf, -1e300, -np.inf, 5e-324]     # (the smallest denormal is a valid depth, on its own)
    out, size = _same_as_restatement(d, 0)
    assert (out[0, 3, :6] == -1.0).all() and (size[0, 3, :6] == 0).all() and (size[0][out[0] > 0] == 40 * 70 - 6).all()
    assert (out[1, 35, 64:69] == -1.0).all() and out[1, 35, 69] == 5e-324 and size[1, 35, 69] == 1
    _same_as_restatement(d, 2)


def test_best_cost_plane():
    rng = np.random.default_rng(5)
    d = random_levels(rng, 3, 67, 129, valid_share=0.95)
    cost = rng.random(d.shape)
    cost[0, 0, :4] = [0.5, np.nan, np.nextafter(0.5, 1.0), np.inf]        # equal to the threshold stays, NaN stays
    d[0, 0, :4] = 2.0
    out, size = _same_as_restatement(d, 4, best_cost=cost, threshold=0.5)
    assert (size[0, 0, :2] > 0).all() and (size[0, 0, 2:4] == 0).all()
    assert 0 < (out > 0).sum() < ((d > 0) & ~(cost > 0.5)).sum()
    plain, plain_size = _gpu(np.where(cost > 0.5, -1.0, d), 4)
    assert plain.tobytes() == out.tobytes() and np.array_equal(plain_size, size)


@functools.lru_cache(maxsize=None)
def _blobs():
    d = random_blobs(np.random.default_rng(21), 12, 97, 131)
    want = S.filter_depth_speckles(d, 30, 0.0, 0.01)
    for a in (d,) + want:
        a.setflags(write=False)
    return d, want


def test_random_blobs_on_a_slope():
    d, (want, want_size) = _blobs()
    out, size = _gpu(d, 30, rel_tolerance=0.01)
    assert np.array_equal(size, want_size) and out.tobytes() == want.tobytes()
    assert 0 < (out > 0).sum() < (d > 0).sum() and len(np.unique(size)) > 20


def test_two_runs_are_identical_and_in_place_is_the_same():
    d, (want, want_size) = _blobs()
    first, second = _gpu(d, 30, rel_tolerance=0.01), _gpu(d, 30, rel_tolerance=0.01)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    work = d.copy()
    out, size = _gpu(work, 30, rel_tolerance=0.01, out=work)
    assert out is work and work.tobytes() == want.tobytes() and np.array_equal(size, want_size)


def test_out_size_and_kernel_ms_may_be_null():
    d, (want, _) = _blobs()
    L = capi.load()
    src, out = np.ascontiguousarray(d), np.full(d.shape, 7.0)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    n, H, W = d.shape
    rc = L.dmi_filter_depth_speckles(dp(src), None, 0.0, n, W, H, 0.0, 0.01, 30, 0, dp(out), None, None)
    assert rc == 0, L.dmi_last_error(None).decode()
    assert out.tobytes() == want.tobytes()


def test_more_than_one_staged_piece():
    """5 views of 3000 x 3000 (360 MB: pieces of three views and of two): view k holds the depth k + 1, cut into four quadrants by a
    cross of -1 at row 1000 and column 1700.  Every size has a closed form; no restatement runs at this size."""
    n, W, H, cy, cx = 5, 3000, 3000, 1000, 1700
    d = np.empty((n, H, W))
    for k in range(n):
        d[k] = k + 1.0
    d[:, cy, :] = -1.0
    d[:, :, cx] = -1.0
    quadrants = [(slice(0, cy), slice(0, cx), cy * cx), (slice(0, cy), slice(cx + 1, W), cy * (W - cx - 1)),
                 (slice(cy + 1, H), slice(0, cx), (H - cy - 1) * cx), (slice(cy + 1, H), slice(cx + 1, W), (H - cy - 1) * (W - cx - 1))]
    assert sorted(q[2] for q in quadrants) == [1299000, 1700000, 2596701, 3398300]
    out, size = _gpu(d, 2000000, out=d)               # in place: the host holds the planes once
    assert out is d
    assert (size[:, cy, :] == 0).all() and (size[:, :, cx] == 0).all() and (d[:, cy, :] == -1.0).all() and (d[:, :, cx] == -1.0).all()
    for rows, cols, pixels in quadrants:
        assert (size[:, rows, cols] == pixels).all(), pixels
        for k in range(n):
            assert (d[k, rows, cols] == (k + 1.0 if pixels >= 2000000 else -1.0)).all(), (k, pixels)
