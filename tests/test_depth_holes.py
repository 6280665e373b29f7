"""dmi_fill_depth_holes on the GPU against its numpy restatement (depth_holes_np.py), bit for bit in out_depth and
out_size, or against closed forms where the case has one: image sizes around the 64 x 32 tile, holes that cross every kind of tile
border, a hole made of many tile-local roots whose records merge into one, walks longer than a tile, the border rule at all four
sides, at the seam of two views and at the row ends, the size threshold, shared rims, an island inside a hole, the ties of the
FILLABLE predicate inside a tile and on tile borders, every kind of invalid depth, and more than one staged piece.  Every case is
milliseconds of kernels."""
import ctypes
import functools

import numpy as np
import pytest

import depth_holes_np as F
from depth_speckle_cases import TIE_PAIRS, random_levels
from test_depth_holes_np import check_argument_refusals
from cudadepthmapintegration_amd import capi, scene

pytestmark = pytest.mark.gpu
OPEN = dict(abs_tolerance=0.0, rel_tolerance=0.5)      # every rim of the slope below is within it


def _views(depth, best_cost=None):
    eye = np.tile(np.eye(4), (depth.shape[0], 1, 1))
    return scene.Views(depth, eye, eye, best_cost)


def _gpu(depth, max_pixels, abs_tolerance=0.0, rel_tolerance=0.0, best_cost=None, threshold=None, **kwargs):
    out, size, ms = capi.fill_depth_holes(_views(depth, best_cost), max_pixels=max_pixels, abs_tolerance=abs_tolerance,
                                          rel_tolerance=rel_tolerance, threshold=threshold, **kwargs)
    assert ms > 0 and out.best_cost is None
    return out.depth, size


def _same_as_restatement(depth, max_pixels, abs_tolerance=0.0, rel_tolerance=0.0, best_cost=None, threshold=None):
    out, size = _gpu(depth, max_pixels, abs_tolerance, rel_tolerance, best_cost, threshold)
    want, want_size = F.fill_depth_holes(depth, max_pixels, abs_tolerance, rel_tolerance, best_cost, threshold)
    assert size.dtype == np.int32 and np.array_equal(size, want_size)
    assert out.tobytes() == want.tobytes()
    return out, size


def _slope(n, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.repeat((5.0 + 0.004 * xx + 0.003 * yy)[None], n, axis=0)


def _filled(out, d):
    """the pixels that had no depth and have one now"""
    return ~F.valid_pixels(d) & (out != -1.0)


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("W,H", [(1, 1), (3, 3), (70, 1), (1, 70), (63, 31), (64, 32), (65, 33), (129, 67)])
def test_sizes_around_the_tile(W, H, n):
    rng = np.random.default_rng(1000 * W + 10 * H + n)
    d = random_levels(rng, n, H, W, valid_share=0.9)
    yy, xx = np.mgrid[0:H, 0:W]
    for m in range(n):                                   # random blobs of invalid pixels
        for _ in range(int(rng.integers(2, 6))):
            cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(1, 5)
            d[m][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = -1.0
    filled = 0
    for max_pixels, abs_tol, rel_tol in ((0, 1.0, 0.0), (6, 0.0, 0.0), (40, 1.0, 0.0), (12, 0.0, 0.5)):
        out, size = _same_as_restatement(d, max_pixels, abs_tol, rel_tol)
        filled += int(_filled(out, d).sum())
        if max_pixels == 0:
            assert not _filled(out, d).any()
    if W * H > 1000:
        assert filled > 0 and (out == -1.0).any() and size.max() > 1


def test_holes_across_tile_borders_and_round_a_corner():
    d = _slope(2, 70, 130)
    d[0, 5, 62:66] = -1.0                     # across a vertical tile border
    d[0, 30:34, 10] = -1.0                    # across a horizontal one
    d[0, 31, 63] = d[0, 31, 64] = d[0, 32, 64] = -1.0       # round a tile corner: three of its four pixels
    d[1, 31:33, 63:65] = -1.0                 # all four
    d[1, 40:50, 127:129] = -1.0               # in the partial tile at the right, not on the border
    out, size = _same_as_restatement(d, 20, **OPEN)
    assert _filled(out, d).sum() == 4 + 4 + 3 + 4 + 20 and (out > 0).all()
    assert size[0, 5, 62:66].tolist() == [4] * 4 and size[0, 30:34, 10].tolist() == [4] * 4 and size[0, 31, 63] == 3
    assert (size[1, 31:33, 63:65] == 4).all() and (size[1, 40:50, 127:129] == 20).all()
    assert np.abs(out - _slope(2, 70, 130)).max() < 1e-12          # a plane is reproduced up to rounding


@functools.lru_cache(maxsize=None)
def _serpentine():
    """(hole mask [150, 200] of a one-pixel-wide path through every even row from 2 to 146 between the columns 1 and 198, its
    length): a row runs left to right and the next one right to left, a pixel on the odd row between them leads on.  It does not
    touch the border, and its 73 rows cross all 4 x 5 tiles: hundreds of tile-local roots, one record."""
    W, H = 200, 150
    hole = np.zeros((H, W), dtype=bool)
    rows = list(range(2, H - 2, 2))
    for k, y in enumerate(rows):
        hole[y, 1:W - 1] = True
        if y != rows[-1]:
            hole[y + 1, W - 2 if k % 2 == 0 else 1] = True
    hole.setflags(write=False)
    return hole, len(rows) * (W - 2) + len(rows) - 1


def test_serpentine_hole_is_one_record():
    hole, length = _serpentine()
    assert int(hole.sum()) == length == 73 * 198 + 72
    d = np.where(hole, -1.0, 2.0)[None]
    out, size = _same_as_restatement(d, length)
    assert (size[0][hole] == length).all() and (size[0][~hole] == 0).all() and (out == 2.0).all()
    out, size = _gpu(d, length - 1)
    assert (size[0][hole] == length).all() and out.tobytes() == d.tobytes()
    # the rim's extremes at the two ends of the path, 146 rows apart: both reach the one record
    d[0, 1, 5], d[0, 147, 190] = 2.5, 1.75
    out, _ = _same_as_restatement(d, length, abs_tolerance=0.75)
    assert (out > 0).all()
    out, _ = _same_as_restatement(d, length, abs_tolerance=float(np.nextafter(0.75, 0.0)))
    assert out.tobytes() == d.tobytes()
    d[0, 1, 5] = 2.0                                   # without the maximum the same tolerance is enough: 2.0 - 1.75
    assert (_same_as_restatement(d, length, abs_tolerance=0.25)[0] > 0).all()


def test_nearest_valid_pixel_more_than_a_tile_away():
    d = _slope(1, 100, 200)
    d[0, 40, 5:151] = -1.0                    # a row of 146: xl = 4 is three tiles from x = 150
    d[0, 3:81, 170] = -1.0                    # a column of 78: yu = 2 is three tiles from y = 80
    out, size = _same_as_restatement(d, 146, **OPEN)
    assert (out > 0).all() and (size[0, 40, 5:151] == 146).all() and (size[0, 3:81, 170] == 78).all()
    out, size = _same_as_restatement(d, 145, **OPEN)
    assert (out[0, 40, 5:151] == -1.0).all() and (out[0, 3:81, 170] > 0).all()


def test_holes_on_the_four_borders_the_view_seam_and_the_row_ends():
    W, H = 130, 70
    d = np.full((2, H, W), 2.0)
    d[0, 0, 20:23] = d[0, 1, 21] = -1.0       # top
    d[0, H - 1, 100] = d[0, H - 2, 100] = -1.0                # bottom
    d[0, 30:33, 0] = d[0, 31, 1] = -1.0       # left
    d[0, 50, W - 2:] = -1.0                   # right
    d[0, 20, 20] = -1.0                       # (and one that is filled)
    d[0, H - 1, 7] = d[1, 0, 7] = -1.0        # the last row of view 0 above the first of view 1: two holes, both on the border
    d[1, 10, W - 1] = d[1, 11, 0] = -1.0      # the end of a row and the start of the next: not neighbours
    out, size = _same_as_restatement(d, 100, abs_tolerance=1.0)
    want = d.copy()
    want[0, 20, 20] = 2.0
    assert out.tobytes() == want.tobytes()
    assert size[0, 0, 21] == 4 and size[0, H - 1, 100] == 2 and size[0, 31, 1] == 4 and size[0, 50, W - 1] == 2 and size[0, 20, 20] == 1
    assert size[0, H - 1, 7] == 1 and size[1, 0, 7] == 1 and size[1, 10, W - 1] == 1 and size[1, 11, 0] == 1


def test_size_exactly_max_pixels_is_filled_one_more_is_not():
    d = np.full((1, 40, 70), 2.0)
    d[0, 10, 10:17] = -1.0                    # 7
    d[0, 20, 60:68] = -1.0                    # 8, across the tile border
    out, size = _same_as_restatement(d, 7)
    assert (out[0, 10, 10:17] == 2.0).all() and (out[0, 20, 60:68] == -1.0).all()
    assert (size[0, 10, 10:17] == 7).all() and (size[0, 20, 60:68] == 8).all()
    assert (_same_as_restatement(d, 8)[0] == 2.0).all()
    assert _same_as_restatement(d, 6)[0].tobytes() == d.tobytes()
    assert (_same_as_restatement(d, 1 << 40)[0] == 2.0).all()


def test_two_holes_touching_diagonally_share_rim_pixels():
    d = np.full((1, 40, 70), 2.0)
    for y, x in ((2, 2), (31, 63)):           # inside a tile, and with the second hole in the tile diagonally below
        d[0, y, x] = d[0, y + 1, x + 1] = -1.0
        d[0, y, x + 1] = 2.5                  # on both rims
        d[0, y + 2, x + 1] = 3.5              # on the second hole's rim only
    out, size = _same_as_restatement(d, 1, abs_tolerance=0.5)
    for y, x in ((2, 2), (31, 63)):
        assert size[0, y, x] == 1 and size[0, y + 1, x + 1] == 1 and out[0, y, x] > 0 and out[0, y + 1, x + 1] == -1.0
    assert size.sum() == 4


@pytest.mark.parametrize("y,x", [(10, 10), (31, 63)])
def test_annular_hole_with_a_valid_island(y, x):
    d = np.full((1, 70, 130), 2.0)
    d[0, y - 1:y + 2, x - 1:x + 2] = -1.0
    d[0, y, x] = 2.25                          # the island: on the ring's rim
    out, size = _same_as_restatement(d, 8, abs_tolerance=0.25)
    assert (size[0, y - 1:y + 2, x - 1:x + 2].reshape(-1) == [8, 8, 8, 8, 0, 8, 8, 8, 8]).all()
    assert out[0, y, x] == 2.25 and (out > 0).all()
    # the island is xr of the pixel left of it: h = (2 * 1 + 2.25 * 1) / 2, v = 2 over a span of 4 -> (2.125 * 4 + 2 * 2) / 6
    assert out[0, y, x - 1] == (2.125 * 4.0 + 2.0 * 2.0) / 6.0 and out[0, y - 1, x - 1] == 2.0
    out, _ = _same_as_restatement(d, 8, abs_tolerance=float(np.nextafter(0.25, 0.0)))
    assert out.tobytes() == d.tobytes()


@pytest.mark.parametrize("pair", range(len(TIE_PAIRS)))
def test_fillable_ties_inside_a_tile_and_on_tile_borders(pair):
    """a on three sides of a one-pixel hole and b on the fourth, once per side and per place: a view each."""
    a, b, abs_tol, rel_tol, linked = TIE_PAIRS[pair]
    places = [(10, 10), (31, 63), (32, 64), (31, 64), (32, 63)]
    sides = [(-1, 0), (0, 1), (1, 0), (0, -1)]
    d = np.full((len(places) * len(sides), 70, 130), a)
    for i, (y, x) in enumerate(places):
        for j, (dy, dx) in enumerate(sides):
            d[i * len(sides) + j, y, x] = -1.0
            d[i * len(sides) + j, y + dy, x + dx] = b
    out, size = _same_as_restatement(d, 1, abs_tol, rel_tol)
    assert size.sum() == len(d) and int(_filled(out, d).sum()) == (len(d) if linked else 0)


def test_every_kind_of_invalid_depth_is_a_hole():
    d = np.full((2, 40, 70), 2.0)
    cost = np.zeros(d.shape)
    kinds = [0.0, -3.0, np.nan, np.inf, -np.inf, -1.0, -0.0]
    for k, v in enumerate(kinds):
        d[0, 3, 2 + 2 * k] = v
        d[1, 31, 60 + k] = v                  # side by side across the tile border: one hole of 7
    cost[0, 20, 20] = 0.75                     # best_cost > threshold
    cost[0, 20, 22] = 0.5                      # equal: stays
    cost[0, 20, 24] = np.nan                   # NaN: stays
    out, size = _same_as_restatement(d, 7, best_cost=cost, threshold=0.5)
    assert (out == 2.0).all() and size[0].sum() == len(kinds) + 1 and size[0, 20, 20] == 1 and (size[1][size[1] > 0] == 7).all()
    assert size[1].sum() == 49
    plain, plain_size = _gpu(np.where(cost > 0.5, -1.0, d), 7)
    assert plain.tobytes() == out.tobytes() and np.array_equal(plain_size, size)


def test_a_wholly_invalid_view_and_a_wholly_valid_one():
    d = np.full((3, 67, 129), -1.0)
    d[1] = _slope(1, 67, 129)[0]
    d[2] = np.nan
    out, size = _same_as_restatement(d, 1 << 20, **OPEN)
    assert (out[0] == -1.0).all() and (out[2] == -1.0).all() and out[1].tobytes() == d[1].tobytes()
    assert (size[0] == 67 * 129).all() and (size[2] == 67 * 129).all() and (size[1] == 0).all()


@functools.lru_cache(maxsize=None)
def _blobs():
    rng = np.random.default_rng(21)
    d = _slope(6, 97, 131)
    yy, xx = np.mgrid[0:97, 0:131]
    for m in range(6):
        for _ in range(30):
            cy, cx, r = rng.integers(0, 97), rng.integers(0, 131), rng.integers(1, 6)
            d[m][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = -1.0
        d[m][rng.random((97, 131)) < 0.05] = -1.0
    want = F.fill_depth_holes(d, 30, 0.0, 0.01)
    for a in (d,) + want:
        a.setflags(write=False)
    return d, want


def test_random_blobs_on_a_slope():
    d, (want, want_size) = _blobs()
    out, size = _gpu(d, 30, rel_tolerance=0.01)
    assert np.array_equal(size, want_size) and out.tobytes() == want.tobytes()
    assert 0 < _filled(out, d).sum() < (~F.valid_pixels(d)).sum() and len(np.unique(size)) > 10


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
    rc = L.dmi_fill_depth_holes(dp(src), None, 0.0, n, W, H, 0.0, 0.01, 30, 0, dp(out), None, None)
    assert rc == 0, L.dmi_last_error(None).decode()
    assert out.tobytes() == want.tobytes()


def test_every_refusal_leaves_the_outputs_untouched():
    check_argument_refusals()
    d = np.full((1, 6, 8), 2.0)
    out = np.full(d.shape, 7.0)
    with pytest.raises(capi.DmiError) as e:
        capi.fill_depth_holes(_views(d), max_pixels=1, device=1 << 20, out=out)
    assert e.value.code == 1 and "device" in str(e.value) and (out == 7.0).all()


def test_more_than_one_staged_piece():
    """5 views of 3000 x 3000 (360 MB: pieces of three views and of two): view k holds the depth k + 1, with a cross of -1 at row
    1000 and column 1700, which touches the border and stays, and four holes of 2 x 2 that are filled with k + 1 again.  Every
    value has a closed form; no restatement runs at this size."""
    n, W, H, cy, cx = 5, 3000, 3000, 1000, 1700
    d = np.empty((n, H, W))
    for k in range(n):
        d[k] = k + 1.0
    d[:, cy, :] = -1.0
    d[:, :, cx] = -1.0
    spots = [(10, 10), (31, 63), (2000, 2900), (2990, 5)]
    for y, x in spots:
        d[:, y:y + 2, x:x + 2] = -1.0
    out, size = _gpu(d, 4, out=d)                     # in place: the host holds the planes once
    assert out is d
    assert (size[:, cy, :] == W + H - 1).all() and (size[:, :, cx] == W + H - 1).all()
    assert (d[:, cy, :] == -1.0).all() and (d[:, :, cx] == -1.0).all()
    for y, x in spots:
        assert (size[:, y:y + 2, x:x + 2] == 4).all()
    assert int(size.astype(np.int64).sum()) == n * ((W + H - 1) ** 2 + 16 * len(spots))
    for k in range(n):
        cross = np.zeros((H, W), dtype=bool)
        cross[cy, :] = cross[:, cx] = True
        assert (d[k][~cross] == k + 1.0).all(), k
