"""The point-cloud stages on the GPU above 2^20 points, where the sort is another algorithm and every capped
pass strides: dmi_thin_point_cloud, dmi_count_point_neighbors and the chain dmi_views_build_points ->
dmi_views_filter_points_radius -> dmi_views_thin_points, byte for byte against the numpy restatements (depth_points_np.py,
depth_points_thin_np.py, depth_points_radius_binned_np.py).  The clouds and their references are depth_points_scale_cases.py's,
computed once.  The tests without the gpu mark pin the references' own numbers: no case is vacuous.

The sort.  thin_sort_pairs sorts (u64 key, u32 index) with rocprim::radix_sort_pairs on a double buffer.  Up to 2^20 items
(merge_sort_limit) rocPRIM sorts by merging and the result is always in the second key array; above, it sorts by Onesweep, a pass
per digit place, and the passes alternate between the arrays: first -> second -> first ...  For gfx950 and these types the tuned
configuration (rocprim/device/detail/config/device_radix_sort_onesweep.hpp) has radix_bits_per_place = 8, so a key of B bits takes
ceil(B / 8) places and the sorted keys end in the second array, keys[1], after an odd number of places and in the first, keys[0],
after an even number.  The head flags, ranks, kept flags and output numbers live in whichever array is free.  The key widths
below hold an odd and an even number of places for every digit width from 4 to 8 bits, should a later rocPRIM tune another.

P0 = 2^20 + 4321 = 1 052 897 points.  At P0 these passes take more than one trip: thin_bounds_kernel (1024 blocks: above 262 144
points), thin_kept_kernel and radius_flags_kernel (4096 blocks: above 1 048 575 entries), and rocPRIM's scans are their
multi-block look-back form.  CPU times are of the reference alone, on one core of the machine the numbers were pinned on.

The thinning, dmi_thin_point_cloud (P = P0 in every case):
  key_bits  bins             places  sorted keys in  reference  what else
  8         8 x 8 x 4        1       keys[1]         0.45 s     cells of about 4100 members, the largest 4308: the wave pass takes
                                                                68 chunks a cell
  12        16^3             2       keys[0]         0.43 s
  15        28^3             2       keys[0]         0.46 s     20 020 cells above the default threshold of 32 members: the wave
                                                                kernel (4096 blocks, 16 384 waves) strides
  16        40^3             2       keys[0]         0.51 s     about 16 members a cell: the lane pass
  21        128^3            3       keys[1]         0.59 s     min_points = 3 drops 51 549 cells of 243 169
  24        256^3            3       keys[1]         0.59 s     normal and pixel absent
  30        2^20 x 2^10 x 1  4       keys[0]         0.53 s
  40        2^20 x 2^20 x 1  5       keys[1]         0.59 s
  63        (2^21 - 1)^3     8       keys[0]         0.53 s
The threshold's knob belongs to the view set, whose cloud is always a build's: the 40^3 cloud cannot run at a threshold of 8.  The
chain below runs at 8 instead, where 47 204 and 25 183 cells of the room's cloud queue for the wave pass.

The neighbour count, dmi_count_point_neighbors (radius 0.3; P = P0: a base cloud of P0 - 2 points and two strays that widen the
search grid; the base's counts took 2.1 s, a mean of 2.4 neighbours, at most 13).  The base has 57 600 work units at the default
knob, above the count kernel's 8192 blocks of four waves: radius_count_kernel strides in every case.
  key_bits  bins of the search grid     places  sorted keys in  min_neighbors
  21        33 x 243 x 240              3       keys[1]         1
  24        250 x 243 x 240             3       keys[1]         0
  28        1299 x 650 x 240            4       keys[0]         4
  30        2598 x 1299 x 240           4       keys[0]         1
  40        79 922 x 39 961 x 240       5       keys[1]         4
  63        1 998 049^3                 8       keys[0]         0
and a cloud of 270 001 points (20 bits, 0.5 s): below the merge-sort limit, so the sort ends in keys[1] whatever the key, and with
61 648 units the count kernel strides all the same: the two are crossed one at a time.

The chain on a resident view set: 4 room views of 640 x 480, every pixel valid, 1 228 800 points (4800 compaction blocks: the first
run of points_scan_kernel's second and third chunk; the numpy build took 0.9 s), the threshold knob at 8.
  "counted"  radius 0.003, min_neighbors 0 (28 bits, 4 places, keys[0]; 2.6 s): at most 63 neighbours, all 1 228 800 points stay;
             thinned at 0.01 with min_points 2 (23 bits, 3 places, keys[1]; 1.0 s); run whole and with a piece of one plane
  "dropped"  radius 0.0034, min_neighbors 1 (27 bits, 4 places, keys[0]; 2.6 s): 1 069 635 points stay; thinned at 0.005 with
             min_points 1 (26 bits, 4 places, keys[0]; 1.0 s)
No radius of this scene has both a maximum below 64 and more than 2^20 points with a neighbour, hence the two.

Not covered here: points_sum_normals_kernel's stride (above 16.7 M pixels), the 32 768-view launch split, anything near 2^32
points."""
import numpy as np
import pytest

import depth_points_radius_np as R
import depth_points_scale_cases as C
import depth_points_thin_np as T
from cudadepthmapintegration_amd import capi

gpu = pytest.mark.gpu
ONESWEEP_DIGIT_BITS = 8      # rocPRIM's radix_bits_per_place for gfx950, u64 keys with u32 values
BUILD_COUNT_NAMES = ("valid", "candidates", "owned", "points", "with_normal")
STRADDLE = ((1 << 20) - 1000, 2000)   # a range of points on both sides of 2^20

# bits -> the reference's (bins, cells, cells_kept, multi_view_cells, largest_cell, with_normal)
THIN_EXPECTED = {
    8: ((8, 8, 4), 256, 256, 256, 4308, 256),
    12: ((16, 16, 16), 4096, 4096, 4096, 325, 4096),
    15: ((28, 28, 28), 21952, 21952, 21952, 124, 21952),
    16: ((40, 40, 40), 64000, 64000, 63999, 40, 64000),
    21: ((128, 128, 128), 243169, 191620, 191265, 23, 191142),
    24: ((256, 256, 256), 307276, 307276, 243960, 19, 0),
    30: ((1 << 20, 1 << 10, 1), 278853, 278853, 239821, 15, 269367),
    40: ((1 << 20, 1 << 20, 1), 258475, 258475, 235803, 16, 252487),
    63: (((1 << 21) - 1,) * 3, 289598, 289598, 241888, 16, 278289),
}
RADIUS_BINS = {21: [33, 243, 240], 24: [250, 243, 240], 28: [1299, 650, 240], 30: [2598, 1299, 240], 40: [79922, 39961, 240],
               63: [1998049] * 3}


def _places(bits, digit=ONESWEEP_DIGIT_BITS):
    return -(-bits // digit)


def _assert_thin_equal(got, report, want, want_report, label=None):
    for name in T.ARRAY_NAMES:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (label, name, got[name].shape, want[name].shape)
        assert got[name].tobytes() == want[name].tobytes(), (label, name)
    assert {k: int(report[k]) for k in T.REPORT_NAMES} == {k: want_report[k] for k in T.REPORT_NAMES}, label


def _assert_radius_report(report, want_report, label=None):
    assert {k: int(report[k]) for k in R.REPORT_NAMES} == {k: want_report[k] for k in R.REPORT_NAMES}, label
    assert int(report["distance_tests"]) >= want_report["neighbor_sum"] and want_report["neighbor_sum"] % 2 == 0, label


def _assert_arrays_equal(got, want, names, label=None):
    for name in names:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (label, name, got[name].shape, want[name].shape)
        assert got[name].tobytes() == want[name].tobytes(), (label, name)


# ---- the references' own numbers (CPU) ----
def test_the_key_widths_end_the_sort_in_either_array_at_every_digit_width():
    for cases in (C.THIN_CASES, C.RADIUS_CASES):
        for digit in range(4, 9):
            assert {_places(bits, digit) % 2 for bits in cases} == {0, 1}, digit
    assert C.P0 > 1 << 20 and C.SMALL_POINTS < 1 << 20


@pytest.mark.parametrize("bits", list(C.THIN_CASES))
def test_the_thinning_cases_are_not_vacuous(bits):
    key_bits, bins = C.thin_key_bits(bits)
    arrays, report = C.thinned(bits)
    assert key_bits == bits and len(C.thin_cloud(bits)["xyz"]) == C.P0
    assert (bins, report["cells"], report["cells_kept"], report["multi_view_cells"], report["largest_cell"],
            report["with_normal"]) == THIN_EXPECTED[bits]
    members = arrays["members"]
    if bits == 8:
        assert report["largest_cell"] > 4096                        # more than 64 chunks of 64 for one wave
    if bits == 15:
        assert int((members > 32).sum()) == 20020                   # > 16 384: the wave kernel strides at the default threshold
    if bits == 16:
        assert int((members > 8).sum()) == 62418 and int((members > 32).sum()) == 52
    if bits >= 21:
        assert int((members >= 3).sum()) > 100000                   # the order of a cell's members shows in its sums


def test_the_neighbour_count_cases_are_not_vacuous():
    base, neighbors = C.radius_base(), C.radius_base_counts()
    assert len(base) == C.P0 - 2
    assert (int(neighbors.sum()), int(neighbors.max()), int((neighbors == 0).sum()), int((neighbors >= 4).sum())) == (2510756, 13, 98537, 230376)
    assert C.search_units(base) == 57600 > 8192 * 4                 # the count kernel strides
    for bits in C.RADIUS_CASES:
        n, key_bits, _ = C.search_grid(C.radius_cloud(bits))
        assert key_bits == bits and n == RADIUS_BINS[bits], bits
    assert {m for _, m in C.RADIUS_CASES.values()} == {0, 1, 4}
    small, neighbors = C.radius_small(), C.radius_small_counts()
    assert len(small) == C.SMALL_POINTS and C.search_grid(small)[:2] == ([10, 250, 250], 20)
    assert (int(neighbors.sum()), int(neighbors.max()), int((neighbors == 0).sum())) == (444898, 11, 52898)
    assert C.search_units(small) == 61648 > 8192 * 4 and C.search_units(small, group=1) == C.SMALL_POINTS


def test_the_build_of_the_chain_is_not_vacuous():
    cloud, report = C.chain_built()
    assert report["points"] == len(cloud["xyz"]) == 1228800 == report["valid"] == report["with_normal"] and report["one_sided"] == 8944
    assert (report["points"] + 255) // 256 == 4800                  # compaction blocks: three chunks of the scan's 2048


@pytest.mark.parametrize("name", list(C.CHAIN_CASES))
def test_the_chain_cases_are_not_vacuous(name):
    radius, min_neighbors = C.CHAIN_CASES[name]
    neighbors = C.chain_counts(name)
    filtered, report = C.chain_filtered(name)
    thinned, thin_report = C.chain_thinned(name)
    members = thinned["members"]
    _, grid_bits, _ = C.search_grid(C.chain_built()[0]["xyz"], radius)
    _, n = T.bins(filtered["xyz"], C.CHAIN_CELLS[name][0])
    thin_bits = (n[0] * n[1] * n[2] - 1).bit_length()
    assert report["points_kept"] > 1 << 20                          # the thinning behind it sorts by Onesweep too
    assert int((members > C.CHAIN_WAVE_CELL_POINTS).sum()) > 16384  # the wave kernel strides
    if name == "counted":
        assert report["max_neighbors"] == 63 < 64 and report["points_kept"] == 1228800 and report["isolated"] == 276848
        assert report["neighbor_sum"] == 8653274 and int((neighbors >= 1).sum()) == 951952 and (grid_bits, thin_bits) == (28, 23)
        assert (thin_report["cells"], thin_report["cells_kept"], thin_report["largest_cell"]) == (105777, 98308, 218)
        assert int((members > 8).sum()) == 47204
    else:
        assert report["max_neighbors"] == 81 and report["points_kept"] == 1069635 and report["neighbor_sum"] == 11512088
        assert (grid_bits, thin_bits) == (27, 26)
        assert thin_report["cells_kept"] == thin_report["cells"] == 265695 and thin_report["largest_cell"] == 56
        assert int((members > 8).sum()) == 25183


# ---- the device against them ----
@gpu
@pytest.mark.parametrize("bits", list(C.THIN_CASES))
def test_the_thinning_equals_the_restatement_at_every_key_width(bits):
    _, cell_size, min_points, _ = C.THIN_CASES[bits]
    cloud = C.thin_cloud(bits)
    want, want_report = C.thinned(bits)
    got, report = capi.thin_point_cloud(*(cloud[name] for name in C.INPUT_NAMES), cell_size=cell_size, min_points=min_points)
    _assert_thin_equal(got, report, want, want_report, bits)
    assert report["points_in"] == C.P0 and report["kernel_ms"] > 0


@gpu
@pytest.mark.parametrize("bits", list(C.RADIUS_CASES))
def test_the_neighbour_counts_equal_the_restatement_at_every_key_width(bits):
    (x, y, z), min_neighbors = C.RADIUS_CASES[bits]
    base, xyz = C.radius_base(), C.radius_cloud(bits)
    # each stray is farther than the radius from every point: beyond the base on an axis, and from the other stray
    assert x * C.RADIUS - base[:, 0].max() > C.RADIUS and y * C.RADIUS - base[:, 1].max() > C.RADIUS
    for stray in (xyz[-2], xyz[-1]):
        d = xyz - stray
        assert int((((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) <= C.RADIUS * C.RADIUS).sum()) == 1   # itself
    want = np.concatenate([C.radius_base_counts(), np.zeros(2, np.uint32)])
    neighbors, keep, report = capi.count_point_neighbors(xyz, radius=C.RADIUS, min_neighbors=min_neighbors)
    assert neighbors.dtype == np.uint32 and neighbors.tobytes() == want.tobytes(), (bits, np.flatnonzero(neighbors != want)[:8])
    assert np.array_equal(keep, want >= min_neighbors), bits
    _assert_radius_report(report, R.report_of(want, min_neighbors), bits)


@gpu
def test_the_neighbour_counts_of_a_cloud_below_the_merge_sort_limit_whose_units_stride():
    want = C.radius_small_counts()
    neighbors, keep, report = capi.count_point_neighbors(C.radius_small(), radius=C.RADIUS, min_neighbors=2)
    assert neighbors.tobytes() == want.tobytes(), np.flatnonzero(neighbors != want)[:8]
    assert np.array_equal(keep, want >= 2)
    _assert_radius_report(report, R.report_of(want, 2))


@gpu
@pytest.mark.parametrize("name,pieces", [("counted", False), ("counted", True), ("dropped", False)])
def test_the_chain_on_a_resident_view_set_equals_the_restatements(name, pieces):
    radius, min_neighbors = C.CHAIN_CASES[name]
    cell_size, min_points = C.CHAIN_CELLS[name]
    views = C.room_views()
    built, built_report = C.chain_built()
    filtered, filtered_report = C.chain_filtered(name)
    thinned, thinned_report = C.chain_thinned(name)
    first, count = STRADDLE
    with capi.ViewSet(C.ROOM["W"], C.ROOM["H"]) as s:
        if pieces:
            s.set_piece_bytes(C.ROOM["W"] * C.ROOM["H"] * 8)
        s.add(views)
        s.set_thin_wave_cell_points(C.CHAIN_WAVE_CELL_POINTS)
        report = s.build_points(**C.BUILD)
        _assert_arrays_equal(s.download_points(), built, C.INPUT_NAMES, (name, "build"))
        assert {k: int(report[k]) for k in BUILD_COUNT_NAMES} == {k: built_report[k] for k in BUILD_COUNT_NAMES}
        part = s.download_points(first, count)
        _assert_arrays_equal(part, {k: built[k][first:first + count] for k in C.INPUT_NAMES}, C.INPUT_NAMES, (name, "build, a range"))
        held, steps = s.info().device_bytes, s.info().steps

        report = s.filter_points_radius(radius, min_neighbors)
        got = s.download_points()
        got["neighbors"] = s.download_point_neighbors()
        _assert_arrays_equal(got, filtered, C.INPUT_NAMES + ("neighbors",), (name, "filter"))
        _assert_radius_report(report, filtered_report, (name, "filter"))
        assert np.all(s.download_point_members(first, count) == 1)
        part = s.download_points(first, count)
        part["neighbors"] = s.download_point_neighbors(first, count)
        _assert_arrays_equal(part, {k: filtered[k][first:first + count] for k in part}, tuple(part), (name, "filter, a range"))
        info = s.info()
        assert info.steps == steps + 1
        assert info.device_bytes == held - 48 * report["points_in"] + 52 * report["points_kept"]   # the scratch is gone, the cloud is held
        held, steps = info.device_bytes, info.steps

        report = s.thin_points(cell_size, min_points)
        got = s.download_points()
        got["members"] = s.download_point_members()
        _assert_thin_equal(got, report, thinned, thinned_report, (name, "thin"))
        info = s.info()
        assert info.steps == steps + 1
        assert info.device_bytes == held - 52 * report["points_in"] + 52 * report["cells_kept"]    # the counts went with the old cloud
        with pytest.raises(capi.DmiError) as e:
            s.download_point_neighbors()
        assert e.value.code == 4
