"""The numpy restatement of the voxel-grid thinning (depth_points_thin_np.py; include/dmi.h states the definition)
checked against the definition's own consequences on hand-made clouds: a cell of one keeps its bits, the order of cells and of
members, sums made left to right, normals that cancel, the maximum count, the first member's view and pixel, min_points, the report
and the refusal limits.  No GPU."""
import numpy as np
import pytest

import depth_points_thin_np as T


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def test_a_cell_of_one_keeps_its_bits():
    xyz = np.array([[0.1, -0.0, 3.0], [5.3, 7.7, -0.0], [-2.5, 1e-300, 9.0]])
    normal = np.array([[0.6, 0.8, -0.0], [0.0, 0.0, 0.0], [0.3, 0.4, 0.5]], np.float32)   # the last one is not a unit vector: copied as it is
    view, pixel, count = np.array([2, 0, 1], np.int32), np.array([7, 8, 9], np.int32), np.array([3, 0, 5], np.int32)
    arrays, report = T.thin(xyz, normal, view, pixel, count, cell_size=1.0)
    order = [1, 0, 2]                       # ascending b_2 = floor(z - (-0.0)): 0, 3, 9
    assert _bits(arrays["xyz"]) == _bits(xyz[order]) and _bits(arrays["normal"]) == _bits(normal[order])
    assert arrays["view"].tolist() == view[order].tolist() and arrays["pixel"].tolist() == pixel[order].tolist()
    assert arrays["count"].tolist() == count[order].tolist() and arrays["members"].tolist() == [1, 1, 1]
    assert np.signbit(arrays["xyz"]).sum() == 3       # both -0.0 and the -2.5 stay negative
    assert report == dict(points_in=3, cells=3, cells_kept=3, multi_view_cells=0, largest_cell=1, with_normal=2)


def test_cells_are_ordered_by_b2_then_b1_then_b0():
    # one point per cell of a 2 x 2 x 2 block, given in reverse
    xyz = np.array([[x, y, z] for z in (1.5, 0.5) for y in (1.5, 0.5) for x in (1.5, 0.5)], dtype=np.float64)
    arrays, _ = T.thin(xyz, pixel=np.arange(8, dtype=np.int32), cell_size=1.0)
    assert arrays["pixel"].tolist() == [7, 6, 5, 4, 3, 2, 1, 0]
    assert arrays["xyz"].tolist() == [[x, y, z] for z in (0.5, 1.5) for y in (0.5, 1.5) for x in (0.5, 1.5)]


def test_members_are_added_left_to_right_in_input_order():
    # 1e16 + 1 + 1 differs from 1 + 1 + 1e16 in f64: the order of the sum shows
    big = 1e16
    a, _ = T.thin(np.array([[big, 0, 0], [1, 0, 0], [1, 0, 0]], dtype=np.float64), cell_size=4e16)
    b, _ = T.thin(np.array([[1, 0, 0], [1, 0, 0], [big, 0, 0]], dtype=np.float64), cell_size=4e16)
    assert a["xyz"][0, 0] == ((big + 1.0) + 1.0) / 3.0 and b["xyz"][0, 0] == ((1.0 + 1.0) + big) / 3.0
    assert a["xyz"][0, 0] != b["xyz"][0, 0] and a["members"].tolist() == [3]


def test_the_first_member_starts_the_sum():
    arrays, _ = T.thin(np.array([[-0.0, 0.0, 0.0], [-0.0, 0.0, 0.0]]), cell_size=1.0)
    assert np.signbit(arrays["xyz"][0, 0])            # (-0.0 + -0.0) / 2; a sum begun at +0.0 would have lost the sign


def test_border_coordinates_fall_into_the_upper_cell():
    xyz = np.array([[0.0, 0, 0], [0.25, 0, 0], [0.5, 0, 0], [0.75, 0, 0], [1.0, 0, 0]])
    arrays, report = T.thin(xyz, cell_size=0.5)
    assert arrays["members"].tolist() == [2, 2, 1] and arrays["xyz"][:, 0].tolist() == [0.125, 0.625, 1.0]
    assert report["cells"] == 3 and report["largest_cell"] == 2


def test_normals_merge_cancel_and_skip_the_absent():
    xyz = np.zeros((6, 3))
    xyz[2:4, 0] = 1.5
    xyz[4:, 0] = 2.5
    normal = np.array([[0, 0, 1], [0, 1, 0],            # merge: (0, 1, 1) / sqrt 2
                       [0, 0, 1], [0, 0, -1],           # cancel exactly: the zero vector
                       [1, 0, 0], [0, 0, 0]], np.float32)  # one member has none: it adds zeros
    arrays, report = T.thin(xyz, normal, cell_size=1.0)
    r = np.float32(1.0 / np.sqrt(2.0))
    assert arrays["normal"].tolist() == [[0.0, r, r], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]
    assert report["with_normal"] == 2


def test_view_pixel_count_and_the_multi_view_cells():
    xyz = np.zeros((5, 3))
    xyz[3:, 1] = 2.0
    view = np.array([1, 1, 4, 2, 2], np.int32)
    pixel = np.array([10, 11, 12, 13, 14], np.int32)
    count = np.array([1, 7, 3, 2, 2], np.int32)
    arrays, report = T.thin(xyz, None, view, pixel, count, cell_size=1.0)
    assert arrays["view"].tolist() == [1, 2] and arrays["pixel"].tolist() == [10, 13] and arrays["count"].tolist() == [7, 2]
    assert arrays["members"].tolist() == [3, 2] and report["multi_view_cells"] == 1 and report["largest_cell"] == 3


def test_min_points_drops_small_cells_and_keeps_the_order():
    xyz = np.array([[0.5, 0, 0], [1.5, 0, 0], [1.6, 0, 0], [2.5, 0, 0], [3.5, 0, 0], [3.6, 0, 0], [3.7, 0, 0]])
    arrays, report = T.thin(xyz, cell_size=1.0, min_points=2)
    assert arrays["members"].tolist() == [2, 3]
    assert report == dict(points_in=7, cells=4, cells_kept=2, multi_view_cells=0, largest_cell=3, with_normal=0)
    none, report = T.thin(xyz, cell_size=1.0, min_points=4)
    assert len(none["xyz"]) == 0 and report["cells_kept"] == 0 and report["largest_cell"] == 3


def test_identical_points_and_a_cell_above_the_bounding_box_are_one_cell():
    same = np.tile(np.array([[3.25, -1.5, 2.0]]), (257, 1))
    arrays, report = T.thin(same, cell_size=1e-3)
    assert arrays["xyz"].tolist() == [[3.25, -1.5, 2.0]] and arrays["members"].tolist() == [257] and report["cells"] == 1
    rng = np.random.default_rng(5)
    cloud = rng.uniform(-1, 1, (100, 3))
    arrays, _ = T.thin(cloud, cell_size=10.0)
    want = cloud[0].copy()
    for row in cloud[1:]:
        want = want + row
    assert _bits(arrays["xyz"]) == _bits(want / 100.0)


def test_an_empty_cloud_is_an_empty_result():
    arrays, report = T.thin(np.zeros((0, 3)), cell_size=1.0)
    assert all(len(arrays[name]) == 0 for name in T.ARRAY_NAMES) and report["points_in"] == 0 and report["cells"] == 0
    assert arrays["members"].dtype == np.uint32 and arrays["normal"].dtype == np.float32


@pytest.mark.parametrize("cell_size", [float("nan"), 0.0, -1.0, float("inf")])
def test_cell_sizes_outside_the_definition_are_refused(cell_size):
    with pytest.raises(ValueError, match="cell_size"):
        T.thin(np.zeros((2, 3)), cell_size=cell_size)


def test_min_points_below_one_and_non_finite_coordinates_are_refused():
    with pytest.raises(ValueError, match="min_points"):
        T.thin(np.zeros((2, 3)), cell_size=1.0, min_points=0)
    for value in (np.nan, np.inf, -np.inf):
        xyz = np.zeros((3, 3))
        xyz[1, 2] = value
        with pytest.raises(ValueError, match="non-finite"):
            T.thin(xyz, cell_size=1.0)


def test_the_bin_limit_is_2_to_the_21_and_the_message_names_the_least_cell_size():
    xyz = np.array([[0.0, 0, 0], [1.0, 0, 0]])
    h = 1.0 / (1 << 21)
    with pytest.raises(ValueError, match="2\\^21 bins.*smallest acceptable cell size"):
        T.thin(xyz, cell_size=h)                        # floor(1 / h) = 2^21: one bin too many
    least = T.min_cell_size(xyz)
    assert least == np.nextafter(h, np.inf)
    arrays, report = T.thin(xyz, cell_size=least)       # exactly 2^21 bins: accepted
    assert report["cells"] == 2 and len(arrays["xyz"]) == 2
    with pytest.raises(ValueError) as e:
        T.thin(xyz, cell_size=h)
    assert repr(least) in str(e.value)
