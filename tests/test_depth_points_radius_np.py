"""The brute-force restatement of the radius neighbour count (depth_points_radius_np.py) against cases worked out by hand: the
tie at exactly the radius and one ulp below it, coincident points, a single point, symmetry."""
import numpy as np
import pytest

import depth_points_radius_np as R


@pytest.mark.parametrize("s", [1.0, 2.0 ** -20, 2.0 ** 30])
def test_a_pair_at_exactly_the_radius_counts_and_one_ulp_less_does_not(s):
    pair = np.array([[0.0, 0.0, 0.0], [3 * s, 4 * s, 0.0]])     # 9 s^2 + 16 s^2 = 25 s^2, all exact for a power of two s
    assert R.count_neighbors(pair, 5 * s).tolist() == [1, 1]
    assert R.count_neighbors(pair, np.nextafter(5 * s, 0.0)).tolist() == [0, 0]
    assert R.count_neighbors(pair, np.nextafter(5 * s, np.inf)).tolist() == [1, 1]


def test_coincident_points_are_neighbours_of_each_other_but_not_of_themselves():
    same = np.tile(np.array([[3.25, -1.5, 2.0]]), (5, 1))
    assert R.count_neighbors(same, 1e-9).tolist() == [4] * 5
    assert R.count_neighbors(np.array([[1.0, 2.0, 3.0]]), 10.0).tolist() == [0]
    assert R.count_neighbors(np.zeros((0, 3)), 1.0).tolist() == []
    assert R.count_neighbors(np.array([[-0.0, 0.0, 0.0], [0.0, -0.0, 0.0]]), 1e-100).tolist() == [1, 1]


def test_the_relation_is_symmetric_and_the_filter_keeps_the_order():
    rng = np.random.default_rng(5)
    xyz = rng.integers(0, 12, (700, 3)).astype(np.float64) * 0.25      # quantised: exact ties abound
    for radius in (0.25, 0.5, np.sqrt(0.1875)):
        neighbors = R.count_neighbors(xyz, radius)
        assert int(neighbors.sum()) % 2 == 0
        # one query against all, written another way
        i = 123
        d = xyz - xyz[i]
        assert neighbors[i] == int((((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) <= radius * radius).sum()) - 1
    arrays = dict(xyz=xyz, view=np.arange(700, dtype=np.int32))
    kept, report = R.filter_radius(arrays, 0.25, 3)
    assert np.all(np.diff(kept["view"]) > 0) and np.array_equal(kept["xyz"], xyz[kept["view"]])
    assert report["points_kept"] == len(kept["view"]) and np.all(kept["neighbors"] >= 3) and report["neighbor_sum"] % 2 == 0
    everything, report = R.filter_radius(arrays, 0.25, 0)
    assert len(everything["view"]) == 700 and report["points_kept"] == 700 and report["isolated"] == int((everything["neighbors"] == 0).sum())


def test_refusals():
    xyz = np.zeros((3, 3))
    for radius in (0.0, -1.0, np.nan, np.inf, 1e-200, 1e200):
        with pytest.raises(ValueError, match="radius"):
            R.count_neighbors(xyz, radius)
    bad = xyz.copy()
    bad[1, 2] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        R.count_neighbors(bad, 1.0)
    with pytest.raises(ValueError, match="min_neighbors"):
        R.filter_radius(dict(xyz=xyz), 1.0, -1)
