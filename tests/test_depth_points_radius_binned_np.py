"""The binned restatement of the radius neighbour count (depth_points_radius_binned_np.py), which the tests at scale use
(test_depth_points_scale.py), against the brute force over all pairs (depth_points_radius_np.py), bit for bit: on the clouds of
test_depth_points_radius.py -- the random ones of both families with their offsets, and the engineered ones where a tie or a cell
border decides -- and on its own refusal.  The candidates of scipy's k-d tree give a third count where scipy is there."""
import numpy as np
import pytest

import depth_points_radius_binned_np as B
import depth_points_radius_np as R


def random_cloud(seed):
    """test_random_clouds' cloud of test_depth_points_radius.py for this seed: (xyz, radius)."""
    rng = np.random.default_rng(2000 + seed)
    n_points = int(rng.integers(100, 2001)) if seed else 2000
    radius = float(rng.choice([0.25, 0.3, 0.5, 1.7])) if seed % 2 else float(rng.uniform(0.05, 2.0))
    extent = (3, 6, 12, 40)[seed % 4]
    offset = 5e6 if seed in (11, 17) else 0.0
    if seed % 3 == 0:                                               # coordinates on the faces of the radius' own cells
        xyz = offset + rng.integers(0, extent, (n_points, 3)).astype(np.float64) * (radius * (1 + 2.0 ** -10))
        xyz[rng.random(n_points) < 0.5] += radius / 4
    else:
        xyz = offset + rng.integers(0, 4 * extent, (n_points, 3)).astype(np.float64) * (radius / 4)   # quantised: exact ties abound
    return xyz, radius


def _same(xyz, radius, label=None):
    want = R.count_neighbors(xyz, radius)
    got = B.count_neighbors(xyz, radius)
    assert got.dtype == np.uint32 and got.tobytes() == want.tobytes(), (label, np.flatnonzero(got != want)[:8])
    return got


@pytest.mark.parametrize("seed", range(20))
def test_random_clouds_equal_the_brute_force(seed):
    xyz, radius = random_cloud(seed)
    neighbors = _same(xyz, radius, seed)
    assert int(neighbors.sum()) > 0
    # the faces of this restatement's own cells too: 1.25 radius, from the cloud's minimum
    rng = np.random.default_rng(4000 + seed)
    own = rng.integers(0, 9, (600, 3)).astype(np.float64) * (B.CELL_FACTOR * radius)
    own[rng.random(600) < 0.5] -= radius
    _same(own + (5e6 if seed in (11, 17) else 0.0), radius, ("own faces", seed))


def test_engineered_clouds_equal_the_brute_force():
    rng = np.random.default_rng(3)
    h = 0.5 * (1 + 2.0 ** -10)                                       # the device's cell size of radius 0.5: points exactly on its faces
    faces = np.array([[i, j, k] for i in range(5) for j in range(4) for k in range(3)], dtype=np.float64) * h
    _same(np.concatenate([faces, faces[:20] + h / 2]), 0.5, "faces")
    line = np.zeros((300, 3))
    line[:, 0] = rng.integers(0, 400, 300) * 0.125                   # collinear: ties at the radius abound
    _same(line, 0.5, "collinear")
    line[:, [0, 2]] = line[:, [2, 0]]
    _same(line, 0.5, "collinear in z")
    zero = np.array([[-0.0, 0.0, -0.0], [0.0, -0.0, 0.0], [-0.0, -0.5, 0.0], [0.25, 0.0, -0.0]])
    assert _same(zero, 0.5, "-0.0").tolist() == [3, 3, 2, 2]
    for s in (1.0, 2.0 ** -20, 2.0 ** 30):                           # 9 s^2 + 16 s^2 == 25 s^2 exactly
        pair = np.array([[0.0, 0.0, 0.0], [3 * s, 4 * s, 0.0]])
        assert _same(pair, 5 * s, ("exact", s)).tolist() == [1, 1]
        assert _same(pair, np.nextafter(5 * s, 0.0), ("one ulp less", s)).tolist() == [0, 0]
        assert _same(pair, np.nextafter(5 * s, np.inf), ("one ulp more", s)).tolist() == [1, 1]
    for n_points in (1, 2, 65):                                      # coincident points: one cell, every other member a neighbour
        same = np.tile(np.array([[3.25, -1.5, 2.0]]), (n_points, 1))
        assert _same(same, 1e-3, ("identical", n_points)).tolist() == [n_points - 1] * n_points
    assert B.count_neighbors(np.zeros((0, 3)), 1.0).tolist() == []
    crowd = np.concatenate([rng.random((200, 3)) * 0.05, 0.5 + np.arange(30)[:, None] * [0.11, 0.0, 0.0], [[0.3, 0.3, 0.3]]])
    assert int(_same(crowd, 0.1, "a cell of 200 beside cells of one").max()) >= 199
    stray = np.concatenate([rng.random((400, 3)) * 0.01, [[1e7, 0.0, 0.0]]])      # 8e9 cells on an axis: still within the keys
    assert _same(stray, 1e-3, "stray")[-1] == 0


def test_the_pair_chunks_do_not_change_a_count(monkeypatch):
    xyz, radius = random_cloud(0)
    want = R.count_neighbors(xyz, radius)
    for pairs in (1, 7, 1000):                                       # an owner at a time, a few, many
        monkeypatch.setattr(B, "PAIRS", pairs)
        assert B.count_neighbors(xyz, radius).tobytes() == want.tobytes(), pairs


def test_refusals():
    xyz = np.zeros((3, 3))
    for radius in (0.0, -1.0, np.nan, np.inf, 1e-200, 1e200):
        with pytest.raises(ValueError, match="radius"):
            B.count_neighbors(xyz, radius)
    bad = xyz.copy()
    bad[1, 2] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        B.count_neighbors(bad, 1.0)
    # too wide for int64 keys: refused, never wrong.  The brute force answers (all isolated but the pair)
    wide = np.array([[0.0, 0.0, 0.0], [1e9, 1e9, 1e9], [1e9, 1e9, 1e9 + 0.5]])
    with pytest.raises(ValueError, match="too wide"):
        B.count_neighbors(wide, 1.0)                                 # 8e8 cells on each of three axes: 5e26 keys
    assert R.count_neighbors(wide, 1.0).tolist() == [0, 1, 1]
    with pytest.raises(ValueError, match="too wide"):
        B.count_neighbors(np.array([[0.0, 0.0, 0.0], [1e300, 0.0, 0.0]]), 1e-3)   # one axis beyond 2^40 cells
    with pytest.raises(ValueError, match="too wide"):
        B.count_neighbors(np.array([[-1e308, 0.0, 0.0], [1e308, 0.0, 0.0]]), 1.0)  # hi - lo overflows
    assert B.count_neighbors(wide * [1.0, 0.0, 1.0], 1.0).tolist() == [0, 1, 1]  # two wide axes: 6e17 keys


def test_the_candidates_of_a_kd_tree_give_the_same_counts():
    spatial = pytest.importorskip("scipy.spatial")
    for seed in (0, 3, 4, 11):
        xyz, radius = random_cloud(seed)
        pairs = spatial.cKDTree(xyz).query_pairs(radius * 1.001, output_type="ndarray")      # a superset by its own arithmetic
        d = xyz[pairs[:, 1]] - xyz[pairs[:, 0]]
        near = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) <= np.float64(radius) * np.float64(radius)
        want = np.bincount(pairs[near].reshape(-1), minlength=len(xyz)).astype(np.uint32)
        assert B.count_neighbors(xyz, radius).tobytes() == want.tobytes(), seed
