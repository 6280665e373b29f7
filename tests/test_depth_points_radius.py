"""The radius neighbour count of point clouds on the GPU (dmi_count_point_neighbors, dmi_views_filter_points_radius)
against its brute-force numpy restatement (depth_points_radius_np.py), byte for byte in every array, the counts and the report: the
resident view set's cloud with and without duplicates at several radii and at three values of the count kernel's knob, engineered
clouds, random clouds with ties on cell faces, the refusals and the life of the filtered cloud.  One small scene (9 views of
37 x 29); every case is milliseconds of kernels."""
import functools

import numpy as np
import pytest

import depth_points_np as P
import depth_points_radius_np as R
from view_set_model import ViewSetModel
from cudadepthmapintegration_amd import capi, scene

pytestmark = pytest.mark.gpu
N, W, H = 9, 37, 29
BUILD = dict(abs_tolerance=0.0, rel_tolerance=0.02, min_views=1)
INPUT_NAMES = ("xyz", "normal", "view", "pixel", "count")
KNOBS = (1, 7, None)   # the most queries a wave takes; None: the default, 64
SET_CASES = [(0, 0.05, 3), (0, 0.1, 8), (0, 0.3, 1), (0, 10.0, 1), (0, 0.02, 1), (0, 0.02, 3), (1, 0.1, 3), (0, 0.1, 0)]


@functools.lru_cache(maxsize=None)
def _views():
    return scene.make_views(N, W, H, seed=1)


@functools.lru_cache(maxsize=None)
def _built(dedupe):
    """The restated build of the scene's cloud (depth_points_np.py)."""
    views = _views()
    model = ViewSetModel()
    model.add(views, None)
    arrays, report = P.build_points(model.depth, views.K4, views.RT4, dedupe=bool(dedupe), **BUILD)
    for a in arrays.values():
        a.setflags(write=False)
    return arrays, report


@functools.lru_cache(maxsize=None)
def _counts(dedupe, radius):
    neighbors = R.count_neighbors(_built(dedupe)[0]["xyz"], radius)
    neighbors.setflags(write=False)
    return neighbors


def _filtered(dedupe, radius, min_neighbors):
    cloud, _ = _built(dedupe)
    neighbors = _counts(dedupe, radius)
    keep = neighbors >= min_neighbors
    arrays = {name: np.ascontiguousarray(cloud[name][keep]) for name in INPUT_NAMES}
    arrays["neighbors"] = neighbors[keep]
    return arrays, R.report_of(neighbors, min_neighbors)


def _assert_equal(got, report, want, want_report, label=None):
    for name in want:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (label, name, got[name].shape, want[name].shape)
        assert got[name].tobytes() == want[name].tobytes(), (label, name)
    assert {k: int(report[k]) for k in R.REPORT_NAMES} == {k: want_report[k] for k in R.REPORT_NAMES}, label
    assert int(report["distance_tests"]) >= want_report["neighbor_sum"] and want_report["neighbor_sum"] % 2 == 0, label


def _new_set(dedupe, piece_bytes=None):
    s = capi.ViewSet(W, H)
    if piece_bytes is not None:
        s.set_piece_bytes(piece_bytes)
    s.add(_views())
    s.build_points(dedupe=bool(dedupe), **BUILD)
    return s


def _download(s, members=False):
    arrays = s.download_points()
    if members:
        arrays["members"] = s.download_point_members()
    arrays["neighbors"] = s.download_point_neighbors()
    return arrays


def test_the_view_set_cases_are_not_vacuous():
    """The restatement's own numbers for the scene, from a brute-force count on the CPU."""
    cloud, report = _built(0)
    assert report["points"] == len(cloud["xyz"]) == 1267 and _built(1)[1]["points"] == 510
    n = _counts(0, 0.02)
    assert int((n == 0).sum()) == 1001 and int(n.max()) == 2
    n = _counts(0, 0.05)
    assert int((n == 0).sum()) == 136 and int((n < 3).sum()) == 1159 and int(n.sum()) == 1798
    assert _filtered(0, 0.05, 3)[1]["points_kept"] == 108
    n = _counts(0, 0.1)
    assert int((n == 0).sum()) == 0 and int((n < 8).sum()) == 520 and int(n.max()) == 13 and int(n.sum()) == 9934
    n = _counts(0, 0.3)
    assert int(n.max()) == 92 and int(n.sum()) == 99270            # above one wave's 64
    assert np.all(_counts(0, 10.0) == 1266)                         # one cell
    n = _counts(1, 0.1)
    assert int((n == 0).sum()) == 15 and int((n < 3).sum()) == 201
    assert _filtered(0, 0.02, 3)[1]["points_kept"] == 0


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("dedupe,radius,min_neighbors", SET_CASES)
def test_the_view_set_cloud_equals_the_restatement(dedupe, radius, min_neighbors, knob):
    want, want_report = _filtered(dedupe, radius, min_neighbors)
    with _new_set(dedupe) as s:
        if knob is not None:
            s.set_radius_group_points(knob)
        held, steps = s.info().device_bytes, s.info().steps
        report = s.filter_points_radius(radius, min_neighbors)
        _assert_equal(_download(s), report, want, want_report, (dedupe, radius, min_neighbors, knob))
        assert report["kernel_ms"] > 0 and report["points_in"] == _built(dedupe)[1]["points"]
        passes = s.radius_pass_ms()
        assert list(passes) == ["bounds", "keys", "sort", "ranks", "permute", "count", "compaction"] and all(v >= 0 for v in passes.values())
        info = s.info()
        assert info.steps == steps + 1                                                         # a step of the set
        assert info.device_bytes == held - 48 * report["points_in"] + 52 * report["points_kept"]   # the scratch is gone, the cloud is held
        assert np.all(s.download_point_members() == 1)


def test_the_context_free_call_gives_the_same_counts_and_flags():
    for dedupe, radius, min_neighbors in ((0, 0.05, 3), (0, 0.3, 1), (1, 0.1, 3), (0, 0.02, 3), (0, 10.0, 0)):
        want = _counts(dedupe, radius)
        neighbors, keep, report = capi.count_point_neighbors(_built(dedupe)[0]["xyz"], radius=radius, min_neighbors=min_neighbors)
        assert neighbors.dtype == np.uint32 and neighbors.tobytes() == want.tobytes(), (dedupe, radius)
        assert np.array_equal(keep, want >= min_neighbors)
        want_report = R.report_of(want, min_neighbors)
        assert {k: int(report[k]) for k in R.REPORT_NAMES} == want_report and report["distance_tests"] >= want_report["neighbor_sum"]


def _compare_cloud(xyz, radius, min_neighbors=1, label=None):
    want = R.count_neighbors(xyz, radius)
    neighbors, keep, report = capi.count_point_neighbors(xyz, radius=radius, min_neighbors=min_neighbors)
    assert neighbors.tobytes() == want.tobytes(), (label, np.flatnonzero(neighbors != want)[:8])
    assert np.array_equal(keep, want >= min_neighbors), label
    assert {k: int(report[k]) for k in R.REPORT_NAMES} == R.report_of(want, min_neighbors), label
    assert report["distance_tests"] >= int(want.sum()), label
    return neighbors, report


def test_engineered_clouds():
    rng = np.random.default_rng(3)
    for n_points in (1, 2, 63, 64, 65, 257):                         # all points identical: hi == lo, one cell, whole and broken waves
        same = np.tile(np.array([[3.25, -1.5, 2.0]]), (n_points, 1))
        neighbors, _ = _compare_cloud(same, 1e-3, label=("identical", n_points))
        assert np.all(neighbors == n_points - 1)
    line = np.zeros((300, 3))
    line[:, 0] = rng.integers(0, 400, 300) * 0.125                   # collinear: n_1 = n_2 = 1, ties at the radius abound
    _compare_cloud(line, 0.5, 2, "collinear")
    line[:, [0, 2]] = line[:, [2, 0]]
    _compare_cloud(line, 0.5, 2, "collinear in z")
    plane = np.zeros((500, 3))
    plane[:, :2] = rng.integers(0, 40, (500, 2)) * 0.25
    _compare_cloud(plane + [0.0, 0.0, 7.0], 0.75, 4, "planar")
    two = rng.random((200, 3)) * [1.9, 0.9, 0.9]                      # two cells wide on x, one on y and z
    _compare_cloud(two, 1.0, 1, "two cells wide")
    h = 0.5 * (1 + 2.0 ** -10)                                       # the cell size of radius 0.5: points exactly on faces and on the upper bounds
    faces = np.array([[i, j, k] for i in range(5) for j in range(4) for k in range(3)], dtype=np.float64) * h
    _compare_cloud(np.concatenate([faces, faces[:20] + h / 2]), 0.5, 1, "faces")
    for s in (1.0, 2.0 ** -20, 2.0 ** 30):                           # 9 s^2 + 16 s^2 == 25 s^2 exactly
        pair = np.array([[0.0, 0.0, 0.0], [3 * s, 4 * s, 0.0]])
        assert _compare_cloud(pair, 5 * s, label=("exact", s))[0].tolist() == [1, 1]
        assert _compare_cloud(pair, np.nextafter(5 * s, 0.0), label=("one ulp less", s))[0].tolist() == [0, 0]
    crowd = np.concatenate([rng.random((200, 3)) * 0.05, 0.5 + np.arange(30)[:, None] * [0.11, 0.0, 0.0], [[0.3, 0.3, 0.3]]])
    neighbors, report = _compare_cloud(crowd, 0.1, 5, "a cell of 200 beside cells of one")
    assert report["max_neighbors"] >= 199 and report["isolated"] >= 1
    geo = np.array([448262.5, 5411932.25, 312.0]) * 10
    _compare_cloud(geo + rng.integers(0, 64, (800, 3)) * 0.125, 0.375, 3, "geo-referenced")
    zero = np.array([[-0.0, 0.0, -0.0], [0.0, -0.0, 0.0], [-0.0, -0.5, 0.0], [0.25, 0.0, -0.0]])
    assert _compare_cloud(zero, 0.5, label="-0.0")[0].tolist() == [3, 3, 2, 2]
    stray = np.concatenate([rng.random((400, 3)) * 0.01, [[1e7, 0.0, 0.0]]])          # the cells are enlarged, the call is not refused
    neighbors, report = _compare_cloud(stray, 1e-3, 1, "stray")
    assert neighbors[-1] == 0 and report["isolated"] >= 1 and report["max_neighbors"] > 0
    _compare_cloud(stray * [1.0, 0.0, 0.0] + [-5e6, 3.0, 3.0], 1e-3, 1, "stray on a line")


@pytest.mark.parametrize("seed", range(20))
def test_random_clouds(seed):
    rng = np.random.default_rng(2000 + seed)
    n_points = int(rng.integers(100, 2001)) if seed else 2000
    radius = float(rng.choice([0.25, 0.3, 0.5, 1.7])) if seed % 2 else float(rng.uniform(0.05, 2.0))
    extent = (3, 6, 12, 40)[seed % 4]
    offset = 5e6 if seed in (11, 17) else 0.0
    if seed % 3 == 0:                                               # coordinates on the faces of the radius' own cells: ties placed there
        xyz = offset + rng.integers(0, extent, (n_points, 3)).astype(np.float64) * (radius * (1 + 2.0 ** -10))
        xyz[rng.random(n_points) < 0.5] += radius / 4
    else:
        xyz = offset + rng.integers(0, 4 * extent, (n_points, 3)).astype(np.float64) * (radius / 4)   # quantised: exact ties abound
    _, report = _compare_cloud(xyz, radius, seed % 5, seed)
    assert report["points_in"] == n_points
    if seed == 0:
        assert report["max_neighbors"] > 64


def test_refusals_and_the_life_of_the_filtered_cloud():
    nan = float("nan")
    with capi.ViewSet(W, H) as s:
        s.add(_views())
        for call in (lambda: s.filter_points_radius(0.1), s.download_point_neighbors, s.radius_pass_ms):   # no build yet
            with pytest.raises(capi.DmiError) as e:
                call()
            assert e.value.code == 4
        s.build_points(dedupe=False, **BUILD)
        points = s.download_points()
        for call in (s.download_point_neighbors, s.radius_pass_ms):                  # built, not filtered
            with pytest.raises(capi.DmiError) as e:
                call()
            assert e.value.code == 4
        held, steps = s.info().device_bytes, s.info().steps

        def unchanged():
            again = s.download_points()
            return all(again[k].tobytes() == points[k].tobytes() for k in points) and s.info().device_bytes == held and s.info().steps == steps

        for radius, min_neighbors, word in ((nan, 1, "radius"), (0.0, 1, "radius"), (-1.0, 1, "radius"), (float("inf"), 1, "radius"),
                                            (1e-200, 1, "radius"), (0.1, -1, "min_neighbors")):
            with pytest.raises(capi.DmiError) as e:
                s.filter_points_radius(radius, min_neighbors)
            assert e.value.code == 1 and word in str(e.value) and "dmi_views_filter_points_radius" in str(e.value)
        for k in (0, 65):
            with pytest.raises(capi.DmiError) as e:
                s.set_radius_group_points(k)
            assert e.value.code == 1
        assert s._lib.dmi_views_filter_points_radius(s._h, 0.1, 1, None, None) == 1 and "n_points" in s._lib.dmi_views_last_error(s._h).decode()
        assert unchanged()
        # a radius far too small for 2^21 bins is not refused: every point is isolated
        report = s.filter_points_radius(1e-9, 0)
        assert report["isolated"] == 1267 - int((_counts(0, 1e-9) > 0).sum()) and report["points_kept"] == 1267
        # the filter twice equals the restatement applied twice
        s.build_points(dedupe=False, **BUILD)
        s.filter_points_radius(0.1, 8)
        once, _ = _filtered(0, 0.1, 8)
        twice, twice_report = R.filter_radius({k: once[k] for k in INPUT_NAMES}, 0.1, 8)
        report = s.filter_points_radius(0.1, 8)
        _assert_equal(_download(s), report, twice, twice_report, "twice")
        # thin after filter equals the context-free thinning of the downloaded filtered arrays; the counts go with the old cloud
        s.build_points(dedupe=False, **BUILD)
        s.filter_points_radius(0.05, 1)
        filtered = s.download_points()
        want, _ = capi.thin_point_cloud(*(filtered[name] for name in INPUT_NAMES), cell_size=0.1)
        s.thin_points(0.1)
        got = s.download_points()
        got["members"] = s.download_point_members()
        assert all(got[k].tobytes() == want[k].tobytes() for k in want)
        with pytest.raises(capi.DmiError) as e:
            s.download_point_neighbors()
        assert e.value.code == 4
        # filter after thin keeps members
        held, steps = s.info().device_bytes, s.info().steps
        report = s.filter_points_radius(0.15, 5)
        thinned_kept, thinned_report = R.filter_radius(got, 0.15, 5)
        _assert_equal(_download(s, members=True), report, thinned_kept, thinned_report, "filter after thin")
        assert 0 < report["points_kept"] < report["points_in"]
        assert s.info().device_bytes == held - 52 * report["points_in"] + 56 * report["points_kept"] and s.info().steps == steps + 1
        # a step that changes D drops the filtered cloud; so do a build and an add
        s.filter_consistency(min_views=0)
        for call in (lambda: s.download_points(0, 0), s.download_point_neighbors, s.radius_pass_ms, lambda: s.filter_points_radius(0.1)):
            with pytest.raises(capi.DmiError) as e:
                call()
            assert e.value.code == 4
        s.build_points(dedupe=False, **BUILD)
        s.filter_points_radius(0.1, 1)
        s.build_points(dedupe=False, **BUILD)
        with pytest.raises(capi.DmiError) as e:
            s.download_point_neighbors()
        assert e.value.code == 4
        s.filter_points_radius(0.1, 1)
        s.add(_views())
        with pytest.raises(capi.DmiError) as e:
            s.download_point_neighbors()
        assert e.value.code == 4
    for device in (-1, 10 ** 6):
        with pytest.raises(capi.DmiError) as e:
            capi.count_point_neighbors(points["xyz"], radius=0.1, device=device)
        assert e.value.code == 1 and "device" in str(e.value)
    bad = points["xyz"].copy()
    bad[617, 1] = nan
    with pytest.raises(capi.DmiError) as e:
        capi.count_point_neighbors(bad, radius=0.1)
    assert e.value.code == 1 and "non-finite" in str(e.value)


@pytest.mark.parametrize("views_per_piece", [2, 1])
def test_a_build_in_pieces_followed_by_the_filter_gives_the_same_bytes(views_per_piece):
    want, want_report = _filtered(0, 0.1, 8)
    with _new_set(0, piece_bytes=views_per_piece * W * H * 8) as s:
        report = s.filter_points_radius(0.1, 8)
        _assert_equal(_download(s), report, want, want_report, views_per_piece)


def test_a_cloud_without_points_filters_to_none():
    views = _views()
    with capi.ViewSet(W, H) as s:
        s.add(scene.Views(np.full_like(views.depth, -1.0), views.K4, views.RT4, None))
        assert s.build_points(**BUILD)["points"] == 0
        report = s.filter_points_radius(0.1)
        assert {k: int(report[k]) for k in R.REPORT_NAMES} == dict.fromkeys(R.REPORT_NAMES, 0)
        assert len(s.download_points()["view"]) == 0 and len(s.download_point_neighbors()) == 0
