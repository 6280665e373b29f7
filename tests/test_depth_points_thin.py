"""The voxel-grid thinning of point clouds on the GPU (dmi_thin_point_cloud, dmi_views_thin_points) against its numpy
restatement (depth_points_thin_np.py), byte for byte in all six arrays and the report: the resident view set's cloud with and without
duplicates at several cell sizes and with the wave pass driven at small cells, engineered clouds, random clouds with border ties,
the refusals and the life of the thinned cloud.  One small scene (9 views of 37 x 29); every case is milliseconds of kernels."""
import functools

import numpy as np
import pytest

import depth_points_np as P
import depth_points_thin_np as T
from view_set_model import ViewSetModel
from cudadepthmapintegration_amd import capi, scene

pytestmark = pytest.mark.gpu
N, W, H = 9, 37, 29
BUILD = dict(abs_tolerance=0.0, rel_tolerance=0.02, min_views=1)
INPUT_NAMES = ("xyz", "normal", "view", "pixel", "count")
KNOBS = (1, 4, None)   # the wave pass takes cells above this many members; None: the default


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
def _thinned(dedupe, cell_size, min_points):
    cloud, _ = _built(dedupe)
    arrays, report = T.thin(*(cloud[name] for name in INPUT_NAMES), cell_size=cell_size, min_points=min_points)
    for a in arrays.values():
        a.setflags(write=False)
    return arrays, report


def _assert_equal(got, report, want, want_report, label=None):
    for name in T.ARRAY_NAMES:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (label, name, got[name].shape, want[name].shape)
        assert got[name].tobytes() == want[name].tobytes(), (label, name)
    assert {k: int(report[k]) for k in T.REPORT_NAMES} == {k: want_report[k] for k in T.REPORT_NAMES}, label


def _new_set(dedupe, piece_bytes=None):
    s = capi.ViewSet(W, H)
    if piece_bytes is not None:
        s.set_piece_bytes(piece_bytes)
    s.add(_views())
    s.build_points(dedupe=bool(dedupe), **BUILD)
    return s


def _download(s):
    arrays = s.download_points()
    arrays["members"] = s.download_point_members()
    return arrays


def _thin_and_compare(s, dedupe, cell_size, min_points, label=None):
    want, want_report = _thinned(dedupe, cell_size, min_points)
    report = s.thin_points(cell_size, min_points)
    _assert_equal(_download(s), report, want, want_report, label)
    return report


def test_the_view_set_cases_are_not_vacuous():
    cloud, report = _built(0)
    assert report["points"] == len(cloud["xyz"]) == 1267
    _, thin = _thinned(0, 0.1, 1)
    assert thin["multi_view_cells"] >= 100 and thin["largest_cell"] >= 3 and thin["cells"] < 1267
    assert _thinned(0, 0.1, 3)[1]["cells_kept"] < thin["cells"]
    assert _thinned(0, 0.3, 1)[1]["largest_cell"] > 32              # above the default threshold: the wave pass runs at every knob
    assert _thinned(0, 10.0, 1)[1]["cells"] == 1 and _thinned(0, 10.0, 1)[0]["members"].tolist() == [1267]
    assert _built(1)[1]["points"] == 510 and _thinned(1, 0.1, 1)[1]["multi_view_cells"] > 0


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("dedupe,cell_size,min_points", [(0, 0.1, 1), (0, 0.1, 3), (1, 0.1, 1), (1, 0.1, 3), (0, 0.3, 1), (0, 0.3, 3),
                                                         (0, 10.0, 1), (0, 10.0, 3)])
def test_the_view_set_cloud_equals_the_restatement(dedupe, cell_size, min_points, knob):
    with _new_set(dedupe) as s:
        if knob is not None:
            s.set_thin_wave_cell_points(knob)
        held, steps = s.info().device_bytes, s.info().steps
        report = _thin_and_compare(s, dedupe, cell_size, min_points, (dedupe, cell_size, min_points, knob))
        assert report["kernel_ms"] > 0 and report["points_in"] == _built(dedupe)[1]["points"]
        passes = s.thin_pass_ms()
        assert list(passes) == ["bounds", "keys", "sort", "ranks", "representatives"] and all(v >= 0 for v in passes.values())
        info = s.info()
        assert info.steps == steps + 1                                                     # a step of the set
        assert info.device_bytes == held - 48 * report["points_in"] + 52 * report["cells_kept"]   # the scratch is gone, the cloud is held


def test_the_context_free_call_gives_the_same_bytes():
    for dedupe, cell_size, min_points in ((0, 0.1, 1), (0, 0.3, 3), (1, 0.1, 1)):
        cloud, _ = _built(dedupe)
        want, want_report = _thinned(dedupe, cell_size, min_points)
        got, report = capi.thin_point_cloud(*(cloud[name] for name in INPUT_NAMES), cell_size=cell_size, min_points=min_points)
        _assert_equal(got, report, want, want_report, (dedupe, cell_size, min_points))


def _compare_cloud(xyz, normal=None, view=None, pixel=None, count=None, label=None, **params):
    want, want_report = T.thin(xyz, normal, view, pixel, count, **params)
    got, report = capi.thin_point_cloud(xyz, normal, view, pixel, count, **params)
    _assert_equal(got, report, want, want_report, label)
    return got, report


def _random_cloud(seed, n_points, h, offset=0.0, extent=6):
    rng = np.random.default_rng(seed)
    xyz = offset + rng.integers(0, 4 * extent, (n_points, 3)).astype(np.float64) * (h / 4)   # quantised to h / 4: border ties abound
    normal = rng.normal(size=(n_points, 3)).astype(np.float32)
    normal /= np.linalg.norm(normal, axis=1, keepdims=True).astype(np.float32)
    normal[rng.random(n_points) < 0.2] = 0.0
    view = np.sort(rng.integers(0, 12, n_points)).astype(np.int32)
    pixel = rng.integers(0, 1 << 20, n_points).astype(np.int32)
    count = rng.integers(0, 12, n_points).astype(np.int32)
    return xyz, normal, view, pixel, count


def test_engineered_clouds():
    h = 0.375   # representable, and so is every lo + m * h below
    # coordinates on exact bin borders, with -0.0 among them
    m = np.array([[i, j, k] for i in range(-3, 4) for j in (-1, 0, 2) for k in (0, 5)], dtype=np.float64)
    border = np.concatenate([m * h, m * h + h / 2, -np.abs(m[:5]) * 0.0])
    got, report = _compare_cloud(border, cell_size=h, label="borders")
    assert report["cells"] < len(border) and np.signbit(border).any()
    got, _ = _compare_cloud(np.array([[-0.0, -0.0, 0.0], [-0.0, 0.0, -0.0]]), cell_size=1.0, label="-0.0")
    assert np.signbit(got["xyz"][0]).tolist() == [True, False, False] and got["members"].tolist() == [2]
    got, _ = _compare_cloud(np.array([[-0.0, 5.0, -0.0]]), np.array([[-0.0, 0.0, 1.0]], np.float32), cell_size=1.0, label="one -0.0")
    assert np.signbit(got["xyz"][0]).tolist() == [True, False, True] and np.signbit(got["normal"][0, 0])
    # all points identical (hi == lo, one cell), P around the block size; nullable inputs absent
    for n_points in (1, 2, 255, 256, 257):
        same = np.tile(np.array([[3.25, -1.5, 2.0]]), (n_points, 1))
        got, report = _compare_cloud(same, cell_size=1e-3, label=("identical", n_points))
        assert got["xyz"].tolist() == [[3.25, -1.5, 2.0]] and got["members"].tolist() == [n_points] and report["with_normal"] == 0
        assert got["view"].tolist() == [0] and got["pixel"].tolist() == [0] and got["count"].tolist() == [0]
        xyz, normal, view, pixel, count = _random_cloud(100 + n_points, n_points, h)
        _compare_cloud(xyz, normal, view, pixel, count, cell_size=h, label=("random", n_points))
        _compare_cloud(xyz, None, view, None, count, cell_size=h, min_points=2, label=("some absent", n_points))
    # P == 0: a success with no points
    got, report = capi.thin_point_cloud(np.zeros((0, 3)), cell_size=1.0)
    assert all(len(got[name]) == 0 for name in T.ARRAY_NAMES) and report["points_in"] == 0 and report["cells"] == 0
    # no cell reaches min_points: a success with no points
    got, report = _compare_cloud(border, cell_size=h, min_points=len(border) + 1, label="none kept")
    assert len(got["xyz"]) == 0 and report["cells_kept"] == 0 and report["cells"] > 1 and report["largest_cell"] >= 1
    # normals that are all zero, and normals that cancel exactly
    xyz, _, view, pixel, count = _random_cloud(7, 300, h, extent=2)
    got, report = _compare_cloud(xyz, np.zeros((300, 3), np.float32), view, pixel, count, cell_size=h, label="zero normals")
    assert report["with_normal"] == 0 and report["largest_cell"] > 1
    pairs = np.repeat(xyz[:150], 2, axis=0)
    up = np.tile(np.array([[0.0, 0.6, 0.8], [-0.0, -0.6, -0.8]], np.float32), (150, 1))
    got, report = _compare_cloud(pairs, up, cell_size=h, label="cancelling normals")
    assert report["with_normal"] == 0 and np.all(got["normal"] == 0.0) and np.all(got["members"] % 2 == 0)


def test_in_place_outputs_and_a_refusal_that_leaves_them_untouched():
    h = 0.5
    xyz, normal, view, pixel, count = _random_cloud(11, 1000, h)
    want, want_report = T.thin(xyz, normal, view, pixel, count, cell_size=h)
    given = [a.copy() for a in (xyz, normal, view, pixel, count)]
    got, report = capi.thin_point_cloud(*given, cell_size=h, in_place=True)
    _assert_equal(got, report, want, want_report, "in place")
    assert all(np.shares_memory(got[name], a) for name, a in zip(INPUT_NAMES, given))
    # a NaN coordinate: refused on the device's bounds, the outputs (the inputs themselves) untouched
    given = [a.copy() for a in (xyz, normal, view, pixel, count)]
    given[0][617, 1] = np.nan
    before = [a.tobytes() for a in given]
    with pytest.raises(capi.DmiError) as e:
        capi.thin_point_cloud(*given, cell_size=h, in_place=True)
    assert e.value.code == 1 and "non-finite" in str(e.value) and "dmi_thin_point_cloud" in str(e.value)
    assert [a.tobytes() for a in given] == before
    with pytest.raises(ValueError, match="non-finite"):
        T.thin(*given, cell_size=h)
    for value in (np.inf, -np.inf):
        bad = xyz.copy()
        bad[3, 0] = value
        with pytest.raises(capi.DmiError) as e:
            capi.thin_point_cloud(bad, cell_size=h)
        assert e.value.code == 1 and "non-finite" in str(e.value)


@pytest.mark.parametrize("seed", range(12))
def test_random_clouds(seed):
    rng = np.random.default_rng(1000 + seed)
    n_points = int(rng.integers(200, 3001)) if seed else 3000
    h = (0.25, 0.3, 1.7)[seed % 3]
    offset = 5e6 if seed == 11 else 0.0                     # geo-referenced magnitudes: lo is subtracted before anything is divided
    extent = (3, 6, 12, 40)[seed % 4]                       # from a few crowded cells (the wave pass) to mostly single ones
    cloud = _random_cloud(seed, n_points, h, offset, extent)
    min_points = 1 + seed % 3
    _, report = _compare_cloud(*cloud, cell_size=h, min_points=min_points, label=seed)
    assert report["points_in"] == n_points and 1 <= report["cells"] <= n_points
    if seed == 0:                                           # 3000 points in 27 cells
        assert report["largest_cell"] > 32


def test_refusals_and_the_life_of_the_thinned_cloud():
    nan, inf = float("nan"), float("inf")
    with capi.ViewSet(W, H) as s:
        s.add(_views())
        for call in (lambda: s.thin_points(0.1), s.download_point_members, s.thin_pass_ms):   # no build yet
            with pytest.raises(capi.DmiError) as e:
                call()
            assert e.value.code == 4
        report = s.build_points(dedupe=False, **BUILD)
        points = _download(s)
        assert points["members"].dtype == np.uint32 and np.all(points["members"] == 1) and len(points["members"]) == report["points"] == 1267
        with pytest.raises(capi.DmiError) as e:
            s.thin_pass_ms()                                 # built, not thinned
        assert e.value.code == 4
        held, steps = s.info().device_bytes, s.info().steps

        def unchanged():
            again = _download(s)
            return all(again[k].tobytes() == points[k].tobytes() for k in points) and s.info().device_bytes == held and s.info().steps == steps

        # cell 1e-9: about 1.2e9 bins on an axis
        with pytest.raises(capi.DmiError) as e:
            s.thin_points(1e-9)
        least = T.min_cell_size(points["xyz"])
        assert e.value.code == 1 and "2^21 bins" in str(e.value) and "smallest acceptable cell size" in str(e.value)
        assert float(str(e.value).rsplit(" ", 1)[1]) == least
        with pytest.raises(ValueError, match="2\\^21"):
            T.thin(points["xyz"], cell_size=1e-9)
        assert unchanged()
        for cell_size in (nan, 0.0, -0.5, inf, -inf):
            with pytest.raises(capi.DmiError) as e:
                s.thin_points(cell_size)
            assert e.value.code == 1 and "cell_size" in str(e.value) and "dmi_views_thin_points" in str(e.value)
            with pytest.raises(capi.DmiError) as e:
                capi.thin_point_cloud(points["xyz"], cell_size=cell_size)
            assert e.value.code == 1 and "cell_size" in str(e.value)
        for min_points in (0, -3):
            with pytest.raises(capi.DmiError) as e:
                s.thin_points(0.1, min_points)
            assert e.value.code == 1 and "min_points" in str(e.value)
            with pytest.raises(capi.DmiError) as e:
                capi.thin_point_cloud(points["xyz"], cell_size=0.1, min_points=min_points)
            assert e.value.code == 1 and "min_points" in str(e.value)
        with pytest.raises(capi.DmiError) as e:
            s.set_thin_wave_cell_points(0)
        assert e.value.code == 1
        assert s._lib.dmi_views_thin_points(s._h, 0.1, 1, None, None) == 1 and "n_points" in s._lib.dmi_views_last_error(s._h).decode()
        assert unchanged()
        # a thinning, and a second one refused: the thinned cloud stays
        _thin_and_compare(s, 0, 0.1, 1, "first")
        thinned = _download(s)
        with pytest.raises(capi.DmiError) as e:
            s.thin_points(0.2)
        assert e.value.code == 4 and "build again" in str(e.value)
        assert all(_download(s)[k].tobytes() == thinned[k].tobytes() for k in thinned)
        # a build replaces it and may be thinned again: two runs give identical bytes
        s.build_points(dedupe=False, **BUILD)
        assert np.all(s.download_point_members() == 1)
        _thin_and_compare(s, 0, 0.1, 1, "second")
        assert all(_download(s)[k].tobytes() == thinned[k].tobytes() for k in thinned)
        # a step that changes D drops the thinned cloud
        before = s.info().device_bytes
        s.filter_consistency(min_views=0)
        assert s.info().device_bytes <= before - 52 * len(thinned["view"])
        for call in (lambda: s.download_points(0, 0), s.download_point_members, s.thin_pass_ms, lambda: s.thin_points(0.1)):
            with pytest.raises(capi.DmiError) as e:
                call()
            assert e.value.code == 4
    # out-of-range arguments of the context-free call
    for device in (-1, 10 ** 6):
        with pytest.raises(capi.DmiError) as e:
            capi.thin_point_cloud(points["xyz"], cell_size=0.1, device=device)
        assert e.value.code == 1 and "device" in str(e.value)


@pytest.mark.parametrize("views_per_piece", [2, 1])
def test_a_build_in_pieces_followed_by_a_thinning_gives_the_same_bytes(views_per_piece):
    with _new_set(0, piece_bytes=views_per_piece * W * H * 8) as s:
        _thin_and_compare(s, 0, 0.1, 3, views_per_piece)


def test_a_cloud_without_points_thins_to_none():
    views = _views()
    with capi.ViewSet(W, H) as s:
        s.add(scene.Views(np.full_like(views.depth, -1.0), views.K4, views.RT4, None))
        assert s.build_points(**BUILD)["points"] == 0
        report = s.thin_points(0.1)
        assert {k: int(report[k]) for k in T.REPORT_NAMES} == dict.fromkeys(T.REPORT_NAMES, 0)
        assert len(s.download_points()["view"]) == 0 and len(s.download_point_members()) == 0
