"""The plane fit of point clouds on the GPU (dmi_fit_point_planes, dmi_views_fit_point_planes) against its brute-force
numpy restatement (depth_points_planes_np.py): every array compared as integer bit patterns, through the context-free call and
through a resident view set.  Engineered clouds at every size at which the kernel takes another path (the unit split at 64 points,
the batch tail at 64 candidates, grids one and two cells wide, a stray that makes the rest one cell), geo-referenced coordinates,
duplicates, the radius tie, random clouds, the knob of the work units, more units than the kernel has waves (33 001 points at knob
1: the restatement's pair matrix of 1.1e9 tests is the slow part, some seconds of CPU), the flags, and the life of the fitted cloud
in the set."""
import functools

import numpy as np
import pytest

import depth_points_np as P
import depth_points_planes_np as F
from view_set_model import ViewSetModel
from cudadepthmapintegration_amd import capi, scene

pytestmark = pytest.mark.gpu
N, W, H = 9, 37, 29
BUILD = dict(abs_tolerance=0.0, rel_tolerance=0.02, min_views=1)
INPUT_NAMES = ("xyz", "normal", "view", "pixel", "count")
BITS = {np.dtype(np.float64): np.uint64, np.dtype(np.float32): np.uint32, np.dtype(np.uint32): np.uint32, np.dtype(np.int32): np.uint32}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(BITS[a.dtype])


def _assert_bits(got, want, label):
    for name in want:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (label, name)
        differ = np.flatnonzero((_bits(got[name]) != _bits(want[name])).reshape(len(want[name]), -1).any(axis=1))
        assert len(differ) == 0, (label, name, differ[:8], got[name][differ[:4]], want[name][differ[:4]])


def _assert_report(report, want, label):
    assert {k: int(report[k]) for k in F.REPORT_NAMES} == {k: want[k] for k in F.REPORT_NAMES}, label
    assert float(report["max_shift"]) == want["max_shift"], label
    assert int(report["distance_tests"]) >= want["neighbor_sum"] + want["points_in"], label


def _compare(xyz, normal, radius, min_neighbors=2, flags=3, label=None):
    want, want_report = F.fit_planes(xyz, normal, radius, min_neighbors, flags)
    got, report = capi.fit_point_planes(xyz, normal, radius=radius, min_neighbors=min_neighbors, move=bool(flags & 1), normals=bool(flags & 2))
    _assert_bits(got, want, label)
    _assert_report(report, want_report, label)
    return got, report


def _bumpy(rng, xy, normals=True):
    """Points over the given xy with a little height, and unit normals roughly upwards or downwards."""
    xyz = np.concatenate([xy, rng.normal(scale=0.01, size=(len(xy), 1))], axis=1)
    if not normals:
        return xyz, None
    normal = rng.normal(scale=0.2, size=(len(xy), 3)) + [0.0, 0.0, 1.0]
    normal[rng.random(len(xy)) < 0.3] *= -1.0
    return xyz, (normal / np.linalg.norm(normal, axis=1)[:, None]).astype(np.float32)


def test_one_two_and_three_points():
    rng = np.random.default_rng(1)
    for n_points in (1, 2, 3):
        xyz = rng.random((n_points, 3)) * 0.1
        got, report = _compare(xyz, None, 1.0, 2, 3, n_points)
        assert report["fitted"] == (3 if n_points == 3 else 0) and report["unsupported"] == n_points - report["fitted"]
        if n_points < 3:
            assert np.all(got["plane_rms"] == -1.0) and got["xyz"].tobytes() == xyz.tobytes()
    none, report = capi.fit_point_planes(np.zeros((0, 3)), radius=1.0)
    assert len(none["plane_rms"]) == 0 and report["points_in"] == 0


@pytest.mark.parametrize("n_points", [64, 65])
def test_a_row_of_64_and_of_65_points_splits_into_units(n_points):
    rng = np.random.default_rng(n_points)
    xy = np.stack([np.arange(n_points) * 0.01, rng.random(n_points) * 0.02], axis=1)    # one grid row at radius 1: one unit, or two
    _, report = _compare(*_bumpy(rng, xy), 1.0, 3, 3, n_points)
    assert report["fitted"] == n_points and report["max_neighbors"] == n_points - 1


@pytest.mark.parametrize("run", [63, 64, 65])
def test_candidate_runs_round_the_batch_of_64(run):
    rng = np.random.default_rng(run)
    xy = rng.random((run, 2)) * 0.05                                   # one cell of `run` points: one run of 63, 64 or 65 candidates
    _, report = _compare(*_bumpy(rng, xy), 0.5, 3, 3, run)
    assert report["fitted"] == run


@pytest.mark.parametrize("wide", [1, 2])
def test_grids_one_and_two_cells_wide(wide):
    rng = np.random.default_rng(10 + wide)
    xyz = rng.random((300, 3)) * [0.95 * wide, 0.9, 0.9]
    _compare(xyz, None, 1.0, 4, 3, wide)
    _compare(xyz[:, [1, 0, 2]], None, 1.0, 4, 1, (wide, "on y"))


def test_a_far_stray_makes_the_rest_one_cell():
    rng = np.random.default_rng(5)
    xyz, normal = _bumpy(rng, rng.random((400, 2)) * 0.05)
    xyz = np.concatenate([xyz, [[1e7, 0.0, 0.0]]])
    normal = np.concatenate([normal, [[0.0, 0.0, 1.0]]]).astype(np.float32)
    got, report = _compare(xyz, normal, 0.01, 3, 3, "stray")            # cells of 1e7 / 2^21 = 4.8: the 400 share one
    assert got["plane_rms"][-1] == -1.0 and report["unsupported"] >= 1 and report["fitted"] > 300


def test_geo_referenced_coordinates_duplicates_and_the_radius_tie():
    rng = np.random.default_rng(6)
    xyz, normal = _bumpy(rng, rng.integers(0, 48, (900, 2)) * 0.125)
    _compare(xyz + 5e6, normal, 0.375, 4, 3, "offset by 5e6")
    twice = np.concatenate([xyz[:300], xyz[:300], xyz[:50]])
    _compare(twice, np.concatenate([normal[:300], normal[:300], normal[:50]]), 0.2, 2, 3, "duplicates")
    same = np.tile(np.array([[3.25, -1.5, 2.0]]), (70, 1))               # C = 0: the procedure's normal
    got, _ = _compare(same, None, 1e-3, 2, 3, "coincident")
    assert np.all(got["normal"] == [1.0, 0.0, 0.0]) and np.all(got["plane_rms"] == 0.0) and got["xyz"].tobytes() == same.tobytes()
    for s in (1.0, 2.0 ** -20, 2.0 ** 30):                              # 9 s^2 + 16 s^2 == 25 s^2 exactly: a member
        tie = np.array([[0.0, 0.0, 0.0], [3 * s, 4 * s, 0.0], [1.5 * s, 2 * s, s]])
        got, report = _compare(tie, None, 5 * s, 2, 3, ("tie", s))
        assert got["neighbors"].tolist() == [2, 2, 2] and report["fitted"] == 3
        got, report = _compare(tie, None, np.nextafter(5 * s, 0.0), 2, 3, ("one ulp less", s))
        assert got["neighbors"].tolist() == [1, 1, 2] and report["fitted"] == 1


@pytest.mark.parametrize("seed", range(4))
def test_random_clouds(seed):
    rng = np.random.default_rng(3000 + seed)
    n_points = 2000
    radius = (0.25, 0.3, 0.11, 1.7)[seed]
    if seed % 2:
        xyz = rng.integers(0, 48, (n_points, 3)).astype(np.float64) * (radius / 4)          # quantised: ties at the radius and at the lattice abound
    else:
        xyz = rng.random((n_points, 3)) * [12 * radius, 12 * radius, 0.5 * radius]
    normal = rng.normal(size=(n_points, 3)).astype(np.float32)
    normal[rng.random(n_points) < 0.1] = 0.0
    _, report = _compare(xyz, normal if seed != 2 else None, radius, 2 + seed, 3, seed)
    assert report["points_in"] == n_points and report["fitted"] > 0 and report["fitted"] + report["unsupported"] == n_points


@functools.lru_cache(maxsize=None)
def _views():
    return scene.make_views(N, W, H, seed=1)


@functools.lru_cache(maxsize=None)
def _built():
    views = _views()
    model = ViewSetModel()
    model.add(views, None)
    arrays, _ = P.build_points(model.depth, views.K4, views.RT4, dedupe=False, **BUILD)
    for a in arrays.values():
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _fitted(radius, min_neighbors, flags):
    cloud = _built()
    return F.fit_planes(cloud["xyz"], cloud["normal"], radius, min_neighbors, flags)


def _new_set():
    s = capi.ViewSet(W, H)
    s.add(_views())
    s.build_points(dedupe=False, **BUILD)
    return s


def _download(s):
    arrays = s.download_points()
    arrays["plane_rms"] = s.download_point_plane_rms()
    return arrays


@pytest.mark.parametrize("knob", [1, 7, 64])
def test_the_view_set_cloud_equals_the_restatement_at_every_knob(knob):
    cloud = _built()
    want, want_report = _fitted(0.1, 5, 3)
    assert 0 < want_report["fitted"] < want_report["points_in"] == 1267
    with _new_set() as s:
        s.set_radius_group_points(knob)
        held, steps = s.info().device_bytes, s.info().steps
        report = s.fit_point_planes(0.1, 5)
        got = _download(s)
        _assert_bits(got, {k: want[k] for k in ("xyz", "normal", "plane_rms")}, knob)
        _assert_bits(got, {k: cloud[k] for k in ("view", "pixel", "count")}, knob)
        _assert_report(report, want_report, knob)
        assert list(s.plane_fit_pass_ms()) == ["bounds", "keys", "sort", "ranks", "permute", "fit"] and report["kernel_ms"] > 0
        assert s.info().steps == steps + 1 and s.info().device_bytes == held + 4 * 1267      # the scratch is gone, plane_rms is held
        neighbors, _, _ = capi.count_point_neighbors(cloud["xyz"], radius=0.1)
        free, _ = capi.fit_point_planes(cloud["xyz"], cloud["normal"], radius=0.1, min_neighbors=5)
        assert free["neighbors"].tobytes() == neighbors.tobytes() == want["neighbors"].tobytes()


def test_more_units_than_the_kernel_has_waves():
    """33 001 points at knob 1 are 33 001 units for the kernel's 32 768 waves: it strides.  One view of 541 x 61 pixels, all of them
    valid, built with min_views = 0: every pixel is a point.  The restatement starts from the downloaded cloud."""
    views = scene.make_views(1, 541, 61, seed=2, dense=True)
    with capi.ViewSet(541, 61) as s:
        s.add(views)
        assert s.build_points(dedupe=False, abs_tolerance=0.0, rel_tolerance=0.02, min_views=0)["points"] == 33001
        cloud = s.download_points()
        radius = 2.5 * float(np.linalg.norm(cloud["xyz"][1] - cloud["xyz"][0]))
        want, want_report = F.fit_planes(cloud["xyz"], cloud["normal"], radius, 5, 3)
        assert want_report["fitted"] > 30000 and want_report["max_neighbors"] < 64
        s.set_radius_group_points(1)
        report = s.fit_point_planes(radius, 5)
        got = _download(s)
        _assert_bits(got, {k: want[k] for k in ("xyz", "normal", "plane_rms")}, "knob 1")
        _assert_bits(got, {k: cloud[k] for k in ("view", "pixel", "count")}, "knob 1")
        _assert_report(report, want_report, "knob 1")


def test_each_flag_alone_keeps_the_other_arrays_bits():
    cloud = _built()
    for flags in (1, 2):
        want, want_report = _fitted(0.1, 5, flags)
        got, report = capi.fit_point_planes(cloud["xyz"], cloud["normal"], radius=0.1, min_neighbors=5, move=bool(flags & 1), normals=bool(flags & 2))
        _assert_bits(got, want, flags)
        _assert_report(report, want_report, flags)
        kept = "normal" if flags == 1 else "xyz"
        assert got[kept].tobytes() == cloud[kept].tobytes() and (report["max_shift"] > 0) == (flags == 1)
        with _new_set() as s:
            s.fit_point_planes(0.1, 5, move=bool(flags & 1), normals=bool(flags & 2))
            _assert_bits(_download(s), {k: want[k] for k in ("xyz", "normal", "plane_rms")}, ("set", flags))


def test_the_life_of_the_fitted_cloud_and_the_refusals():
    cloud = _built()
    with capi.ViewSet(W, H) as s:
        s.add(_views())
        for call in (lambda: s.fit_point_planes(0.1), s.download_point_plane_rms, s.plane_fit_pass_ms):          # no cloud yet
            with pytest.raises(capi.DmiError) as e:
                call()
            assert e.value.code == 4
        s.build_points(dedupe=False, **BUILD)
        for call in (s.download_point_plane_rms, s.plane_fit_pass_ms):                                           # built, not fitted
            with pytest.raises(capi.DmiError) as e:
                call()
            assert e.value.code == 4
        held, steps = s.info().device_bytes, s.info().steps
        for args, word in (((float("nan"), 5), "radius"), ((0.0, 5), "radius"), ((1e-200, 5), "radius"), ((0.1, 1), "min_neighbors")):
            with pytest.raises(capi.DmiError) as e:
                s.fit_point_planes(*args)
            assert e.value.code == 1 and word in str(e.value) and "dmi_views_fit_point_planes" in str(e.value)
        with pytest.raises(capi.DmiError) as e:
            s.fit_point_planes(0.1, 5, move=False, normals=False)
        assert e.value.code == 1 and "flags" in str(e.value)
        again = s.download_points()
        assert all(again[k].tobytes() == cloud[k].tobytes() for k in INPUT_NAMES) and s.info().device_bytes == held and s.info().steps == steps
        # twice is a second pass over the first's result
        once, _ = _fitted(0.1, 5, 3)
        twice, twice_report = F.fit_planes(once["xyz"], once["normal"], 0.1, 5, 3)
        s.fit_point_planes(0.1, 5)
        report = s.fit_point_planes(0.1, 5)
        _assert_bits(_download(s), {k: twice[k] for k in ("xyz", "normal", "plane_rms")}, "twice")
        _assert_report(report, twice_report, "twice")
        assert s.info().device_bytes == held + 4 * 1267
        # a thinning after a fit equals the context-free thinning of the downloaded arrays, and drops plane_rms
        fitted = s.download_points()
        want, _ = capi.thin_point_cloud(*(fitted[name] for name in INPUT_NAMES), cell_size=0.1)
        s.thin_points(0.1)
        got = s.download_points()
        assert all(got[k].tobytes() == want[k].tobytes() for k in got)
        with pytest.raises(capi.DmiError) as e:
            s.download_point_plane_rms()
        assert e.value.code == 4
        # a fit of the thinned cloud keeps its layout and members
        members = s.download_point_members()
        held = s.info().device_bytes
        thin_fit, thin_report = F.fit_planes(got["xyz"], got["normal"], 0.25, 4, 3)
        report = s.fit_point_planes(0.25, 4)
        _assert_bits(_download(s), {k: thin_fit[k] for k in ("xyz", "normal", "plane_rms")}, "thinned")
        _assert_report(report, thin_report, "thinned")
        assert s.download_point_members().tobytes() == members.tobytes() and s.info().device_bytes == held + 4 * len(members)
        # the radius filter behind a fit drops plane_rms; a fit behind the filter keeps the filter's counts
        s.filter_points_radius(0.25, 2)
        with pytest.raises(capi.DmiError) as e:
            s.download_point_plane_rms()
        assert e.value.code == 4
        counts, before = s.download_point_neighbors(), s.download_points()
        want, want_report = F.fit_planes(before["xyz"], before["normal"], 0.25, 4, 2)
        report = s.fit_point_planes(0.25, 4, move=False)
        _assert_bits(_download(s), {k: want[k] for k in ("xyz", "normal", "plane_rms")}, "filtered")
        _assert_report(report, want_report, "filtered")
        assert s.download_point_neighbors().tobytes() == counts.tobytes() and len(s.radius_pass_ms()) == 7
        # whatever changes the depths, and a build, drop it
        s.build_points(dedupe=False, **BUILD)
        with pytest.raises(capi.DmiError) as e:
            s.download_point_plane_rms()
        assert e.value.code == 4
        s.fit_point_planes(0.1, 5)
        s.filter_consistency(min_views=0)
        for call in (s.download_point_plane_rms, s.plane_fit_pass_ms, lambda: s.fit_point_planes(0.1)):
            with pytest.raises(capi.DmiError) as e:
                call()
            assert e.value.code == 4
    for device in (-1, 10 ** 6):
        with pytest.raises(capi.DmiError) as e:
            capi.fit_point_planes(cloud["xyz"], radius=0.1, device=device)
        assert e.value.code == 1 and "device" in str(e.value)
    bad = cloud["xyz"].copy()
    bad[617, 1] = float("nan")
    with pytest.raises(capi.DmiError) as e:
        capi.fit_point_planes(bad, radius=0.1)
    assert e.value.code == 1 and "non-finite" in str(e.value)


def test_a_cloud_without_points_fits_to_none():
    views = _views()
    with capi.ViewSet(W, H) as s:
        s.add(scene.Views(np.full_like(views.depth, -1.0), views.K4, views.RT4, None))
        assert s.build_points(**BUILD)["points"] == 0
        report = s.fit_point_planes(0.1)
        assert report["points_in"] == 0 and report["fitted"] == 0 and len(s.download_point_plane_rms()) == 0
