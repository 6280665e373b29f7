"""The fused point cloud of the resident view set on the GPU (dmi_views_build_points / dmi_views_download_points)
against its numpy restatement (depth_points_np.py), byte for byte: on the set right after the add, after the canonical chain, in
pieces, the hand cases of test_depth_points_np.py, the life of the points, and the refusals.  One small input (view_set_cases.py);
every case is milliseconds of kernels."""
import functools

import numpy as np
import pytest

import depth_points_np as P
from test_depth_points_np import identity_views, plane_views, ridge_depth
from view_set_cases import BOUNDS, CHAIN, CONSISTENCY, H, N, W, view_set_scene
from view_set_model import ViewSetModel
from cudadepthmapintegration_amd import capi, scene

pytestmark = pytest.mark.gpu
PLANE_BYTES = W * H * 8
AGREEMENT = dict(abs_tolerance=CONSISTENCY["abs_tolerance"], rel_tolerance=CONSISTENCY["rel_tolerance"])
NORMALS = dict(normal_abs_tolerance=0.03, normal_rel_tolerance=0.0)
STEP_METHODS = {"speckles": "filter_speckles", "holes": "fill_holes", "smooth": "smooth", "consistency": "filter_consistency"}
COUNT_NAMES = ("valid", "candidates", "owned", "points", "with_normal")
# DESIGN.md 8n's table, from a numpy reading of the definition: (min_views, pixel_step) -> (candidates, emitted with dedupe)
EXPECTED = {(0, 1): (50950, 44965), (0, 2): (12717, 12321), (1, 1): (11567, 5722), (1, 2): (2899, 2512), (2, 1): (944, 388),
            (2, 2): (235, 191)}
CASES = [(m, k, d) for m in (0, 1, 2) for k in (1, 2) for d in (0, 1)]


def _new_set(piece_bytes=None):
    views, threshold = view_set_scene()
    s = capi.ViewSet(W, H)
    if piece_bytes is not None:
        s.set_piece_bytes(piece_bytes)
    s.add(views, threshold)
    return s


@functools.lru_cache(maxsize=None)
def _start_depth():
    views, threshold = view_set_scene()
    model = ViewSetModel()
    model.add(views, threshold)
    model.depth.setflags(write=False)
    return model.depth


@functools.lru_cache(maxsize=None)
def _chain_depth():
    views, threshold = view_set_scene()
    model = ViewSetModel()
    model.add(views, threshold)
    for name, params in CHAIN:
        model.step(name, params)
    model.depth.setflags(write=False)
    return model.depth


@functools.lru_cache(maxsize=None)
def _reference(which, min_views, pixel_step, dedupe, normals=True):
    views, _ = view_set_scene()
    depth = _start_depth() if which == "start" else _chain_depth()
    arrays, report = P.build_points(depth, views.K4, views.RT4, min_views=min_views, pixel_step=pixel_step, dedupe=bool(dedupe),
                                    **AGREEMENT, **(NORMALS if normals else {}))
    for a in arrays.values():
        a.setflags(write=False)
    return arrays, report


def _assert_equal(got, report, want, want_report, label=None):
    for name in ("xyz", "normal", "view", "pixel", "count"):
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (label, name)
        assert got[name].tobytes() == want[name].tobytes(), (label, name)
    assert {k: int(report[k]) for k in COUNT_NAMES} == {k: want_report[k] for k in COUNT_NAMES}, label


def _build_and_compare(s, which, min_views, pixel_step, dedupe, normals=True):
    want, want_report = _reference(which, min_views, pixel_step, dedupe, normals)
    report = s.build_points(min_views=min_views, pixel_step=pixel_step, dedupe=bool(dedupe), **AGREEMENT, **(NORMALS if normals else {}))
    _assert_equal(s.download_points(), report, want, want_report, (which, min_views, pixel_step, dedupe))
    return report


@pytest.mark.parametrize("min_views,pixel_step,dedupe", CASES)
def test_points_equal_the_restatement_after_the_add(min_views, pixel_step, dedupe):
    _, want_report = _reference("start", min_views, pixel_step, dedupe)
    candidates, emitted = EXPECTED[(min_views, pixel_step)]
    assert want_report["valid"] == 50950 and want_report["candidates"] == candidates
    assert want_report["points"] == (emitted if dedupe else candidates)
    with _new_set() as s:
        before = s.download()
        report = _build_and_compare(s, "start", min_views, pixel_step, dedupe)
        assert report["kernel_ms"] > 0
        assert s.download().tobytes() == before.tobytes()   # D is not changed
        assert set(np.unique(s.download_points()["view"]).tolist()) == set(range(N))   # every view keeps at least one point
        info = s.info()
        assert info.steps == 1 and info.device_bytes >= 2 * N * PLANE_BYTES + 48 * report["points"]


def test_the_comparison_is_not_vacuous():
    want, want_report = _reference("start", 1, 1, 1)
    assert want_report["owned"] > 0 and 0 < want_report["with_normal"] < want_report["points"] and want_report["one_sided"] > 0
    assert np.any(want["count"] > 1) and np.any(np.all(want["normal"] == 0.0, axis=1))
    # the whole views with the normal tolerances of the comparison: most pixels have a normal, some by a one-sided tangent
    _, everything = _reference("start", 0, 1, 0)
    assert (everything["with_normal"], everything["one_sided"]) == (48585, 8681) and everything["points"] - 48585 == 2365


def test_normal_tolerances_default_to_the_agreement_pair():
    with _new_set() as s:
        _build_and_compare(s, "start", 1, 1, 1, normals=False)


@pytest.mark.parametrize("dedupe", [0, 1])
def test_points_equal_the_restatement_after_the_chain(dedupe):
    with _new_set() as s:
        for name, params in CHAIN:
            getattr(s, STEP_METHODS[name])(**params)
        assert s.download().tobytes() == _chain_depth().tobytes()
        report = _build_and_compare(s, "chain", 1, 1, dedupe)
        assert report["points"] > 0 and s.info().steps == len(CHAIN) + 1


@pytest.mark.parametrize("views_per_piece", [2, 1])
def test_pieces_do_not_change_a_byte(views_per_piece):
    with _new_set(piece_bytes=views_per_piece * PLANE_BYTES) as s:
        _build_and_compare(s, "start", 1, 1, 1)
        _build_and_compare(s, "start", 0, 2, 0)   # a second build replaces the first


def test_download_in_ranges_and_the_life_of_the_points():
    views, threshold = view_set_scene()
    want, want_report = _reference("start", 1, 1, 1)
    total = want_report["points"]
    with _new_set() as s:
        with pytest.raises(capi.DmiError) as e:   # no build yet
            s.download_points(0, 0)
        assert e.value.code == 4
        report = s.build_points(min_views=1, **AGREEMENT, **NORMALS)
        whole = s.download_points()
        _assert_equal(whole, report, want, want_report)
        cut = total // 3
        first, second = s.download_points(0, cut), s.download_points(cut, total - cut)
        for name in whole:
            assert np.concatenate([first[name], second[name]]).tobytes() == whole[name].tobytes(), name
        assert s.download_points(total, 0)["view"].size == 0
        # (the last: a sum that wraps around 64 bits is refused like any other range beyond the points)
        for lo, count in ((0, total + 1), (total + 1, 0), (total, 1), (2 ** 64 - 1, 2)):
            with pytest.raises(capi.DmiError) as e:
                s.download_points(lo, count)
            assert e.value.code == 1 and "first + count" in str(e.value)
        # the bounds estimate and a download of D keep the points
        s.estimate_bounds(**BOUNDS)
        s.download(1, 2)
        _assert_equal(s.download_points(), report, want, want_report)
        # a step, an add and a clear drop them
        held = s.info().device_bytes
        s.filter_consistency(min_views=0)
        assert s.info().device_bytes <= held - 48 * total
        for change in (None, lambda: s.add(scene.Views(views.depth[:1], views.K4[:1], views.RT4[:1], None)), s.clear):
            if change is not None:
                s.build_points(min_views=0, pixel_step=4, **AGREEMENT)
                assert s.download_points()["view"].size > 0
                change()
            with pytest.raises(capi.DmiError) as e:
                s.download_points(0, 0)
            assert e.value.code == 4 and "build_points" in str(e.value)
            with pytest.raises(capi.DmiError) as e:
                s.points_pass_ms()
            assert e.value.code == 4


def _device_points(views, **params):
    n, h, w = views.depth.shape
    with capi.ViewSet(w, h) as s:
        s.add(views)
        report = s.build_points(**params)
        return s.download_points(), report


def _compare_hand_case(views, **params):
    want, want_report = P.build_points(views.depth, views.K4, views.RT4, **params)
    got, report = _device_points(views, **params)
    _assert_equal(got, report, want, want_report)
    return got, report


def test_hand_cases_on_the_device():
    tolerances = dict(abs_tolerance=0.01, rel_tolerance=0.0)
    # a fronto-parallel plane under an identity camera: (0, 0, -1) exactly in every pixel, corners included
    got, report = _compare_hand_case(plane_views(1, 9, 7), min_views=0, **tolerances)
    assert report["points"] == report["with_normal"] == 63
    assert np.all(got["normal"] == np.float32([0.0, 0.0, -1.0]))
    # a ridge one pixel wide, higher than the normal tolerance: no normal on it, one-sided tangents beside it
    ridge = identity_views(ridge_depth(8, 11, column=5)[None])
    got, report = _compare_hand_case(ridge, min_views=0, **tolerances)
    on_ridge = got["pixel"] % 11 == 5
    assert np.all(got["normal"][on_ridge] == 0.0) and np.all(got["normal"][~on_ridge, 2] == -1.0) and report["with_normal"] == 80
    # W == 1 and H == 1: points without normals
    for h, w in ((1, 6), (6, 1), (1, 1)):
        got, report = _compare_hand_case(plane_views(2, h, w), min_views=0, dedupe=False, **tolerances)
        assert report["points"] == 2 * h * w and report["with_normal"] == 0
    # two identical views: the lower keeps every point with dedupe, both keep all without
    twins = plane_views(2, 20, 37)
    got, report = _compare_hand_case(twins, min_views=1, dedupe=True, **tolerances)
    assert report["owned"] == report["points"] == 20 * 37 and np.all(got["view"] == 0) and np.all(got["count"] == 1)
    got, report = _compare_hand_case(twins, min_views=1, dedupe=False, **tolerances)
    assert report["points"] == 2 * 20 * 37 and report["owned"] == 0
    # a step beyond the image leaves pixel (0, 0) of each view
    got, report = _compare_hand_case(twins, min_views=0, pixel_step=38, dedupe=False, **tolerances)
    assert got["pixel"].tolist() == [0, 0] and got["view"].tolist() == [0, 1]
    # depths that are no depths are never emitted and never usable neighbours
    odd = np.array(plane_views(1, 6, 8).depth)
    odd[0, 2, 3], odd[0, 2, 5], odd[0, 3, 2], odd[0, 0, 0] = np.nan, 0.0, -2.0, np.inf
    got, report = _compare_hand_case(identity_views(odd), min_views=0, **tolerances)
    assert report["valid"] == report["points"] == 44 and np.isfinite(got["xyz"]).all()
    # nothing valid at all: zero points, and a download of none
    nothing = identity_views(np.full((3, 5, 9), -1.0))
    got, report = _compare_hand_case(nothing, min_views=0, **tolerances)
    assert {k: int(report[k]) for k in COUNT_NAMES} == dict.fromkeys(COUNT_NAMES, 0) and got["xyz"].shape == (0, 3)


def test_refusals_name_the_argument_and_change_nothing():
    views, _ = view_set_scene()
    nan, inf = float("nan"), float("inf")
    ok = dict(abs_tolerance=0.02, rel_tolerance=0.01)
    illegal = [
        (dict(ok, abs_tolerance=-1.0), "abs_tolerance"), (dict(ok, abs_tolerance=nan), "abs_tolerance"),
        (dict(ok, rel_tolerance=inf), "rel_tolerance"), (dict(ok, normal_abs_tolerance=-0.5), "normal_abs_tolerance"),
        (dict(ok, normal_rel_tolerance=nan), "normal_rel_tolerance"), (dict(ok, min_views=-1), "min_views"),
        (dict(ok, pixel_step=0), "pixel_step"), (dict(ok, dedupe=2), "dedupe"), (dict(ok, dedupe=-1), "dedupe"),
    ]
    with _new_set() as s:
        before = s.download()
        report = s.build_points(**ok)
        points = s.download_points()
        for params, name in illegal:
            with pytest.raises(capi.DmiError) as e:
                s.build_points(**params)
            assert e.value.code == 1 and name in str(e.value) and "dmi_views_build_points" in str(e.value), params
        assert s._lib.dmi_views_build_points(s._h, 0.02, 0.01, 0.02, 0.01, 1, 1, 1, None, None) == 1
        assert "n_points" in s._lib.dmi_views_last_error(s._h).decode()
        # the set, its depths and the points of the earlier build are as they were
        info = s.info()
        assert s.download().tobytes() == before.tobytes() and (info.n, info.steps) == (N, 1)
        again = s.download_points()
        assert all(again[k].tobytes() == points[k].tobytes() for k in points) and again["view"].size == report["points"]
    with capi.ViewSet(W, H) as empty:
        with pytest.raises(capi.DmiError) as e:
            empty.build_points(**ok)
        assert e.value.code == 1 and "holds no views" in str(e.value)
    bad_k = np.array(views.K4)
    bad_k[3, 1, 0] = 0.25
    with capi.ViewSet(W, H) as odd:
        odd.add(scene.Views(views.depth, bad_k, views.RT4, None))
        with pytest.raises(capi.DmiError) as e:
            odd.build_points(**ok)
        assert e.value.code == 1 and "view 3" in str(e.value)
