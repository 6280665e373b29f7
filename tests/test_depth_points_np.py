"""Hand cases of the point cloud's definition (include/dmi.h: dmi_views_build_points) whose answers are known without running
anything, put to the numpy restatement (depth_points_np.py) the GPU is compared with; test_depth_points.py puts the same cases to
the device.  Identity cameras throughout: K4 = RT4 = I, so that pixel (px, py) with depth d is the point (px*d, py*d, d), every
product is exact for the small integers and halves used, and two views with equal depths see each pixel in itself."""
import numpy as np

import depth_points_np as P
from cudadepthmapintegration_amd import scene

TOLERANCES = dict(abs_tolerance=0.01, rel_tolerance=0.0)


def identity_views(depth):
    """Views of depth [n, H, W] (vtk row order) under identity cameras."""
    depth = np.asarray(depth, dtype=np.float64)
    eye = np.tile(np.eye(4), (depth.shape[0], 1, 1))
    return scene.Views(depth, eye, eye.copy(), None)


def plane_views(n, h, w, d=2.0):
    """n identical views of the fronto-parallel plane z = d."""
    return identity_views(np.full((n, h, w), d))


def ridge_depth(h, w, column, d=2.0, height=0.5):
    """[h, w]: the plane z = d with one column `height` farther."""
    depth = np.full((h, w), d)
    depth[:, column] = d + height
    return depth


def _points(views, **params):
    return P.build_points(views.depth, views.K4, views.RT4, **{**TOLERANCES, **params})


def test_fronto_parallel_plane_has_the_normal_towards_the_camera_everywhere():
    arrays, report = _points(plane_views(1, 9, 7), min_views=0)
    assert report["valid"] == report["candidates"] == report["points"] == report["with_normal"] == 63 and report["owned"] == 0
    assert arrays["normal"].dtype == np.float32 and np.all(arrays["normal"] == np.float32([0, 0, -1]))   # (-0.0 where m was negated)
    # corners and edges took one-sided tangents: everything but the 7 x 5 interior
    assert report["one_sided"] == 63 - 35
    # the positions are the pixels scaled by the depth
    px, py = arrays["pixel"] % 7, arrays["pixel"] // 7
    assert np.array_equal(arrays["xyz"], np.stack([px * 2.0, py * 2.0, np.full(63, 2.0)], axis=1))
    assert np.all(arrays["count"] == 0) and np.all(arrays["view"] == 0)


def test_depth_step_gives_one_sided_tangents_and_no_normal_on_a_ridge():
    arrays, report = _points(identity_views(ridge_depth(8, 11, column=5)[None]), min_views=0)
    on_ridge = arrays["pixel"] % 11 == 5
    assert report["points"] == 88 and on_ridge.sum() == 8
    assert np.all(arrays["normal"][on_ridge] == 0.0)                 # neither neighbour along x is usable
    assert np.all(arrays["normal"][~on_ridge] == np.float32([0, 0, -1]))   # its neighbours turn to their other side
    assert report["with_normal"] == 80
    # a step below the tolerance is no edge: every pixel has a normal, and beside the step it is tilted
    arrays, report = _points(identity_views(ridge_depth(8, 11, column=5, height=0.005)[None]), min_views=0)
    assert report["with_normal"] == 88 and np.any(arrays["normal"][:, 0] != 0.0)


def test_single_row_or_column_has_points_without_normals():
    for h, w in ((1, 6), (6, 1), (1, 1)):
        arrays, report = _points(plane_views(2, h, w), min_views=0, dedupe=False)
        assert report["points"] == 2 * h * w and report["with_normal"] == 0 and np.all(arrays["normal"] == 0.0)


def test_identical_views_keep_the_surface_in_the_lowest_view():
    twins = plane_views(2, 20, 37)
    arrays, report = _points(twins, min_views=1, dedupe=True)
    assert report["candidates"] == 2 * 740 and report["owned"] == 740 and report["points"] == 740
    assert np.all(arrays["view"] == 0) and np.all(arrays["count"] == 1) and np.array_equal(arrays["pixel"], np.arange(740))
    arrays, report = _points(twins, min_views=1, dedupe=False)
    assert report["owned"] == 0 and report["points"] == 2 * 740 and (arrays["view"] == 1).sum() == 740
    # three views: the third is owned by the first already, the count sees both others
    arrays, report = _points(plane_views(3, 4, 5), min_views=2, dedupe=True)
    assert report["owned"] == 40 and np.all(arrays["view"] == 0) and np.all(arrays["count"] == 2)
    # an owner must be a candidate itself: with depths that disagree nobody owns anything
    apart = identity_views(np.stack([np.full((4, 5), 2.0), np.full((4, 5), 3.0)]))
    arrays, report = _points(apart, min_views=0, dedupe=True)
    assert report["owned"] == 0 and report["points"] == 40


def test_ownership_needs_the_owner_to_take_part():
    """min_views = 1 with three views of which the lowest disagrees: view 0 has no agreeing view and is no candidate, so it owns
    nothing; view 1 keeps the surface and owns view 2's."""
    views = identity_views(np.stack([np.full((4, 5), 3.0), np.full((4, 5), 2.0), np.full((4, 5), 2.0)]))
    arrays, report = _points(views, min_views=1, dedupe=True)
    assert report["candidates"] == 40 and report["owned"] == 20 and np.all(arrays["view"] == 1)


def test_pixel_step_beyond_the_image_leaves_the_first_pixel():
    arrays, report = _points(plane_views(2, 20, 37), min_views=0, pixel_step=38, dedupe=False)
    assert arrays["view"].tolist() == [0, 1] and arrays["pixel"].tolist() == [0, 0] and report["candidates"] == 2
    # pixel (0, 0) is the image's top left: the LAST vtk row's first value
    depth = np.full((1, 3, 4), 2.0)
    depth[0, 2, 0] = 5.0
    arrays, _ = _points(identity_views(depth), min_views=0, pixel_step=100)
    assert arrays["xyz"].tolist() == [[0.0, 0.0, 5.0]]


def test_output_order_is_view_then_row_then_column():
    rng = np.random.default_rng(5)
    depth = np.where(rng.random((3, 6, 7)) < 0.6, 2.0, -1.0)
    arrays, report = _points(identity_views(depth), min_views=0, dedupe=False)
    keys = arrays["view"].astype(np.int64) * 42 + arrays["pixel"]
    assert report["points"] == int((depth > 0).sum()) and np.all(np.diff(keys) > 0)
    # pixel = py * W + px in image coordinates: vtk row H-1-py
    for v, p in zip(arrays["view"], arrays["pixel"]):
        assert depth[v, 5 - p // 7, p % 7] == 2.0
    # with a step, the pixels are those whose image coordinates are multiples of it
    arrays, _ = _points(identity_views(np.full((1, 6, 7), 2.0)), min_views=0, pixel_step=3)
    assert arrays["pixel"].tolist() == [0, 3, 6, 21, 24, 27]


def test_values_that_are_no_depths_are_never_emitted_nor_usable():
    depth = np.full((1, 6, 8), 2.0)
    depth[0, 2, 3], depth[0, 2, 5], depth[0, 3, 2], depth[0, 0, 0] = np.nan, 0.0, -2.0, np.inf
    arrays, report = _points(identity_views(depth), min_views=0)
    assert report["valid"] == report["points"] == 44 and np.isfinite(arrays["xyz"]).all()
    emitted = set(arrays["pixel"].tolist())
    for row, col in ((2, 3), (2, 5), (3, 2), (0, 0)):
        assert (5 - row) * 8 + col not in emitted
    # (2, 4) stands between two of them along x: no tangent there, no normal; every other point has (0, 0, -1)
    between = arrays["pixel"] == (5 - 2) * 8 + 4
    assert between.sum() == 1 and np.all(arrays["normal"][between] == 0.0)
    assert np.all(arrays["normal"][~between] == np.float32([0, 0, -1])) and report["with_normal"] == 43
    # nothing valid at all
    arrays, report = _points(identity_views(np.full((3, 5, 9), -1.0)), min_views=0)
    assert report["points"] == report["valid"] == 0 and arrays["xyz"].shape == (0, 3) and arrays["normal"].dtype == np.float32


def test_view_set_scene_gives_the_expected_counts():
    """The table of DESIGN.md 8n on the resident view set's test input, right after the add."""
    from view_set_cases import CONSISTENCY, view_set_scene
    views, threshold = view_set_scene()
    expected = {(0, 1): (50950, 44965), (0, 2): (12717, 12321), (1, 1): (11567, 5722), (1, 2): (2899, 2512), (2, 1): (944, 388),
                (2, 2): (235, 191)}
    for (min_views, pixel_step), (candidates, emitted) in expected.items():
        _, report = P.build_points(views.depth, views.K4, views.RT4, CONSISTENCY["abs_tolerance"], CONSISTENCY["rel_tolerance"], 0.03, 0.0,
                                   min_views, pixel_step, True, views.best_cost, threshold)
        assert (report["valid"], report["candidates"], report["points"]) == (50950, candidates, emitted)
        assert report["owned"] == candidates - emitted
