"""The resident view set's test input (view_set_cases.py) is not vacuous: on the CPU, with the numpy restatements of the four
filters in the canonical order of the chain, every step does something and leaves something."""
import numpy as np

import depth_consistency_np
import depth_holes_np
import depth_smooth_np
import depth_speckle_np
from view_set_cases import BORDER_HOLE, CONSISTENCY, H, HOLES, ISLANDS, N, SMOOTH, SPECKLES, W, WRONG_PATCH, view_set_scene
from view_set_model import groups_of_sizes, normalised, step_report


def test_every_step_of_the_chain_has_work_and_leaves_work():
    views, threshold = view_set_scene()
    assert views.depth.shape == (N, H, W) and views.best_cost.shape == (N, H, W)
    d0 = normalised(views.depth, views.best_cost, threshold)
    assert 0 < (d0 == -1.0).sum() < d0.size // 4

    # speckles: at least one segment goes -- every island does -- and at least one stays
    d1, size = depth_speckle_np.filter_depth_speckles(d0, **SPECKLES)
    r = step_report("speckles", SPECKLES, d0, d1, size)
    assert r["groups"] > r["groups_kept"] >= 1 and r["changed"] == r["valid_before"] - r["valid_after"] > 0
    for m, y, x, half in ISLANDS:
        assert d0[m, y, x] > 0 and d1[m, y, x] == -1.0 and 0 < size[m, y, x] < SPECKLES["min_pixels"]
    m, rows, cols = WRONG_PATCH
    assert np.all(d1[m, rows, cols][d0[m, rows, cols] > 0] > 0), "the wrong patch is large enough to pass as a segment"

    # holes: at least one is filled, at least one is left: the one on the border
    d2, hole_size = depth_holes_np.fill_depth_holes(d1, **HOLES)
    r = step_report("holes", HOLES, d1, d2, hole_size)
    assert r["groups"] > r["groups_kept"] >= 1 and r["changed"] == r["valid_after"] - r["valid_before"] > 0
    m, rows, cols = BORDER_HOLE
    assert np.all(d2[m, rows, cols] == -1.0) and np.all(hole_size[m, rows, cols] >= 15)
    assert groups_of_sizes(hole_size) == depth_holes_np.hole_counts(d1, d2, hole_size)[0]

    # smoothing: some pixel moves, and to a depth that is no f32
    s = depth_smooth_np.spatial_weights(SMOOTH["sigma"], SMOOTH["truncate"])
    d3, taps = depth_smooth_np.smooth_depths(d2, s, SMOOTH["abs_tolerance"], SMOOTH["rel_tolerance"], SMOOTH["iterations"])
    r = step_report("smooth", SMOOTH, d2, d3, taps)
    assert r["changed"] > 0 and r["valid_before"] == r["valid_after"] and r["aux_sum"] > r["valid_after"]
    assert np.array_equal(d1, d1.astype(np.float32).astype(np.float64)), "before the fill every depth is an f32"
    assert not np.array_equal(d3, d3.astype(np.float32).astype(np.float64))

    # consistency: some valid pixel goes -- most of the wrong patch does -- and some stays
    d4, count = depth_consistency_np.filter_depth_consistency(d3, views.K4, views.RT4, **CONSISTENCY)
    r = step_report("consistency", CONSISTENCY, d3, d4, count)
    assert 0 < r["valid_after"] < r["valid_before"] and r["changed"] == r["valid_before"] - r["valid_after"]
    m, rows, cols = WRONG_PATCH
    inner = (slice(rows.start + 3, rows.stop - 3), slice(cols.start + 3, cols.stop - 3))
    assert np.all(d3[m][inner] > 0) and np.all(d4[m][inner] == -1.0)
