"""The scenes of tests/potential_tie_cases.py are what they claim -- proven on the CPU with the oracle alone, so that the GPU
tests (tests/test_gpu_potential_ties.py) compare the library with grids in which every strict compare of the reference's ray
potential (cu:105-120) is at its tie, and in which a `>=` for a `>` is visible."""
import numpy as np
import pytest

import potential_tie_cases as tc
from helpers import bits_equal

MAIN = tc.PARAM_SETS["main"]
SCENES = [(f, g) for g in tc.GRIDS for f in tc.FAMILIES]


def _ties(rp):
    """diff values, in layers, at which the parameter set has a tie."""
    t, d = round(rp.thickness / tc.S), round(rp.delta / tc.S)
    assert t * tc.S == rp.thickness and d * tc.S == rp.delta
    return sorted({0, t, -t, d, -d} if t <= d else {0, d, -d})   # a thickness beyond delta is never compared at its own value


def test_rho_and_thickness_separate_the_ramp_from_the_plateau():
    """At |diff| == thick the reference takes the linear branch: fl(rho / thick) thick must not be rho, or `>=` would pass."""
    ramp = (MAIN.rho / MAIN.thickness) * MAIN.thickness
    assert ramp == 0.8999999999999999 and ramp != MAIN.rho
    for rho, thick in ((0.8, 3 * tc.S), (-0.5, 3 * tc.S), (1.0, 3 * tc.S)):   # pairs that would NOT do
        assert (rho / thick) * thick == rho


def test_one_views_column_has_a_value_of_its_own_at_every_tie():
    grid, views = tc.tie_scene("+k", "identity")
    m = tc.view_layers().index(20)
    col = tc.numpy_grid(grid, MAIN, views, m, 1)[0][:, 3, 5]
    assert list(col[13:28]) == [-0.027, -0.027, -0.9, -0.9, -0.8999999999999999, -0.6, -0.3, 0.0, 0.3, 0.6,
                                0.8999999999999999, 0.9, 0.9, 0.0, 0.0]
    assert -0.03 * 0.9 == -0.027


@pytest.mark.parametrize("family,grid_kind", SCENES)
def test_cz_is_the_intended_dyadic_value_and_every_voxel_is_fused(family, grid_kind):
    for kind in ("plain", "general_k"):
        grid, views = tc.tie_scene(family, grid_kind, kind)
        cz, px, py, ok = tc.project(grid, views.subset(0, 1))
        want = np.array([tc.cz_of_layer(family, L) for L in range(tc.NA)])
        assert np.array_equal(tc.layers_first(grid, family, cz[0]), np.broadcast_to(want[:, None, None], (tc.NA, tc.NC, tc.NC)))
        assert want.min() == 6.03125 and want.max() == 9.96875
        assert ok.all()                                             # the whole grid projects inside the image: all reach cu:211
        assert abs(px - tc.PC[0]).max() <= 16 and abs(py - tc.PC[1]).max() <= 16
        # ... and the depth of view m IS c.z of its layer L0: diff = s (L - L0) / 16 exactly
        for m, L0 in enumerate(tc.view_layers()):
            assert np.all(views.depth[m] == tc.cz_of_layer(family, L0))


@pytest.mark.parametrize("param_set", list(tc.PARAM_SETS))
def test_every_tie_lies_on_whole_layers_at_every_alignment(param_set):
    """diff == tie on a full layer, for every tie of the set and every layer of the grid (so: first and last layer of an
    8-brick, a 16-brick, a 32-box and the grid) -- and just outside the grid, where the tie layer itself is missing."""
    rp = tc.PARAM_SETS[param_set]
    for family in tc.FAMILIES:
        grid, views = tc.tie_scene(family, "identity")
        cz = tc.layers_first(grid, family, tc.project(grid, views.subset(0, 1))[0][0])
        s = tc.sign_of(family)
        for t in _ties(rp):
            seen = set()
            for m, L0 in enumerate(tc.view_layers()):
                L = L0 + int(s) * t
                if 0 <= L < tc.NA:
                    assert np.all(cz[L] - views.depth[m][0, 0] == t * tc.S)
                    seen.add(L)
            assert seen == set(range(tc.NA)), (family, t)
            # views whose tie layer is the first one outside the grid, on either side
            assert {L0 + int(s) * t for L0 in tc.view_layers()} >= {-1, tc.NA}


@pytest.mark.parametrize("tk", [8, 16, 32])
def test_delta_ties_on_the_outer_layers_of_bricks_and_boxes(tk):
    """-delta on the LAST layer of a brick / box as seen from the camera (fl(czmax - dmin) < -delta must not hold), +delta on the
    FIRST one (fl(czmin - dmax) > delta must not hold) -- at boundaries of tk-layer bricks that are no boundaries of larger ones
    where there are such."""
    d = round(MAIN.delta / tc.S)
    for family in tc.FAMILIES:
        s = int(tc.sign_of(family))
        last, first = set(), set()
        for L0 in tc.view_layers():
            for t, hits in ((-d, last), (d, first)):
                L = L0 + s * t
                if 0 <= L < tc.NA:
                    p = L if s > 0 else tc.NA - 1 - L           # position as seen from the camera
                    if (t < 0 and p % tk == tk - 1) or (t > 0 and p % tk == 0):
                        hits.add(p)
        assert last == set(range(tk - 1, tc.NA, tk)) and first == set(range(0, tc.NA, tk)), (family, last, first)


def _tie_layers(family, rp, which):
    """{(group, layer)}: the layers on which a view of the group has diff == +-thick (which = "thick") or +-delta."""
    s = int(tc.sign_of(family))
    t = round((rp.thickness if which == "thick" else rp.delta) / tc.S)
    per = len(tc.view_layers()) // tc.GROUP_STRIDE
    out = set()
    for m, L0 in enumerate(tc.view_layers()):
        out |= {(m // per, L0 + s * sg * t) for sg in (-1, 1) if 0 <= L0 + s * sg * t < tc.NA}
    return out


@pytest.mark.parametrize("family,grid_kind", SCENES)
def test_mutated_thresholds_are_seen_on_every_tie_layer(family, grid_kind):
    """The difference between `>` and `>=`, oracle only: with delta (thick) one ulp smaller the grids of the view groups differ
    from the expectation on every view's tie layers, on all of each layer; with both one ulp larger nothing changes.  The sum
    of all 76 views is NOT that sensitive (asserted too: it is why the GPU tests also fuse by groups)."""
    grid, views = tc.tie_scene(family, grid_kind)
    want = tc.expected(family, grid_kind, "plain", "main")
    for which in ("thick", "delta"):
        rp = tc.scene.RayPotential(MAIN.thickness, MAIN.rho, MAIN.eta, MAIN.delta)
        if which == "thick":
            rp.thickness = float(np.nextafter(MAIN.thickness, 0.0))
        else:
            rp.delta = float(np.nextafter(MAIN.delta, 0.0))
        for g, (first, count) in enumerate(tc.groups()):
            got = tc.layers_first(grid, family, tc.oracle_grid(grid, rp, views, first, count, count_hits=False)[0])
            differs = tc.layers_first(grid, family, want["groups"][g]).view(np.uint64) != got.view(np.uint64)
            for (gg, L) in _tie_layers(family, MAIN, which):
                if gg == g:
                    assert differs[L].all(), (which, g, L)
    up = tc.scene.RayPotential(float(np.nextafter(MAIN.thickness, np.inf)), MAIN.rho, MAIN.eta, float(np.nextafter(MAIN.delta, np.inf)))
    # (rho / thick changes with thick: the ramp's own layers may move by an ulp; the tie layers, where `>` decides, must not)
    assert up.rho / up.thickness == MAIN.rho / MAIN.thickness
    for g, (first, count) in enumerate(tc.groups()):
        assert bits_equal(tc.oracle_grid(grid, up, views, first, count, count_hits=False)[0], want["groups"][g])
    assert bits_equal(tc.oracle_grid(grid, up, views)[0], want["all"][0])


def test_the_sum_of_all_views_hides_a_one_ulp_error_that_the_groups_show():
    grid, views = tc.tie_scene("+k", "identity")
    rp = tc.scene.RayPotential(float(np.nextafter(MAIN.thickness, 0.0)), MAIN.rho, MAIN.eta, MAIN.delta)
    want = tc.expected("+k", "identity", "plain", "main")
    differs = tc.oracle_grid(grid, rp, views)[0].view(np.uint64) != want["all"][0].view(np.uint64)
    assert not differs.all(axis=(1, 2)).all()      # some layer's sum is the same with the mutated thickness


@pytest.mark.parametrize("kind", tc.KINDS)
@pytest.mark.parametrize("grid_kind", tc.GRIDS)
def test_c_and_numpy_oracles_agree_on_every_tie_scene(grid_kind, kind):
    for family in tc.FAMILIES:
        grid, views = tc.tie_scene(family, grid_kind, kind)
        for name in (tc.PARAM_SETS if kind in ("plain", "holes") else ("main", "thick_zero")):
            rp = tc.PARAM_SETS[name]
            init = tc.init_grid(grid.n_voxels) if name == "main" else None
            a, b = tc.oracle_grid(grid, rp, views, init=init), tc.numpy_grid(grid, rp, views, init=init)
            assert bits_equal(a[0], b[0]), (family, name)
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (family, name)
            if name == "thick_zero" and kind == "plain":
                # diff == 0 with thick == 0 is the reference's NaN (cu:119): the sum of all views holds nothing else, a
                # group's grid has it on its views' own layers only
                assert np.isnan(a[0]).all()
                for g, (first, count) in enumerate(tc.groups()):
                    nan = np.isnan(tc.layers_first(grid, family, tc.expected(family, grid_kind, kind, name)["groups"][g]))
                    own = [L0 for L0 in tc.view_layers()[first:first + count] if 0 <= L0 < tc.NA]
                    assert nan[own].all() and not np.delete(nan, own, axis=0).any()


@pytest.mark.parametrize("grid_kind", tc.GRIDS)
def test_variants_keep_the_ties_and_add_what_they_are_for(grid_kind):
    for family in tc.FAMILIES:
        grid, plain = tc.tie_scene(family, grid_kind)
        n_vox = grid.n_voxels
        # split: both halves of the image are used by voxels of every layer
        _, split = tc.tie_scene(family, grid_kind, "split")
        _, px, _, ok = tc.project(grid, split.subset(0, 1))
        left = tc.layers_first(grid, family, px[0] < tc.SPLIT_X)
        assert ok.all() and left.any(axis=(1, 2)).all() and (~left).any(axis=(1, 2)).all()
        assert tc.SPLIT_X % 8 != 0
        # holes: about a tenth of the voxels of every view return at cu:202, on every layer
        _, holes = tc.tie_scene(family, grid_kind, "holes")
        mh = tc.oracle_grid(grid, MAIN, holes)[2]
        assert np.all((mh > 0.8 * n_vox) & (mh < 0.97 * n_vox)), mh
        # general K: the same pixels as the plain scene
        _, gk = tc.tie_scene(family, grid_kind, "general_k")
        assert gk.K4[0, 2, 2] == 2.0
        a, b = tc.project(grid, plain.subset(0, 1)), tc.project(grid, gk.subset(0, 1))
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        # border: part of the grid inside the image, part up to 32 pixels outside / part further out than that
        for kind, (lo, hi) in (("border_in_margin", (-32, -8)), ("border_beyond_margin", (tc.H + 32, tc.H + 64))):
            _, v = tc.tie_scene(family, grid_kind, kind)
            cz, px, py, ok = tc.project(grid, v.subset(0, 1))
            assert 0.2 * n_vox < np.count_nonzero(ok) < 0.9 * n_vox, (kind, np.count_nonzero(ok))
            u, vv = tc.image_coordinates(grid, v)
            far = u.min() if kind == "border_in_margin" else vv.max()
            assert lo <= far <= hi, (kind, far)


# ---- outward rounding ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,grid_kind", SCENES)
def test_outward_rounding_scenes_satisfy_their_inequalities(family, grid_kind):
    grid, views, sides, layers, Fs, e1s = tc.rounding_scene(family, grid_kind)
    delta = MAIN.delta
    assert tc.ROUNDING_OFFSETS[0] == 2.0 ** -46
    cz, _, _, ok = tc.project(grid, views)
    assert ok.all()
    near = tc.narrowed(views)
    for m, (side, L) in enumerate(zip(sides, layers)):
        e1 = e1s[m]
        z = tc.layers_first(grid, family, cz[m])[L]
        d = views.depth[m][0, 0]
        assert np.all(z == z[0, 0]) and np.all(views.depth[m] == d)
        z = float(z[0, 0])
        assert float(np.float32(Fs[m])) == Fs[m] and float(np.float32(d)) != d and np.all(near.depth[m] == Fs[m])
        if side == "free":
            assert z - d == -delta + e1 and z - d > -delta          # not free: the reference gives -rho
            assert z - Fs[m] == -delta - e1 and z - Fs[m] < -delta        # free with the depth rounded to nearest
            assert d < Fs[m]
        else:
            assert z - d == delta - e1 and z - d < delta            # not behind: the reference gives +rho
            assert z - Fs[m] == delta + e1 and z - Fs[m] > delta          # behind with the depth rounded to nearest
            assert d > Fs[m]
    # the aimed-at layers are the outer layers of 8-bricks, 16-bricks, 32-boxes and the grid as the camera sees them
    pos = [L if tc.sign_of(family) > 0 else tc.NA - 1 - L for L in layers]
    for e1 in tc.ROUNDING_OFFSETS:
        assert sorted(p for p, sd, e in zip(pos, sides, e1s) if sd == "free" and e == e1) == [7, 15, 31, 63]
        assert sorted(p for p, sd, e in zip(pos, sides, e1s) if sd == "behind" and e == e1) == [0, 8, 16, 32]
    # the two expectations, view by view: they differ in the aimed-at layer, and nowhere else among the layers of a constant
    # value (the ramp's layers, |diff| <= thick, follow the depth's 2^-45; the view's other delta tie is decided the other way)
    s = int(tc.sign_of(family))
    for m, (side, L) in enumerate(zip(sides, layers)):
        a = tc.layers_first(grid, family, tc.oracle_grid(grid, MAIN, views, m, 1)[0])
        b = tc.layers_first(grid, family, tc.oracle_grid(grid, MAIN, near, m, 1)[0])
        assert bits_equal(a, tc.layers_first(grid, family, tc.numpy_grid(grid, MAIN, views, m, 1)[0]))
        differs = (a.view(np.uint64) != b.view(np.uint64))
        L0 = L + 5 * s if side == "free" else L - 5 * s         # the layer the depth lies in
        follows = [L0 + s * t for t in (-3, -2, -1, 0, 1, 2, 3, 5, -5) if 0 <= L0 + s * t < tc.NA and L0 + s * t != L]
        assert differs[L].all() and not np.delete(differs, [L] + follows, axis=0).any()
        if side == "free":
            assert np.all(a[L] == -0.9) and np.all(b[L] == -0.027)
            if 0 <= L - s < tc.NA:
                assert np.all(a[L - s] == -0.027)
        else:
            assert np.all(a[L] == 0.9) and np.all(b[L] == 0.0)
            if 0 <= L + s < tc.NA:
                assert np.all(a[L + s] == 0.0) and not np.signbit(a[L + s]).any()


# ---- depth values at the ends of the range -----------------------------------------------------------------------------------------
def test_every_range_end_value_is_fused_by_some_voxel():
    grid, rp, views, names = tc.range_ends_scene()
    _, px, py, ok = tc.project(grid, views)
    seen, seen_narrow = set(), set()
    near = tc.narrowed(views)
    for m in range(views.n):
        sel = names[m][views.height - 1 - py[m][ok[m]], px[m][ok[m]]]
        d = views.depth[m][views.height - 1 - py[m][ok[m]], px[m][ok[m]]]
        d32 = near.depth[m][views.height - 1 - py[m][ok[m]], px[m][ok[m]]]
        seen |= set(sel[(sel != None) & (d != -1.0)])            # noqa: E711 (elementwise)
        seen_narrow |= set(sel[(sel != None) & (d32 != -1.0)])   # noqa: E711
    assert seen == set(tc.RANGE_END_VALUES)
    # narrowed to f32 the two neighbours of -1 ARE the sentinel, the f64 subnormal is 0, twice FLT_MAX is +inf
    assert seen_narrow == set(tc.RANGE_END_VALUES) - {"just_above_sentinel", "just_below_sentinel"}
    v = tc.RANGE_END_VALUES
    assert np.float32(v["just_above_sentinel"]) == -1.0 and np.float32(v["just_below_sentinel"]) == -1.0
    assert v["just_above_sentinel"] != -1.0 and v["just_below_sentinel"] != -1.0
    with np.errstate(over="ignore"):
        assert np.float32(v["f64_subnormal"]) == 0.0 and np.isinf(np.float32(v["twice_flt_max"])) and np.isfinite(v["twice_flt_max"])
    assert 0 < v["f32_subnormal"] < np.finfo(np.float32).tiny and float(np.float32(v["f32_subnormal"])) == v["f32_subnormal"]
    a, b = tc.oracle_grid(grid, rp, views), tc.numpy_grid(grid, rp, views)
    assert bits_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    c = tc.oracle_grid(grid, rp, near)
    assert not bits_equal(a[0], c[0]) and not np.array_equal(a[2], c[2])
    assert bits_equal(c[0], tc.numpy_grid(grid, rp, near)[0])
