"""tests/mesh_sequence_model.py against itself, on hand-made meshes, one test per rule of include/dmi.h the model follows; and the
generator of tests/test_gpu_mesh_sequence_fuzz.py held to its purpose on the model alone, so that the GPU tests cannot pass
vacuously.  No GPU; the restatements the model calls are checked bit for bit against the library by their stages' own files."""
import os

import numpy as np
import pytest

import point_smooth_np as PS
import test_gpu_mesh_sequence_fuzz as F
from cudadepthmapintegration_amd import capi, scene
from mesh_sequence_model import INVALID_ARGUMENT, RULES, STATE, MeshSequenceModel, ModelRefusal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_rule_cites_the_header():
    lines = open(os.path.join(ROOT, "include", "dmi.h")).read().split("\n")
    for operation, rules in RULES.items():
        for what, line, words in rules:
            assert words in lines[line - 1], (operation, what, line, lines[line - 1])
    assert "DMI_ERR_INVALID_ARGUMENT = 1," in lines[63] and "DMI_ERR_STATE = 4" in lines[66]
    assert (INVALID_ARGUMENT, STATE) == (1, 4)


def test_the_weights_of_the_model_are_the_librarys():
    """the library is the authority on the Gaussian's weights: numpy's exp gives another last bit at sigma 2 (so the models of the
    sequences take capi.point_smoothing_weights, which needs no device), and no more than that at any sigma the sequences set"""
    for sigma in (1.0, 2.0, 0.5):
        ours, theirs = PS.weights_np(sigma, 3.0), capi.point_smoothing_weights(sigma, 3.0)
        assert ours.shape == theirs.shape and (np.abs(ours - theirs) <= 2 * np.spacing(theirs)).all(), sigma
    assert F.new_model(F.config(0)).weights is capi.point_smoothing_weights and F.new_model(F.config(2)).weights is capi.point_smoothing_weights


# ---- hand-made meshes -----------------------------------------------------------------------------------------------------
def _refused(call, code=INVALID_ARGUMENT):
    with pytest.raises(ModelRefusal) as e:
        call()
    assert e.value.code == code, (e.value.code, code)


def _views(n=2, w=24, h=18):
    return scene.make_views(n, w, h, seed=2, with_best_cost=True)


def _model(with_views=True, with_colors=True, planes=False):
    """An 8^3 grid around a sphere's field, two views of 24 x 18 and their colours."""
    grid = scene.default_grid(8)
    m = MeshSequenceModel(grid, scene.default_ray_potential(grid))
    z, y, x = np.mgrid[0:8, 0:8, 0:8].astype(np.float64)
    m.upload_grid(2.6 - np.sqrt((x - 3.4) ** 2 + (y - 3.6) ** 2 + (z - 3.5) ** 2))
    views = _views()
    if with_views:
        m.add_views(views, 0.8)
    if with_colors:
        m.c_add_views(scene.make_colors(2, 24, 18, seed=4), views.K4, views.RT4, depths=views.depth if planes else None)
    return m


def _open_model():
    """The same with a sheet that leaves the grid: a mesh with a boundary (a rim of many edges)."""
    m = _model()
    z, y, x = np.mgrid[0:8, 0:8, 0:8].astype(np.float64)
    m.upload_grid(6.6 - np.sqrt((x - 3.4) ** 2 + (y - 3.6) ** 2 + (z + 3.0) ** 2))   # a cap of a sphere centred below the grid
    return m


def _everything(m):
    m.filter_components("min_triangles", 0)
    m.support(0, 0.5, facing=m.normals is not None)
    m.color(None)
    assert m.regions is not None and m.support_counts is not None and m.colors is not None


def test_an_extraction_drops_normals_unless_asked_and_regions_support_and_colours():
    m = _model()
    nv, nt = m.extract(0.0, normals=True)
    assert nv > 50 and nt > 50 and m.normals is not None and m.normals.dtype == np.float32 and len(m.normals) == nv
    _everything(m)
    m.extract(0.0, normals=False)
    assert m.normals is None and m.regions is None and m.support_counts is None and m.colors is None
    for download in (m.download_normals, m.download_regions, m.download_support, m.download_colors):
        _refused(download)
    assert m.download_mesh()[0] is m.vertices
    m.extract(0.0, normals=True)
    _everything(m)
    m.extract(0.0, normals=True)
    assert m.normals is not None and m.regions is None and m.support_counts is None and m.colors is None


def test_a_refused_extraction_leaves_everything():
    m = _model()
    for call in (m.download_mesh, lambda: m.smooth(1), lambda: m.fill(16), lambda: m.decimate(0.1), lambda: m.filter_components(),
                 lambda: m.support(0, 0.1, False), lambda: m.color(None), m.render):
        _refused(call)                                # before any extraction
    m.extract(0.0, normals=True)
    _everything(m)
    before = m.digest()
    _refused(lambda: m.extract(float("nan")))
    _refused(lambda: m.extract(float("nan"), normals=True))
    assert m.digest() == before


def test_calls_that_change_nothing_drop_nothing():
    m = _model()
    m.extract(0.0, normals=True)
    _everything(m)
    before = m.digest()
    assert m.support(0, 0.5, True) == m.counts          # min_views 0: the counts only (the same counts again)
    assert m.digest() == before
    assert m.fill(65536)[2] == 0 and m.fill(2)[2] == 0   # a closed surface has no rim; below three edges nothing is a loop
    assert m.digest() == before
    m.smooth(0)
    assert m.digest() == before
    left = m.support(1, 0.5, True)
    assert 0 < left[0] < before[2][0][0]
    _everything(m)
    before = m.digest()
    assert m.support(1, 0.5, True) == left == m.counts   # a trim that removes nothing: the trim is idempotent
    assert m.regions is not None and m.colors is not None and (m.support_counts >= 1).all()
    m.support(0, 0.5, True)
    assert m.digest() == before


def test_a_trim_that_removes_something_drops_colours_and_regions_and_keeps_its_counts():
    m = _model()
    nv, _ = m.extract(0.0, normals=True)
    _everything(m)
    counts = m.support_counts.copy()
    assert 0 < (counts >= 1).sum() < nv
    left = m.support(1, 0.5, True)
    assert 0 < left[0] < nv and m.regions is None and m.colors is None
    assert len(m.support_counts) == left[0] and (m.support_counts >= 1).all() and len(m.normals) == left[0]
    assert m.support(1, 0.5, True) == left               # idempotent: the second removes nothing
    assert m.support(3, 0.5, True) == (0, 0) and len(m.support_counts) == 0


def test_a_fill_that_fills_drops_regions_support_and_colours():
    m = _open_model()
    nv, nt = m.extract(0.0, normals=True)
    _everything(m)
    rim = m.fill(4)[3]
    assert m.fill(4)[2] == 0 and rim > 4 and m.regions is not None  # the one rim is longer than four edges
    got = m.fill(65536)
    assert got[2] == 1 and got[0] == nv + 1 and got[1] == nt + rim and got[3] == 0
    assert m.regions is None and m.support_counts is None and m.colors is None and len(m.normals) == nv + 1


def test_smoothing_and_the_component_filter():
    m = _open_model()
    nv, _ = m.extract(0.0, normals=True)
    _everything(m)
    v0, n0 = m.vertices.copy(), m.normals.copy()
    m.smooth(2, 0.5, -0.53)
    assert m.regions is not None and m.support_counts is None and m.colors is None        # the regions stay
    assert (m.vertices != v0).any() and (m.normals != n0).any() and len(m.vertices) == nv
    _everything(m)
    assert m.filter_components("largest") == (nv, len(m.triangles), 1, 1)
    assert m.regions is not None and m.support_counts is None and m.colors is None        # labels only, and yet the mesh "changed"
    for bad in ((-1, 0.5, -0.53), (1001, 0.5, -0.53), (1, 0.0, -0.53), (1, 1.5, -0.53), (1, 0.5, 0.1), (1, 0.5, float("nan"))):
        _refused(lambda: m.smooth(*bad))


def test_a_decimation_drops_the_regions_and_refuses_what_the_header_says():
    m = _model()
    nv, _ = m.extract(0.0, normals=True)
    _everything(m)
    before = m.digest()
    for cell in (0.0, -1.0, float("nan"), float("inf"), 1e-9):
        for placement in ("mean", "quadric"):
            _refused(lambda: m.decimate(cell, placement))
    assert m.digest() == before
    left = m.decimate(0.5, "quadric")
    assert 0 < left[0] < nv and m.regions is None and m.support_counts is None and m.colors is None and len(m.normals) == left[0]
    # a non-finite coordinate refuses both placements, and the mesh stays
    m.vertices[0, 1] = np.nan
    before = m.digest()
    _refused(lambda: m.decimate(0.5, "quadric"))
    _refused(lambda: m.decimate(0.5, "mean"))
    assert m.digest() == before
    _refused(lambda: m.fill((1 << 20) + 1))


def test_the_grid_and_the_point_smoothing_leave_the_mesh_and_change_the_next_extraction():
    m = _model()
    nv, _ = m.extract(0.0, normals=True)
    _everything(m)
    cells, before = m.cells.copy(), m.digest()[2:]
    m.reset_grid()
    m.fuse()
    m.upload_grid(cells * 0.5 - 0.2)
    m.set_point_smoothing(1.0)
    assert m.digest()[2:] == before                                 # mesh, normals, regions, counts, colours, planes
    for bad in ((-1.0, 3.0), (float("nan"), 3.0), (6.0, 3.0), (1.0, 5.0), (1.0, 0.0)):
        _refused(lambda: m.set_point_smoothing(*bad))
    assert tuple(m.sigma) == (1.0, 1.0, 1.0) and m.truncate == 3.0  # the old setting kept
    assert m.extract(0.0, normals=True)[0] != nv
    smoothed = m.vertices.copy()
    m.set_point_smoothing(0.0)
    m.extract(0.0, normals=True)
    assert m.vertices.shape != smoothed.shape or (m.vertices != smoothed).any()


def test_support_and_fused_colouring_need_views_and_facing_needs_normals():
    m = _model()
    m.extract(0.0, normals=False)
    _refused(lambda: m.support(1, 0.1, True))                       # no normals
    _refused(lambda: m.support(-1, 0.1, False))
    _refused(lambda: m.support(1, float("nan"), False))
    assert m.color(0.1) == len(m.vertices)
    m.clear_views()
    _refused(lambda: m.support(1, 0.1, False), STATE)
    _refused(lambda: m.support(1, 0.1, True))                       # the argument checks come first
    _refused(lambda: m.color(0.1))                                  # two views there, none here: the counts are unequal
    assert m.color(None) == len(m.vertices)
    bare = _model(with_views=False, with_colors=False)
    bare.extract(0.0)
    for call in (lambda: bare.color(None), lambda: bare.color(0.1), bare.render, lambda: bare.support(0, 0.1, False)):
        _refused(call, STATE)


def test_the_colour_contexts_depth_test_and_the_rendering():
    m = _model()
    m.extract(0.0)
    plain = m.color(None) and m.colors
    m.c_set_depth_test(True, 0.1)
    before = m.digest()
    _refused(lambda: m.color(None))                                 # its views have no planes
    _refused(lambda: m.color(0.1))                                  # one test at a time
    assert m.digest() == before                                     # a failed colouring leaves the colours
    m.render()
    assert m.c_planes.shape == (2, 18, 24) and (m.c_planes > 0).any() and (m.c_planes == -1).any()
    assert m.colors is not None                                     # rendering changes no array of the mesh
    m.color(None)
    assert (m.colors[2] <= plain[2]).all() and (m.colors[2] < plain[2]).any()   # its own far side is hidden
    m.c_set_depth_test(False)
    _refused(lambda: m.color(-1.0))
    m.decimate(10.0)                                                # everything collapses: an empty mesh
    assert m.counts == (0, 0) and m.color(None) == 0 and len(m.colors[2]) == 0
    m.render()
    assert (m.c_planes == -1).all()


# ---- the generator ----------------------------------------------------------------------------------------------------
def _sequences():
    return [F.generate(seed) for seed in range(F.SEEDS)]


def _stage_sizes(trace):
    """per stage that ran on a mesh with vertices: (its vertices, the largest mesh the context has held, the largest it had held before
    this mesh came to be)"""
    largest, current, before_current, out = 0, None, 0, []
    for t in trace:
        if t["kind"] in F.STAGES and F.ran(t) and t["before"]["nv"]:
            out.append((t["before"]["nv"], largest, before_current))
        for nv in t["sizes"]:
            if nv != current:
                before_current, current = largest, nv
            largest = max(largest, nv or 0)
    return out


def test_the_generator_covers_what_it_is_for():
    sequences = _sequences()
    assert all(8 <= len(ops) <= 14 for _, ops, _ in sequences), [len(ops) for _, ops, _ in sequences]
    short = []   # every condition that is not met, so that one run shows them all
    for kind in F.KINDS:
        with_kind = sum(any(op["kind"] == kind for op in ops) for _, ops, _ in sequences)
        if with_kind * 5 < F.SEEDS:
            short.append((kind, with_kind))
    short += [("no unobserved stage-to-stage chain", cfg["seed"]) for cfg, ops, trace in sequences if not F.unobserved_chain(ops, trace)]
    # the stale-scratch hazard and growth after swaps
    small_after_large = large_after_small = 0
    for _, ops, trace in sequences:
        stages = _stage_sizes(trace)
        small_after_large += any(4 * nv <= largest for nv, largest, _ in stages)
        large_after_small += any(before > 0 and nv >= 4 * before for nv, _, before in stages)
    if small_after_large * 3 < F.SEEDS or large_after_small * 3 < F.SEEDS:
        short.append(("small after large, large after small", small_after_large, large_after_small))

    def count(predicate):
        return sum(bool(predicate(ops, trace)) for _, ops, trace in sequences)

    def empty_then_processed(ops, trace):
        return any(t["kind"] in F.STAGES and F.ran(t) and t["before"]["nv"] == 0 for t in trace)

    def fill_nothing_behind_everything(ops, trace):
        return any(t["kind"] == "fill" and F.ran(t) and t["results"][0][2] == 0 and t["before"]["regions"] and t["before"]["support"] and
                   t["before"]["colors"] and t["after"]["regions"] and t["after"]["support"] and t["after"]["colors"] for t in trace)

    def fill_something(ops, trace):
        return any(t["kind"] == "fill" and F.ran(t) and t["results"][0][2] > 0 for t in trace)

    def trim(removes):
        def predicate(ops, trace):
            return any(t["kind"] == "support" and F.ran(t) and op["min_views"] > 0 and t["before"]["nv"] > 0 and
                       (t["after"]["nv"] != t["before"]["nv"] or t["changed"]) == removes for op, t in zip(ops, trace))
        return predicate

    def normals_still_queued(ops, trace):
        return any(a["kind"] == "decimate" and F.ran(a) and a["before"]["normals"] and a["after"]["nv"] > 0 and not F.looks(op) and
                   b["kind"] in ("color", "support", "render") and F.ran(b) for op, a, b in zip(ops, trace, trace[1:]))

    def extraction_behind_a_smoothing_change(ops, trace):
        pending = False
        for op, t in zip(ops, trace):
            if t["kind"] in ("extract", "extract_normals") and pending and F.ran(t):
                return True
            if t["kind"] == "point_smoothing" and F.ran(t) and t["sigma_changed"]:
                pending = True
            elif t["kind"] in ("extract", "extract_normals", "refused"):
                pending = False     # (a refused bundle may extract)
            if op["points"]:
                pending = False     # download_point_data computes the point data
        return False

    for name, predicate in (("an empty mesh is processed", empty_then_processed), ("a fill fills nothing behind regions, counts and colours", fill_nothing_behind_everything),
                            ("a fill fills something", fill_something), ("a trim removes nothing", trim(False)), ("a trim removes something", trim(True)),
                            ("the decimation's normals are still queued", normals_still_queued),
                            ("an extraction behind a change of the point smoothing", extraction_behind_a_smoothing_change)):
        if count(predicate) < 4:
            short.append((name, count(predicate)))
    both_fills = count(lambda ops, trace: fill_nothing_behind_everything(ops, trace) and fill_something(ops, trace))
    if both_fills < 4:
        short.append(("both fills in one sequence", both_fills))
    # a refused call of every kind
    downloads = {"download_normals": "normals", "download_regions": "regions", "download_support": "support", "download_colors": "colors"}
    for kind, code in F.REFUSALS.items():
        if kind in downloads:   # a download the runner makes where the generator looks, of an array that is not there
            n = count(lambda ops, trace: any(F.looks(op) and t["after"]["nv"] is not None and not t["after"][downloads[kind]] for op, t in zip(ops, trace)))
        else:
            n = count(lambda ops, trace: any(kind in t.get("refusals", ()) for t in trace))
        if n < 4:
            short.append(("refused: " + kind, n))
    assert not short, short
    for _, ops, trace in sequences:
        for op, t in zip(ops, trace):
            if "decimate_non_finite" not in t.get("refusals", ()):
                assert t["before"]["finite"] and t["after"]["finite"] and t["finite_within"], (op, t)
            assert all(nv is None or nv < 20000 for nv in t["sizes"])
    # both configurations, both depth stores, the colour context with and without planes of its own
    assert sum(cfg["lattice"] for cfg, _, _ in sequences) * 3 == F.SEEDS
    fused = [cfg for cfg, _, _ in sequences if not cfg["lattice"]]
    assert sum(cfg["exact_f32"] for cfg in fused) * 2 == len(fused) and sum(cfg["own_depths"] for cfg in fused) * 2 == len(fused)
    assert {(cfg["exact_f32"], cfg["own_depths"]) for cfg in fused} == {(a, b) for a in (False, True) for b in (False, True)}


def test_the_lattice_refuses_support_and_colouring_and_keeps_the_mesh():
    cfg = F.config(2)
    assert cfg["lattice"]
    m = F.new_model(cfg)
    m.extract(0.0, normals=True)
    before = m.digest()
    for call in (lambda: m.support(1, 0.1, False), lambda: m.support(0, 0.1, True), lambda: m.color(0.1), lambda: m.color(None), m.render):
        _refused(call, STATE)
    assert m.digest() == before


def test_the_scene_of_the_fused_configuration_is_the_one_it_names():
    m = F.new_model(F.config(0))
    assert m.extract(0.0, normals=True)[0] == 7044 and m.support(1, 0.1, True)[0] == 1186
    assert m.extract(1.0, normals=True)[0] == 1790 and m.support(1, 0.1, True)[0] == 1628
    assert m.extract(3.0)[0] == 466
    lattice = F.new_model(F.config(2))
    assert lattice.extract(0.0)[0] == 212
    lattice.upload_grid(F._field(F.config(2), "large")[0])
    assert lattice.extract(1.0)[0] == 3895


def test_the_same_seed_gives_the_same_sequence_and_the_same_model_results():
    for seed in (1, 2):
        a, b = F._generate(seed), F._generate(seed)
        assert repr(a[1]) == repr(b[1]) and repr(a[2]) == repr(b[2]), seed
        digests = []
        for _ in range(2):
            m = F.new_model(a[0])
            results = [F.step(m, a[0], op) for op in a[1]]
            digests.append((repr(results), m.digest()))
        assert digests[0] == digests[1] and digests[0][0] == repr([t["results"] for t in a[2]]), seed
