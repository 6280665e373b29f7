"""The table of refused calls behind tests/golden/mesh_call_refusals.json: every entry point of the C ABI that works on the context's
iso-surface mesh -- the extractions, the stages, the colouring, the downloads and the getters -- with a null in each pointer
position, with one bad parameter at a time, with pairs of them (which pin the order of the checks) and in every state that refuses
a call: before any extraction, without normals, regions, support counts or colours, after a stage that drops them, without views,
with a colour context in the wrong state, in a z-slab context, with too small a decimation cell and with a non-finite vertex.  A
case is (state, entry, overrides of the entry's good arguments); Runner makes the states one after the other, each once, and
call() returns (code, text).  The scene is that of tests/test_mesh_sequence_model.py: an 8^3 grid round a sphere's field, two views
of 24 x 18.  The cases of the state "null context" need no device.

tests/golden/make_mesh_call_refusals.py records the table's outcomes from a library built from the commit the refactoring started
at; tests/test_mesh_call_refusals.py replays them against the library of the tree."""
import ctypes
import math

import numpy as np

from cudadepthmapintegration_amd import capi, scene

NAN, INF, MINUS_INF = "nan", "inf", "-inf"   # how a non-finite argument is written in the table (JSON has no word for them)
NULL_CONTEXT = "null context"

# The good arguments of every entry, in the order of its parameters.  "ctx" and "c" are the state's fusion and colour contexts
# (False: null); a name that starts with '*' is a pointer: True stands for an array large enough, False for null.
_COUNTS = [("*n_vertices", True), ("*n_triangles", True)]
GOOD = {
    "dmi_extract_isosurface": [("ctx", True), ("iso", 0.0)] + _COUNTS,
    "dmi_extract_isosurface_normals": [("ctx", True), ("iso", 0.0)] + _COUNTS,
    "dmi_download_isosurface": [("ctx", True), ("*vertices", True), ("*triangles", True)],
    "dmi_download_isosurface_normals": [("ctx", True), ("*normals", True)],
    "dmi_get_isosurface_kernel_ms": [("ctx", True), ("*last", True)],
    "dmi_filter_isosurface_components": [("ctx", True), ("mode", 0), ("min_triangles", 0)] + _COUNTS + [("*n_components", True), ("*n_components_kept", True)],
    "dmi_download_isosurface_regions": [("ctx", True), ("*region_id", True), ("*region_size", True)],
    "dmi_get_isosurface_filter_kernel_ms": [("ctx", True), ("*last", True)],
    "dmi_get_isosurface_filter_pass_ms": [("ctx", True), ("*out", True)],
    "dmi_get_isosurface_filter_cas_retries": [("ctx", True), ("*last", True)],
    "dmi_smooth_isosurface": [("ctx", True), ("iterations", 1), ("lambda", 0.5), ("mu", -0.53)],
    "dmi_get_isosurface_smooth_kernel_ms": [("ctx", True), ("*last", True)],
    "dmi_get_isosurface_smooth_pass_ms": [("ctx", True), ("*out", True)],
    "dmi_decimate_isosurface": [("ctx", True), ("cell_size", 0.5)] + _COUNTS,
    "dmi_decimate_isosurface_placed": [("ctx", True), ("cell_size", 0.5), ("placement", 1)] + _COUNTS,
    "dmi_get_isosurface_decimate_kernel_ms": [("ctx", True), ("*last", True)],
    "dmi_get_isosurface_decimate_pass_ms": [("ctx", True), ("*out", True)],
    "dmi_fill_isosurface_holes": [("ctx", True), ("max_edges", 16)] + _COUNTS + [("*n_filled", True), ("*boundary_edges_left", True)],
    "dmi_get_isosurface_holes_kernel_ms": [("ctx", True), ("*last", True)],
    "dmi_get_isosurface_holes_pass_ms": [("ctx", True), ("*out", True)],
    "dmi_filter_isosurface_support": [("ctx", True), ("min_views", 1), ("tolerance", 0.5), ("require_facing", 0)] + _COUNTS,
    "dmi_download_isosurface_support": [("ctx", True), ("*support", True)],
    "dmi_get_isosurface_support_kernel_ms": [("ctx", True), ("*last", True)],
    "dmi_get_isosurface_support_pass_ms": [("ctx", True), ("*out", True)],
    "dmi_color_process_isosurface": [("c", True), ("ctx", True), ("fused_depth_test", 0), ("tolerance", 0.0), ("*n_vertices", True)],
    "dmi_color_render_isosurface_depths": [("c", True), ("ctx", True)],
    "dmi_download_isosurface_colors": [("ctx", True), ("*mean", True), ("*median", True), ("*count", True)],
    "dmi_get_isosurface_color_kernel_ms": [("ctx", True), ("*last", True)],
    "dmi_get_point_smoothing_kernel_ms": [("ctx", True), ("*last", True)],
}
GETTERS = tuple(e for e in GOOD if e.startswith("dmi_get_"))
# the entries that refuse a context without a mesh, and the downloads that ask for more than a mesh
NEED_A_MESH = tuple(e for e in GOOD if e not in GETTERS and not e.startswith("dmi_extract_"))
_FUSED = {"fused_depth_test": 1, "tolerance": 0.1}


def cases():
    """[(state, entry, {argument: value})]: what differs from the entry's good arguments, in the order of the states."""
    table = []

    def add(state, entry, *overrides):
        for o in overrides:
            table.append((state, entry, dict(o)))

    # ---- no context: needs no device.  Every entry, and for the two colour entries either context
    for entry, good in GOOD.items():
        add(NULL_CONTEXT, entry, {"ctx": False})
        if good[0][0] == "c":
            add(NULL_CONTEXT, entry, {"c": False, "ctx": False})
    add(NULL_CONTEXT, "dmi_extract_isosurface", {"ctx": False, "iso": NAN})
    add(NULL_CONTEXT, "dmi_smooth_isosurface", {"ctx": False, "iterations": -1})
    add(NULL_CONTEXT, "dmi_decimate_isosurface_placed", {"ctx": False, "cell_size": 0.0, "placement": 9})
    add(NULL_CONTEXT, "dmi_fill_isosurface_holes", {"ctx": False, "max_edges": (1 << 20) + 1})
    add(NULL_CONTEXT, "dmi_filter_isosurface_support", {"ctx": False, "min_views": -1})

    # ---- before any extraction: views and colours are there, a mesh is not
    state = "before any extraction"
    for entry in NEED_A_MESH:
        add(state, entry, {})
    add(state, "dmi_color_process_isosurface", _FUSED, {"c": False})
    add(state, "dmi_color_render_isosurface_depths", {"c": False})
    # the parameters come before the mesh, the null arguments before both
    add(state, "dmi_filter_isosurface_components", {"mode": 7}, {"*n_components": False, "mode": 7})
    add(state, "dmi_smooth_isosurface", {"iterations": -1}, {"lambda": 0.0}, {"mu": 0.1})
    add(state, "dmi_decimate_isosurface", {"cell_size": 0.0}, {"*n_vertices": False})
    add(state, "dmi_decimate_isosurface_placed", {"placement": 9})
    add(state, "dmi_fill_isosurface_holes", {"max_edges": (1 << 20) + 1})
    add(state, "dmi_filter_isosurface_support", {"min_views": -1}, {"tolerance": NAN}, {"require_facing": 1})
    add(state, "dmi_download_isosurface", {"*vertices": False})
    add(state, "dmi_download_isosurface_normals", {"*normals": False})
    add(state, "dmi_download_isosurface_support", {"*support": False})
    add(state, "dmi_color_process_isosurface", dict(_FUSED, tolerance=-1.0))   # the mesh comes before the tolerance
    for entry in GETTERS:
        add(state, entry, {("*out" if entry.endswith("_pass_ms") else "*last"): False})
    for entry in ("dmi_extract_isosurface", "dmi_extract_isosurface_normals"):
        add(state, entry, {"iso": NAN}, {"*n_vertices": False}, {"*n_triangles": False}, {"*n_vertices": False, "iso": NAN})

    # ---- a mesh without normals: every pointer, every parameter, pairs of them
    state = "extracted without normals"
    for entry in ("dmi_extract_isosurface", "dmi_extract_isosurface_normals"):
        add(state, entry, {"iso": NAN}, {"*n_vertices": False}, {"*n_triangles": False}, {"*n_triangles": False, "iso": NAN})
    add(state, "dmi_download_isosurface", {"*vertices": False}, {"*triangles": False})
    add(state, "dmi_download_isosurface_normals", {}, {"*normals": False})
    add(state, "dmi_download_isosurface_regions", {})
    add(state, "dmi_download_isosurface_support", {}, {"*support": False})
    add(state, "dmi_download_isosurface_colors", {})
    add(state, "dmi_filter_isosurface_components", {"*n_vertices": False}, {"*n_triangles": False}, {"*n_components": False},
        {"*n_components_kept": False}, {"mode": 7}, {"mode": -1}, {"*n_triangles": False, "mode": 7})
    add(state, "dmi_smooth_isosurface", {"iterations": -1}, {"iterations": 1001}, {"lambda": 0.0}, {"lambda": NAN}, {"lambda": 1.5},
        {"mu": 0.1}, {"mu": MINUS_INF}, {"mu": NAN}, {"iterations": -1, "lambda": 0.0}, {"iterations": 1001, "mu": 0.1},
        {"lambda": NAN, "mu": MINUS_INF}, {"iterations": 0, "lambda": 0.0})
    for entry in ("dmi_decimate_isosurface", "dmi_decimate_isosurface_placed"):
        add(state, entry, {"*n_vertices": False}, {"*n_triangles": False}, {"cell_size": 0.0}, {"cell_size": -1.0}, {"cell_size": NAN},
            {"cell_size": INF}, {"*n_triangles": False, "cell_size": NAN})
    add(state, "dmi_decimate_isosurface_placed", {"placement": 9}, {"placement": -1}, {"cell_size": 0.0, "placement": 9},
        {"*n_vertices": False, "placement": 9})
    add(state, "dmi_fill_isosurface_holes", {"*n_vertices": False}, {"*n_triangles": False}, {"max_edges": (1 << 20) + 1},
        {"max_edges": (1 << 64) - 1}, {"*n_triangles": False, "max_edges": (1 << 20) + 1})
    add(state, "dmi_filter_isosurface_support", {"*n_vertices": False}, {"*n_triangles": False}, {"min_views": -1}, {"tolerance": -0.5},
        {"tolerance": NAN}, {"tolerance": INF}, {"require_facing": 1}, {"min_views": -1, "tolerance": NAN}, {"tolerance": NAN, "require_facing": 1},
        {"*n_vertices": False, "min_views": -1}, {"min_views": 0, "require_facing": 1})
    add(state, "dmi_color_process_isosurface", {"c": False}, {"*n_vertices": False}, dict(_FUSED, tolerance=-1.0), dict(_FUSED, tolerance=NAN),
        dict(_FUSED, tolerance=INF), {"*n_vertices": False, "fused_depth_test": 1, "tolerance": NAN})
    add(state, "dmi_color_render_isosurface_depths", {"c": False})
    # a decimation cell that needs more than 2^21 bins on an axis: the message carries the smallest size that would do
    add(state, "dmi_decimate_isosurface", {"cell_size": 1e-9})
    add(state, "dmi_decimate_isosurface_placed", {"cell_size": 1e-9}, {"cell_size": 1e-9, "placement": 0})

    # ---- regions, counts and colours, then the stages that drop them
    state = "after a smoothing behind regions, counts and colours"   # the regions stay
    add(state, "dmi_download_isosurface_support", {})
    add(state, "dmi_download_isosurface_colors", {})
    state = "after a decimation behind regions, counts and colours"
    add(state, "dmi_download_isosurface_regions", {})
    add(state, "dmi_download_isosurface_support", {})
    add(state, "dmi_download_isosurface_colors", {})
    state = "after a trim that removes something behind regions and colours"   # its counts stay
    add(state, "dmi_download_isosurface_regions", {})
    add(state, "dmi_download_isosurface_colors", {})
    state = "after an extraction behind regions, counts and colours"
    add(state, "dmi_download_isosurface_normals", {})
    add(state, "dmi_download_isosurface_regions", {})
    add(state, "dmi_download_isosurface_support", {})
    add(state, "dmi_download_isosurface_colors", {})

    # ---- views
    state = "no views in the fusion context"
    add(state, "dmi_filter_isosurface_support", {}, {"min_views": 0}, {"min_views": -1}, {"require_facing": 1})
    add(state, "dmi_color_process_isosurface", _FUSED)   # two views there, none here
    state = "no views in the colour context"
    add(state, "dmi_color_process_isosurface", {}, _FUSED, dict(_FUSED, tolerance=NAN))
    add(state, "dmi_color_render_isosurface_depths", {})
    state = "the colour context's own depth test is on"
    add(state, "dmi_color_process_isosurface", {}, _FUSED, dict(_FUSED, tolerance=-1.0))   # (its views have no planes of their own)
    state = "three views in the colour context, two in the fusion context"
    add(state, "dmi_color_process_isosurface", _FUSED)

    # ---- the context itself
    state = "a z-slab context"
    for entry in ("dmi_extract_isosurface", "dmi_extract_isosurface_normals"):
        add(state, entry, {}, {"iso": NAN}, {"*n_vertices": False})
    add(state, "dmi_smooth_isosurface", {})
    state = "a mesh with a non-finite vertex"
    add(state, "dmi_decimate_isosurface", {})
    add(state, "dmi_decimate_isosurface_placed", {}, {"placement": 0})
    return table


def null_context_cases():
    return [c for c in cases() if c[0] == NULL_CONTEXT]


def _number(v):
    return {NAN: math.nan, INF: math.inf, MINUS_INF: -math.inf}.get(v, v) if isinstance(v, str) else v


def _field():
    z, y, x = np.mgrid[0:8, 0:8, 0:8].astype(np.float64)
    return 2.6 - np.sqrt((x - 3.4) ** 2 + (y - 3.6) ** 2 + (z - 3.5) ** 2)


class Runner:
    """Makes the states in the order the table names them (each once: a state is left behind for good) and the calls in them."""

    def __init__(self, L):
        self.L = L
        self.state = None
        self.ctx = self.color = None
        self.arrays = {}

    def close(self):
        for c in (self.ctx, self.color):
            if c is not None:
                c.close()
        self.ctx = self.color = None

    def _enter(self, state):
        self.close()
        if state == NULL_CONTEXT:
            return
        grid = scene.default_grid(8)
        views = scene.make_views(2, 24, 18, seed=2, with_best_cost=True)
        colors = scene.make_colors(2, 24, 18, seed=4)
        self.ctx = ctx = capi.FusionContext(grid, scene.default_ray_potential(grid), z_first=32 if state == "a z-slab context" else 0)
        self.color = color = capi.ColorContext()
        field = _field()
        if state == "a mesh with a non-finite vertex":   # as tests/test_gpu_mesh_sequence_fuzz.py makes one: eight cells of -inf
            field[3:5, 3:5, 0:2] = -np.inf
        ctx.upload_grid(field)
        if state != "no views in the fusion context":
            ctx.add_views(views, 0.8)
        if state == "three views in the colour context, two in the fusion context":
            more = scene.make_views(3, 24, 18, seed=2, with_best_cost=True)
            color.add_views(scene.make_colors(3, 24, 18, seed=4), more.K4, more.RT4)
        elif state != "no views in the colour context":
            color.add_views(colors, views.K4, views.RT4)
        if state in ("before any extraction", "a z-slab context"):
            return
        if state in ("extracted without normals", "no views in the colour context", "three views in the colour context, two in the fusion context"):
            ctx.extract_isosurface(0.0)
        else:
            ctx.extract_isosurface_with_normals(0.0)
        if state == "the colour context's own depth test is on":
            color.set_depth_test(True, 0.1)
        if state.startswith("after "):
            ctx.filter_isosurface_components("min_triangles", 0)
            ctx.filter_isosurface_support(0, 0.5, True)
            ctx.color_isosurface(color)
            ctx.download_isosurface_regions(), ctx.download_isosurface_support(), ctx.download_isosurface_colors()   # all three are there
            nv = len(ctx.download_isosurface()[0])
            if state.startswith("after a smoothing"):
                ctx.smooth_isosurface(1)
            elif state.startswith("after a decimation"):
                assert 0 < ctx.decimate_isosurface(0.5)[0] < nv
            elif state.startswith("after a trim"):
                assert 0 < ctx.filter_isosurface_support(1, 0.5, True)[0] < nv
            else:
                ctx.extract_isosurface(0.0)

    def call(self, state, entry, overrides):
        """(return code, text of the last error) of the case."""
        if state != self.state:
            self._enter(state)
            self.state = state
        fn = getattr(self.L, entry)
        values = dict(GOOD[entry])
        assert set(overrides) <= set(values), (entry, overrides)
        values.update(overrides)
        handle = None
        keep, args = [], []
        for (name, _), ctype in zip(GOOD[entry], fn.argtypes):
            if name in ("ctx", "c"):
                owner = self.ctx if name == "ctx" else self.color
                h = owner._h if values[name] and owner is not None else None
                handle = h if name == "ctx" else handle
                args.append(h)
            elif name.startswith("*"):
                a = np.full(1 << 15, 7, dtype=np.uint8) if values[name] else None   # 32 KiB: ten times the scene's largest array
                keep.append(a)
                args.append(None if a is None else ctypes.cast(a.ctypes.data, ctype))
            else:
                args.append(_number(values[name]))
        rc = fn(*args)
        return rc, self.L.dmi_last_error(handle).decode()
