"""Sequences of mesh calls on ONE capi.FusionContext (and the capi.ColorContext that goes with it) against a replay by the numpy
restatements (tests/mesh_sequence_model.py).  Every mesh stage has a test file of its own that checks it bit for bit on a freshly
extracted mesh; none checks what a context carries from one stage to the next: the flags Mesh::{valid, has_normals, filtered,
colored, support_counted}, CellToPoint::valid and PointSmoothing::on; six mesh buffers with an alternate each, swapped in by the
filter, the smoother, the decimations, the fill and the trim, so that after any stage the two have different capacities and hold
different stale meshes; scratch the smoother, the decimations and the fill share and keep "while large enough", so that a stage
behind one on a larger mesh finds another stage's leftovers behind its own n + 1 entries; work ordered across streams by events
alone (a decimation's normals, the colour context's chunks); and capi.FusionContext._mesh_counts, the binding's second bookkeeping
of the mesh's sizes, by which every download sizes its arrays.  A wrong flag, a missing drop, a read past n, a missing wait or a
stale count shows on the third or sixth call on a context, never on the first.

generate(seed) yields a configuration, 8-14 operations and the model's trace of them.  Two configurations:
  fused    the scene of tests/test_isosurface_support.py: scene.default_grid(32), 6 views of 96 x 72 (seed 3, best costs, threshold
           0.8), scene.make_colors(seed=5), fused once; its iso 0 mesh has 7044 vertices, its iso 1 mesh 1790, its iso 3 mesh 466; the
           trim with min_views 1 and tolerance 0.1 leaves 1186 and 1628.  Half of these seeds hold one depth that is no f32 (the
           depth store is f64).  The colour context holds the same views, half the time with the unthresholded depths as planes.
  lattice  24 x 20 x 16 cells, no views in either context: upload_grid of the `small` and `large` fields of
           test_gpu_mesh_buffers_grow_across_swaps_and_reach_a_steady_state (212 and 3895 vertices) and of an all-zero field (the
           empty mesh).  Support, colouring and rendering are refused here, and the mesh stays.
The generator runs the model as it goes, so it knows the mesh it is about to hand to a stage: a sequence is a few motifs chosen by
the seed -- a stage on a mesh a quarter the size of an earlier one, one on a mesh four times larger than any before, an empty mesh
put through the stages, a fill that fills nothing behind regions, counts and colours, a trim that removes nothing, a colouring
straight behind a decimation with normals, an extraction behind a change of the point smoothing, refused calls of every kind --
and random operations between them.  tests/test_mesh_sequence_model.py holds it to that on the CPU.

The runner drives the context through capi's methods only and never writes _mesh_counts.  After every operation the counts the
call returned (or its refusal's status) are compared with the model's; an extraction's own download is compared as well (the
binding makes it anyway).  At operations the generator marks "observe", and always after the last, the mesh, the normals, the
regions, the support counts and the colours are downloaded -- or their refusals -- and compared bit for bit; at those marked
"points" the point data too.  The generator, not the runner, decides where to look: a download synchronises and sizes its arrays
by _mesh_counts, and would hide a missing wait or mend nothing but show a stale count only where it looks.  The model runs on from
its own state, never from what was downloaded.

Directed sequences beside the seeds: shared scratch behind a larger user; every stage on a mesh trimmed to nothing; regions across
a fill that fills nothing and one that fills; every stage that must drop regions, counts or colours, each looked at; a refused
extraction (found here: the binding forgot the mesh's sizes before an extraction, so that after one refused for a NaN iso-value
every download said "no mesh" while the library still held it); the same ten operations on two fresh contexts.

SEEDS = 24.  Measured on an MI355X: the whole file (24 seeds, 4 of them for 14 repetitions, 6 directed cases) takes 5.3 s, the
slowest case 0.76 s (test_a_second_round_of_a_sequence_allocates_nothing[0]), the slowest seed 0.50 s; the model's replay of all 24
seeds alone takes about 5 s on one slow CPU thread."""
import functools

import numpy as np
import pytest

import isosurface_components_np as C
from cudadepthmapintegration_amd import capi, scene
from mesh_sequence_model import INVALID_ARGUMENT, STATE, MeshSequenceModel, ModelRefusal

pytestmark = pytest.mark.gpu

SEEDS = 24
N_VIEWS, W, H = 6, 96, 72
THRESHOLD, TOLERANCE = 0.8, 0.1
LATTICE = (24, 20, 16)
KINDS = ("upload", "refuse", "point_smoothing", "extract", "extract_normals", "components", "support", "fill", "smooth", "decimate", "color",
         "render", "clear_views_then_support", "refused")
STAGES = ("components", "support", "fill", "smooth", "decimate", "color", "render")
SIGMAS = (0.0, 1.0, (0.0, 2.0, 0.5))
# a refused call of each of these kinds is in four sequences at least (test_the_generator_covers_what_it_is_for)
REFUSALS = {"no_mesh": INVALID_ARGUMENT, "extract_nan": INVALID_ARGUMENT, "smooth_arguments": INVALID_ARGUMENT, "decimate_cell": INVALID_ARGUMENT,
            "decimate_bins": INVALID_ARGUMENT, "decimate_non_finite": INVALID_ARGUMENT, "fill_max_edges": INVALID_ARGUMENT,
            "support_arguments": INVALID_ARGUMENT, "support_facing_without_normals": INVALID_ARGUMENT, "support_without_views": STATE,
            "fused_color_views_unequal": INVALID_ARGUMENT, "color_fused_tolerance": INVALID_ARGUMENT, "color_fused_with_own_test": INVALID_ARGUMENT,
            "color_own_test_without_planes": INVALID_ARGUMENT, "color_context_without_views": STATE, "point_smoothing_arguments": INVALID_ARGUMENT,
            "download_normals": INVALID_ARGUMENT, "download_regions": INVALID_ARGUMENT, "download_support": INVALID_ARGUMENT,
            "download_colors": INVALID_ARGUMENT}


# ---- scenes -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fused_scene(exact_f32):
    """(grid, ray, views, colors); exact_f32 False: one depth of view 0 is not an f32 (tests/test_isosurface_support.py: _scene)"""
    grid = scene.default_grid(32)
    ray = scene.default_ray_potential(grid)
    views = scene.make_views(N_VIEWS, W, H, seed=3, with_best_cost=True)
    if not exact_f32:
        row, col = np.argwhere((views.depth[0] > 0) & (views.best_cost[0] <= THRESHOLD))[0]
        views.depth[0, row, col] += 2.0 ** -40
        assert np.float64(np.float32(views.depth[0, row, col])) != views.depth[0, row, col]
    colors = scene.make_colors(N_VIEWS, W, H, seed=5)
    for a in (views.depth, views.best_cost, views.K4, views.RT4, colors):
        a.setflags(write=False)
    return grid, ray, views, colors


@functools.lru_cache(maxsize=None)
def _fused_cells(exact_f32):
    grid, ray, views, _ = _fused_scene(exact_f32)
    m = MeshSequenceModel(grid, ray)
    m.add_views(views, THRESHOLD)
    m.fuse()
    m.cells.setflags(write=False)
    return m.cells


def _with_a_hole_of_minus_infinity(cells, at):
    """eight cells of -inf: the lattice points between them are -inf, and an edge that leaves such a point for an inside one has
    t = inf / inf -- a vertex with a NaN coordinate, which both decimations refuse"""
    out = np.array(cells)
    k, j, i = at
    out[k:k + 2, j:j + 2, i:i + 2] = -np.inf
    return out


@functools.lru_cache(maxsize=None)
def _fields(lattice, exact_f32=True):
    """name -> (cells, the iso-values to contour it at).  The lattice's `small` and `large` are those of
    tests/test_isosurface_smooth.py::test_gpu_mesh_buffers_grow_across_swaps_and_reach_a_steady_state."""
    if lattice:
        z, y, x = np.mgrid[0:LATTICE[2] + 1, 0:LATTICE[1] + 1, 0:LATTICE[0] + 1].astype(np.float64)
        blob = lambda c, r: r - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
        p = np.maximum(blob((9.3, 9.8, 8.1), 3.3), blob((19.2, 6.4, 5.7), 1.7))
        s = p.shape
        small = 0.125 * sum(p[dz:s[0] - 1 + dz, dy:s[1] - 1 + dy, dx:s[2] - 1 + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1))
        large = np.random.default_rng(17).uniform(-1.5, 2.5, size=LATTICE[::-1])
        out = {"small": (small, (0.0, 0.25)), "large": (large, (1.0, 0.0)), "zero": (np.zeros(LATTICE[::-1]), (0.5,)),
               "minus_inf": (_with_a_hole_of_minus_infinity(small, (7, 9, 8)), (0.0,))}
    else:
        cells = _fused_cells(exact_f32)
        out = {"fused": (cells, (0.0, 1.0, 3.0)), "shifted": (cells - 1.0, (0.0, 2.0)), "zero": (np.zeros(cells.shape), (0.5,)),
               "minus_inf": (_with_a_hole_of_minus_infinity(cells, (15, 15, 3)), (0.0,))}
    for cells, _ in out.values():
        cells.setflags(write=False)
    return out


def config(seed):
    lattice = seed % 3 == 2
    return dict(seed=seed, lattice=lattice, exact_f32=lattice or seed % 3 == 0, own_depths=not lattice and (seed // 3) % 2 == 1)


def _field(cfg, name):
    return _fields(cfg["lattice"], cfg["exact_f32"])[name]


def _grid(cfg):
    return scene.default_grid(LATTICE) if cfg["lattice"] else _fused_scene(cfg["exact_f32"])[0]


def new_model(cfg):
    """The model of a context of this configuration as the runner creates it: the fused scene fused once, or the lattice's small field."""
    if cfg["lattice"]:
        m = MeshSequenceModel(_grid(cfg), scene.default_ray_potential(_grid(cfg)), weights=capi.point_smoothing_weights)
        m.upload_grid(_field(cfg, "small")[0])
        return m
    grid, ray, views, colors = _fused_scene(cfg["exact_f32"])
    m = MeshSequenceModel(grid, ray, weights=capi.point_smoothing_weights)
    m.add_views(views, THRESHOLD)
    m.upload_grid(_fused_cells(cfg["exact_f32"]))   # (what new_contexts' one fuse leaves: the cache spares the oracle's second run)
    m.c_add_views(colors, views.K4, views.RT4, depths=views.depth if cfg["own_depths"] else None)
    return m


# ---- one operation, on the model or on the contexts -------------------------------------------------------------------
class Contexts:
    """A capi.FusionContext and its capi.ColorContext under the model's method names; a DmiError becomes a ModelRefusal."""

    def __init__(self, ctx, color_ctx):
        self.ctx, self.c, self.extracted = ctx, color_ctx, None

    def _do(self, call, *args, **kw):
        try:
            return call(*args, **kw)
        except capi.DmiError as e:
            raise ModelRefusal(e.code, str(e))

    def upload_grid(self, cells): self._do(self.ctx.upload_grid, cells)
    def reset_grid(self): self._do(self.ctx.reset_grid)
    def fuse(self): self._do(self.ctx.fuse)
    def clear_views(self): self._do(self.ctx.clear_views)
    def add_views(self, views, threshold): self._do(self.ctx.add_views, views, threshold=threshold)
    def set_point_smoothing(self, sigma, truncate=3.0): self._do(self.ctx.set_point_smoothing, sigma, truncate)
    def point_data(self): return self._do(self.ctx.download_point_data)

    def extract(self, iso, normals=False):
        self.extracted = None
        got = self._do(self.ctx.extract_isosurface_with_normals if normals else self.ctx.extract_isosurface, iso)
        self.extracted = got
        return len(got[0]), len(got[1])

    def filter_components(self, mode, min_triangles): return self._do(self.ctx.filter_isosurface_components, mode, min_triangles)
    def smooth(self, iterations, lam, mu): return self._do(self.ctx.smooth_isosurface, iterations, lam, mu)
    def decimate(self, cell_size, placement): return self._do(self.ctx.decimate_isosurface, cell_size, placement)
    def fill(self, max_edges): return self._do(self.ctx.fill_isosurface_holes, max_edges)
    def support(self, min_views, tolerance, facing): return self._do(self.ctx.filter_isosurface_support, min_views, tolerance, facing)

    def c_set_depth_test(self, enable, tolerance=0.0):
        try:
            self.c.set_depth_test(enable, tolerance)
        except capi.DmiError as e:
            raise ModelRefusal(e.code, str(e))

    def color(self, fused_depth_tolerance=None): return self._do(self.ctx.color_isosurface, self.c, fused_depth_tolerance)
    def render(self): return self._do(self.ctx.render_isosurface_depths, self.c)
    def download_mesh(self): return self._do(self.ctx.download_isosurface)
    def download_normals(self): return self._do(self.ctx.download_isosurface_normals)
    def download_regions(self): return self._do(self.ctx.download_isosurface_regions)
    def download_support(self): return self._do(self.ctx.download_isosurface_support)
    def download_colors(self): return self._do(self.ctx.download_isosurface_colors)


def _call(t, cfg, name, *args):
    """One call on the model or on the contexts: what it returns, or ("refused", status)."""
    try:
        if name == "upload_field":
            return t.upload_grid(_field(cfg, args[0])[0])
        if name == "add_the_views":
            return t.add_views(_fused_scene(cfg["exact_f32"])[2], THRESHOLD)
        return getattr(t, name)(*args)
    except ModelRefusal as e:
        return ("refused", e.code)


def calls_of(op):
    """The calls an operation stands for, by the model's method names."""
    k = op["kind"]
    if k == "upload":
        return [("upload_field", op["field"])]
    if k == "refuse":
        return [("reset_grid",), ("fuse",)]
    if k == "point_smoothing":
        return [("set_point_smoothing", op["sigma"])]
    if k in ("extract", "extract_normals"):
        return [("extract", op["iso"], k == "extract_normals")]
    if k == "components":
        return [("filter_components", op["mode"], op["min_triangles"])]
    if k == "support":
        return [("support", op["min_views"], TOLERANCE, op["facing"])]
    if k == "fill":
        return [("fill", op["max_edges"])]
    if k == "smooth":
        return [("smooth", op["iterations"], 0.5, op["mu"])]
    if k == "decimate":
        return [("decimate", op["cell"], op["placement"])]
    if k == "color":   # plain, own (the colour context's depth test), fused (this context's depths)
        return [("c_set_depth_test", op["how"] == "own", TOLERANCE), ("color", TOLERANCE if op["how"] == "fused" else None)]
    if k == "render":
        return [("render",), ("c_set_depth_test", True, TOLERANCE), ("color", None)]
    if k == "clear_views_then_support":
        return [("clear_views",), ("support", 1, TOLERANCE, False), ("c_set_depth_test", False, 0.0), ("color", TOLERANCE), ("add_the_views",)]
    assert k == "refused", k
    return op["calls"]


def step(t, cfg, op):
    return [_call(t, cfg, *call) for call in calls_of(op)]


# ---- the generator ----------------------------------------------------------------------------------------------------
def _state(m):
    return dict(nv=len(m.vertices) if m.has_mesh else None, normals=m.normals is not None, regions=m.regions is not None,
                support=m.support_counts is not None, colors=m.colors is not None,
                finite=not m.has_mesh or bool(np.isfinite(m.vertices).all()))


def ran(t):
    """the operation of this trace entry was not refused"""
    return not any(isinstance(r, tuple) and r and r[0] == "refused" for r in t["results"])


def looks(op):
    return op["observe"] or op["points"]


def unobserved_chain(ops, trace):
    """a stage on a mesh that an earlier stage, not an extraction, left, with no download between the two"""
    fresh = False   # the mesh is one a stage produced and nothing has downloaded it
    for op, t in zip(ops, trace):
        if t["kind"] in STAGES and ran(t) and fresh and (t["before"]["nv"] or 0) > 0:
            return True
        if t["kind"] in STAGES and ran(t) and t["changed"]:
            fresh = True
        elif t["kind"] in ("extract", "extract_normals", "refused"):
            fresh = False
        if looks(op):
            fresh = False
    return False


class _Generator:
    def __init__(self, cfg):
        self.cfg, self.rng = cfg, np.random.default_rng([cfg["seed"], 41])
        self.m = new_model(cfg)
        self.ops, self.trace = [], []
        self.field = "small" if cfg["lattice"] else "fused"
        self.voxel = float(max(self.m.grid_desc.spacing))

    # -- emitting
    def emit(self, op, observe=None, **notes):
        m = self.m
        before, sigma = _state(m), tuple(m.sigma)
        mesh = (m.vertices.tobytes(), m.triangles.tobytes()) if m.has_mesh else None
        results, sizes, finite = [], [], True
        for call in calls_of(op):   # (step, call by call: the meshes a bundle of calls passes through are part of the trace)
            results.append(_call(m, self.cfg, *call))
            now = _state(m)
            sizes.append(now["nv"])
            finite = finite and now["finite"]
        dropped = any(before[k] and not now[k] for k in ("regions", "support", "colors"))   # a drop is looked at more often than not
        op["observe"] = bool(self.rng.random() < (0.6 if dropped else 0.25)) if observe is None else observe
        op["points"] = bool(self.rng.random() < 0.12) and op["kind"] != "refused" and observe is not False   # (observe=False: nothing looks)
        self.ops.append(op)
        changed = mesh != ((m.vertices.tobytes(), m.triangles.tobytes()) if m.has_mesh else None)
        self.trace.append(dict(kind=op["kind"], before=before, after=_state(m), results=results, sizes=sizes, finite_within=finite, changed=changed,
                               sigma_changed=tuple(m.sigma) != sigma, **notes))
        if op["kind"] == "upload":
            self.field = op["field"]
        if op["kind"] == "refuse":
            self.field = "fused"
        return results

    def room(self):
        return 14 - len(self.ops)

    # -- parameters
    def an_iso(self):
        isos = _field(self.cfg, self.field)[1]
        return float(isos[int(self.rng.integers(0, len(isos)))])

    def extract(self, iso=None, normals=None, **kw):
        normals = bool(self.rng.random() < 0.6) if normals is None else normals
        return self.emit(dict(kind="extract_normals" if normals else "extract", iso=self.an_iso() if iso is None else iso), **kw)

    def a_stage(self, kind=None, working=False, **kw):
        """a stage with random parameters (kw fixes some); working: one that is not refused in this configuration"""
        m, rng = self.m, self.rng
        kinds = STAGES if not self.cfg["lattice"] else ("components", "fill", "smooth", "decimate") + (() if working else ("support", "color"))
        weights = {"components": 1.2, "support": 1.3, "fill": 1.2, "smooth": 1.2, "decimate": 1.3, "color": 1.2, "render": 0.9}
        if self.cfg["lattice"]:
            weights.update(support=0.3, color=0.3)
        if kind is None:
            p = np.array([weights[k] for k in kinds])
            kind = str(rng.choice(kinds, p=p / p.sum()))
        if kind == "components":
            how = int(rng.integers(0, 3))
            op = dict(kind=kind, mode="largest" if how == 2 else "min_triangles", min_triangles=0)
            if how == 1 and m.has_mesh and len(m.triangles):
                size = C.components(len(m.vertices), m.triangles)[1]
                op["min_triangles"] = int(np.median(size[size > 0])) + 1
        elif kind == "support":
            facing = bool(m.normals is not None and rng.random() < 0.6)
            op = dict(kind=kind, min_views=int(rng.choice([0, 1, 1, 3])), facing=facing)
        elif kind == "fill":
            op = dict(kind=kind, max_edges=int(rng.choice([2, 4, 16, 65536])))
        elif kind == "smooth":
            op = dict(kind=kind, iterations=int(rng.choice([0, 1, 3])), mu=float(rng.choice([0.0, -0.53])))
        elif kind == "decimate":
            cell = 1e-5 if rng.random() < 0.2 else float(rng.uniform(1.5, 3.0)) * self.voxel   # tiny: the weld
            op = dict(kind=kind, placement=str(rng.choice(["mean", "quadric"])), cell=cell)
        elif kind == "color":
            hows = ["plain", "fused"] + (["own"] if m.c_planes is not None or self.cfg["lattice"] else [])
            op = dict(kind=kind, how=str(rng.choice(hows)))
        else:
            op = dict(kind="render")
        op.update({k: v for k, v in kw.items() if k in ("min_views", "facing", "max_edges", "iterations", "mu", "placement", "cell", "how", "mode", "min_triangles")})
        return self.emit(op, **{k: v for k, v in kw.items() if k in ("observe",)})

    # -- refused calls
    def refused(self, names, observe=None):
        m, calls, kinds, expect = self.m, [], [], []
        at = {"color_fused_tolerance": (1,), "color_fused_with_own_test": (1,), "color_own_test_without_planes": (1,), "decimate_non_finite": (3, 4)}
        for name in names:
            if name == "no_mesh" and not m.has_mesh:
                new = [[("smooth", 1, 0.5, -0.53)], [("fill", 16)], [("decimate", self.voxel, "mean")], [("filter_components", "largest", 0)]][int(self.rng.integers(0, 4))]
            elif name == "extract_nan":
                new = [("extract", float("nan"), bool(self.rng.random() < 0.5))]
            elif name == "smooth_arguments":
                new = [[("smooth", -1, 0.5, -0.53)], [("smooth", 1, 0.0, -0.53)], [("smooth", 1, 0.5, 0.1)], [("smooth", 1001, 0.5, 0.0)]][int(self.rng.integers(0, 4))]
            elif name == "decimate_cell":
                new = [("decimate", [0.0, float("nan"), float("inf"), -1.0][int(self.rng.integers(0, 4))], str(self.rng.choice(["mean", "quadric"])))]
            elif name == "decimate_bins" and m.has_mesh and len(m.vertices) > 1:
                new = [("decimate", 1e-9, str(self.rng.choice(["mean", "quadric"])))]
            elif name == "fill_max_edges":
                new = [("fill", (1 << 20) + 1)]
            elif name == "support_arguments":
                new = [[("support", -1, TOLERANCE, False)], [("support", 1, float("nan"), False)], [("support", 1, -0.5, False)]][int(self.rng.integers(0, 3))]
            elif name == "support_facing_without_normals" and m.has_mesh and m.normals is None:
                new = [("support", 1, TOLERANCE, True)]
            elif name == "support_without_views" and self.cfg["lattice"] and m.has_mesh:
                new = [("support", int(self.rng.integers(0, 2)), TOLERANCE, False)]
            elif name == "color_context_without_views" and self.cfg["lattice"] and m.has_mesh:
                new = [[("color", None)], [("render",)], [("color", TOLERANCE)]][int(self.rng.integers(0, 3))]
            elif name == "color_fused_tolerance" and not self.cfg["lattice"] and m.has_mesh:
                new = [("c_set_depth_test", False, 0.0), ("color", [-1.0, float("nan"), float("inf")][int(self.rng.integers(0, 3))])]
            elif name == "color_fused_with_own_test" and not self.cfg["lattice"] and m.has_mesh:
                new = [("c_set_depth_test", True, TOLERANCE), ("color", TOLERANCE), ("c_set_depth_test", False, 0.0)]
            elif name == "color_own_test_without_planes" and not self.cfg["lattice"] and m.has_mesh and len(m.vertices) and m.c_planes is None:
                new = [("c_set_depth_test", True, TOLERANCE), ("color", None), ("c_set_depth_test", False, 0.0)]
            elif name == "point_smoothing_arguments":
                new = [[("set_point_smoothing", -1.0)], [("set_point_smoothing", 6.0)], [("set_point_smoothing", 1.0, 5.0)],
                       [("set_point_smoothing", float("nan"))]][int(self.rng.integers(0, 4))]
            elif name == "decimate_non_finite":
                # the directed one: the only operation whose model mesh holds a non-finite coordinate; it ends with a mesh that has none
                # (with the smoothing off: the Gaussian would spread the hole over the surface)
                back, sigma = self.field, [float(x) for x in m.sigma]
                new = [("set_point_smoothing", 0.0), ("upload_field", "minus_inf"), ("extract", 0.0, True), ("decimate", 2.0 * self.voxel, "quadric"),
                       ("decimate", 2.0 * self.voxel, "mean"), ("set_point_smoothing", sigma), ("upload_field", back),
                       ("extract", _field(self.cfg, back)[1][0], bool(self.rng.random() < 0.5))]
            else:
                continue
            expect += [(name, len(calls) + a) for a in at.get(name, (0,))]
            calls += new
            kinds.append(name)
        if calls:
            results = self.emit(dict(kind="refused", calls=calls), observe=observe, refusals=kinds)
            for name, a in expect:
                assert results[a] == ("refused", REFUSALS[name]), (name, calls[a], results[a])

    # -- motifs
    def grow(self):
        """a small mesh, a stage, then one four times larger than any before and a stage on it"""
        if self.cfg["lattice"]:
            self.extract(0.0)
            self.a_stage()
            self.emit(dict(kind="upload", field="large"))
            self.extract(1.0)
        else:
            self.extract(3.0)
            self.a_stage()
            self.extract(0.0)
        self.moving_stage()
        self.a_stage(working=True)

    def moving_stage(self):
        """a stage that leaves another mesh than it found, and nothing looks at it"""
        if self.rng.random() < 0.5:
            self.a_stage("smooth", iterations=int(self.rng.choice([1, 3])), observe=False)
        else:
            self.a_stage("decimate", cell=float(self.rng.uniform(1.5, 3.0)) * self.voxel, observe=False)
        self.ops[-1]["points"] = False

    def shrink(self):
        """a large mesh, then a stage on one a quarter its size at most, with nothing looking in between"""
        if self.cfg["lattice"]:
            self.emit(dict(kind="upload", field="large"))
            self.extract(1.0)
            self.a_stage(str(self.rng.choice(["smooth", "decimate", "fill"])), observe=False)
            self.emit(dict(kind="upload", field="small"), observe=False)
            self.extract(0.0, observe=False)
        else:
            self.extract(0.0, normals=True)
            if self.rng.random() < 0.5:
                self.a_stage("support", min_views=1, observe=False)
            else:
                self.a_stage("decimate", cell=3.0 * self.voxel, observe=False)
        self.moving_stage()
        self.a_stage(working=True)

    def empty(self):
        if self.cfg["lattice"]:
            self.emit(dict(kind="upload", field="zero"))
            self.extract(0.5)
        else:
            self.extract(1e30)
        for _ in range(int(self.rng.integers(2, 4))):
            self.a_stage(observe=False)
        self.extract_something()

    def extract_something(self):
        if self.field == "zero":
            self.emit(dict(kind="upload", field="small" if self.cfg["lattice"] else "fused"))
        self.extract()

    def fills(self):
        """regions, counts and colours, a fill that fills nothing -- they must all survive --, a trim, and a fill that fills something"""
        self.extract(1.0, normals=True)
        self.a_stage("components", mode="min_triangles", min_triangles=0, observe=False)
        self.a_stage("support", min_views=0, observe=False)
        self.a_stage("color", how=str(self.rng.choice(["plain", "fused"])), observe=False)
        self.a_stage("fill", max_edges=int(self.rng.choice([2, 4])), observe=True)
        self.a_stage("support", min_views=1, observe=False)
        self.a_stage("fill", max_edges=16)

    def trims(self):
        """a trim that removes something and the same trim again, which removes nothing"""
        if not self.m.has_mesh or len(self.m.vertices) < 100:
            self.extract(float(self.rng.choice([0.0, 1.0])))
        facing = bool(self.m.normals is not None and self.rng.random() < 0.5)
        self.a_stage("support", min_views=1, facing=facing, observe=False)
        self.a_stage("support", min_views=1, facing=facing)

    def decimate_then_use_the_normals(self):
        """a decimation with normals and, directly behind it, a colouring or a count: the decimation's normals kernel is still queued"""
        if not self.m.has_mesh or self.m.normals is None or len(self.m.vertices) < 100:
            self.extract(float(self.rng.choice([0.0, 1.0])), normals=True)
        self.a_stage("decimate", cell=float(self.rng.uniform(1.5, 3.0)) * self.voxel, observe=False)
        if self.rng.random() < 0.5:
            self.a_stage("color")
        else:
            self.a_stage("support", min_views=0, facing=True)

    def smoothing_change(self):
        """a change of the point smoothing and an extraction with nothing computing the point data in between"""
        now = tuple(self.m.sigma)
        others = [s for s in SIGMAS if tuple(np.broadcast_to(np.asarray(s, dtype=np.float64), (3,))) != now]
        op = dict(kind="point_smoothing", sigma=others[int(self.rng.integers(0, len(others)))])
        self.emit(op, observe=False)
        self.ops[-1]["points"] = False
        if not self.cfg["lattice"]:
            self.emit(dict(kind="refuse"), observe=False)
            self.ops[-1]["points"] = False
        if self.field == "zero":
            self.emit(dict(kind="upload", field="small" if self.cfg["lattice"] else "fused"), observe=False)
            self.ops[-1]["points"] = False
        self.extract()

    def anything(self):
        rng, m = self.rng, self.m
        r = rng.random() if self.room() >= 4 else 1.0
        if not m.has_mesh or (r < 0.14 and self.room() >= 2):
            self.extract_something()
        elif r < 0.22:
            names = [n for n in _fields(self.cfg["lattice"], self.cfg["exact_f32"]) if n != "minus_inf"]
            self.emit(dict(kind="upload", field=str(rng.choice(names))))
            self.extract_something()
        elif r < 0.28:
            self.smoothing_change()
        elif r < 0.36 and not self.cfg["lattice"]:
            self.emit(dict(kind="refuse"))
            self.extract()
        elif r < 0.44:
            self.refused([GENERIC_REFUSALS[int(rng.integers(0, len(GENERIC_REFUSALS)))] for _ in range(3)])
        else:
            self.a_stage()


GENERIC_REFUSALS = ("extract_nan", "smooth_arguments", "decimate_cell", "decimate_bins", "fill_max_edges", "support_arguments",
                    "support_facing_without_normals", "point_smoothing_arguments", "color_fused_tolerance", "color_fused_with_own_test",
                    "color_own_test_without_planes")


def _generate(seed):
    cfg = config(seed)
    g = _Generator(cfg)
    lattice, i = cfg["lattice"], seed // 3 if cfg["lattice"] else seed - seed // 3 - (1 if seed % 3 == 2 else 0)   # the index among its configuration's seeds
    if seed % 2 == 0:
        g.refused(["no_mesh", "point_smoothing_arguments"], observe=bool(seed % 4 == 0))
    motifs = []
    if lattice:
        motifs.append("grow" if i % 2 == 0 else "shrink")
        if i % 2 == 1:
            motifs.append("empty")
        if i % 4 == 0:
            motifs.append("smoothing_change")
    else:
        if i % 3 == 0:
            motifs.append("grow")
        if i % 3 == 1:
            motifs.append("shrink")
        motifs.append(("fills", "trims", "empty", "decimate_then_use_the_normals")[i % 4])
        if i % 5 in (1, 3):
            motifs.append(("trims", "decimate_then_use_the_normals", "fills", "empty")[i % 4])
        if i % 3 == 2:
            motifs.append("clear_views_then_support")
        if i % 2 == 1:
            motifs.append("smoothing_change")
    generic = [GENERIC_REFUSALS[(5 * seed + j) % len(GENERIC_REFUSALS)] for j in range(4)]
    longest = dict(grow=6, shrink=7, empty=7, fills=7, trims=3, decimate_then_use_the_normals=3, smoothing_change=4, clear_views_then_support=2)
    for n, name in enumerate(motifs):
        if g.room() < longest[name] + (n == 0):
            continue
        if name == "clear_views_then_support":
            if not g.m.has_mesh:
                g.extract()
            results = g.emit(dict(kind="clear_views_then_support"), refusals=["support_without_views", "fused_color_views_unequal"])
            assert results[1] == ("refused", STATE) and results[3] == ("refused", INVALID_ARGUMENT), results
        else:
            getattr(g, name)()
        if n == 0:
            g.refused(generic + (["support_without_views", "color_context_without_views"] if lattice else ["support_facing_without_normals", "color_own_test_without_planes"]))
    if not unobserved_chain(g.ops, g.trace):
        if not g.m.has_mesh or len(g.m.vertices) < 100:
            home = "small" if lattice else "fused"
            if g.field != home:
                g.emit(dict(kind="upload", field=home), observe=False)
            g.extract(_field(cfg, home)[1][0])
        g.a_stage("smooth", iterations=int(g.rng.choice([1, 3])), observe=False)
        g.ops[-1]["points"] = False
        g.a_stage(working=True)
    if seed % 6 in (1, 2):
        g.refused(["decimate_non_finite"])
    while g.room() > 0 and (len(g.ops) < 8 or g.rng.random() < 0.7):
        g.anything()
    for op in g.ops:
        op.setdefault("observe", False)
    g.ops[-1]["observe"] = True
    return cfg, g.ops, g.trace


@functools.lru_cache(maxsize=None)
def generate(seed):
    """(configuration, operations, the model's trace of them: per operation the state before and after and what the calls returned)"""
    return _generate(seed)


# ---- the runner -------------------------------------------------------------------------------------------------------
def _different_rows(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"shape {a.shape} {a.dtype} against {b.shape} {b.dtype}"
    if a.tobytes() == b.tobytes():
        return 0
    rows = a.reshape(len(a), -1).view(np.uint8) != b.reshape(len(b), -1).view(np.uint8)
    return int(rows.any(axis=1).sum())


DOWNLOADS = ("download_mesh", "download_normals", "download_regions", "download_support", "download_colors")


def _is_refusal(x):
    return isinstance(x, tuple) and len(x) == 2 and isinstance(x[0], str)


def _compare(got, want, where):
    if _is_refusal(got) or _is_refusal(want):
        assert _is_refusal(got) and _is_refusal(want) and got == want, (where, "refused" if _is_refusal(got) else "answered",
                                                                     "by the library,", "refused" if _is_refusal(want) else "answered", "by the model",
                                                                     got if _is_refusal(got) else None, want if _is_refusal(want) else None)
        return
    got, want = (got, want) if isinstance(want, tuple) else ((got,), (want,))
    assert len(got) == len(want), where
    for n, (a, b) in enumerate(zip(got, want)):
        d = _different_rows(a, b)
        assert d == 0, (where, f"array {n}", f"{d} rows differ" if isinstance(d, int) else d)


def observe(t, model, cfg, where, points=False):
    for name in DOWNLOADS:
        _compare(_call(t, cfg, name), _call(model, cfg, name), where + (name,))
    if points:
        _compare(t.point_data(), model.point_data(), where + ("point data",))


def new_contexts(cfg):
    grid = _grid(cfg)
    ctx = capi.FusionContext(grid, scene.default_ray_potential(grid))
    c = capi.ColorContext()
    if cfg["lattice"]:
        ctx.upload_grid(_field(cfg, "small")[0])
    else:
        _, _, views, colors = _fused_scene(cfg["exact_f32"])
        ctx.add_views(views, threshold=THRESHOLD)
        ctx.fuse()
        assert ctx.info().depth_storage_in_use == (capi.DMI_DEPTH_F32 if cfg["exact_f32"] else capi.DMI_DEPTH_F64)
        c.add_views(colors, views.K4, views.RT4, depths=views.depth if cfg["own_depths"] else None)
    return ctx, c


def run_operations(t, model, cfg, ops, round_=0):
    for q, op in enumerate(ops):
        where = (cfg["seed"], round_, q, op["kind"])
        got, want = step(t, cfg, op), step(model, cfg, op)
        assert got == want, (where, "what the calls returned", got, want, calls_of(op))
        if op["kind"] in ("extract", "extract_normals") and t.extracted is not None:   # the binding's own download of the extraction
            _compare(t.extracted, (model.vertices, model.triangles) + ((model.normals,) if op["kind"] == "extract_normals" else ()), where + ("extraction",))
        if op["observe"] or op["points"] or q == len(ops) - 1:
            observe(t, model, cfg, where, op["points"])


def run_sequence(cfg, ops, rounds=(1,)):
    """The operations on fresh contexts against a fresh model, rounds[0] times over, then rounds[1] times ...; info().device_bytes
    after each round."""
    model = new_model(cfg)
    ctx, c = new_contexts(cfg)
    device_bytes, n = [], 0
    with ctx, c:
        t = Contexts(ctx, c)
        for repeats in rounds:
            for _ in range(repeats):
                run_operations(t, model, cfg, ops, n)
                n += 1
            device_bytes.append(int(ctx.info().device_bytes))
    return device_bytes


# ---- the seeds --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(SEEDS))
def test_a_sequence_of_mesh_calls_is_its_replay(seed):
    cfg, ops, _ = generate(seed)
    run_sequence(cfg, ops)


@pytest.mark.parametrize("seed", [0, 1, 2, 5])
def test_a_second_round_of_a_sequence_allocates_nothing(seed):
    """The first two seeds of either configuration (an f32 and an f64 depth store; two of the lattice): the same operations again and
    again on the same contexts, the model running on, and info().device_bytes after a second round where the first left it.

    A round is the sequence several times over, not once.  The buffers of a group change places at every stage that builds its result
    beside its input -- own and alternate; with the smoother's second position buffer, and with the support counts' work and compacted
    arrays, three of them --, and each is "kept while large enough, else reallocated at exactly the size asked for" (DESIGN.md).  A
    sequence that leaves a group's members in other places than it found them asks, the next time, the smaller member for the larger
    mesh: seed 0 run once and once more holds 4914674 bytes and then 4984264.  That growth is the design's, is bounded by the group's
    largest request and is no leak.  From its third repetition on a sequence finds the state its predecessor found (every operation
    sets the grid, the smoothing, the planes and the depth test to values of its own, and the mesh is whatever the last extraction
    and the stages behind it left), so every repetition permutes each group in the same way, and a permutation of two or of three
    buffers is the identity after six applications.  Round one: two repetitions to get there and six more; round two: another six,
    which make the same requests of the same buffers in the same places.  A buffer that grows with every call, or one that is
    allocated anew at every call, still shows."""
    cfg, ops, _ = generate(seed)
    first, second = run_sequence(cfg, ops, rounds=(8, 6))
    print(f"seed {seed}: device_bytes {first} after round one, {second} after round two")
    assert first == second > 0


# ---- the directed sequences -------------------------------------------------------------------------------------------
FUSED = dict(seed="directed", lattice=False, exact_f32=True, own_depths=False)


def _op(kind, observe=False, points=False, **kw):
    return dict(kind=kind, observe=observe, points=points, **kw)


def test_shared_scratch_after_a_larger_user():
    """large mesh with normals -> quadric decimation (3 T corner keys in the smoother's key arrays, its sort's storage in the smoother's
    temp) -> a small extraction without normals -> fill -> smooth: the two find the decimation's leftovers behind their own entries"""
    voxel = 2.0 / 32
    ops = [_op("extract_normals", iso=0.0), _op("decimate", placement="quadric", cell=1.5 * voxel), _op("extract", iso=3.0),
           _op("fill", max_edges=65536), _op("smooth", iterations=3, mu=-0.53, observe=True),
           _op("support", min_views=1, facing=False), _op("fill", max_edges=16), _op("smooth", iterations=1, mu=0.0, observe=True)]
    run_sequence(FUSED, ops)


def test_every_stage_on_a_mesh_trimmed_to_nothing():
    """min_views above the number of views leaves (0, 0); every stage takes the empty mesh; the next extraction is whole again"""
    voxel = 2.0 / 32
    ops = [_op("extract_normals", iso=1.0), _op("components", mode="min_triangles", min_triangles=0), _op("color", how="plain"),
           _op("support", min_views=N_VIEWS + 1, facing=True, observe=True), _op("components", mode="largest", min_triangles=0),
           _op("fill", max_edges=16), _op("smooth", iterations=3, mu=-0.53), _op("decimate", placement="mean", cell=2 * voxel),
           _op("decimate", placement="quadric", cell=2 * voxel), _op("support", min_views=1, facing=True), _op("color", how="fused"),
           _op("render", observe=True), _op("extract_normals", iso=1.0, observe=True), _op("support", min_views=1, facing=True, observe=True)]
    run_sequence(FUSED, ops)


def test_regions_survive_a_fill_that_fills_nothing_and_go_with_one_that_fills():
    """components largest -> fill(2) -> the regions are still there -> fill(65536) -> refused.  The fused scene's iso 0 mesh: its largest
    component (7038 of 7044 vertices) holds the sheets that end where no view saw, with rims of many lengths."""
    cfg = FUSED
    model = new_model(cfg)
    ctx, c = new_contexts(cfg)
    ops = [_op("extract", iso=0.0), _op("components", mode="largest", min_triangles=0), _op("fill", max_edges=2, observe=True)]
    with ctx, c:
        t = Contexts(ctx, c)
        run_operations(t, model, cfg, ops)
        region_id, region_size = ctx.download_isosurface_regions()
        assert len(region_id) == len(model.vertices) > 0 and len(region_size) == 1
        run_operations(t, model, cfg, [_op("fill", max_edges=65536, observe=True)])
        assert model.regions is None and len(model.vertices) > len(region_id)
        with pytest.raises(capi.DmiError) as e:
            ctx.download_isosurface_regions()
        assert e.value.code == INVALID_ARGUMENT


def test_every_stage_that_changes_the_mesh_drops_what_no_longer_describes_it():
    """regions, counts and colours before each of: a smoothing, a decimation, a trim that removes something, a fill that fills
    something, the component filter, an extraction -- and a look at all five downloads behind each (one flag a stage, three flags
    a context: every one of these drops has its own line in the library)"""
    voxel = 2.0 / 32
    everything = [_op("components", mode="min_triangles", min_triangles=0), _op("support", min_views=0, facing=True), _op("color", how="fused")]
    ops = [_op("extract_normals", iso=1.0)]
    for stage in (_op("smooth", iterations=1, mu=-0.53), _op("decimate", placement="mean", cell=1.5 * voxel), _op("support", min_views=1, facing=True),
                  _op("fill", max_edges=16), _op("components", mode="largest", min_triangles=0), _op("extract_normals", iso=0.0),
                  _op("decimate", placement="quadric", cell=2 * voxel)):
        ops += [dict(op) for op in everything] + [dict(stage, observe=True)]
    run_sequence(FUSED, ops)


def test_the_same_sequence_on_two_fresh_contexts_gives_the_same_bytes():
    voxel = 2.0 / 32
    ops = [_op("extract_normals", iso=0.0), _op("support", min_views=1, facing=True), _op("fill", max_edges=16),
           _op("components", mode="min_triangles", min_triangles=20), _op("smooth", iterations=3, mu=-0.53),
           _op("decimate", placement="quadric", cell=1.5 * voxel), _op("support", min_views=0, facing=True), _op("render"),
           _op("color", how="fused"), _op("fill", max_edges=65536)]
    assert len(ops) == 10
    cfg = FUSED
    downloads = []
    for _ in range(2):
        ctx, c = new_contexts(cfg)
        with ctx, c:
            t = Contexts(ctx, c)
            for op in ops:
                step(t, cfg, op)
            got = [_call(t, cfg, name) for name in DOWNLOADS] + [c.download_depths()]
        flat = []
        for g in got:
            flat += list(g) if isinstance(g, tuple) else [g]
        downloads.append([a if isinstance(a, (str, int)) else (a.shape, a.dtype.str, a.tobytes()) for a in flat])
    assert downloads[0] == downloads[1] and len(downloads[0]) >= 9


def test_a_refused_extraction_leaves_the_mesh_and_its_arrays():
    """extract, regions, counts, colours; an extraction at a NaN iso-value is refused -- and every download is still answered, the
    binding's included (it had forgotten the mesh's sizes before the call)"""
    ops = [_op("extract_normals", iso=1.0), _op("components", mode="min_triangles", min_triangles=0), _op("support", min_views=0, facing=True),
           _op("color", how="plain", observe=True), _op("refused", calls=[("extract", float("nan"), False), ("extract", float("nan"), True)], observe=True),
           _op("smooth", iterations=1, mu=-0.53, observe=True)]
    run_sequence(FUSED, ops)
