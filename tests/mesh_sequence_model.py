"""The mesh side of a fusion context as a caller sees it, replayed on the CPU: the cell grid and the point-smoothing setting, the
current mesh (vertices, triangles, normals or None), the region arrays, the support counts and the colours (each present or
None: the library's "valid" bit), the resident views with their thresholded depths and, for the colour context that goes with it,
its views, its depth planes and its depth-test setting.  One method per operation of capi.FusionContext; each computes its result
with the numpy restatement its stage's own test file checks bit for bit, and adds no arithmetic of its own.  The model holds no
flag, swap, scratch array or count of the library's: it is what those must never change.  tests/test_mesh_sequence_model.py checks
it against itself and holds the generator of tests/test_gpu_mesh_sequence_fuzz.py to its purpose; that file runs sequences of
operations through a context and through the model and compares what can be read back.

What an operation drops or keeps, and what it refuses with which status, is include/dmi.h's; RULES below holds one table per
operation, every rule with the header line it is taken from and words of that line (test_every_rule_cites_the_header keeps the
citations true).  A refused call raises ModelRefusal(code) and leaves the model untouched.

Where the header is silent the model says so and keeps out of the way:
  - fuse, reset_grid, upload_grid and set_point_smoothing are not said to touch the mesh; the mesh is replaced by "the next
    extraction" only (dmi.h:331, 377, 415), so they leave the mesh and its arrays and change what the next extraction sees;
  - the colouring of an EMPTY mesh with the colour context's own depth test on and a view without planes is not decided by the
    header (an empty mesh is a success; the test without planes is refused): the model refuses to answer (AssertionError) and the
    generator does not ask;
  - the order of the refusals of the colouring is stated only for the support trim (dmi.h:540); calls with two reasons for a
    refusal of different status are not generated, except the one the header decides: no views anywhere is DMI_ERR_STATE."""
import numpy as np

import coloration_depth_np as CD
import isosurface_components_np as C
import isosurface_decimate_np as D
import isosurface_decimate_quadric_np as Q
import isosurface_holes_np as H
import isosurface_normals_np as N
import isosurface_np as R
import isosurface_smooth_np as SM
import isosurface_support_np as S
import mesh_depth_np as MD
import point_smooth_np as PS
from oracle import oracle_np

INVALID_ARGUMENT, STATE = 1, 4   # DMI_ERR_INVALID_ARGUMENT, DMI_ERR_STATE (include/dmi.h:64, 67)

# operation -> [(what the model does, header line, words of that line)]
RULES = {
    "point_data": [
        ("the point data is the cell -> point pass of the grid", 224, "gets the mean of its 1..8"),
        ("... followed by the passes while a sigma is set, for every consumer", 252, "is followed by the passes"),
        ("a setting marks the point data stale: the next extraction reads the new field", 251, "marks the point data"),
        ("all sigmas 0 switch it off", 254, "All sigmas 0 switches it off"),
        ("refused with the old setting kept: INVALID_ARGUMENT", 256, "DMI_ERR_INVALID_ARGUMENT, the old setting kept"),
        ("sigma finite and >= 0, truncate in (0, 4]", 238, "each finite and >= 0"),
        ("a radius above 16 is refused", 240, "r_a > 16 is refused"),
    ],
    "extract": [
        ("reads the point data as it is now", 275, "Runs dmi_cell_to_point first if the grid changed"),
        ("an empty surface is a success", 287, "An empty surface is a success (0 and 0)"),
        ("a NaN iso: INVALID_ARGUMENT", 287, "DMI_ERR_INVALID_ARGUMENT for a NaN iso"),
        ("a refused extraction leaves the mesh of the last successful one", 288, "a call refused for these leaves the last mesh"),
        ("drops the normals unless asked for them", 306, "when the last successful one was a plain dmi_extract_isosurface"),
        ("drops the regions", 338, "when no filter has run since the last one"),
        ("drops the support counts", 545, "after anything that has changed the mesh since: an extraction"),
        ("drops the colours", 666, "a successful extraction, dmi_filter_isosurface_components, dmi_smooth_isosurface with iterations > 0 or"),
    ],
    "components": [
        ("no mesh: INVALID_ARGUMENT", 332, "no successful extraction yet"),
        ("a mesh filtered to nothing is a success", 329, "A mesh filtered to nothing is a success (0, 0)"),
        ("an empty mesh stays empty", 324, "an empty mesh stays empty"),
        ("normals are copied", 326, "normals when the extraction had them, are the original bits"),
        ("the regions exist afterwards (min_triangles 0: labels only)", 322, "0 keeps everything: labels only"),
        ("drops the support counts", 545, "the component"),
        ("drops the colours", 666, "dmi_filter_isosurface_components"),
    ],
    "smooth": [
        ("regions stay", 352, "RegionId and RegionSize are not touched"),
        ("iterations 0 changes nothing, normals included; bad arguments INVALID_ARGUMENT", 371, "iterations == 0 is a success that changes nothing"),
        ("an empty mesh is a success", 372, "an empty mesh is a success"),
        ("no mesh: INVALID_ARGUMENT", 372, "before any"),
        ("a refused call leaves the mesh", 374, "A call that fails leaves the context's mesh as"),
        ("normals become the geometric ones", 364, "if the mesh carries normals (dmi_extract_isosurface_normals) and iterations > 0, they are replaced"),
        ("iterations > 0 drops the support counts", 546, "a smoothing with iterations > 0"),
        ("iterations > 0 drops the colours", 666, "dmi_smooth_isosurface with iterations > 0"),
    ],
    "decimate": [
        ("a non-finite coordinate refuses the call", 394, "a non-finite coordinate anywhere refuses the call"),
        ("normals become the geometric ones; none stay none", 410, "if the mesh carries normals they are replaced by the geometric normals"),
        ("drops the regions", 413, "RegionId and RegionSize of an earlier filter no longer describe this mesh"),
        ("an empty mesh is a success", 416, "An empty mesh is a success (0, 0)"),
        ("refusals: INVALID_ARGUMENT", 417, "DMI_ERR_INVALID_ARGUMENT: a null context or null count"),
        ("a refused call leaves mesh, normals and regions", 419, "A call that fails leaves the context's mesh,"),
        ("the quadric placement refuses and guarantees the same", 453, "All refusals and guarantees of"),
        ("drops the support counts", 546, "or a decimation"),
        ("drops the colours", 667, "dmi_decimate_isosurface drops the colours"),
    ],
    "fill": [
        ("a fill drops regions, support counts and colours", 494, "RegionId / RegionSize, the support counts and the colours no longer describe a mesh that was filled"),
        ("a call that fills nothing leaves all of them", 495, "A call that fills nothing"),
        ("... max_edges < 3 included", 496, "max_edges < 3"),
        ("normals of old vertices stay, new ones are geometric", 491, "keeps those of its old vertices"),
        ("max_edges > 2^20, no mesh: INVALID_ARGUMENT", 502, "max_edges > 2^20, no extraction yet"),
    ],
    "support": [
        ("min_views 0: the counts only", 533, "min_views == 0 changes nothing in the mesh and only computes the counts"),
        ("more than the views leaves (0, 0)", 533, "min_views > the number of views leaves (0, 0)"),
        ("a trim that removes anything drops colours and regions", 535, "After a call that removes anything the colours are dropped"),
        ("a refused call leaves everything", 537, "a call that fails leaves the mesh, normals, regions, colours and any earlier support array"),
        ("bad arguments, no mesh, facing without normals: INVALID_ARGUMENT", 538, "DMI_ERR_INVALID_ARGUMENT: null pointers; min_views < 0"),
        ("no views: STATE, after the argument checks", 539, "DMI_ERR_STATE: no views resident"),
        ("an empty mesh without views is STATE", 540, "an empty mesh in a context without views is DMI_ERR_STATE"),
        ("the counts are those of the mesh as the call left it", 544, "one count per vertex of the mesh as that call left it"),
    ],
    "color": [
        ("a failed colouring leaves the colours", 668, "A call that fails leaves mesh, normals, regions and"),
        ("plain: the colour context's own settings, its depth test included", 670, "fused_depth_test == 0: bit for bit what dmi_color_process"),
        ("own depth test with a view without planes: INVALID_ARGUMENT", 652, "dmi_color_process fails with DMI_ERR_INVALID_ARGUMENT if a"),
        ("fused: the thresholded fusion depth", 676, "REPLACED BY -1 WHERE ITS BEST COST EXCEEDED THE THRESHOLD"),
        ("no mesh, bad fused tolerance, own test on, view counts unequal: INVALID_ARGUMENT", 683, "DMI_ERR_INVALID_ARGUMENT: null c, ctx or n_vertices; no successful extraction yet"),
        ("no views in the colour context: STATE; an empty mesh is a success", 685, "DMI_ERR_STATE: no views in c"),
    ],
    "render": [
        ("the planes of every view are replaced", 699, "EVERY view resident in `c`"),
        ("no triangles: every plane empty", 721, "n_triangles == 0 is a success that leaves every plane empty"),
        ("no mesh INVALID_ARGUMENT, no views STATE", 723, "refusals as dmi_color_process_isosurface (no extraction yet"),
        ("downloaded as vtk rows, -1 where empty", 726, "-1 where the plane is +inf"),
    ],
    "download": [
        ("the mesh: INVALID_ARGUMENT before any successful extraction", 291, "DMI_ERR_INVALID_ARGUMENT before any successful extraction"),
        ("normals: refused after a plain extraction", 306, "when the last successful one was a plain dmi_extract_isosurface"),
        ("regions: refused when no filter has run", 338, "when no filter has run since the last one"),
        ("support: refused when the mesh has changed", 544, "Refused"),
        ("colours: refused when dropped", 667, "dmi_download_isosurface_colors is then"),
    ],
    "grid": [
        ("reset_grid zeroes the grid", 177, "Zero the grid"),
        ("the mesh is replaced by the next extraction only", 331, "the next extraction replaces it"),
    ],
}


class ModelRefusal(Exception):
    """The library refuses this call (DmiError there, with this code); the model is unchanged."""

    def __init__(self, code, why=""):
        super().__init__(f"{code}: {why}")
        self.code = int(code)


def _finite(x):
    return bool(np.isfinite(x))


class MeshSequenceModel:
    def __init__(self, grid, ray=None, weights=PS.weights_np):
        """weights(sigma, truncate): the Gaussian's k_0..k_r.  point_smooth_np.weights_np restates the formula, but the library is the
        authority on these numbers (one libm's exp differs from another's in the last bit; dmi.h:243): a model that is compared with
        the library is given capi.point_smoothing_weights, pure host code, as tests/test_point_smoothing.py gives it to the restatement."""
        self.grid_desc, self.ray, self.weights = grid, ray, weights
        nx, ny, nz = (int(c) for c in grid.cell_dims)
        self.shape = (nz, ny, nx)
        self.cells = np.zeros(self.shape)
        self.sigma, self.truncate = np.zeros(3), 3.0
        self.vertices = self.triangles = self.normals = None     # vertices None: no successful extraction yet
        self.regions = self.support_counts = self.colors = None  # (region_id, region_size); [V] i32; (mean, median, count)
        self.depth = self.K4 = self.RT4 = None                   # the resident views, depths thresholded
        self.c_colors = self.c_K4 = self.c_RT4 = self.c_planes = None   # the colour context (planes in vtk rows, None: no planes)
        self.c_test = None                                       # its own depth test: None off, else the tolerance

    # ---- the fusion context's views and grid
    @property
    def n_views(self):
        return 0 if self.depth is None else int(self.depth.shape[0])

    def add_views(self, views, threshold=None):
        assert self.depth is None, "one batch per context is all the mesh sequences need"
        depth = np.array(views.depth, dtype=np.float64)
        if views.best_cost is not None and threshold is not None:
            depth = np.where(views.best_cost > threshold, -1.0, depth)   # (RD.cxx:138-167, as tests/test_isosurface_support.py)
        self.depth, self.K4, self.RT4 = depth, np.array(views.K4, dtype=np.float64), np.array(views.RT4, dtype=np.float64)

    def clear_views(self):
        self.depth = self.K4 = self.RT4 = None

    def reset_grid(self):
        self.cells = np.zeros(self.shape)

    def upload_grid(self, cells):
        self.cells = np.array(cells, dtype=np.float64).reshape(self.shape)

    def fuse(self):
        if self.n_views == 0:
            raise ModelRefusal(STATE, "no views resident")
        g, r = self.grid_desc, self.ray
        self.cells = oracle_np.fuse(g.cell_dims, g.origin, g.spacing, g.grid_matrix, r.thickness, r.rho, r.eta, r.delta,
                                    self.depth, self.K4, self.RT4, init_grid=self.cells)[0]

    # ---- point data
    def set_point_smoothing(self, sigma, truncate=3.0):
        s = np.array(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (3,)))
        if not (np.isfinite(s).all() and (s >= 0).all() and _finite(truncate) and 0 < truncate <= 4):
            raise ModelRefusal(INVALID_ARGUMENT, "sigma or truncate outside the definition")
        if any(PS.radius(float(x), float(truncate)) > 16 for x in s):
            raise ModelRefusal(INVALID_ARGUMENT, "a radius above 16")
        self.sigma, self.truncate = s, float(truncate)

    def point_data(self):
        P = oracle_np.cell_to_point_np(self.cells)
        if (self.sigma > 0).any():
            P = PS.smooth(P, [self.weights(float(x), self.truncate) if x > 0 else np.ones(1) for x in self.sigma])
        return P

    # ---- the mesh
    @property
    def has_mesh(self):
        return self.vertices is not None

    @property
    def counts(self):
        return (len(self.vertices), len(self.triangles))

    def _need_mesh(self):
        if not self.has_mesh:
            raise ModelRefusal(INVALID_ARGUMENT, "no mesh")

    def _set_mesh(self, v, t, n):
        self.vertices = np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 3)
        self.triangles = np.ascontiguousarray(t, dtype=np.int64).reshape(-1, 3)
        self.normals = None if n is None else np.ascontiguousarray(n, dtype=np.float32).reshape(-1, 3)

    def extract(self, iso, normals=False):
        if iso != iso:
            raise ModelRefusal(INVALID_ARGUMENT, "the iso-value is a NaN")
        g = self.grid_desc
        P, M = self.point_data(), np.asarray(g.grid_matrix, dtype=np.float64)
        if normals:
            self._set_mesh(*N.extract_with_normals(P, iso, g.origin, g.spacing, M))
        else:
            self._set_mesh(*R.extract(P, iso, g.origin, g.spacing, M), None)
        self.regions = self.support_counts = self.colors = None
        return self.counts

    def filter_components(self, mode="min_triangles", min_triangles=0):
        self._need_mesh()
        out = C.filter_mesh(self.vertices, self.triangles, self.normals, {"min_triangles": C.MIN_TRIANGLES, "largest": C.LARGEST}[mode],
                            min_triangles)
        self._set_mesh(out["vertices"], out["triangles"], out["normals"])
        self.regions = (np.ascontiguousarray(out["region_id"], dtype=np.int64), np.ascontiguousarray(out["region_size"], dtype=np.int64))
        self.support_counts = self.colors = None
        return tuple(int(x) for x in out["counts"])

    def smooth(self, iterations, lam=0.5, mu=-0.53):
        if not (0 <= iterations <= 1000 and _finite(lam) and 0 < lam <= 1 and _finite(mu) and mu <= 0):
            raise ModelRefusal(INVALID_ARGUMENT, "iterations, lambda or mu outside the definition")
        self._need_mesh()
        if iterations == 0:
            return
        v, n = SM.smooth(self.vertices, self.triangles, iterations, lam, mu, self.normals)
        self._set_mesh(v, self.triangles, n)
        self.support_counts = self.colors = None

    def decimate(self, cell_size, placement="mean"):
        if not (_finite(cell_size) and cell_size > 0):
            raise ModelRefusal(INVALID_ARGUMENT, "cell_size is not a finite number > 0")
        self._need_mesh()
        try:
            if placement == "mean":
                out = D.decimate(self.vertices, self.triangles, cell_size, self.normals)
            else:
                out = Q.decimate(self.vertices, self.triangles, cell_size, self.normals)
        except ValueError as e:    # a non-finite coordinate, more than 2^21 bins
            raise ModelRefusal(INVALID_ARGUMENT, str(e))
        self._set_mesh(*out)
        self.regions = self.support_counts = self.colors = None
        return self.counts

    def fill(self, max_edges):
        if max_edges > 1 << 20:
            raise ModelRefusal(INVALID_ARGUMENT, "max_edges above 2^20")
        self._need_mesh()
        out = H.fill(self.vertices, self.triangles, max_edges, self.normals)
        if out["n_filled"]:
            self._set_mesh(out["vertices"], out["triangles"], out["normals"])
            self.regions = self.support_counts = self.colors = None
        return self.counts + (int(out["n_filled"]), int(out["boundary_edges_left"]))

    def support(self, min_views, tolerance, facing=True):
        if min_views < 0:
            raise ModelRefusal(INVALID_ARGUMENT, "min_views is negative")
        if not (_finite(tolerance) and tolerance >= 0):
            raise ModelRefusal(INVALID_ARGUMENT, "the tolerance must be finite and >= 0")
        self._need_mesh()
        if facing and self.normals is None:
            raise ModelRefusal(INVALID_ARGUMENT, "require_facing needs normals")
        if self.n_views == 0:
            raise ModelRefusal(STATE, "no views resident")
        counts = S.support(self.vertices, self.normals, self.depth, self.K4, self.RT4, tolerance, facing)
        v, t, n = S.filter_mesh(self.vertices, self.triangles, self.normals, counts, min_views)
        if (len(v), len(t)) != self.counts:   # something went; the counts that stay are those of the vertices that stay
            keep = np.zeros(len(self.vertices), dtype=bool)
            keep[self.triangles[(counts[self.triangles] >= min_views).all(axis=1)].reshape(-1)] = True
            assert int(keep.sum()) == len(v)
            counts = counts[keep]
            self._set_mesh(v, t, n)
            self.regions = self.colors = None
        self.support_counts = np.ascontiguousarray(counts, dtype=np.int32)
        return self.counts

    # ---- the colour context
    @property
    def c_n_views(self):
        return 0 if self.c_colors is None else int(self.c_colors.shape[0])

    def c_add_views(self, colors, K4, RT4, depths=None):
        assert self.c_colors is None
        self.c_colors, self.c_K4, self.c_RT4 = np.asarray(colors), np.array(K4, dtype=np.float64), np.array(RT4, dtype=np.float64)
        self.c_planes = None if depths is None else np.array(depths, dtype=np.float64)

    def c_set_depth_test(self, enable, tolerance=0.0):
        if not (_finite(tolerance) and tolerance >= 0):
            raise ModelRefusal(INVALID_ARGUMENT, "the tolerance must be finite and >= 0")
        self.c_test = float(tolerance) if enable else None

    def color(self, fused_depth_tolerance=None):
        self._need_mesh()
        fused = fused_depth_tolerance is not None
        reasons = set()
        if fused:
            if not (_finite(fused_depth_tolerance) and fused_depth_tolerance >= 0):
                reasons.add(INVALID_ARGUMENT)
            if self.c_test is not None:
                reasons.add(INVALID_ARGUMENT)
            if self.c_n_views > 0 and (self.n_views != self.c_n_views or self.depth.shape[1:] != self.c_colors.shape[1:3]):
                reasons.add(INVALID_ARGUMENT)
        if self.c_n_views == 0:
            reasons.add(STATE)
        if not fused and self.c_test is not None and self.c_planes is None and self.c_n_views > 0:
            assert len(self.vertices) > 0, "the header does not decide this call (see the module's docstring)"
            reasons.add(INVALID_ARGUMENT)
        if reasons:
            assert len(reasons) == 1 or (fused and self.n_views == 0 and self.c_n_views == 0), "the header does not order these refusals"
            raise ModelRefusal(STATE if STATE in reasons else INVALID_ARGUMENT, "colouring refused")
        if fused:
            depths, tol = self.depth, float(fused_depth_tolerance)
        else:
            depths, tol = self.c_planes, self.c_test
        self.colors = tuple(np.ascontiguousarray(a) for a in CD.color_mesh_depth_np(self.vertices, self.c_colors, depths, self.c_K4, self.c_RT4, tol))
        return len(self.vertices)

    def render(self):
        self._need_mesh()
        if self.c_n_views == 0:
            raise ModelRefusal(STATE, "no views resident in the colour context")
        H_, W_ = self.c_colors.shape[1:3]
        self.c_planes = MD.to_vtk_depths(MD.render_depths_np(self.vertices, self.triangles, self.c_K4, self.c_RT4, W_, H_))

    # ---- what can be read back
    def download_mesh(self):
        self._need_mesh()
        return self.vertices, self.triangles

    def download_normals(self):
        self._need_mesh()
        if self.normals is None:
            raise ModelRefusal(INVALID_ARGUMENT, "the mesh has no normals")
        return self.normals

    def download_regions(self):
        self._need_mesh()
        if self.regions is None:
            raise ModelRefusal(INVALID_ARGUMENT, "no regions")
        return self.regions

    def download_support(self):
        self._need_mesh()
        if self.support_counts is None:
            raise ModelRefusal(INVALID_ARGUMENT, "no counts")
        return self.support_counts

    def download_colors(self):
        self._need_mesh()
        if self.colors is None:
            raise ModelRefusal(INVALID_ARGUMENT, "no colours")
        return self.colors

    def digest(self):
        """Every array the model holds, as bytes (for the determinism test)."""
        parts = [self.cells, self.sigma, self.vertices, self.triangles, self.normals, self.support_counts, self.c_planes]
        parts += list(self.regions or (None, None)) + list(self.colors or (None, None, None))
        return tuple(None if a is None else (a.shape, a.dtype.str, a.tobytes()) for a in parts)
