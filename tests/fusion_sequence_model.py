"""A fusion context as a caller sees it, replayed on the CPU: the grid, the hit counters and the resident views, each operation of
capi.FusionContext answered with the C oracle (oracle.fuse with the model's grid as init_grid, oracle.cell_to_point).  The model
holds no flag of the library's -- no deferred fill, no "layer is zero", no "free of -0.0", no record capacity --: it is what those
flags must never change.  tests/test_fusion_sequence_model.py checks it against itself, tests/test_gpu_sequence_fuzz.py runs
sequences of operations through a context and through the model and compares what can be read back.

  fuse(first, count)   oracle.fuse of those views onto the model grid.
  fuse_slab(z0, zc)    the same whole-grid oracle call over every resident view, of which only layers [z0, z0 + zc) are taken -- grid
                       and voxel hits.  Voxels are independent of each other, and the grid's origin is not moved (another origin
                       would round the voxel centres differently).  The views' hit counts of a slab step: one single-view oracle
                       call per view, its voxel hits summed over the slab's layers (only when the model counts hits).
  f32 grid             the model keeps the f32 values (as f64 numbers); a call widens them, fuses in f64 and rounds once to f32:
                       the rule tests/test_gpu_parity.py::test_f32_grid_is_one_rounding_away pins for one call.  That is one
                       rounding per LAUNCH, so f32 sequences keep to views of one K kind (one launch per call).  The library stores
                       +0.0f for either zero (test_f32_grid_never_stores_negative_zero); the model does not follow that: f32 grids
                       are compared by value (same_grid), f64 grids bit for bit.
  reset_grid           +0.0 everywhere, voxel and view hit counters zero (include/dmi.h: "Zero the grid (and the hit counters)").
  upload_grid          replaces the grid (rounded to f32 for an f32 grid); the hit counters stay.
  clear_views          no view is resident.  include/dmi.h says nothing about the hit counters here: the voxel counters go on
                       counting (nothing but reset_grid zeroes them), and what the VIEWS' counters hold for the views added next is
                       not stated -- map_hits_known turns False and the views' counts are left out of every comparison until the
                       next reset_grid.
  refused calls        a range outside the resident views, a fuse without views, a slab off the alignment: ModelRefusal, and
                       nothing has changed.

The model asserts nothing about the reference beyond what the oracle does."""
import numpy as np

from oracle import oracle

SLAB_ALIGNMENT = 32   # DMI_SLAB_ALIGNMENT (include/dmi.h)


class ModelRefusal(Exception):
    """The library refuses this call (DmiError there); the model is unchanged."""


class FusionSequenceModel:
    def __init__(self, grid, ray, grid_dtype="f64", count_hits=False):
        self.grid_desc, self.ray, self.grid_dtype, self.count_hits = grid, ray, grid_dtype, bool(count_hits)
        nx, ny, nz = (int(c) for c in grid.cell_dims)
        self.shape = (nz, ny, nx)
        self.grid = np.zeros(self.shape)
        self.voxel_hits = np.zeros(self.shape, dtype=np.uint32)
        self.map_hits = np.zeros(0, dtype=np.uint64)
        self.map_hits_known = True
        self._clear()

    # ---- views
    def _clear(self):
        self.depth = self.K4 = self.RT4 = None   # [n, H, W] thresholded f64, [n, 4, 4], [n, 4, 4]

    @property
    def n_views(self):
        return 0 if self.depth is None else int(self.depth.shape[0])

    def add_views(self, views, threshold=None):
        depth = np.array(views.depth, dtype=np.float64)
        if views.best_cost is not None and threshold is not None:
            depth = oracle.apply_depth_threshold(depth, views.best_cost, float(threshold)).reshape(depth.shape)
        if self.depth is None:
            self.depth, self.K4, self.RT4 = depth, np.array(views.K4, dtype=np.float64), np.array(views.RT4, dtype=np.float64)
        else:
            if self.depth.shape[1:] != depth.shape[1:]:
                raise ModelRefusal("all views of a context share W and H")
            self.depth = np.concatenate([self.depth, depth])
            self.K4 = np.concatenate([self.K4, views.K4])
            self.RT4 = np.concatenate([self.RT4, views.RT4])
        self.map_hits = np.concatenate([self.map_hits, np.zeros(depth.shape[0], dtype=np.uint64)])

    def clear_views(self):
        self._clear()
        self.map_hits = np.zeros(0, dtype=np.uint64)
        self.map_hits_known = False

    # ---- grid
    def _stored(self, g):
        return g.astype(np.float32).astype(np.float64) if self.grid_dtype == "f32" else g

    def reset_grid(self):
        self.grid = np.zeros(self.shape)
        self.voxel_hits[...] = 0
        self.map_hits[...] = 0
        self.map_hits_known = True

    def upload_grid(self, g):
        self.grid = self._stored(np.array(g, dtype=np.float64).reshape(self.shape))

    def _params(self):
        g, r = self.grid_desc, self.ray
        return oracle.make_params(g.cell_dims, g.origin, g.spacing, g.grid_matrix, r.thickness, r.rho, r.eta, r.delta,
                                  self.depth.shape[2], self.depth.shape[1])

    def _check_range(self, first, count):
        n = self.n_views
        if first < 0 or count < 0 or first > n or count > n - first:
            raise ModelRefusal("range outside the resident views")

    def _fuse(self, first, count, z0, zc):
        sl = slice(first, first + count)
        g, vh, mh = oracle.fuse(self._params(), self.depth[sl], self.K4[sl], self.RT4[sl], init_grid=self.grid, n_threads=oracle.max_threads())
        z = slice(z0, z0 + zc)
        self.grid = self.grid.copy()
        self.grid[z] = self._stored(g[z])
        if not self.count_hits:
            return
        self.voxel_hits[z] += vh[z]
        if (z0, zc) == (0, self.shape[0]):
            self.map_hits[sl] += mh
        else:
            for m in range(first, first + count):   # a view's hits inside the slab: its own voxel hits there
                one = oracle.fuse(self._params(), self.depth[m:m + 1], self.K4[m:m + 1], self.RT4[m:m + 1])[1]
                self.map_hits[m] += np.uint64(one[z].sum(dtype=np.uint64))

    def fuse(self, first=None, count=None):
        if self.n_views == 0:
            raise ModelRefusal("no views resident")
        first, count = (0, self.n_views) if first is None else (int(first), int(count))
        self._check_range(first, count)
        if count > 0:
            self._fuse(first, count, 0, self.shape[0])

    def fuse_slab(self, z0, zc):
        nz = self.shape[0]
        if z0 < 0 or zc < 0 or z0 > nz or zc > nz - z0:
            raise ModelRefusal("layers outside the grid")
        if z0 % SLAB_ALIGNMENT != 0 or (z0 + zc != nz and (z0 + zc) % SLAB_ALIGNMENT != 0):
            raise ModelRefusal("slab boundaries off the alignment")
        if zc == 0:
            return
        if self.n_views == 0:
            raise ModelRefusal("no views resident")
        self._fuse(0, self.n_views, z0, zc)

    def fuse_download(self, first, count):
        """dmi_fuse_range_download: in however many slabs, the bits of fuse(first, count) and a download; count == 0 is a plain
        download and needs no view."""
        self._check_range(int(first), int(count))
        if count > 0:
            self._fuse(int(first), int(count), 0, self.shape[0])
        return self.grid

    def point_data(self):
        return oracle.cell_to_point(self.grid)


def same_grid(got, model):
    """The comparison of a downloaded grid with the model's: an f64 grid bit for bit (a NaN by a NaN), an f32 grid by value."""
    got = np.ascontiguousarray(got)
    if got.dtype == np.float32:
        want = model.grid.astype(np.float32)
        return got.shape == want.shape and bool(np.all((got == want) | (np.isnan(got) & np.isnan(want))))
    a, b = got.astype(np.float64, copy=False), np.ascontiguousarray(model.grid)
    return a.shape == b.shape and bool(np.all((np.isnan(a) & np.isnan(b)) | (a.view(np.uint64) == b.view(np.uint64))))
