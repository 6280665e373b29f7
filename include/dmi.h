/*
 * dmi.h -- C ABI of the MI355X-native depth-map-integration (TSDF fusion) path.
 *
 * This is the drop-in boundary for ONE path of bastienjacquet/CudaDepthMapIntegration:
 * the two free functions that vtkCudaReconstructionFilter forward-declares and calls
 * (Reconstruction/vtkCudaReconstructionFilter.cxx:65-71, :171-176), defined in
 * Reconstruction/CudaReconstruction.cu:
 *
 *     void CudaInitialize(vtkMatrix4x4*, int dims[3], double orig[3], double spacing[3],
 *                         double thick, double rho, double eta, double delta, int depthDims[2]);   cu:269-298
 *     template<class T> bool ProcessDepthMap(std::vector<std::string> vti, std::vector<std::string> krtd,
 *                         double thresholdBestCost, vtkDoubleArray* io_scalar);                     cu:302-386
 *
 * Those take VTK objects and file names and do disk I/O inside the GPU loop.  Here the seam
 * is split: the host side (VTK or the VTK-free mirror in cudadepthmapintegration_amd/csrc/host)
 * loads or generates the views; this library only sees plain pointers and sizes.
 *
 * Conventions (all taken from the reference):
 *   - the voxel grid is the CELL grid of the filter's input vtkImageData: cell_dims = point
 *     dims - 1 (filt.cxx:123-124, cu:128-133, cu:330-331); linear voxel id = (k*ny + j)*nx + i,
 *     x fastest (cu:126-134) = vtk cell-id order of the "reconstruction_scalar" array (filt.cxx:129-135);
 *   - 4x4 matrices are row-major as vtkMatrix4x4 / cu:220-230; only rows 0..2 are used (cu:88-93);
 *   - a depth table is W*H values in vtkImageData point order: row 0 is the BOTTOM image row
 *     (cu:141-149); the value -1 means "no depth" (cu:202; Sources/ReconstructionData.cxx:164);
 *   - arithmetic is IEEE fp64 in the reference's expression order, every multiply and add rounded
 *     separately; results are bit-identical to oracle/tsdf_oracle.c on one GPU with an f64 grid.
 *
 * Every function returns DMI_OK (0) or a dmi_status error code and never calls exit()
 * (the reference's gpuAssert does, cu:68-76).  dmi_last_error() gives the message.
 * A context is not thread-safe; distinct contexts may be used from distinct threads
 * (the reference keeps global __constant__ state, cu:55-64, and is not re-entrant).
 */
#ifndef DMI_H_
#define DMI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMI_ABI_VERSION 5 /* 3: dmi_info grew (pixels_without_depth); dmi_iso_active_cells, DMI_EXCHANGE_PEER_COPY, dmi_multi_peer_chunk
                           * 4: dmi_get_window_pair_count, dmi_get_upload_kernel_ms, dmi_sizeof_info / dmi_sizeof_timings
                           * 5: dmi_get_view_paths; later, additions only: dmi_extract_isosurface,
                           *    dmi_download_isosurface, dmi_get_isosurface_kernel_ms; dmi_extract_isosurface_normals,
                           *    dmi_download_isosurface_normals; dmi_filter_isosurface_components, dmi_download_isosurface_regions,
                           *    dmi_get_isosurface_filter_kernel_ms, dmi_get_isosurface_filter_pass_ms,
                           *    dmi_get_isosurface_filter_cas_retries; dmi_smooth_isosurface, dmi_get_isosurface_smooth_kernel_ms,
                           *    dmi_get_isosurface_smooth_pass_ms; dmi_decimate_isosurface, dmi_get_isosurface_decimate_kernel_ms,
                           *    dmi_get_isosurface_decimate_pass_ms; dmi_color_process_isosurface, dmi_download_isosurface_colors,
                           *    dmi_get_isosurface_color_kernel_ms; dmi_filter_isosurface_support, dmi_download_isosurface_support,
                           *    dmi_get_isosurface_support_kernel_ms, dmi_get_isosurface_support_pass_ms;
                           *    dmi_decimate_isosurface_placed; dmi_filter_depth_consistency;
                           *    dmi_estimate_scene_bounds; dmi_fill_isosurface_holes, dmi_get_isosurface_holes_kernel_ms,
                           *    dmi_get_isosurface_holes_pass_ms; dmi_point_smoothing_weights, dmi_set_point_smoothing,
                           *    dmi_get_point_smoothing, dmi_get_point_smoothing_kernel_ms; dmi_filter_depth_speckles;
                           *    dmi_fill_depth_holes; dmi_depth_smoothing_weights, dmi_smooth_depths; dmi_views_build_points, dmi_views_download_points, dmi_views_get_points_pass_ms; dmi_thin_point_cloud, dmi_views_thin_points, dmi_views_download_point_members, dmi_views_get_thin_pass_ms, dmi_views_set_thin_wave_cell_points; dmi_count_point_neighbors, dmi_views_filter_points_radius, dmi_views_download_point_neighbors, dmi_views_get_radius_pass_ms, dmi_views_set_radius_group_points; dmi_fit_point_planes, dmi_views_fit_point_planes, dmi_views_download_point_plane_rms, dmi_views_get_plane_fit_pass_ms */

typedef struct dmi_context dmi_context;

typedef enum dmi_status {
  DMI_OK = 0,
  DMI_ERR_INVALID_ARGUMENT = 1,
  DMI_ERR_DEVICE = 2, /* a HIP runtime call failed; message holds hipGetErrorString */
  DMI_ERR_OUT_OF_MEMORY = 3,
  DMI_ERR_STATE = 4 /* call order violated, e.g. fuse with no views */
} dmi_status;

typedef enum dmi_dtype { DMI_F32 = 0, DMI_F64 = 1 } dmi_dtype;

/* How depth tables are kept in HBM.  AUTO keeps f32 while every uploaded depth is exactly
 * representable in f32 (then f32 storage changes no result bit) and promotes the store to
 * f64 the moment one is not. */
typedef enum dmi_depth_storage { DMI_DEPTH_AUTO = 0, DMI_DEPTH_F32 = 1, DMI_DEPTH_F64 = 2 } dmi_depth_storage;

/* Replaces the grid part of CudaInitialize's arguments (cu:269-272) = the reference's
 * __constant__ c_gridMatrix / c_gridDims / c_gridOrig / c_gridSpacing (cu:55-58). */
typedef struct dmi_grid_desc {
  int32_t cell_dims[3];   /* voxels per axis (vtk point dims - 1) */
  double origin[3];       /* vtkImageData origin (filt.cxx:121-122) */
  double spacing[3];      /* vtkImageData spacing (filt.cxx:125-126) */
  double grid_matrix[16]; /* row-major 4x4, rows = gridVecX/Y/Z (Reconstruction/main.cxx:345-359) */
} dmi_grid_desc;

/* Replaces c_rayPotentialThick/Rho/Eta/Delta (cu:60-63; CudaInitialize cu:273-276). */
typedef struct dmi_ray_potential {
  double thickness;
  double rho;
  double eta;
  double delta;
} dmi_ray_potential;

typedef struct dmi_options {
  int32_t device;         /* HIP device ordinal */
  int32_t grid_dtype;     /* dmi_dtype of the device grid.  DMI_F64 = the reference's contract
                             (ProcessDepthMap<double>, filt.cxx:175); DMI_F32 rounds once per fuse */
  int32_t depth_storage;  /* dmi_depth_storage */
  int32_t count_hits;     /* != 0: keep per-voxel u32 and per-map u64 hit counters (not a reference
                             output; they expose every in-frustum / sentinel decision for parity) */
  int32_t kernel_variant; /* 0 = default; bit field of tuning / test switches (DESIGN.md "kernel_variant"):
                             1 exact division in the general kernel, 2 ignore K structure, 4|8 block shape of
                             the general kernel, 16 never use the tiled kernel, 32..224 tile shape, 256.. the tiled kernel's
                             switches */
  int32_t z_first;        /* this context's grid is the z-slab [z_first, z_first + cell_dims[2]) of a taller grid
                             with the same origin and spacing: voxel k has the centre of global cell z_first + k
                             (cu:78-83 with the global index), so slabs fused on different GPUs are bit-identical
                             to one fusion of the whole grid.  0 = the whole grid */
  void *stream;           /* hipStream_t to run on; NULL = a stream owned by the context */
  void *external_grid;    /* device pointer to a caller-owned grid of grid_dtype[n_voxels]
                             (e.g. a torch tensor that is later all-reduced); NULL = context-owned */
} dmi_options;

typedef struct dmi_timings {
  double last_fuse_kernel_ms; /* hipEvent time of all launches of the last dmi_fuse, on its stream */
  double total_fuse_kernel_ms;
  uint64_t fuse_launches;
  double last_upload_ms; /* host wall time of the last dmi_add_views (copy + convert, synchronised) */
  double last_download_ms; /* host wall time of the last download; for dmi_fuse_range_download the whole call: its slabs' fusions
                              and their copies, which overlap */
  double last_cell_to_point_ms; /* hipEvent time of the last dmi_cell_to_point kernel */
  /* of last_fuse_kernel_ms / total_fuse_kernel_ms, the fusion kernel proper (without the brick classification, the window
   * origins and the workgroup ordering that precede it).  A launch without brick classes -- at most 1024 bricks and fewer than 48
   * views -- is timed as a whole, its one table kernel included: the two are equal then */
  double last_fuse_main_kernel_ms;  /* (a launch without brick classes -- at most 1024 bricks -- is timed as a whole: its one table
                                       kernel included, = last_fuse_kernel_ms) */
  double total_fuse_main_kernel_ms;
} dmi_timings;

typedef struct dmi_info {
  int64_t n_voxels;
  int32_t n_views;
  int32_t depth_width;
  int32_t depth_height;
  int32_t depth_storage_in_use; /* DMI_DEPTH_F32 or DMI_DEPTH_F64 */
  int32_t grid_dtype;
  int32_t k_mode; /* 0 general 4x4 K rows, 1 pinhole with skew, 2 pinhole (chosen from the uploaded Ks) */
  int32_t kernel_variant;
  int32_t tiled_kernel; /* 1: the resident views and the grid meet the preconditions of the register-tiled
                           kernel (axis-aligned grid matrix, pinhole K), 0: the general kernel runs */
  uint64_t device_bytes; /* HBM held by the context */
  uint64_t pixels_without_depth; /* of the resident depth tables, after the best-cost threshold (cu:202's -1; counted on the
                                    device at upload) */
} dmi_info;

/* Fills *opt with the defaults: device 0, f64 grid, AUTO depth storage, no hit counters. */
void dmi_default_options(dmi_options *opt);

/* Replaces CudaInitialize (cu:269-298) and the grid cudaMalloc of ProcessDepthMap (cu:326).
 * The grid starts zero-filled, as RequestData fills it (filt.cxx:133).  opt may be NULL. */
int dmi_create(const dmi_grid_desc *grid, const dmi_ray_potential *ray, const dmi_options *opt, dmi_context **out);

/* Replaces the cudaFree/delete block (cu:374-381). */
void dmi_destroy(dmi_context *ctx);

/* Message of the last failing call on ctx; ctx == NULL gives the calling thread's last
 * dmi_create failure.  Never NULL.  Replaces gpuAssert's fprintf+exit (cu:68-76). */
const char *dmi_last_error(const dmi_context *ctx);

/* Replaces the per-depth-map body of ProcessDepthMap (cu:347-360): best-cost threshold
 * (ReconstructionData::ApplyDepthThresholdFilter, RD.cxx:138-167: best_cost > threshold => depth = -1;
 * skipped when best_cost == NULL), marshalling (cu:351-353) and the three H2D copies (cu:358-360).
 * Appends n views; they stay resident in HBM until dmi_clear_views.
 *   depth     [n][H][W] f64 host, vtk point order        ("Depths" array, cu:249)
 *   best_cost [n][H][W] f64 host or NULL                 ("Best Cost Values", RD.cxx:146)
 *   K4, RT4   [n][16]   f64 host, row-major 4x4          (Get4MatrixK / GetMatrixTR, RD.cxx:128-136)
 * All views of a context share W and H (the reference reads them from map 0 only, filt.cxx:167-168). */
int dmi_add_views(dmi_context *ctx, const double *depth, const double *best_cost, double threshold, const double *K4,
                  const double *RT4, int32_t n, int32_t width, int32_t height);

/* Same with f32 depth tables (already thresholded or best_cost given as f32 == NULL only). */
int dmi_add_views_f32(dmi_context *ctx, const float *depth, const double *K4, const double *RT4, int32_t n,
                      int32_t width, int32_t height);

int dmi_clear_views(dmi_context *ctx);

/* Zero the grid (and the hit counters): filt.cxx:133. */
int dmi_reset_grid(dmi_context *ctx);

/* Start from a caller-supplied grid, as ProcessDepthMap uploads io_scalar before accumulating
 * onto it (cu:323-327).  grid: n_voxels f64 host, x fastest. */
int dmi_upload_grid(dmi_context *ctx, const double *grid);

/* Replaces the kernel launches of the depth-map loop (cu:363, one per map in the reference):
 * fuses every resident view into the grid, each voxel accumulated in view order (cu:211).
 * Asynchronous on the context's stream. */
int dmi_fuse(dmi_context *ctx);

/* Fuse only views [first, first+count): lets a caller shard or batch the resident views. */
int dmi_fuse_range(dmi_context *ctx, int32_t first, int32_t count);

/* Fuse every resident view into the cell layers [z_first, z_first + z_count) only.  Lets a caller pipeline a
 * fusion with what consumes the grid (bench.py overlaps the RCCL all-reduce of slab i with the fusion of slab
 * i+1).  Slabs fused one after the other give the same bits as one dmi_fuse.  z_first and z_first + z_count
 * must be multiples of DMI_SLAB_ALIGNMENT or the end of the grid. */
#define DMI_SLAB_ALIGNMENT 32
int dmi_fuse_slab(dmi_context *ctx, int32_t z_first, int32_t z_count);

int dmi_synchronize(dmi_context *ctx);

/* Replace the D2H copy and the per-tuple copy into io_scalar (cu:368-371).  They synchronise.  When the requested type
 * is not the grid's, the conversion runs on the device and the host side is plain copies: `out` in pinned memory
 * (dmi_alloc_pinned, or a buffer the caller registered) is filled at DMA speed, pageable memory at the runtime's
 * staging speed.  The same holds for dmi_upload_grid into an f32 grid. */
int dmi_download_grid_f64(dmi_context *ctx, double *out);
int dmi_download_grid_f32(dmi_context *ctx, float *out);

/* The last step of a chunked reconstruction in one call (cu:343-371: the last maps' kernels, then the copy back): fuse views
 * [first, first + count) -- count may be 0 -- and bring the whole grid to `out` (out_dtype: DMI_F32 or DMI_F64; [n_voxels], pinned
 * memory for DMA speed).  When out_dtype is the grid's own type the grid is fused in n_slabs z-slabs (clamped to 1 .. the number of
 * DMI_SLAB_ALIGNMENT units of the grid) and every slab's copy starts when its fusion ends, on a stream of its own, under the
 * fusion of the next slabs: at 512^3 the copy (9-19 ms) hides all of the fusion but its first slab.  Bit for bit what
 * dmi_fuse_range + dmi_download_grid_* return.  Synchronises.  (Added in round 4; dmi_abi_version() stays 4.) */
int dmi_fuse_range_download(dmi_context *ctx, int32_t first, int32_t count, void *out, int32_t out_dtype, int32_t n_slabs);

/* voxel_hits [n_voxels] u32 and/or map_hits [n_views] u64 (either may be NULL).
 * Needs count_hits at creation.  A view added since the last fusion reads 0; the views before it keep their counts. */
int dmi_download_hits(dmi_context *ctx, uint32_t *voxel_hits, uint64_t *map_hits);

/* Device pointer of the grid (context-owned or external) for zero-copy consumers. */
int dmi_grid_device_pointer(dmi_context *ctx, void **ptr);

/* The step right after the filter in the reference's CLI (Reconstruction/main.cxx:151-155): vtkCellDataToPointData
 * over "reconstruction_scalar".  Point (i, j, k) of the (nx+1)(ny+1)(nz+1) lattice gets the mean of its 1..8
 * adjacent cells, accumulated as VTK does (w = 1/count; c += w*v in vtkStructuredData::GetPointCells order), f64.
 * dmi_cell_to_point runs the kernel on the context's stream into a context-owned device buffer (asynchronous);
 * dmi_download_point_data_f64 runs it if the grid changed since, then copies (nx+1)(ny+1)(nz+1) doubles, x fastest,
 * to `out` and synchronises; dmi_point_data_device_pointer hands the device buffer to a zero-copy consumer. */
int dmi_cell_to_point(dmi_context *ctx);
int dmi_download_point_data_f64(dmi_context *ctx, double *out);
int dmi_point_data_device_pointer(dmi_context *ctx, void **ptr);

/* A separable Gaussian over the point data, between dmi_cell_to_point and the contour: what a vtkImageGaussianSmooth in front of
 * vtkContourFilter does to the voxel-scale noise of the summed ray potentials (only the intent is shared with that filter, not the
 * numbers).  Additions to ABI 5, dmi_abi_version() stays 5; csrc/point_smooth.hip.  The input is the point data P on the lattice
 * (nx+1) x (ny+1) x (nz+1), x fastest, exactly what dmi_cell_to_point produces; the output Q has the same shape and REPLACES it
 * for every consumer.  Definition, met bit for bit:
 *   - sigma[3] in LATTICE STEPS, one per grid axis (not world units: the filter acts on the lattice), each finite and >= 0;
 *     truncate finite and in (0, 4];
 *   - the radius on axis a is r_a = (int)ceil(truncate * sigma[a]); r_a > 16 is refused; sigma[a] == 0 means the axis is skipped,
 *     and its pass is the identity on bits, not a multiplication by 1;
 *   - weights, on the host, f64: w_i = exp(-(double)(i*i) / (2*sigma*sigma)) for i = 0..r, S = w_0 + 2*(((w_1 + w_2) + ...) + w_r),
 *     k_i = w_i / S.  The library is the authority on these numbers (one libm's exp may differ from another's in the last bit):
 *     dmi_point_smoothing_weights returns them;
 *   - three passes, x then y then z, each over the full f64 result of the one before.  For a point with index q on the pass's axis,
 *     which has N points: v(t) = the value at clamp(t, 0, N-1) (the border replicated, so a constant field stays constant up to the
 *     rounding of the sum of the k); acc = k_0 * v(q); then for i = 1..r ascending acc = acc + k_i * (v(q-i) + v(q+i));
 *   - f64, every operation rounded, no FMA, no reassociation; NaN, +-inf and signed zeros come out as this arithmetic makes them.
 * dmi_point_smoothing_weights: pure host code, no device needed: *radius and weights[0..r] = k_0..k_r (room for 17) for one axis.
 * DMI_ERR_INVALID_ARGUMENT for a sigma, truncate or radius outside the definition and for null pointers.
 * dmi_set_point_smoothing is a SETTING of the context, not a one-shot filter: it stores the parameters and marks the point data
 * stale; from then on every computation of the point data (dmi_cell_to_point, and whatever runs it) is followed by the passes, and
 * dmi_download_point_data_f64, dmi_point_data_device_pointer, dmi_iso_active_cells, both extractions and the gradient normals
 * read Q.  All sigmas 0 switches it off: the state after dmi_create, bit-identical to a context in which it was never set.  While it
 * is on the context holds one more buffer of the point data's size.  Setting the values that are set already invalidates nothing.
 * DMI_ERR_INVALID_ARGUMENT, the old setting kept: null pointers, parameters outside the definition, and a context created with
 * dmi_options.z_first != 0 (a z-slab's lattice has the wrong borders, as for the extraction).
 * dmi_get_point_smoothing returns the setting (zeros and 3 after dmi_create).  dmi_get_point_smoothing_kernel_ms: hipEvent time of
 * the smoothing kernels of the last computation of the point data (dmi_timings.last_cell_to_point_ms stays the cell -> point kernel
 * alone); 0 while the setting is off.  Synchronises if that computation is still running. */
int dmi_point_smoothing_weights(double sigma, double truncate, int32_t *radius, double *weights /* [17]: k_0..k_r */);
int dmi_set_point_smoothing(dmi_context *ctx, const double sigma[3], double truncate);
int dmi_get_point_smoothing(dmi_context *ctx, double sigma[3], double *truncate);
int dmi_get_point_smoothing_kernel_ms(dmi_context *ctx, double *last);

/* The pre-pass of the step after that (Reconstruction/main.cxx:169-173: vtkContourFilter at `contour` over the point data,
 * i.e. marching cubes over every cell): which cells can produce triangles at all.  A corner is inside when its point value
 * is >= iso (the marching-cubes case bit; a NaN is outside); a cell is ACTIVE when it has both inside and outside corners.
 * *count receives the number of active cells; cell_ids (nullable) the first min(*count, capacity) of them as linear cell
 * ids (k*ny + j)*nx + i in ascending order -- the cells a host marching cubes has to visit, instead of all of them.  Runs
 * dmi_cell_to_point first if the grid changed.  Synchronises. */
int dmi_iso_active_cells(dmi_context *ctx, double iso, uint64_t *count, int64_t *cell_ids, uint64_t capacity);

/* Marching cubes over the point data at `iso` (the vtkContourFilter + vtkTransformFilter steps of
 * Reconstruction/main.cxx:166-182), on the device.  Runs dmi_cell_to_point first if the grid changed.  The mesh stays on
 * the device until the next call; *n_vertices / *n_triangles receive its size.  Synchronises.  (Added after round 5;
 * dmi_abi_version() stays 5.)  Semantics, restated exactly and met bit for bit:
 *   - a lattice point is inside when its value is >= iso; a NaN is outside (the test of dmi_iso_active_cells);
 *   - one vertex per crossed lattice edge (exactly one inside endpoint), shared by every cell around the edge; the edge is
 *     owned by its lower endpoint a; vertices are numbered by (a's linear id (k*(ny+1) + j)*(nx+1) + i, axis x < y < z);
 *   - position, f64, every operation rounded: t = (iso - v_a) / (v_b - v_a), or 0 / 1 when a NaN endpoint leaves a / b
 *     the inside one; corner c = origin + idx * spacing per axis; along the edge's axis d x_d = c_a[d] + t*(c_b[d] - c_a[d]),
 *     the other two coordinates c_a's; world w_r = M[r][0]*x + M[r][1]*y + M[r][2]*z + M[r][3], left to right;
 *   - triangles from a generated 256-case table (corner c = x + 2y + 4z; at most 5 per cell; closed, oriented from the
 *     inside to the outside), by ascending cell id, then table order; degenerate ones (t = 0 or 1) are kept;
 *   - the cells that emit triangles are exactly the dmi_iso_active_cells ids.
 * An empty surface is a success (0 and 0).  DMI_ERR_INVALID_ARGUMENT for a NaN iso, null pointers and a context created
 * with dmi_options.z_first != 0 (a z-slab's lattice has the wrong borders); a call refused for these leaves the last mesh. */
int dmi_extract_isosurface(dmi_context *ctx, double iso, uint64_t *n_vertices, uint64_t *n_triangles);
/* The mesh of the last dmi_extract_isosurface: vertices [n][3] f64 world coordinates, triangles [m][3] int64 vertex ids
 * (vtkIdType).  DMI_ERR_INVALID_ARGUMENT before any successful extraction.  Synchronises. */
int dmi_download_isosurface(dmi_context *ctx, double *vertices, int64_t *triangles);
/* dmi_extract_isosurface with the checks, errors, vertices and triangles of that call, bit for bit, plus one normal per vertex
 * ([n][3] f32, kept on the device; what vtkContourFilter's ComputeNormals and vtkTransformFilter make of it).  (Added after
 * round 5; dmi_abi_version() stays 5.)  Definition, f64 and every operation rounded until the last step:
 *   - minus the gradient at lattice point p, per axis e with p's index q, N cells on the axis and h = spacing[e]:
 *     G_e = (P[p] - P[p+e]) / h at q == 0, (P[p-e] - P[p]) / h at q == N, (0.5 * (P[p-e] - P[p+e])) / h otherwise;
 *   - a vertex on the edge (a, b = a + e_d) with its own t: g_r = G(a)_r + t * (G(b)_r - G(a)_r);
 *   - Nm = the cofactors of the grid matrix's upper-left 3x3 A, C[r][c] = A[r+1][c+1]*A[r+2][c+2] - A[r+1][c+2]*A[r+2][c+1]
 *     (indices mod 3), negated when det A = A[0][0]*C[0][0] + A[0][1]*C[0][1] + A[0][2]*C[0][2] < 0 (inverse(A)^T up to a
 *     positive factor; the identity for the identity);
 *   - w_r = Nm[r][0]*g_0 + Nm[r][1]*g_1 + Nm[r][2]*g_2, L = sqrt((w_0*w_0 + w_1*w_1) + w_2*w_2), n = w / L unless L == 0
 *     (then n = w), each n_r rounded to f32 (nearest even).  The normals point from the inside (>= iso) to the outside. */
int dmi_extract_isosurface_normals(dmi_context *ctx, double iso, uint64_t *n_vertices, uint64_t *n_triangles);
/* The normals [n][3] f32 of the last extraction.  DMI_ERR_INVALID_ARGUMENT for a null pointer, before any successful
 * extraction, and when the last successful one was a plain dmi_extract_isosurface.  Synchronises. */
int dmi_download_isosurface_normals(dmi_context *ctx, float *normals);
/* hipEvent time of the kernels of the last dmi_extract_isosurface or dmi_extract_isosurface_normals (both passes and the scans
 * between them). */
int dmi_get_isosurface_kernel_ms(dmi_context *ctx, double *last);

/* What vtkPolyDataConnectivityFilter does after the reference's contour, on the device: label the connected components of the
 * context's mesh, keep some of them and compact the mesh (additions to ABI 5; csrc/isosurface_components.hip).  The input is
 * the mesh the context holds: that of the last successful extraction (with or without normals), or of the last filter since --
 * V vertices, T triangles [T][3] of vertex ids.  Definition (all results are integers or copied bits):
 *   - connectivity is by vertex ID, never by position: two vertices are adjacent when one triangle names both, a component is
 *     a class of the transitive closure.  Vertices that coincide in position (t = 0 or 1) but have different ids are joined
 *     only through the degenerate triangles that name them, which the extraction keeps.  A vertex no triangle names is a
 *     component of its own with 0 triangles (a marching-cubes mesh has none);
 *   - the LABEL of a component is its smallest vertex id, its SIZE the number of triangles whose vertices lie in it, degenerate
 *     ones included;
 *   - mode DMI_COMPONENTS_MIN_TRIANGLES keeps every component with size >= min_triangles (0 keeps everything: labels only);
 *     mode DMI_COMPONENTS_LARGEST keeps the one component of greatest size, ties going to the smallest label (min_triangles is
 *     ignored); an empty mesh stays empty;
 *   - the new mesh: the surviving vertices in ascending old id, renumbered 0, 1, 2, ...; the surviving triangles in their
 *     original order with their ids remapped; positions, and normals when the extraction had them, are the original bits;
 *   - the kept components are numbered 0, 1, 2, ... by ascending label: RegionId[v] (one per surviving vertex) is its
 *     component's number and RegionSize[r] (one per kept component) its size.
 * Returns the new mesh's sizes, the components found and the components kept.  A mesh filtered to nothing is a success (0, 0),
 * as an empty extraction is.  The filter is idempotent for the same arguments.  Afterwards dmi_download_isosurface and
 * dmi_download_isosurface_normals return the filtered mesh; the next extraction replaces it.
 * DMI_ERR_INVALID_ARGUMENT: a null pointer, an unknown mode, no successful extraction yet, or a mesh of 2^32 or more vertices
 * or triangles (labels and sizes are 32-bit on the device: refused, never wrapped).  Synchronises once, to read the counts. */
enum { DMI_COMPONENTS_MIN_TRIANGLES = 0, DMI_COMPONENTS_LARGEST = 1 };
int dmi_filter_isosurface_components(dmi_context *ctx, int mode, uint64_t min_triangles, uint64_t *n_vertices, uint64_t *n_triangles,
                                     uint64_t *n_components, uint64_t *n_components_kept);
/* RegionId [n_vertices] and RegionSize [n_components_kept] of the last filter, int64; either pointer may be null (not wanted).
 * DMI_ERR_INVALID_ARGUMENT before any successful extraction and when no filter has run since the last one.  Synchronises. */
int dmi_download_isosurface_regions(dmi_context *ctx, int64_t *region_id, int64_t *region_size);
/* hipEvent time of all kernels of the last dmi_filter_isosurface_components (separate from dmi_get_isosurface_kernel_ms), and
 * pass by pass: out[0] labels (initialisation, hooking, flattening), out[1] sizes (and the maximum for LARGEST), out[2] the three
 * scans, out[3] the compaction. */
int dmi_get_isosurface_filter_kernel_ms(dmi_context *ctx, double *last);
int dmi_get_isosurface_filter_pass_ms(dmi_context *ctx, double out[4]);
/* Diagnostic: how many compare-and-swaps of the last filter's hooking pass lost a race and were retried (0 = no contention). */
int dmi_get_isosurface_filter_cas_retries(dmi_context *ctx, uint64_t *last);

/* Taubin lambda|mu smoothing of the context's mesh on the device: what a smoothing filter placed behind the contour and the
 * connectivity filter does (vtkSmoothPolyDataFilter without boundary and feature-edge smoothing; only the intent is shared, not
 * the numbers).  Additions to ABI 5; csrc/isosurface_smooth.hip.  The input is the mesh the context holds: V vertices (f64 world
 * positions p) and T triangles of vertex ids -- the last extraction's or the last component filter's.  The triangles, their
 * order, the vertex ids, RegionId and RegionSize are not touched.  Definition, met bit for bit:
 *   - neighbours are by vertex ID, never by position (as in the components filter): N(v) is the set of distinct ids u != v that
 *     share a triangle with v, in ascending id.  Vertices that coincide in position (t = 0 or 1) stay separate vertices;
 *   - an undirected edge {a, b}, a != b, named by exactly one triangle is a BOUNDARY edge (where the surface leaves the grid; a
 *     triangle that names an edge twice, (a, b, a), is one triangle).  Both endpoints of a boundary edge are FIXED: a fixed
 *     vertex never moves, but it is a neighbour like any other.  A vertex with an empty N(v) never moves;
 *   - one STEP with factor f: for every vertex that is not fixed and has k = |N(v)| >= 1, with neighbours n_0 < n_1 < ...,
 *     s_d = ((p[n_0][d] + p[n_1][d]) + p[n_2][d]) + ... added left to right, m_d = s_d / (double)k,
 *     p'[v][d] = p[v][d] + f * (m_d - p[v][d]); f64, every operation rounded, no FMA; every vertex reads the positions of the
 *     PREVIOUS step (Jacobi); non-finite coordinates propagate as the arithmetic makes them;
 *   - one ITERATION: a step with lambda, then, if mu != 0, a step with mu (mu == 0: plain Laplacian smoothing); `iterations` of
 *     them are run;
 *   - NORMALS: if the mesh carries normals (dmi_extract_isosurface_normals) and iterations > 0, they are replaced by geometric
 *     normals of the smoothed mesh (the gradient normals describe the unsmoothed field).  For vertex v, over the triangles
 *     (a, b, c), as stored, that name it (each once), in ascending triangle index: e = p[b] - p[a], g = p[c] - p[a],
 *     x = (e_1*g_2 - e_2*g_1, e_2*g_0 - e_0*g_2, e_0*g_1 - e_1*g_0) (the area-weighted cross product; it points from the inside
 *     to the outside, as the gradient normals do); w = the x added left to right ((0, 0, 0) without a triangle);
 *     L = sqrt((w_0*w_0 + w_1*w_1) + w_2*w_2); n = w / L when L != 0 (a NaN L included), else n = w; each n_r rounded to f32
 *     (nearest even).
 * iterations in [0, 1000]; lambda finite and in (0, 1]; mu finite and <= 0.  iterations == 0 is a success that changes nothing,
 * normals included; an empty mesh is a success.  DMI_ERR_INVALID_ARGUMENT for anything else, for a null context, before any
 * successful extraction, and for a mesh of 2^32 or more vertices or triangles (ids are 32-bit on the device, as in the filter;
 * the offsets into the 6 T directed edges too: 6 T >= 2^32 is refused as well).  A call that fails leaves the context's mesh as
 * it was.  Afterwards dmi_download_isosurface and dmi_download_isosurface_normals return the smoothed mesh,
 * dmi_download_isosurface_regions still works if a filter had run, a later dmi_filter_isosurface_components takes the smoothed
 * mesh as its input, and the next extraction replaces it.  Synchronises once, at its end. */
int dmi_smooth_isosurface(dmi_context *ctx, int32_t iterations, double lambda, double mu);
/* hipEvent time of all kernels of the last dmi_smooth_isosurface, and pass by pass: out[0] the adjacency (edge keys, sort, CSR,
 * fixed bits, and the triangle incidence of the normals), out[1] all steps, out[2] the normals.  Zeros after a call that had
 * nothing to do. */
int dmi_get_isosurface_smooth_kernel_ms(dmi_context *ctx, double *last);
int dmi_get_isosurface_smooth_pass_ms(dmi_context *ctx, double out[3]);

/* Decimation of the context's mesh on the device by vertex clustering (Rossignac-Borrel): what a vtkQuadricClustering or, with a
 * tiny cell, a vtkCleanPolyData placed behind the contour does (only the intent is shared, not the numbers).  This entry places a
 * cluster's vertex at the mean of its members and so shares only the clustering with vtkQuadricClustering;
 * dmi_decimate_isosurface_placed below also places it by the quadric error of the cluster's triangles, as that filter does.
 * Additions to ABI 5;
 * csrc/isosurface_decimate.hip.  The input is the mesh the context holds: V vertices (f64 world positions p) and T triangles of
 * vertex ids -- the last extraction's, the last component filter's or the last smoothing's.  Definition, met bit
 * for bit:
 *   - BOUNDS: lo_d and hi_d are the minimum and the maximum of p[v][d] over all V vertices (exact, independent of order);
 *   - a non-finite coordinate anywhere refuses the call;
 *   - BINS, with h = cell_size: b_d(v) = floor((p[v][d] - lo_d) / h) in f64, the subtraction and the division each rounded, no
 *     reciprocal; n_d = b_d evaluated at hi_d, plus 1; any n_d > 2^21 refuses the call (the key (b_2*n_1 + b_1)*n_0 + b_0 stays
 *     within 63 bits);
 *   - a CLUSTER is the set of all input vertices with the same (b_0, b_1, b_2), whether a triangle names them or not; clusters
 *     are ordered by ascending (b_2, b_1, b_0);
 *   - the REPRESENTATIVE of a cluster with k members of ascending old id m_0 < m_1 < ...:
 *     s_d = ((p[m_0][d] + p[m_1][d]) + p[m_2][d]) + ... added left to right, r_d = s_d / (double)k; f64, no FMA (a cluster of
 *     one keeps its vertex's bits);
 *   - TRIANGLES: each id is replaced by its cluster; a triangle with two equal new ids is DEGENERATE and dropped; two
 *     non-degenerate triangles whose new ids are the same SET (any order, either orientation) are DUPLICATES, and of each such
 *     group only the one with the lowest original index survives; the survivors keep their original relative order and their
 *     stored vertex order (orientation is kept); a triangle that names an id >= V is dropped (the filter and the smoother skip
 *     such triangles in the same way);
 *   - VERTICES: only clusters named by at least one surviving triangle are output, numbered 0, 1, 2, ... in cluster order, and
 *     the triangles carry these numbers: the output has no unreferenced vertex, no degenerate and no duplicate triangle;
 *   - NORMALS: if the mesh carries normals they are replaced by the geometric normals of the decimated mesh, dmi_smooth_isosurface's
 *     definition word for word (the area-weighted cross products of the incident triangles in ascending triangle index, their
 *     sum normalised unless its length is 0, rounded to f32) and its kernel; a mesh without normals stays without;
 *   - REGIONS: RegionId and RegionSize of an earlier filter no longer describe this mesh (a cluster may join components): after
 *     a successful decimation dmi_download_isosurface_regions is refused, exactly as after a fresh extraction, until a filter
 *     runs again.  A later filter or smoothing takes the decimated mesh as its input; the next extraction replaces it.
 * Returns the new mesh's sizes.  An empty mesh is a success (0, 0); a mesh whose every triangle collapses (cell_size exceeds the
 * bounding box) is a success that leaves 0 vertices and 0 triangles.  DMI_ERR_INVALID_ARGUMENT: a null context or null count
 * pointers; a cell_size that is NaN, infinite or <= 0; no successful extraction yet; a non-finite vertex coordinate; any
 * n_d > 2^21 (the message names the smallest acceptable cell size); V or T >= 2^32.  A call that fails leaves the context's mesh,
 * normals and regions exactly as they were: no kernel writes the mesh's own buffers, the result is built in the alternates and
 * swapped in last.  Synchronises twice: once to learn the bounds (and to refuse), once for the counts; the normals are enqueued
 * behind the second and nothing waits for them. */
int dmi_decimate_isosurface(dmi_context *ctx, double cell_size, uint64_t *n_vertices, uint64_t *n_triangles);
/* The same decimation with the placement of the representatives chosen.  DMI_DECIMATE_MEAN is dmi_decimate_isosurface itself:
 * the same code path, results, life cycle and timings.  DMI_DECIMATE_QUADRIC places every cluster's vertex where the planes of
 * the cluster's triangles meet in the least-squares sense (what vtkQuadricClustering's quadric error does), so that a crease or a
 * corner inside a cell stays one instead of being sawn off, and a convex shape does not shrink.  Everything about bounds, bins,
 * clusters, their order, the triangle remap, the degenerate and duplicate removal, the output numbering, the normals and the
 * regions is dmi_decimate_isosurface's, word for word: the triangle array and the vertex count of the output are identical to the
 * mean placement's; only the representative's coordinates change.  Definition, met bit for bit by the device and
 * by tests/isosurface_decimate_quadric_np.py; all arithmetic f64, every operation rounded, no FMA:
 *   - CORNERS: every input triangle t whose three ids are below V has three corners 3t + e, e = 0, 1, 2; corner 3t + e belongs
 *     to the cluster of vertex tris[t][e].  Triangles that the clustering makes degenerate or duplicate are included (a triangle
 *     wholly inside a cell is exactly what describes the surface there, and it counts three times in its cell, as in
 *     vtkQuadricClustering);
 *   - PER CORNER, with o the mean representative of the corner's cluster (dmi_decimate_isosurface's value) and (a, b, c) the
 *     triangle's stored ids: u = p[b] - p[a], v = p[c] - p[a], n = (u1*v2 - u2*v1, u2*v0 - u0*v2, u0*v1 - u1*v0), q = p[a] - o,
 *     d = -((n0*q0 + n1*q1) + n2*q2); the corner contributes (n0*n0, n0*n1, n0*n2, n1*n1, n1*n2, n2*n2) to A and (n0*d, n1*d,
 *     n2*d) to g.  Nothing is normalised (the weight is 4 area^2); the origin is local (o), so large world coordinates lose
 *     nothing;
 *   - SUMS: A and g of a cluster are its corners' contributions added left to right in ascending corner index 3t + e, the first
 *     contribution starting the sum;
 *   - SOLVE: tr = (A00 + A11) + A22, mu = 2^-10 * tr, M = A with mu added to its three diagonal entries; the cofactors
 *     c00 = M11*M22 - M12*M12, c01 = M02*M12 - M01*M22, c02 = M01*M12 - M02*M11, c11 = M00*M22 - M02*M02,
 *     c12 = M01*M02 - M00*M12, c22 = M00*M11 - M01*M01; det = (M00*c00 + M01*c01) + M02*c02;
 *     x_r = -(((c_r0*g0 + c_r1*g1) + c_r2*g2) / det) with c_10 = c01, c_20 = c02, c_21 = c12.  The regularisation is the
 *     deterministic stand-in for VTK's truncated SVD: directions the planes do not determine keep the mean's coordinate;
 *   - PLACEMENT: y_d = o_d + x_d, clamped to the cluster's cell: with b_d the cluster's bin, L_d = lo_d + (double)b_d * h and
 *     U_d = lo_d + (double)(b_d + 1) * h; y_d < L_d gives L_d, y_d > U_d gives U_d.  The representative is the mean o, all three
 *     coordinates, when the cluster has no corner, when tr is not a finite number > 0, when det is not a finite number > 0, or
 *     when any y_d is NaN.
 * The quadric placement's passes (corner keys, one stable radix sort over the cluster bits, a lane per cluster) run behind the
 * triangle pass and are timed as out[1] of dmi_get_isosurface_decimate_pass_ms.  All refusals and guarantees of
 * dmi_decimate_isosurface hold, the messages naming this entry; besides, DMI_ERR_INVALID_ARGUMENT for a placement that is neither
 * constant and, with DMI_DECIMATE_QUADRIC, for 3 T >= 2^32 (corner indices are u32 on the device). */
#define DMI_DECIMATE_MEAN 0
#define DMI_DECIMATE_QUADRIC 1
int dmi_decimate_isosurface_placed(dmi_context *ctx, double cell_size, int32_t placement, uint64_t *n_vertices,
                                   uint64_t *n_triangles);
/* hipEvent time of all kernels of the last dmi_decimate_isosurface or dmi_decimate_isosurface_placed (the sum of its passes), and
 * pass by pass: out[0] clustering (bounds, keys, sort, ranks), out[1] representatives (with the quadric placement: its corner
 * keys, their sort and its kernel), out[2] triangles (remap, degenerate and duplicate removal, vertex and
 * triangle compaction), out[3] normals.  Zeros after a call that had nothing to do.  Waits for the last call's normals. */
int dmi_get_isosurface_decimate_kernel_ms(dmi_context *ctx, double *last);
int dmi_get_isosurface_decimate_pass_ms(dmi_context *ctx, double out[4]);

/* Small holes of the context's mesh closed on the device: the counterpart of a vtkFillHolesFilter behind the contour, for the
 * pinholes the support trim and the consistency filter leave, whose rims the smoother would otherwise pin.  Additions to ABI 5;
 * csrc/isosurface_holes.hip.  The mesh is the one the context holds, whichever call left it: V vertices p ([V][3] f64), T
 * triangles ([T][3] int64).  Definition, met bit for bit by the device and by tests/isosurface_holes_np.py:
 *   half-edges   a triangle (a, b, c) with three distinct ids below V names the half-edges a->b, b->c, c->a.  A triangle that
 *                names an id twice names none (the smoother counts the one real edge of (a, b, a); here such a triangle is not
 *                there at all), nor does one that names an id >= V.
 *   boundary     the undirected edge {a, b} is a boundary edge when exactly one triangle names it (the smoother's rule; an edge
 *                three or more triangles name is none).  Its boundary half-edge is the one half-edge over it, in the direction
 *                its triangle stores.
 *   vertices     a vertex at which a boundary half-edge starts or ends is SIMPLE when exactly one starts and exactly one ends
 *                there, else COMPLEX (a bow-tie, a vertex on a non-manifold seam).  next(a) of a simple vertex a is the end of the
 *                half-edge that starts at a.
 *   loops        a loop is a cycle h_0, h_1 = next(h_0), ..., h_{L-1} with next(h_{L-1}) = h_0 of simple vertices, h_0 the
 *                smallest id among them.  A chain that reaches a complex vertex is no loop and is never filled.  Loops are
 *                ordered by ascending h_0.
 *   fill         a loop is filled when 3 <= L <= max_edges.  L == 3 adds the triangle (h_0, h_2, h_1) and no vertex.  L >= 4 adds
 *                one vertex c, c_d = s_d / (double)L with s_d = ((p[h_0][d] + p[h_1][d]) + p[h_2][d]) + ... added left to right
 *                in walk order (f64, every operation rounded, no FMA), and the L triangles (h_{(i+1) mod L}, h_i, c), i = 0 ..
 *                L-1: the rim's direction reversed, so the patch is oriented like its neighbours.  Non-finite coordinates
 *                propagate as the arithmetic makes them.
 *   output       the first V vertices and the first T triangles are the input's, bit for bit and in place; the new vertices are
 *                V, V+1, ... over the filled loops with L >= 4 in loop order; the new triangles follow loop by loop in loop
 *                order, inside a loop in the order above.
 *   normals      a mesh that carries normals keeps those of its old vertices (a former rim vertex too); a new vertex gets the
 *                geometric normal of dmi_smooth_isosurface's definition over its L triangles in ascending index, which is the
 *                walk order.  A mesh without normals stays without.
 * RegionId / RegionSize, the support counts and the colours no longer describe a mesh that was filled: they are dropped as the
 * decimation drops them (the downloads are refused until their producer runs again).  A call that fills nothing -- an empty
 * mesh, no loop of 3 .. max_edges edges, max_edges < 3 -- is a success that leaves the mesh and all of these untouched.
 * Nothing here is clever: the rim of an open sheet is a loop like any other, the rim of an isolated triangle is closed by its
 * mirror image, and a fan round the centroid of a rim that is far from flat or from convex may fold.  max_edges is what keeps
 * large rims open; dmi_reconstruction runs the fill behind its component flags, which have removed the isolated pieces.
 * n_vertices, n_triangles: the mesh afterwards.  n_filled, boundary_edges_left (each may be null): the loops filled, and the
 * boundary edges of the mesh afterwards (those of complex chains and of loops not filled).
 * DMI_ERR_INVALID_ARGUMENT: a null context or null size pointers, max_edges > 2^20, no extraction yet, input or output V or T >=
 * 2^32 or 6 T >= 2^32 (ids and edge positions are u32 on the device), and input V >= 2^31 (an edge key is two ids and the
 * stored direction in 64 bits).  A failing call leaves the mesh exactly as it was: the result is built in the alternate buffers
 * and swapped in last.  Synchronises the context's stream three times (the boundary vertices, the additions, the result). */
int dmi_fill_isosurface_holes(dmi_context *ctx, uint64_t max_edges, uint64_t *n_vertices, uint64_t *n_triangles,
                              uint64_t *n_filled, uint64_t *boundary_edges_left);
/* hipEvent time of all kernels of the last dmi_fill_isosurface_holes, and pass by pass: out[0] boundary (keys, sort, half-edges,
 * vertex classes), out[1] loops (labels, lengths, scans), out[2] fill (copy, centroids, triangles, normals).  Zeros after a call
 * that filled nothing. */
int dmi_get_isosurface_holes_kernel_ms(dmi_context *ctx, double *last);
int dmi_get_isosurface_holes_pass_ms(dmi_context *ctx, double out[3]);

/* Trim of the context's mesh by view support, on the device: what every TSDF pipeline does to the back shell and to the sheets
 * between seen and unseen space that an iso-contour of the summed ray potential carries besides the surface.  Additions to ABI 5;
 * csrc/isosurface_support.hip.  The mesh is the one the context holds: V vertices p, T triangles, and normals n (f32, widened to
 * f64) when it carries them.  The views are all that are resident in this context, W x H each.  Definition, met bit
 * for bit; all arithmetic is f64, every operation is rounded, there is no FMA.  View m SUPPORTS vertex v when all of these hold:
 *   - CAMERA COORDINATES: c_r = ((RT[4r]*x + RT[4r+1]*y) + RT[4r+2]*z) + RT[4r+3] for r = 0, 1, 2;
 *   - PROJECTION: h_r = ((K[4r]*c_0 + K[4r+1]*c_1) + K[4r+2]*c_2) + K[4r+3], the fusion's own projection order;
 *   - IN FRONT OF THE CAMERA: c_2 > 0;
 *   - PIXEL: u = h_0/h_2, v = h_1/h_2, px = round(u), py = round(v) with half away from zero; a non-finite u or v, or one of
 *     magnitude >= 2^31, is outside the image; then 0 <= px < W and 0 <= py < H;
 *   - DEPTH: d is view m's resident fusion depth at image pixel (px, py), widened to f64 -- the value dmi_color_process_isosurface's
 *     fused test reads: -1 where the best cost exceeded the threshold, the f32-rounded value under a forced DMI_DEPTH_F32 -- and
 *     the test is d > 0 and fabs(c_2 - d) <= tolerance, the difference rounded; NaN, -1 and infinite depths reject the pair;
 *   - FACING, only if require_facing != 0: m_r = (RT[4r]*n_0 + RT[4r+1]*n_1) + RT[4r+2]*n_2, s = (m_0*c_0 + m_1*c_1) + m_2*c_2, and
 *     the pair counts iff s < 0: the normal, which points from inside to outside, points towards the camera; a NaN or zero s rejects.
 * support[v] is the number of supporting views, an int32.  The filter:
 *   - triangle (a, b, c) survives iff all three ids are < V and min(support[a], support[b], support[c]) >= min_views;
 *   - a vertex survives iff a surviving triangle names it: the result has no unreferenced vertex;
 *   - survivors keep ascending old id and original triangle order; positions and normals are copied bit for bit;
 *   - min_views == 0 changes nothing in the mesh and only computes the counts; min_views > the number of views leaves (0, 0) and
 *     is a success; the counts depend only on position and normal, so the filter is idempotent for the same arguments.
 * Returns the mesh's sizes after the call.  After a call that removes anything the colours are dropped and
 * dmi_download_isosurface_regions is refused until a component filter runs again, as after a decimation.  Results are built in the
 * alternates and swapped in last: a call that fails leaves the mesh, normals, regions, colours and any earlier support array
 * exactly as they were.  DMI_ERR_INVALID_ARGUMENT: null pointers; min_views < 0; a NaN, infinite or negative tolerance; no
 * successful extraction yet; require_facing on a mesh without normals; V or T >= 2^32.  DMI_ERR_STATE: no views resident.  An
 * empty mesh is a success.  The checks come in this order, so an empty mesh in a context without views is DMI_ERR_STATE: the
 * counts are about the views, and there are none.  Synchronises once. */
int dmi_filter_isosurface_support(dmi_context *ctx, int32_t min_views, double tolerance, int32_t require_facing, uint64_t *n_vertices,
                                  uint64_t *n_triangles);
/* support[V] of the last dmi_filter_isosurface_support: one count per vertex of the mesh as that call left it.  Refused
 * (DMI_ERR_INVALID_ARGUMENT) before any such call and after anything that has changed the mesh since: an extraction, the component
 * filter, a smoothing with iterations > 0 or a decimation -- as the colours are dropped. */
int dmi_download_isosurface_support(dmi_context *ctx, int32_t *support);
/* hipEvent time of all kernels of the last dmi_filter_isosurface_support, and pass by pass: out[0] counts, out[1] triangle flags,
 * marks and scans, out[2] compaction.  Zeros for the passes a call did not run (min_views == 0: the counts only). */
int dmi_get_isosurface_support_kernel_ms(dmi_context *ctx, double *last);
int dmi_get_isosurface_support_pass_ms(dmi_context *ctx, double out[3]);

/* Diagnostic: how many (8 x 8 x column brick, view) pairs of the last dmi_fuse were proven to be handled
 * uniformly.  out[0] mixed (per-voxel path), out[1] all voxels accumulate -eta*rho, out[2] all accumulate 0,
 * out[3] no voxel reaches the accumulate.  All zero when the last fuse ran the general kernel or classes
 * are switched off.  Synchronises. */
int dmi_get_brick_class_histogram(dmi_context *ctx, uint64_t out[4]);

/* Diagnostic: why the mixed pairs of the last dmi_fuse could not be proven uniform.  out[1] non-finite corner value,
 * out[2] the camera plane cuts the brick (c.z <= 0 or too small for the footprint bound), out[3] the footprint is
 * partly outside the depth map, out[4] NaN depths in the footprint, out[5] "no depth" pixels next to depths, out[6]
 * depths within delta of the brick (a surface is near), out[7] every depth of the footprint far behind the brick, with "no depth"
 * pixels among them (free space seen through holes: the FREE column); out[0] unused.  Synchronises. */
int dmi_get_mixed_reason_histogram(dmi_context *ctx, uint64_t out[8]);

/* Diagnostic: how many of the "free space or no depth" pairs (out[7] above) of the last dmi_fuse the fusion kernel served from a
 * window of validity bits (one coalesced fetch per pair) instead of one gather per voxel.  Synchronises. */
int dmi_get_window_pair_count(dmi_context *ctx, uint64_t *out);

/* Which path each resident view takes through the fusion (decided per view from its K, [R|T] and the grid, at dmi_add_views*):
 *   out[0] general kernel (the tiled kernel's bounds do not hold for the view: 6 x slower per view at cfg 3)
 *   out[1] tiled kernel, general K (third row not 0 0 1 0): pixels selected in fp64 only
 *   out[2] tiled kernel, pinhole, fp64 selection only (tier 1 declined: maps beyond 2^24 pixels, bounds not finite)
 *   out[3] tiled kernel, tier 1 with one margin for the view
 *   out[4] tiled kernel, tier 1 with a margin per lane (the camera stands inside or next to the volume)
 *   out[5] of the views counted in [3] and [4]: those with a window record (the window form of the FREE column can serve them)
 * INTEGRATION.md "Magnitudes" says at which coordinate magnitudes a view changes rows. */
int dmi_get_view_paths(dmi_context *ctx, uint64_t out[6]);

/* dmi_get_info / dmi_get_timings fill sizeof(dmi_info) / sizeof(dmi_timings) bytes AS THIS LIBRARY WAS BUILT: a caller compiled
 * against an older header (a shorter struct) must check dmi_abi_version() == DMI_ABI_VERSION -- or compare its own sizeof with
 * dmi_sizeof_info() / dmi_sizeof_timings() -- before passing its buffer. */
int dmi_get_timings(dmi_context *ctx, dmi_timings *out);
int dmi_get_info(dmi_context *ctx, dmi_info *out);
size_t dmi_sizeof_info(void);
size_t dmi_sizeof_timings(void);

/* hipEvent time of the upload pass (the one kernel per staged chunk that thresholds, flips and narrows the tables and builds the
 * pyramid base, the validity bytes and bits, plus the upper pyramid levels) of the last dmi_add_views* call, and summed over
 * the context's life; the copies are not in it.  A call whose tables are staged in several chunks (more than 256 MiB of f64
 * tables) times its LAST chunk and scales it to the call's views: an extrapolation then, a measurement for calls of one chunk
 * (bench.py's calls of 32 views are).  Either pointer may be null. */
int dmi_get_upload_kernel_ms(dmi_context *ctx, double *last, double *total);

/* Pinned host memory for the SoA staging buffers of the host side (hipHostMalloc). */
int dmi_alloc_pinned(size_t bytes, void **out);
int dmi_free_pinned(void *ptr);
/* Diagnostic: the host <-> device copy rates (GB/s, pinned memory, one hipMemcpyAsync of `bytes` each way, best of two)
 * that bound every PCIe-inclusive figure of this path -- the roof next to which bench.py quotes its end-to-end numbers. */
int dmi_pcie_probe(int32_t device, size_t bytes, double *h2d_GBps, double *d2h_GBps);
/* Diagnostic: the fp64 vector rate this device sustains right now (TFLOP/s; a kernel of dependent-free v_fma_f64 chains
 * on every SIMD for about `milliseconds`, best of three).  The fusion kernel is bound by fp64 vector issue, and boxes of
 * the same model differ and drift: bench.py quotes this next to its figures so that runs on different boxes compare. */
int dmi_fp64_probe(int32_t device, double milliseconds, double *tflops);

/* ---- MeshColoration pass (Coloration/MeshColoration.cxx:98-199; the reference runs it on the CPU) ----
 * For every mesh vertex: the views whose projection of the vertex (RD.cxx:169-182: no z-sign test, no depth
 * test) falls inside the image contribute that pixel's RGB (RD.cxx:92-116); outputs are the reference's three
 * point-data arrays "MeanColoration" (u8 x 3, integer mean), "MedianColoration" (u8 x 3) and
 * "NbProjectedDepthMap" (i32), zero where no view sees the vertex.
 *   points [n_points][3] f64 (vtkPoints of the mesh); colors [n_views][H][W][3] u8, the "Color" arrays in vtk
 *   point order; K4, RT4 [n_views][16] row-major (Get4MatrixK / GetMatrixTR).  One-shot: uploads, runs two
 *   kernels, downloads.  Bit-identical to the reference arithmetic (everything after the projection is integer). */
int dmi_color_mesh(const double *points, int64_t n_points, const uint8_t *colors, const double *K4, const double *RT4,
                   int32_t n_views, int32_t width, int32_t height, int32_t device, uint8_t *mean, uint8_t *median,
                   int32_t *count);
const char *dmi_color_last_error(void);

/* The same pass with the colour planes and camera records RESIDENT in HBM: upload the views once, colour any number
 * of vertex sets (BASELINE config 5: the mesh is sharded by vertex across the GPUs, every GPU holds all views, no
 * exchange step).  dmi_color_process works through the vertices in chunks that bound its scratch memory (1 GiB). */
typedef struct dmi_color_context dmi_color_context;
int dmi_color_create(int32_t device, dmi_color_context **out);
void dmi_color_destroy(dmi_color_context *ctx);
/* appends n views: colors [n][H][W][3] u8 in vtk point order, K4 / RT4 [n][16] row-major */
int dmi_color_add_views(dmi_color_context *ctx, const uint8_t *colors, const double *K4, const double *RT4, int32_t n,
                        int32_t width, int32_t height);
int dmi_color_clear_views(dmi_color_context *ctx);
int dmi_color_process(dmi_color_context *ctx, const double *points, int64_t n_points, uint8_t *mean, uint8_t *median,
                      int32_t *count);
/* Upper bound, in bytes, of the device scratch one chunk of vertices may use (default 1 GiB, at least 1024): a smaller
 * budget means more, smaller chunks, never a different result. */
int dmi_color_set_scratch_budget(dmi_color_context *ctx, uint64_t bytes);
/* enable != 0: the vertices of a chunk are worked through along a Z-order curve of their bounding box (device-side key +
 * radix sort), whatever order the caller has them in; inputs and outputs keep the caller's order and no result bit
 * changes.  Worth it for vertices in no particular order (scattered colour gathers become neighbouring ones); a mesh
 * whose vertices already come in a spatially coherent order is faster without.  Default off. */
int dmi_color_set_vertex_reorder(dmi_color_context *ctx, int32_t enable);
/* hipEvent time of the kernels (projection + median) of the last dmi_color_process, summed over its chunks */
int dmi_color_get_kernel_ms(dmi_color_context *ctx, double *out);
/* Opt-in visibility test (not in the reference, whose colouring has neither a z-sign nor a depth test, so occluders and
 * views from behind blend into a vertex's colour).  (Added after round 5; dmi_abi_version() stays 5.)  Definition (DESIGN.md
 * 8b), met bit for bit: for vertex p = (x, y, z) f64 and view m with W x H images,
 *   - (px, py) is the pixel the plain pass selects, with the same bounds test;
 *   - cz = ((RT[8]*x + RT[9]*y) + RT[10]*z) + RT[11], every operation rounded, no FMA (TransformPoint's camera z, RD.cxx:173);
 *   - d = depths_m[(H-1-py)*W + px], the f64 "Depths" value in vtk point order (no best-cost threshold);
 *   - with the test on and tolerance tol the pair counts iff the bounds test passes, cz > 0, d > 0 and fabs(cz - d) <= tol
 *     (the difference rounded).  A comparison with a NaN is false: NaN, -1 and infinite depths reject the pair.
 * Mean, median and count are then those of the pairs that count; a vertex without any is all zeros.
 * dmi_color_add_views_with_depth appends views exactly as dmi_color_add_views and keeps their depth planes ([n][H][W] f64,
 * vtk point order) resident; dmi_color_clear_views drops them.  dmi_color_set_depth_test: DMI_ERR_INVALID_ARGUMENT for a
 * NaN, infinite or negative tolerance; while the test is on, dmi_color_process fails with DMI_ERR_INVALID_ARGUMENT if a
 * resident view was added without depths.  Default off: every output is then the plain pass's. */
int dmi_color_add_views_with_depth(dmi_color_context *ctx, const uint8_t *colors, const double *depths, const double *K4,
                                   const double *RT4, int32_t n, int32_t width, int32_t height);
int dmi_color_set_depth_test(dmi_color_context *ctx, int32_t enable, double tolerance);

/* ---- Coloration of the device mesh (added after round 5, dmi_abi_version() stays 5) ----
 * dmi_color_process_isosurface colours the mesh `ctx` holds -- the last extraction's, or what the filter, the smoother or the
 * decimation left -- with the views resident in `c`, reading the vertices ([V][3] f64) where they are: no vertex is copied to
 * the device and no result to the host.  It waits for whatever is still queued on the context's stream (a decimation's normals)
 * before it starts, brings a sample of at most 1536 vertices to the host to choose the order of work as dmi_color_process does
 * (a choice that changes no result bit) and synchronises once at its end.  The three results stay on the device, owned by `ctx`
 * and counted in its device_bytes: mean [V][3] u8, median [V][3] u8, count [V] i32; dmi_download_isosurface_colors copies them
 * out (any of its three pointers may be null: not wanted; it synchronises).  *n_vertices receives V.
 * LIFE CYCLE: a successful extraction, dmi_filter_isosurface_components, dmi_smooth_isosurface with iterations > 0 or
 * dmi_decimate_isosurface drops the colours, because they no longer describe the mesh; dmi_download_isosurface_colors is then
 * refused with DMI_ERR_INVALID_ARGUMENT, as it is before any colouring.  A call that fails leaves mesh, normals, regions and
 * colours as they were, a colouring that fails included (the results are built in alternates and swapped in last).
 * fused_depth_test == 0: bit for bit what dmi_color_process(c, <the downloaded vertices>, ...) returns with c's current
 *   settings (its own depth test and planes, dmi_color_set_vertex_reorder, dmi_color_set_scratch_budget), in the same chunks.
 * fused_depth_test != 0: the visibility test of dmi_color_set_depth_test with the depth taken from the FUSION context instead of
 *   from planes of `c` (none are needed: at 256 views of 720p that is 1.9 GB of HBM and of upload less).  For vertex p and view m
 *   the pair counts iff the bounds test passes, cz > 0, d > 0 and fabs(cz - d) <= tolerance, with cz and the pixel (px, py)
 *   exactly as there and d = view m's resident fusion depth at image pixel (px, py) widened to f64: what dmi_add_views* was given
 *   at vtk index (H-1-py)*W + px, REPLACED BY -1 WHERE ITS BEST COST EXCEEDED THE THRESHOLD (RD.cxx:138-167).  Under
 *   DMI_DEPTH_AUTO and DMI_DEPTH_F64 that is the thresholded f64 depth bit for bit; under a forced DMI_DEPTH_F32 it is the
 *   stored value, i.e. the depth rounded to f32.  NaN, -1 and infinite depths reject the pair.  Unlike the own-planes test (and
 *   --depthTolerance of dmi_coloration), whose planes are the unthresholded "Depths", a pixel that the best-cost threshold
 *   removed no longer vouches for a vertex: the fusion did not believe that depth, and neither does the colouring.
 *   VIEWS CORRESPOND BY INDEX: view m of `c` must be view m of `ctx` (same K, [R|T], image).  That is the caller's contract; only
 *   the view counts and the image sizes are compared.
 * DMI_ERR_INVALID_ARGUMENT: null c, ctx or n_vertices; no successful extraction yet; c and ctx on different devices; with the
 * fused test a NaN, infinite or negative tolerance, c's own depth test switched on, or ctx's view count, width or height not
 * equal to c's.  DMI_ERR_STATE: no views in c, as in dmi_color_process.  An empty mesh is a success with *n_vertices = 0: empty
 * colours then exist and download as nothing.  Errors are reported through dmi_last_error(ctx). */
int dmi_color_process_isosurface(dmi_color_context *c, dmi_context *ctx, int32_t fused_depth_test, double tolerance,
                                 uint64_t *n_vertices);
int dmi_download_isosurface_colors(dmi_context *ctx, uint8_t *mean, uint8_t *median, int32_t *count);
/* hipEvent time of the kernels of the last dmi_color_process_isosurface (the span of its chunks' kernels: nothing else runs
 * between them); zero after an empty mesh */
int dmi_get_isosurface_color_kernel_ms(dmi_context *ctx, double *last);

/* ---- Rendered depth planes: the mesh's own z-buffer as coloration visibility (DESIGN.md 8b''; added after round 5,
 * dmi_abi_version() stays 5) ----
 * The depth planes the visibility test compares against can be RENDERED from the mesh that is being coloured instead of taken from
 * the depth maps: no holes, no noise, valid after smoothing or decimation, and available for a mesh that has no depth maps at all.
 * dmi_color_render_depths rasterises a triangle mesh (points [n_points][3] f64, triangles [n_triangles][3] ids, host arrays,
 * uploaded in pieces) into EVERY view resident in `c` and leaves each view with a tiled f64 depth plane of its own: a view added
 * without depths gets one, the planes of dmi_color_add_views_with_depth are replaced.  dmi_color_clear_views drops them.  The
 * consumer is unchanged: render, dmi_color_set_depth_test(c, 1, tol), then dmi_color_process or
 * dmi_color_process_isosurface(c, ctx, 0, ...).
 * Definition, met bit for bit (all arithmetic f64, every operation rounded, no FMA).  For view m (W x H, K, [R|T]) and a triangle
 * with vertices p_0, p_1, p_2:
 *   - (cx, cy, cz) and (dx, dy, dz) of each vertex as in the colouring (TransformPoint left to right, then the 3x3 K without
 *     translation); u = dx/dz, v = dy/dz.  The triangle is skipped for this view unless all three vertices have cz > 0, dz > 0
 *     and finite u, v.  THERE IS NO NEAR-PLANE CLIPPING: a triangle that crosses the camera plane does not occlude.
 *   - pixel (x, y) has its centre at integer coordinates (the colouring's round(u)); candidates are
 *     x in [max(0, ceil(min u)), min(W-1, floor(max u))], likewise y.
 *   - e0 = (u2-u1)*(y-v1) - (v2-v1)*(x-u1), e1 = (u0-u2)*(y-v2) - (v0-v2)*(x-u2), e2 = (u1-u0)*(y-v0) - (v1-v0)*(x-u0); the pixel is
 *     covered iff all three are >= 0 or all three are <= 0, and s = (e0+e1)+e2 != 0: both windings occlude, edges are inclusive,
 *     zero-area triangles cover nothing.
 *   - q = (e0/cz0 + e1/cz1) + e2/cz2, d = s/q, kept iff finite and > 0: the perspective-correct camera z, exact for a K whose last
 *     row is (0, 0, 1) (all that SetMatrixK produces); for a general K it is an approximation.
 *   - the plane holds the MINIMUM of d over the covering triangles and +inf where nothing covers (+inf fails the test's
 *     fabs(cz - d) <= tol).  A minimum does not depend on order: the same bits from run to run, in whatever order the triangles
 *     come.
 * COST: the planes are 8 bytes per pixel and view, 1.9 GB at 256 views of 1280 x 720 (twice that while a rendering replaces an
 * earlier one: the new planes are built beside the old and swapped in last).
 * Errors: an id outside [0, n_points) -> DMI_ERR_INVALID_ARGUMENT, checked on the device before anything is rendered; no views ->
 * DMI_ERR_STATE; a call that fails leaves the planes as they were.  n_triangles == 0 is a success that leaves every plane empty.
 * dmi_color_render_isosurface_depths does the same from the mesh `ctx` holds, where it is (no copy), bit for bit what
 * dmi_color_render_depths gives on the downloaded mesh; refusals as dmi_color_process_isosurface (no extraction yet, different
 * devices: DMI_ERR_INVALID_ARGUMENT; no views: DMI_ERR_STATE), reported through dmi_last_error(ctx).
 * dmi_color_download_depths: the planes of views [first, first + count) as out [count][H][W] f64 in vtk point order -- the layout
 * dmi_color_add_views_with_depth takes --, -1 where the plane is +inf; DMI_ERR_INVALID_ARGUMENT when a view of the range has no
 * plane.  dmi_color_get_render_kernel_ms: the hipEvent span of the last rendering's kernels.
 * dmi_color_set_render_queue_capacity: triangles whose pixel range in a view is large are queued for a pass of their own; a
 * rendering that needs more entries than the queue starts with (default 1 Mi, at least 1) grows it and renders the views
 * concerned again.  As with the scratch budget, a smaller value never changes a bit. */
int dmi_color_render_depths(dmi_color_context *c, const double *points, int64_t n_points, const int64_t *triangles,
                            int64_t n_triangles);
int dmi_color_render_isosurface_depths(dmi_color_context *c, dmi_context *ctx);
int dmi_color_download_depths(dmi_color_context *c, int32_t first, int32_t count, double *out);
int dmi_color_get_render_kernel_ms(dmi_color_context *c, double *last);
/* The same rendering pass by pass (hipEvents between the kernels): out[0] the fill with +inf, out[1] the small passes (one lane
 * per triangle), out[2] the large passes (one wave per queued pair), each summed over the view groups -- a group that ran again
 * after a queue overflow counts both times.  And how many (triangle, view) pairs the large passes took. */
int dmi_color_get_render_pass_ms(dmi_color_context *c, double out[3]);
int dmi_color_get_render_queued_pairs(dmi_color_context *c, uint64_t *out);
int dmi_color_set_render_queue_capacity(dmi_color_context *c, uint64_t entries);

/* ---- Depth maps filtered by cross-view consistency before they are fused (added after round 5,
 * dmi_abi_version() stays 5) ----
 * The reference puts only the best-cost threshold between a stereo depth map and the fusion; a pixel that passes it with a wrong
 * depth is fused as if it were surface.  dmi_filter_depth_consistency keeps a depth only if enough other views, looking at the same
 * world point, hold a depth that agrees.  Context-free, like dmi_color_mesh: it uploads, runs its kernels, downloads and frees.
 *   depth     [n][H][W] f64 host, vtk point order (image pixel (px, py) is stored at row H-1-py)
 *   best_cost [n][H][W] f64 host or NULL, with `threshold`
 *   K4, RT4   [n][16]   f64 host, row-major 4x4, exactly what dmi_add_views takes
 *   out_depth [n][H][W] f64 host; may be `depth` itself (the device works on its own copy)
 *   out_count [n][H][W] int32 host or NULL;  kernel_ms (nullable): hipEvent time of the kernels alone
 * Every K4 must have K4[1][0] == 0, the third row (0, 0, 1, 0) and non-zero K4[0][0] and K4[1][1]: all that SetMatrixK or a .krtd
 * file produces.  THE 3 x 3 BLOCK OF RT4 IS TAKEN AS ORTHONORMAL, as a .krtd gives it: the back-projection uses its transpose.
 * Definition, met bit for bit by the device and by tests/depth_consistency_np.py.  All arithmetic is f64, every operation is
 * rounded on its own, nothing is contracted; comparisons with a NaN are false.
 *   1. D_m = depth_m with -1 wherever best_cost_m > threshold (RD.cxx:138-167).  A pixel is VALID iff D > 0 and D < +inf: false for
 *      NaN, -1, 0 and negatives.
 *   2. Back-projection of valid pixel (px, py) of view s with depth d; K = K4_s, R[i][j] = RT4_s[i][j], T_i = RT4_s[i][3]:
 *      yn = (py - K[1][2]) / K[1][1];  xn = ((px - K[0][2]) - K[0][1]*yn) / K[0][0];  c = (xn*d, yn*d, d);  q_i = c_i - T_i;
 *      w_j = (R[0][j]*q_0 + R[1][j]*q_1) + R[2][j]*q_2 for j = 0, 1, 2.  The divisions are correctly rounded.
 *   3. Every other view t != s (the result is a count: the order does not matter):
 *      c'_i = ((RT4_t[i][0]*w_0 + RT4_t[i][1]*w_1) + RT4_t[i][2]*w_2) + RT4_t[i][3];
 *      h_i = ((K4_t[i][0]*c'_0 + K4_t[i][1]*c'_1) + K4_t[i][2]*c'_2) + K4_t[i][3];  c'_2 > 0 is required;
 *      the pixel by the fusion's rule: h_2 < 0 is out; u = h_0/h_2, v = h_1/h_2; round half away from zero; the bounds
 *      0 <= round(u) < W and 0 <= round(v) < H tested in f64; non-finite is out;  d' = D_t at that pixel;
 *      the pair AGREES iff d' > 0 and fabs(c'_2 - d') <= abs_tolerance + rel_tolerance*c'_2 (the product rounded, then the sum,
 *      then the difference).
 *   4. out_count = the number of agreeing views, 0 at a pixel that is not valid.  out_depth = D where the pixel is valid and its
 *      count >= min_views, exactly -1.0 everywhere else.  The counts are always taken against the INPUT D of the other views, never
 *      against an already filtered one; min_views == 0 therefore returns D with every invalid value normalised to -1, and the counts.
 * Host data goes up and comes down in pieces of at most 256 MiB.  Device memory: 12 bytes per pixel and view plus the pieces.
 * All arguments are checked before the device is touched.  DMI_ERR_INVALID_ARGUMENT, the message naming the argument: a null depth,
 * K4, RT4 or out_depth; n < 1; W or H outside [1, 32768]; min_views < 0; a negative, NaN or infinite abs_tolerance or rel_tolerance;
 * a NaN threshold when best_cost is given; a K4 outside the form above (the message names the view).  Then DMI_ERR_DEVICE without a
 * device.  A refused call leaves out_depth and out_count untouched.  The call never exits and never throws; a failure's text is
 * dmi_last_error(NULL)'s.  Synchronises. */
int dmi_filter_depth_consistency(const double *depth, const double *best_cost, double threshold, const double *K4, const double *RT4,
                                 int32_t n, int32_t W, int32_t H, double abs_tolerance, double rel_tolerance, int32_t min_views,
                                 int32_t device, double *out_depth, int32_t *out_count, double *kernel_ms);

/* ---- The bounds of the scene the depth maps see (added after round 5, dmi_abi_version() stays 5) ----
 * --gridOrigin and --gridEnd had to come from outside the data.  dmi_estimate_scene_bounds takes them from the depth maps and
 * cameras the fusion reads: per grid axis, exact order statistics of the back-projected pixels, so that a handful of wild depths
 * does not decide the box.  Context-free, like dmi_filter_depth_consistency: it uploads, runs its kernels, downloads six numbers
 * and frees.
 *   depth, best_cost, threshold, K4, RT4, n, W, H   exactly as dmi_filter_depth_consistency takes them, the K4 form included
 *   axes9     [9] f64 host, row-major 3 x 3, or NULL for the identity: the axes the coordinates are measured along
 *   trim_fraction  in [0, 0.5];  pixel_step >= 1
 *   lo, hi    [3] f64 host;  n_points: the points that were ordered;  kernel_ms (nullable): hipEvent time of the kernels alone
 * Definition, met bit for bit by the device and by tests/scene_bounds_np.py.  All arithmetic is f64, every operation is rounded on
 * its own, nothing is contracted; comparisons with a NaN are false.
 *   1. D and VALID are steps 1 and 2's validity of dmi_filter_depth_consistency: D_m = depth_m with -1 wherever best_cost_m >
 *      threshold; a pixel is valid iff D > 0 and D < +inf.  A valid pixel (px, py) TAKES PART iff px % pixel_step == 0 and
 *      py % pixel_step == 0; (px, py) are image coordinates, vtk row r is image row H-1-r.
 *   2. w = the back-projection of step 2 of dmi_filter_depth_consistency, operation for operation.
 *   3. s_a = (A[a][0]*w_0 + A[a][1]*w_1) + A[a][2]*w_2 for a = 0, 1, 2, A = axes9.  A point is COUNTED iff all three s_a are finite.
 *      N = the number of counted points; *n_points = N.
 *   4. The s_a of the counted points are ordered by the key bits ^ (bits >> 63 ? ~0 : 1 << 63) of their f64 bits: ascending key
 *      order is numeric order, with -0.0 before +0.0.  k = min((uint64_t)(trim_fraction * (double)N), (N - 1) / 2).  lo[a] = the
 *      element of rank k (0-based) of axis a, hi[a] = the element of rank N-1-k; the ranks are taken per axis, independently of the
 *      other axes.  trim_fraction == 0 gives the exact minimum and maximum.
 *   5. N == 0: DMI_OK, *n_points = 0, all six outputs NaN.
 * Host data goes up in pieces of whole views, as many as fit 256 MiB (a single view larger than that goes up whole, as in
 * dmi_filter_depth_consistency).  Device memory: 8 bytes per pixel and view plus the pieces; the points themselves are never stored.
 * All arguments are checked before the device is touched.  DMI_ERR_INVALID_ARGUMENT, the message naming the argument: everything
 * dmi_filter_depth_consistency refuses for the arguments the two calls share (a null depth, K4 or RT4; n < 1; W or H outside
 * [1, 32768]; a NaN threshold when best_cost is given; a K4 outside the form, the message naming the view); a null lo, hi or
 * n_points; a NaN or negative trim_fraction or one above 0.5; pixel_step < 1; an axes9 entry that is not finite; n*W*H >= 2^53.
 * Then DMI_ERR_DEVICE without a device.  A refused call leaves lo, hi and *n_points untouched.  The call never exits and never
 * throws; a failure's text is dmi_last_error(NULL)'s.  Synchronises. */
int dmi_estimate_scene_bounds(const double *depth, const double *best_cost, double threshold, const double *K4, const double *RT4,
                              int32_t n, int32_t W, int32_t H, const double *axes9 /* nullable: identity */, double trim_fraction,
                              int32_t pixel_step, int32_t device, double lo[3], double hi[3], uint64_t *n_points, double *kernel_ms);

/* ---- Small depth-map segments removed before the maps are fused (added after round 5, dmi_abi_version()
 * stays 5) ----
 * The speckle filter of every stereo pipeline: a small island of pixels whose depth is continuous among themselves but not with
 * their surroundings is a matching error, and needs no second view to be recognised.  Fused, it leaves a floating speck and carves
 * along its rays through the surface behind it.  dmi_filter_depth_speckles labels the connected segments of every view and keeps
 * the depths of the segments that are large enough.  Context-free, like dmi_filter_depth_consistency: it uploads, runs its kernels,
 * downloads and frees.  It takes no cameras.
 *   depth, best_cost, threshold   exactly as dmi_filter_depth_consistency takes them: [n][H][W] f64 host in vtk point order,
 *             best_cost nullable
 *   out_depth [n][H][W] f64 host; may be `depth` itself
 *   out_size  [n][H][W] int32 host or NULL;  kernel_ms (nullable): hipEvent time of the kernels alone, summed over the pieces
 * Definition, met bit for bit by the device and by tests/depth_speckle_np.py.  All arithmetic is f64, every operation is rounded
 * on its own, nothing is contracted; comparisons with a NaN are false.
 *   1. D_m = depth_m with -1 wherever best_cost_m > threshold.  A pixel is VALID iff D > 0 and D < +inf.
 *   2. Two valid pixels of the SAME view that are 4-neighbours are LINKED iff
 *      fabs(Da - Db) <= abs_tolerance + rel_tolerance * fmin(Da, Db): the product rounded, then the sum, then the difference.
 *      4-neighbours are the same row with adjacent columns, or the same column with adjacent rows; the row order does not matter
 *      to this relation, so nothing is flipped.  The last pixel of a row and the first of the next are not neighbours; pixels of
 *      different views are never neighbours.  The relation is symmetric because of fmin.
 *   3. A SEGMENT is a connected component of the valid pixels of one view under LINKED.  Its SIZE is its number of pixels.
 *   4. out_size = the pixel's segment size, 0 at a pixel that is not valid.
 *   5. out_depth = D where the pixel is valid and its size >= min_pixels, exactly -1.0 elsewhere.  min_pixels == 0 returns D with
 *      every invalid value normalised to -1, and the sizes.
 * The result depends only on the partition into segments, so it is the same to the bit whatever order the hardware runs in: two
 * calls give identical bytes.
 * Host data goes up and comes down in pieces of whole views, as many as fit 256 MiB (a single larger view goes whole, as in
 * dmi_estimate_scene_bounds).  The device holds the planes of one piece at a time -- 16 bytes per pixel of the piece, 8 more with
 * best_cost, 4 more with out_size --, so device memory does not grow with n.
 * All arguments are checked before the device is touched.  DMI_ERR_INVALID_ARGUMENT, the message naming the argument: a null depth
 * or out_depth; n < 1; W or H outside [1, 32768]; min_pixels < 0; a negative, NaN or infinite abs_tolerance or rel_tolerance; a NaN
 * threshold when best_cost is given.  Then DMI_ERR_DEVICE without a device.  A refused call leaves out_depth and out_size
 * untouched.  The call never exits and never throws; a failure's text is dmi_last_error(NULL)'s.  Synchronises. */
int dmi_filter_depth_speckles(const double *depth, const double *best_cost, double threshold, int32_t n, int32_t W, int32_t H,
                              double abs_tolerance, double rel_tolerance, int64_t min_pixels, int32_t device, double *out_depth,
                              int32_t *out_size, double *kernel_ms);

/* ---- Small depth-map holes filled before the maps are fused (added after round 5, dmi_abi_version() stays 5) ----
 * The gap interpolation of stereo pipelines: the best-cost threshold scatters single-pixel holes, the speckle filter cuts out
 * islands, and a pixel without a depth casts no ray -- it adds no surface and carves no free space.  A small hole inside a smooth
 * wall is not missing information.  dmi_fill_depth_holes labels the connected components of the pixels WITHOUT a depth in every
 * view and interpolates the small ones whose rim is continuous.  Context-free, like dmi_filter_depth_speckles: it uploads, runs
 * its kernels, downloads and frees.  It takes no cameras.
 *   depth, best_cost, threshold   exactly as dmi_filter_depth_speckles takes them: [n][H][W] f64 host in vtk point order,
 *             best_cost nullable
 *   out_depth [n][H][W] f64 host; may be `depth` itself
 *   out_size  [n][H][W] int32 host or NULL;  kernel_ms (nullable): hipEvent time of the kernels alone, summed over the pieces
 * Definition, met bit for bit by the device and by tests/depth_holes_np.py.  All arithmetic is f64, every operation is rounded
 * on its own, nothing is contracted; comparisons with a NaN are false.
 *   1. D_m = depth_m with -1 wherever best_cost_m > threshold.  A pixel is VALID iff D > 0 and D < +inf (step 1 of
 *      dmi_filter_depth_speckles).
 *   2. A HOLE is a connected component of the NOT-valid pixels of one view under 4-neighbourhood: the same row with adjacent
 *      columns, or the same column with adjacent rows.  The last pixel of a row and the first of the next are not neighbours;
 *      pixels of different views are never neighbours; nothing is flipped.  Its SIZE is its number of pixels.  It TOUCHES THE
 *      BORDER iff one of its pixels has x == 0, x == W-1, y == 0 or y == H-1.
 *   3. The RIM of a hole is the set of valid pixels that are 4-neighbours of any of its pixels.  lo is the smallest D on the rim,
 *      hi the largest: exact minima and maxima, so the order of evaluation does not matter.
 *   4. A hole is FILLABLE iff SIZE <= max_pixels, it does not touch the border, and
 *      hi - lo <= abs_tolerance + rel_tolerance * lo: the product rounded, then the sum, then the difference.  For a rim of two
 *      depths this is the LINKED predicate of dmi_filter_depth_speckles.
 *   5. For a pixel (x, y) of a fillable hole, xl < x < xr are the nearest valid columns in its row and yu < y < yd the nearest
 *      valid rows in its column.  All four exist and lie on this hole's own rim, because the hole does not touch the border.
 *      With the integer spans converted to f64 exactly:
 *        h    = (D[y][xl]*(xr-x) + D[y][xr]*(x-xl)) / (xr-xl)
 *        v    = (D[yu][x]*(yd-y) + D[yd][x]*(y-yu)) / (yd-yu)
 *        fill = (h*(yd-yu) + v*(xr-xl)) / ((yd-yu) + (xr-xl))
 *      so the shorter span gets the larger weight.  The divisions are correctly rounded; each sum is taken left to right as
 *      written.  Only INPUT depths are read, never a filled one.
 *   6. out_depth = D at a valid pixel, fill at a pixel of a fillable hole, exactly -1.0 elsewhere.  out_size = the pixel's hole
 *      size, 0 at a valid pixel; the pixels of a hole that is not fillable get their size too.  max_pixels == 0 returns D with
 *      every invalid value normalised to -1, and the sizes.
 * The result depends only on the partition into holes, on exact minima and maxima and on input depths, so it is the same to the
 * bit whatever order the hardware runs in: two calls give identical bytes.
 * Host data goes up and comes down in pieces of whole views, as many as fit 256 MiB (a single larger view goes whole, as in
 * dmi_filter_depth_speckles).  The device holds the planes of one piece at a time -- 32 bytes per pixel of the piece, 8 more with
 * best_cost, 4 more with out_size --, so device memory does not grow with n.
 * All arguments are checked before the device is touched.  DMI_ERR_INVALID_ARGUMENT, the message naming the argument: a null depth
 * or out_depth; n < 1; W or H outside [1, 32768]; max_pixels < 0; a negative, NaN or infinite abs_tolerance or rel_tolerance; a NaN
 * threshold when best_cost is given.  Then DMI_ERR_DEVICE without a device.  A refused call leaves out_depth and out_size
 * untouched.  The call never exits and never throws; a failure's text is dmi_last_error(NULL)'s.  Synchronises. */
int dmi_fill_depth_holes(const double *depth, const double *best_cost, double threshold, int32_t n, int32_t W, int32_t H,
                         double abs_tolerance, double rel_tolerance, int64_t max_pixels, int32_t device, double *out_depth,
                         int32_t *out_size, double *kernel_ms);

/* ---- Depth maps smoothed, edges preserved, before the maps are fused (added after round 5, dmi_abi_version() stays 5) ----
 * The bilateral filter that every TSDF pipeline since KinectFusion runs over each depth map first.  The filters above decide
 * WHETHER a pixel holds a depth; none changes a depth that stays, so per-pixel depth noise goes into the fusion untouched, and a
 * depth a voxel too far has carved free space that no smoothing of the fused field gives back.  dmi_smooth_depths moves every
 * valid depth to a weighted mean of the valid depths round it that lie within a tolerance of it: a spatial Gaussian times
 * Tukey's biweight of the depth difference, written so that it needs no division per tap and no transcendental on the device.
 * Context-free, like dmi_fill_depth_holes: it uploads, runs its kernel once per iteration, downloads and frees.  It takes no
 * cameras.
 *   depth, best_cost, threshold   exactly as dmi_fill_depth_holes takes them: [n][H][W] f64 host in vtk point order, best_cost
 *             nullable; best cost > threshold gives -1, applied once, before the first iteration
 *   out_depth [n][H][W] f64 host; may be `depth` itself
 *   out_count [n][H][W] int32 host or NULL: the taps taken at the pixel in the LAST iteration
 *   kernel_ms (nullable): hipEvent time of the kernels alone, summed over the pieces
 * Definition, met bit for bit by the device and by tests/depth_smooth_np.py.  All arithmetic is f64, every operation is rounded
 * on its own, nothing is contracted; comparisons with a NaN are false.
 *   Validity.  A pixel is VALID iff D > 0 and D < +inf (step 1 of dmi_filter_depth_speckles).  A pixel that is not valid comes
 *   out as -1.0, with count 0.  A valid pixel stays valid.
 *   Spatial weights (dmi_depth_smoothing_weights, host code, no device needed: *radius and weights[0..r], room for 9).
 *     r = (int)ceil(truncate * sigma)
 *     s[0] = 1, s[i] = exp(-(double)(i*i) / (2*sigma*sigma)) for i = 1..r
 *   computed on the host in double and NOT normalised: the quotient below cancels any scale.  r == 0 is legal and gives the
 *   identity on valid pixels.
 *   One iteration at a valid centre c:
 *     tau = abs_tolerance + rel_tolerance * c;   T = tau * tau;   num = 0;  den = 0;  count = 0
 *     for dy = -r..r (outer), dx = -r..r (inner), tap q inside the image and valid:
 *         delta = q - c;  u = delta * delta
 *         if (u < T):
 *             g = T - u
 *             w = (s[|dy|] * s[|dx|]) * (g * g)
 *             num = num + w * delta;  den = den + w;  count += 1
 *     out = c + num / den
 *     if !(den > 0 && den < inf && out > 0 && out < inf): out = c
 *   The test u < T is strict; a tap that fails it adds nothing.  (g * g) is (1 - u/T)^2, Tukey's biweight, up to the factor T^2
 *   that the quotient cancels.  The division is correctly rounded.  count is the number of taps taken; the centre counts
 *   whenever T > 0.  Taps never cross a row end or a view seam: a tap outside the image does not exist.
 *   Iteration k+1 reads the complete output of iteration k.  out_count is the last iteration's.
 * Consequences: a step higher than tau is not crossed, and plateaus on either side of it come out bit-identical; |out - c| <= tau
 * per iteration, up to a relative 1e-12; both tolerances zero give the identity.
 * Every output pixel depends on its iteration's input plane alone and is summed in the one order above, so the result is the
 * same to the bit whatever order the hardware runs in: two calls give identical bytes.
 * Host data goes up and comes down in pieces of whole views, as many as fit 256 MiB (a single larger view goes whole).  The device
 * holds two depth planes of one piece at a time -- 16 bytes per pixel of the piece, 8 more with best_cost, 4 more with out_count.
 * All arguments are checked before the device is touched.  DMI_ERR_INVALID_ARGUMENT, the message naming the argument: a null depth
 * or out_depth; n < 1; W or H outside [1, 32768]; a sigma that is not finite or is negative; a truncate outside (0, 4]; a radius
 * above 8; a negative, NaN or infinite abs_tolerance or rel_tolerance; iterations outside [1, 16]; a NaN threshold when best_cost
 * is given.  Then DMI_ERR_DEVICE without a device.  A refused call leaves out_depth and out_count untouched.  The call never
 * exits and never throws; a failure's text is dmi_last_error(NULL)'s.  Synchronises.
 * dmi_depth_smoothing_weights refuses (DMI_ERR_INVALID_ARGUMENT, nothing written) null pointers and the sigma, truncate and radius
 * that dmi_smooth_depths refuses. */
int dmi_depth_smoothing_weights(double sigma, double truncate, int32_t *radius, double *weights /* [9]: s[0]..s[r] */);
int dmi_smooth_depths(const double *depth, const double *best_cost, double threshold, int32_t n, int32_t W, int32_t H,
                      double sigma, double truncate, double abs_tolerance, double rel_tolerance, int32_t iterations,
                      int32_t device, double *out_depth, int32_t *out_count, double *kernel_ms);

/* ---- A resident view set: the depth maps stay on the device from the first filter to the fusion (added after
 * round 5, dmi_abi_version() stays 5) ----
 * The five calls above are context-free: each uploads the depth planes, runs a few milliseconds of kernels, downloads and frees,
 * and dmi_add_views uploads the result once more.  A dmi_view_set is bound to one device and one image size and OWNS the planes
 * between the steps: one upload (dmi_views_add), the steps on the device, and a hand-over to a fusion context that does not pass
 * through the host (dmi_add_views_from_set).  No arithmetic differs: every result is, byte for byte, what the context-free call
 * gives.
 *   D          the set's depths, [n][H][W] f64 on the device in vtk point order, NORMALISED: a valid depth (> 0 and < +inf) or -1.
 *   dmi_views_add   appends n views.  It stores step 1 of dmi_filter_depth_speckles: D = depth, with -1 wherever best_cost
 *              (nullable) > threshold and wherever the value is not valid.  The threshold is applied here, once; the costs are not
 *              kept.  K4 and RT4 ([n][16] each) are kept as they came.  May be called repeatedly.
 *   The four steps.  Each replaces D by exactly the out_depth that its context-free counterpart returns for depth = D, best_cost =
 *              NULL, the same parameters, the set's K4 / RT4, n, W and H:
 *                dmi_views_filter_speckles     dmi_filter_depth_speckles
 *                dmi_views_fill_holes          dmi_fill_depth_holes
 *                dmi_views_smooth              dmi_smooth_depths
 *                dmi_views_filter_consistency  dmi_filter_depth_consistency
 *              out_size / out_count: a nullable host array [n][H][W], exactly the counterpart's; downloaded only when asked for.
 *   dmi_views_estimate_bounds   exactly dmi_estimate_scene_bounds on D.  D is not changed.
 *   dmi_views_download          D of the views [first, first + count), [count][H][W] f64 host in vtk point order.
 *   "Exactly" means byte for byte, for every piece size: the filters work per view and the consistency count does not depend on an
 *   order, so cutting the views into pieces cannot change a bit.  dmi_views_set_piece_bytes bounds the f64 planes of the views a
 *   pass works on at a time (as many whole views as fit, at least one; the default is the context-free calls' 256 MiB); it exists
 *   to bound the scratch, and so that a test can prove the sentence before at small shapes.
 *   dmi_views_step_report (r, nullable) is computed on the device, from one read of the planes before and after the step and
 *   from the roots the labelling passes hold; no plane is downloaded for it:
 *     step          valid_before / valid_after            changed                      groups / groups_kept               aux_sum
 *     speckles      pixels with a depth / pixels kept     removed pixels               segments / segments >= min_pixels  0
 *     holes         valid pixels before / after           filled pixels                holes / holes filled               0
 *     smooth        valid pixels (equal)                  pixels whose value differs   0 / 0                              sum of the last
 *                                                         from before the call                                           iteration's taps
 *     consistency   pixels with a depth / pixels kept     removed pixels               0 / 0                              0
 *   kernel_ms is the hipEvent time of the counterpart's kernels alone, summed over the pieces; the report's own kernels are timed
 *   apart (dmi_views_info::last_report_kernel_ms).
 *   dmi_add_views_from_set leaves ctx in the state that dmi_add_views(ctx, D[first .. first + count), NULL, 0, K4, RT4, count, W, H)
 *   would: the same tables and the same DMI_DEPTH_AUTO decision (the promotion to f64 when a depth is not an f32 included), the
 *   same pyramids, validity maps and hole counters, therefore the same fused grid, dmi_get_view_paths and dmi_get_info
 *   (device_bytes apart: nothing is staged).  The upload pass reads the set's planes where they are: no staging buffer, no host copy.  The context copies and never aliases: the
 *   set stays unchanged and may be destroyed afterwards.  The call orders the set's stream before the context's upload stream and
 *   synchronises as dmi_add_views does.  Both must be on one device and the set's size must be that of the context's views
 *   (DMI_ERR_INVALID_ARGUMENT otherwise); ctx and the set must not be used by another thread meanwhile.
 * Memory.  16 bytes per pixel and view for the two planes (a step writes the alternate plane and the two change places when it
 * has succeeded: a failed step leaves D as it was); the scratch of one piece (per pixel of the piece: 16 during an add, 8 for the
 * speckle filter, 24 for the hole fill, up to 12 for the smoothing, 4 more with out_size / out_count); during a consistency or
 * bounds pass the planes in image row order and the counts, 12 bytes per pixel and view, freed when the pass ends.  For 256 views of
 * 1280 x 720 that is about 3.8 GB resident and 6.6 GB at the peak.  dmi_views_info::device_bytes is what the set holds now.
 *   dmi_views_info   n, W, H, device; device_bytes; steps: the steps that have succeeded since creation (the four, and the bounds
 *              estimates); h2d_plane_bytes / d2h_plane_bytes: the image-sized data the set has moved over PCIe since creation
 *              (depths and costs up; downloads, sizes and counts down) -- matrices and the few hundred bytes of a report do not
 *              count; last_report_kernel_ms: the hipEvent time of the last step's report kernels.
 * Errors.  Every argument check of the counterpart applies, with the same texts apart from the entry's name, and all checks run
 * before the device is touched.  DMI_ERR_INVALID_ARGUMENT besides: a null set; a step, estimate, download or hand-over on an empty
 * set; first < 0, count < 1 or first + count > n; an add whose n < 1 or whose depth, K4 or RT4 is null, or whose threshold is NaN
 * with a best_cost; piece bytes of 0.  dmi_views_create refuses a null `out` and W or H outside [1, 32768] with
 * DMI_ERR_INVALID_ARGUMENT before it reports a missing device (DMI_ERR_DEVICE) or an ordinal out of range.  A refused or failed
 * call leaves D, n and the host arrays as they were.  No call exits or throws; a failure's text is dmi_views_last_error(s)'s (s ==
 * NULL: the thread's last create failure), for dmi_add_views_from_set dmi_last_error(ctx)'s.  Every call synchronises.
 * dmi_views_clear drops the views and keeps the allocations; dmi_views_destroy(NULL) is a no-op. */
typedef struct dmi_view_set dmi_view_set;
typedef struct dmi_views_info {
  int32_t n, W, H, device;
  uint64_t device_bytes;
  uint64_t steps;
  uint64_t h2d_plane_bytes, d2h_plane_bytes;
  double last_report_kernel_ms;
} dmi_views_info;
typedef struct dmi_views_step_report {
  uint64_t valid_before, valid_after, changed, groups, groups_kept, aux_sum;
  double kernel_ms;
} dmi_views_step_report;
int dmi_views_create(int32_t device, int32_t W, int32_t H, dmi_view_set **out);
void dmi_views_destroy(dmi_view_set *s);
const char *dmi_views_last_error(const dmi_view_set *s);
int dmi_views_add(dmi_view_set *s, const double *depth, const double *best_cost, double threshold, const double *K4,
                  const double *RT4, int32_t n);
int dmi_views_clear(dmi_view_set *s);
int dmi_views_get_info(dmi_view_set *s, dmi_views_info *out);
size_t dmi_sizeof_views_info(void);
int dmi_views_set_piece_bytes(dmi_view_set *s, uint64_t bytes);
int dmi_views_filter_speckles(dmi_view_set *s, double abs_tolerance, double rel_tolerance, int64_t min_pixels, int32_t *out_size,
                              dmi_views_step_report *r);
int dmi_views_fill_holes(dmi_view_set *s, double abs_tolerance, double rel_tolerance, int64_t max_pixels, int32_t *out_size,
                         dmi_views_step_report *r);
int dmi_views_smooth(dmi_view_set *s, double sigma, double truncate, double abs_tolerance, double rel_tolerance, int32_t iterations,
                     int32_t *out_count, dmi_views_step_report *r);
int dmi_views_filter_consistency(dmi_view_set *s, double abs_tolerance, double rel_tolerance, int32_t min_views, int32_t *out_count,
                                 dmi_views_step_report *r);
int dmi_views_estimate_bounds(dmi_view_set *s, const double *axes9, double trim_fraction, int32_t pixel_step, double lo[3],
                              double hi[3], uint64_t *n_points, double *kernel_ms);
int dmi_views_download(dmi_view_set *s, int32_t first, int32_t count, double *out_depth);
int dmi_add_views_from_set(dmi_context *ctx, const dmi_view_set *s, int32_t first, int32_t count);

/* ---- The fused point cloud of a resident view set (added after round 5, dmi_abi_version() stays 5) ----
 * The other product of a set of filtered depth maps: the points the views agree on, each once, with a normal.
 * dmi_views_build_points builds it on the device from the set's current D; dmi_views_download_points brings ranges of it to the
 * host.  Definition, met bit for bit by the device and by tests/depth_points_np.py.
 * All arithmetic is f64, with every operation rounded on its own and nothing contracted.  Comparisons with a NaN are false.
 * Divisions and the square root are correctly rounded.
 * D, VALID, image coordinates (px, py) (vtk row r = image row H-1-r) and the K4 form are exactly those of
 * dmi_filter_depth_consistency.
 * Parameters: abs_tolerance, rel_tolerance: agreement.  normal_abs_tolerance, normal_rel_tolerance: normals.  min_views >= 0.
 * pixel_step >= 1.  dedupe (0/1).
 *   1. Counts.  count is step 4's out_count of dmi_filter_depth_consistency on the set's current D, with abs_tolerance,
 *      rel_tolerance.
 *   2. Candidates.  A pixel is a CANDIDATE iff it is valid, px % pixel_step == 0, py % pixel_step == 0 and count >= min_views.
 *   3. Ownership (only with dedupe).  A candidate of view s is OWNED iff there is a view t < s for which both of these hold:
 *      the pair AGREES (step 3 of the consistency definition, operation for operation, with w from step 2); the pixel of t it lands
 *      on is itself a candidate.  A candidate is EMITTED iff it is not owned.  The rule is deliberately one-directional and needs no
 *      ordering between workgroups.  The lowest view that holds a surface keeps it.
 *   4. Position.  w of step 2, as three f64.
 *   5. Normal.  c(x, y) is step 2's camera-space point of pixel (x, y) with its own depth.  A neighbour (x', y') inside the image
 *      is USABLE iff it is valid (whether or not it takes part) and fabs(d' - d) <= normal_abs_tolerance + normal_rel_tolerance*d
 *      (product rounded, then the sum, then the difference).
 *      tx: if (px+1, py) and (px-1, py) are both usable: c(px+1,py) - c(px-1,py).  If only the right one is usable:
 *      c(px+1,py) - c(px,py).  If only the left one is usable: c(px,py) - c(px-1,py).  Otherwise there is no normal.
 *      ty: likewise with (px, py+1) as the "plus" neighbour and (px, py-1) as the "minus" one.
 *      m_0 = tx_1*ty_2 - tx_2*ty_1, m_1 = tx_2*ty_0 - tx_0*ty_2, m_2 = tx_0*ty_1 - tx_1*ty_0.
 *      s = (m_0*c_0 + m_1*c_1) + m_2*c_2.  If s > 0, m = -m, so the normal faces the camera.
 *      g_j = (R[0][j]*m_0 + R[1][j]*m_1) + R[2][j]*m_2.
 *      L = sqrt((g_0*g_0 + g_1*g_1) + g_2*g_2).
 *      The point HAS A NORMAL iff tx and ty exist and L is finite and > 0.  Then n_j = g_j / L rounded to f32.  This is the form
 *      dmi_extract_isosurface_normals already uses for its last step.  Otherwise n = (0, 0, 0).
 *   6. Order.  The emitted points are stored in ascending (view, py, px).
 *   7. Per-point outputs.  xyz f64[3].  normal f32[3].  view int32.  pixel int32 = py*W + px.  count int32.
 * Build.  D is not changed.  The points stay on the device until the next dmi_views_add, dmi_views_clear, step that replaces D, or
 * build; dmi_views_estimate_bounds and dmi_views_download keep them.  A successful build counts as a step in dmi_views_info::steps,
 * and the point buffers (48 bytes per point, allocated after the scan at exactly the size needed) count in device_bytes.  If that
 * allocation fails the call returns DMI_ERR_OUT_OF_MEMORY and leaves the set, its D and any earlier points as they were.  During
 * the call the set holds the planes in image row order, the counts, a flag byte per pixel and 12 bytes per 256 pixels besides: 13
 * bytes per pixel and view, freed when the call ends.  *n_points: the number of points; zero points is DMI_OK.
 *   dmi_views_points_report (r, nullable)   valid: the valid pixels of D; candidates, owned: steps 2 and 3; points: the emitted
 *              candidates; with_normal: the points that have a normal; kernel_ms: the hipEvent time of the kernels of the build.
 *   dmi_views_get_points_pass_ms   the same time by pass: the planes' flip, the counts, the candidate and ownership flags, the block
 *              counts with their scan, the scatter.  DMI_ERR_STATE without a current build.
 * Download.  The points [first, first + count) into the arrays given, each nullable: xyz [count][3] f64, normal [count][3] f32,
 * view, pixel and n_views (the count of step 7) [count] int32.  DMI_ERR_STATE without a current build; DMI_ERR_INVALID_ARGUMENT when
 * first + count exceeds the point count.
 * The result is byte for byte the same for every dmi_views_set_piece_bytes.
 * DMI_ERR_INVALID_ARGUMENT before the device is touched, the message naming the argument: a null set or n_points; a negative, NaN
 * or infinite tolerance; min_views < 0; pixel_step < 1; dedupe outside {0, 1}; an empty set; n * ceil(W * H / 256) >= 2^31; a K4
 * outside the form (the message names the view).  A refused call leaves the set as it was.  The calls never exit, never throw, and
 * synchronise, like the rest of the section. */
typedef struct dmi_views_points_report {
  uint64_t valid, candidates, owned, points, with_normal;
  double kernel_ms;
} dmi_views_points_report;
int dmi_views_build_points(dmi_view_set *s, double abs_tolerance, double rel_tolerance, double normal_abs_tolerance,
                           double normal_rel_tolerance, int32_t min_views, int32_t pixel_step, int32_t dedupe, uint64_t *n_points,
                           dmi_views_points_report *r /* nullable */);
int dmi_views_download_points(dmi_view_set *s, uint64_t first, uint64_t count, double *xyz, float *normal, int32_t *view,
                              int32_t *pixel, int32_t *n_views /* each nullable */);
int dmi_views_get_points_pass_ms(dmi_view_set *s, double out_ms[5]);

/* ---- A point cloud thinned and merged on a voxel grid (added after round 5, dmi_abi_version() stays 5) ----
 * One point per occupied cell of a grid of one cell size, at the mean of the points that fell into it, with a merged normal: what
 * PCL's VoxelGrid or Open3D's voxel_down_sample does to a cloud (only the intent is shared, not the numbers); cells with fewer than
 * min_points members can be dropped, which is the density outlier filter of those tools.  On a cloud built with dedupe = 0 the
 * members of a cell are the same surface element as several views saw it, and the mean averages their independent depth noise.
 * csrc/depth_points_thin.hip.  Definition, met bit for bit by the device and by tests/depth_points_thin_np.py.
 * The input is a cloud of P points in a given order, each with xyz f64[3], normal f32[3] (the zero vector: no normal), view, pixel and
 * count int32; an absent input array is one of zeros.  Parameters: cell_size, min_points.  All arithmetic is f64, with every
 * operation rounded on its own, no FMA and no reassociation; comparisons with a NaN are false; divisions and the square root are
 * correctly rounded.
 *   1. BOUNDS and BINS are dmi_decimate_isosurface's, word for word, with p = xyz: lo_d and hi_d are the minimum and the maximum of
 *      xyz[i][d] over all P points (exact, independent of order); a non-finite coordinate anywhere refuses the call; with
 *      h = cell_size, b_d(i) = floor((xyz[i][d] - lo_d) / h), the subtraction and the division each rounded, no reciprocal;
 *      n_d = b_d evaluated at hi_d, plus 1; any n_d > 2^21 refuses the call (the message names the smallest acceptable cell size);
 *      the key (b_2*n_1 + b_1)*n_0 + b_0 stays within 63 bits.
 *   2. CELLS.  A cell is the set of all input points with the same (b_0, b_1, b_2).  Cells are ordered by ascending (b_2, b_1, b_0);
 *      the members m_0 < m_1 < ... of a cell are taken in ascending input index (for a view set's cloud: ascending (view, py, px)).
 *   3. KEPT.  A cell of k members is kept iff k >= min_points (min_points >= 1).
 *   4. One output point per kept cell, in cell order:
 *      xyz_d = (((xyz[m_0][d] + xyz[m_1][d]) + xyz[m_2][d]) + ...) / (double)k, the first member starting the sum (a cell of one
 *      keeps its point's bits, a -0.0 included);
 *      normal: with k == 1 the member's, copied.  Otherwise t_j = (((double)normal[m_0][j] + (double)normal[m_1][j]) + ...) over all
 *      members (one without a normal adds its zeros), L = sqrt((t_0*t_0 + t_1*t_1) + t_2*t_2), and n_j = (float)(t_j / L) iff L is
 *      finite and > 0; otherwise the normal is (0, 0, 0);
 *      view and pixel: those of m_0 (a colour looked up through them is a real member's);
 *      count: the maximum of the members' counts;  members (uint32): k.
 *   5. REPORT (dmi_points_thin_report).  points_in: P.  cells: the occupied cells.  cells_kept: the kept ones = the output's points.
 *      multi_view_cells: kept cells whose first and last member differ in view.  largest_cell: the most members any cell has, kept
 *      or not.  with_normal: output points whose normal is not the zero vector.  kernel_ms: the hipEvent time of the call's kernels.
 *
 * dmi_thin_point_cloud is context-free, like the depth-map filters: host arrays in, host arrays out; it uploads in pieces, runs the
 * kernels, downloads and frees.  normal, view, pixel and count are nullable, and so are out_members and r; the other output arrays
 * hold P entries and may be the input arrays.  *n_out: the output's points.  P == 0 is a success with 0 points that touches no
 * device.  DMI_ERR_INVALID_ARGUMENT before the device is touched: a cell_size that is NaN, infinite or <= 0; min_points < 1;
 * P >= 2^32; a null xyz, output array or n_out; a device out of range.  The refusals of step 1, made on the device's bounds, return
 * DMI_ERR_INVALID_ARGUMENT too.  A call that is refused or fails leaves the outputs untouched.  dmi_last_error(NULL) has the text.
 *
 * dmi_views_thin_points replaces the set's current cloud (dmi_views_build_points) by exactly what dmi_thin_point_cloud returns for
 * it: the same implementation, with no copy to the host.  The result is built beside the old cloud and swapped in last: a call that
 * is refused or fails leaves the old cloud.  DMI_ERR_STATE without a current build, and on a cloud that is thinned already (a
 * centroid of centroids is not the centroid: build again).  A success counts as a step in dmi_views_info::steps; the thinned cloud
 * (52 bytes a point) counts in device_bytes; whatever drops the built cloud drops this one.  dmi_views_download_points serves the
 * thinned cloud as it serves the built one.  During the call the set holds 68 bytes per input point besides the two clouds
 * (DESIGN.md 8o), freed when it ends.  It synchronises three times: for the bounds, for the counts, for the report.
 *   dmi_views_download_point_members   k of the points [first, first + count); 1 for every point of a cloud that is not thinned.
 *              DMI_ERR_STATE without a current build.
 *   dmi_views_get_thin_pass_ms   the last thinning's kernel time by pass: bounds, keys, sort, ranks with their scans,
 *              representatives.  DMI_ERR_STATE unless the current cloud is a thinned one.
 *   dmi_views_set_thin_wave_cell_points   a cell of more than k members (k >= 1) is summed by a wave of its own, any other by one
 *              lane.  Like dmi_color_set_render_queue_capacity, no value changes a bit of the result; it lets a test drive the wave
 *              pass at small shapes.  dmi_thin_point_cloud uses the default, 32. */
typedef struct dmi_points_thin_report {
  uint64_t points_in, cells, cells_kept, multi_view_cells, largest_cell, with_normal;
  double kernel_ms;
} dmi_points_thin_report;
int dmi_thin_point_cloud(const double *xyz, const float *normal /* nullable */, const int32_t *view /* nullable */,
                         const int32_t *pixel /* nullable */, const int32_t *count /* nullable */, uint64_t n_points, double cell_size,
                         int32_t min_points, int32_t device, double *out_xyz, float *out_normal, int32_t *out_view, int32_t *out_pixel,
                         int32_t *out_count, uint32_t *out_members /* nullable */, uint64_t *n_out,
                         dmi_points_thin_report *r /* nullable */);
int dmi_views_thin_points(dmi_view_set *s, double cell_size, int32_t min_points, uint64_t *n_points,
                          dmi_points_thin_report *r /* nullable */);
int dmi_views_download_point_members(dmi_view_set *s, uint64_t first, uint64_t count, uint32_t *out);
int dmi_views_get_thin_pass_ms(dmi_view_set *s, double out_ms[5]);
int dmi_views_set_thin_wave_cell_points(dmi_view_set *s, int32_t k);

/* ---- Point-cloud outliers dropped by radius neighbour count (added after round 5, dmi_abi_version() stays 5) ----
 * Every point's number of other points within a radius, and the cloud without the points that have too few: what PCL's
 * RadiusOutlierRemoval or Open3D's remove_radius_outlier does to a cloud.  A count in a ball depends on no grid -- min_points of the
 * thinning drops good surface that a cell face cuts off, and keeps a stray next to a full cell -- and, being an integer, is defined
 * to the bit whatever the schedule.  csrc/depth_points_radius.hip.  Definition, met bit for bit by the device and by
 * tests/depth_points_radius_np.py, which counts over all pairs.
 * The input is P points xyz f64[P][3] in a given order.  Parameters: radius, min_neighbors.  All arithmetic is f64, with every
 * operation rounded on its own and no FMA; comparisons with a NaN are false.
 *   1. r2 = radius * radius.
 *   2. For points i != j: d_k = xyz[j][k] - xyz[i][k], d2 = (d_0*d_0 + d_1*d_1) + d_2*d_2.
 *   3. j is a NEIGHBOUR of i iff d2 <= r2.  The relation is symmetric; coincident points are neighbours of each other; a point is
 *      never its own neighbour, by index, not by position.
 *   4. neighbors[i] (uint32) is the number of neighbours of i.
 *   5. KEPT iff neighbors[i] >= min_neighbors.
 *   6. The output is the kept points in input order, every array of a kept point carried bit for bit -- xyz, normal, view, pixel,
 *      count, and members when the cloud is a thinned one --, with its neighbors[i], counted in the input cloud.
 *   7. REPORT (dmi_points_radius_report).  points_in: P.  points_kept.  isolated: points with neighbors == 0.  max_neighbors.
 *      neighbor_sum: the sum of the counts (always even).  distance_tests: the d2 the implementation evaluated for its queries; not
 *      part of the definition, only >= neighbor_sum, there so that the search's overhead can be computed.  kernel_ms: the hipEvent
 *      time of the call's kernels.
 * The search grid is an implementation detail: cells of h = max(radius * (1 + 2^-10), the smallest h with at most 2^21 bins on every
 * axis), so a far-away stray makes the cells larger -- which costs time -- instead of refusing the call; the radius is never refused
 * for being small against the cloud's extent.  DMI_ERR_INVALID_ARGUMENT, before the device is touched: a radius that is NaN,
 * infinite or <= 0, or whose square is not a normal positive number; min_neighbors < 0; P >= 2^32; null pointers; a device out of
 * range.  A non-finite coordinate, found by the bounds pass, is refused with the same code.  Nothing else is refused.
 *
 * dmi_count_point_neighbors is context-free: the coordinates go up in pieces, out_neighbors[P] and (nullable) out_keep[P], 1 where
 * kept, come back, *n_kept is the number kept; compacting host arrays is the caller's one line.  P == 0 is a success that touches no
 * device.  A call that is refused or fails leaves the outputs untouched.  dmi_last_error(NULL) has the text.
 *
 * dmi_views_filter_points_radius runs the same implementation on the set's current cloud, built or thinned, and replaces it by the
 * kept points: a buffer of its own at exactly the size needed, swapped in last, so a call that is refused or fails leaves the old
 * cloud.  DMI_ERR_STATE without a current build.  It may be called repeatedly (each call counts in the cloud it finds);
 * min_neighbors = 0 drops nothing and only annotates; zero kept points is DMI_OK.  A success counts as a step in
 * dmi_views_info::steps; device_bytes follows every allocation, and after the call holds 48 + 4 bytes per kept point (52 + 4 for a
 * thinned cloud) in place of the old cloud.  dmi_views_download_points and dmi_views_download_point_members serve the filtered cloud
 * unchanged; dmi_views_thin_points on a filtered cloud that was not thinned before gives what dmi_thin_point_cloud gives for the
 * downloaded filtered arrays, and drops the counts with the old cloud; whatever drops the built cloud drops this one.  During the
 * call the set holds 56 bytes per input point besides the two clouds, freed when it ends.
 *   dmi_views_download_point_neighbors   neighbors of the points [first, first + count).  DMI_ERR_STATE unless the current cloud
 *              came out of the filter.
 *   dmi_views_get_radius_pass_ms   the last filter's kernel time by pass: bounds, keys, sort, ranks, permute, count, compaction.
 *              DMI_ERR_STATE unless the current cloud came out of the filter.
 *   dmi_views_set_radius_group_points   a wave of the count kernel takes at most k points of one grid row as its queries
 *              (1 <= k <= 64).  No value changes a bit of the result; it lets a test drive every path at small shapes.
 *              dmi_count_point_neighbors uses the default, 64. */
typedef struct dmi_points_radius_report {
  uint64_t points_in, points_kept, isolated, max_neighbors, neighbor_sum, distance_tests;
  double kernel_ms;
} dmi_points_radius_report;
int dmi_count_point_neighbors(const double *xyz, uint64_t n_points, double radius, int32_t min_neighbors, int32_t device,
                              uint32_t *out_neighbors /* [n_points] */, uint8_t *out_keep /* [n_points], nullable */, uint64_t *n_kept,
                              dmi_points_radius_report *r /* nullable */);
int dmi_views_filter_points_radius(dmi_view_set *s, double radius, int32_t min_neighbors, uint64_t *n_points,
                                   dmi_points_radius_report *r /* nullable */);
int dmi_views_download_point_neighbors(dmi_view_set *s, uint64_t first, uint64_t count, uint32_t *out);
int dmi_views_get_radius_pass_ms(dmi_view_set *s, double out_ms[7]);
int dmi_views_set_radius_group_points(dmi_view_set *s, int32_t k);

/* ---- Local planes fitted to the point cloud: denoised positions, new normals (added after round 5,
 * dmi_abi_version() stays 5) ----
 * A plane fitted to the points within a radius of every point, the point moved onto it along the plane's normal and its normal
 * replaced by the plane's: what PCL's MovingLeastSquares (a plane, unweighted) and NormalEstimation, or Open3D's estimate_normals,
 * do to a cloud (only the intent is shared, not the numbers).  A floating-point sum over neighbours depends on its order; here the
 * sums are sums of integers -- the offsets are rounded to a power-of-two lattice of 2^-15 to 2^-16 of the radius --, and the fit
 * from them is written down operation for operation, so the result is defined to the bit whatever the schedule.
 * csrc/depth_points_planes.hip, csrc/depth_points_planes_rules.h.  Definition, met bit for bit by the device and by
 * tests/depth_points_planes_np.py, which goes over all pairs.
 * The input is P points xyz f64[P][3] in a given order and, optionally, normal f32[P][3] (absent: zeros).  Parameters: radius,
 * min_neighbors >= 2, flags (DMI_PLANE_FIT_MOVE, DMI_PLANE_FIT_NORMALS or both; 0 is refused).  All arithmetic is f64, with every
 * operation rounded on its own and no FMA; comparisons with a NaN are false; divisions and the square root are correctly rounded.
 *   1. MEMBERS.  r2 = radius * radius.  For every j, j = i included: d_k = xyz[j][k] - xyz[i][k], d2 = (d_0*d_0 + d_1*d_1) + d_2*d_2;
 *      j is a MEMBER of i's ball iff d2 <= r2.  m is the number of members and neighbors[i] = m - 1: exactly
 *      dmi_count_point_neighbors' count.
 *   2. LATTICE.  radius = f * 2^e with f in [0.5, 1) (frexp).  s = 2^(15 - e), inv_s = 2^(e - 15).  q_k = rint(d_k * s), ties to
 *      even, an integer.  For a member |d_k| <= radius (1 + 2^-51), so |q_k| <= 2^15.
 *   3. MOMENTS over the members: S_k = sum q_k, T_ab = sum q_a q_b for ab in 00, 01, 02, 11, 12, 22.  Sums of integers: any order
 *      gives the same value, and with m <= 2^22 every partial sum is below 2^52, exact in an f64.  A point with m > 2^22 is CROWDED:
 *      it is left as it is and counted.
 *   4. FIT, only if m - 1 >= min_neighbors; otherwise the point is UNSUPPORTED and left as it is.  c_k = S_k / m.
 *      C_ab = T_ab / m - c_a*c_b (the quotient, the product, then the difference).  A = C, V = the identity.  Six sweeps of cyclic
 *      Jacobi over the pairs (p, q) = (0,1), (0,2), (1,2), r the third index, a = A_pq; the pair is skipped if a == 0, otherwise:
 *        theta = (A_qq - A_pp) / (2*a);  t = sgn(theta) / (fabs(theta) + sqrt(theta*theta + 1)), sgn(x) = -1 iff x < 0, else +1 (an
 *        infinite theta*theta gives t = +-0);  c = 1 / sqrt(t*t + 1);  sigma = t*c;
 *        A_pp = A_pp - t*a;  A_qq = A_qq + t*a;  A_pq = 0;
 *        (A_rp, A_rq) = (c*A_rp - sigma*A_rq, sigma*A_rp + c*A_rq), from the old values;
 *        (V_kp, V_kq) = (c*V_kp - sigma*V_kq, sigma*V_kp + c*V_kq) for k = 0, 1, 2.
 *      lambda_k = A_kk.  The normal n is column k of V for the smallest lambda_k (the lowest index at ties: 1 replaces 0 iff
 *      lambda_1 < lambda_0, 2 replaces that iff lambda_2 is smaller still), divided by sqrt((n_0*n_0 + n_1*n_1) + n_2*n_2).
 *   5. ORIENTATION.  o = the point's old normal widened to f64.  g = (n_0*o_0 + n_1*o_1) + n_2*o_2.  g < 0 negates n.  If g == 0 (a
 *      zero old normal, or no normals given) the component of largest magnitude is made positive (the lowest index at ties).
 *   6. RESULTS.  plane_rms[i] = (float)(sqrt(max(lambda_min, 0)) * inv_s): the RMS distance of the ball's lattice points from the
 *      plane.  With MOVE: t = ((c_0*n_0 + c_1*n_1) + c_2*n_2) * inv_s and xyz'[i][k] = xyz[i][k] + t*n_k (the product, then the sum).
 *      With NORMALS: normal'[i][k] = (float)n_k.  An array whose flag is not set keeps its bits.  Unsupported and crowded points keep
 *      the bits of both arrays and get plane_rms = -1.  Everything is computed from the input cloud; nothing is iterated: a second
 *      call is a second pass.  The order and every other array of the cloud keep their bits.
 *   7. REPORT (dmi_points_planes_report).  points_in: P.  fitted, unsupported, crowded: they add up to P.  max_neighbors,
 *      neighbor_sum, distance_tests: as in dmi_points_radius_report (distance_tests counts a point's test against itself).
 *      max_shift: the largest fabs(t) of step 6 (0 without MOVE).  kernel_ms: the hipEvent time of the call's kernels.
 * The lattice's cost: on a noisy sphere cap (sigma 0.004, radii 0.05 and 0.1) the moved positions differ from those of the same fit
 * on a 2^20 lattice by at most 1.2e-5 of the radius, 3 to 4 thousand times below the noise.
 * DMI_ERR_INVALID_ARGUMENT, before the device is touched: what dmi_count_point_neighbors refuses in a radius, and a radius for which
 * s or inv_s is not a normal finite number; min_neighbors < 2; flags outside {1, 2, 3}; P >= 2^32; a null xyz, or a null output
 * whose flag is set; a device out of range.  A non-finite coordinate, found by the bounds pass, is refused with the same code.
 *
 * dmi_fit_point_planes is context-free: the coordinates go up in pieces; out_xyz[P][3] (with MOVE), out_normal[P][3] (with NORMALS),
 * out_plane_rms[P] and out_neighbors[P] come back, each nullable where not asked for (an output whose flag is not set is not
 * written).  P == 0 is a success that touches no device.  A call that is refused or fails leaves the outputs untouched.
 * dmi_last_error(NULL) has the text.
 *
 * dmi_views_fit_point_planes runs the same implementation on the set's current cloud -- built, thinned or filtered -- and replaces it
 * by a cloud of the same layout (members and the filter's neighbors stay where they are) with the new positions and normals: a
 * buffer of its own, swapped in last, so a call that is refused or fails leaves the old cloud.  DMI_ERR_STATE without a current
 * cloud.  It may be called repeatedly: each call is a pass over the cloud it finds.  A success counts as a step in
 * dmi_views_info::steps; device_bytes follows every allocation, and after the call holds the cloud's bytes and 4 bytes per point of
 * plane_rms, in a buffer of its own that whatever replaces or drops the cloud drops: a build, dmi_views_thin_points,
 * dmi_views_filter_points_radius, a change of the depths.  dmi_views_thin_points after a fit gives what dmi_thin_point_cloud gives
 * for the downloaded arrays.  dmi_views_set_radius_group_points applies to the fit kernel as to the count kernel.  During the call
 * the set holds 60 bytes per point besides the two clouds, freed when it ends.
 *   dmi_views_download_point_plane_rms   plane_rms of the points [first, first + count).  DMI_ERR_STATE unless the fit was the
 *              cloud's last step.
 *   dmi_views_get_plane_fit_pass_ms   the last fit's kernel time by pass: bounds, keys, sort, ranks, permute, fit.  DMI_ERR_STATE
 *              unless the fit was the cloud's last step. */
#define DMI_PLANE_FIT_MOVE 1
#define DMI_PLANE_FIT_NORMALS 2
typedef struct dmi_points_planes_report {
  uint64_t points_in, fitted, unsupported, crowded, max_neighbors, neighbor_sum, distance_tests;
  double max_shift, kernel_ms;
} dmi_points_planes_report;
int dmi_fit_point_planes(const double *xyz, const float *normal /* nullable */, uint64_t n_points, double radius, int32_t min_neighbors,
                         int32_t flags, int32_t device, double *out_xyz, float *out_normal, float *out_plane_rms,
                         uint32_t *out_neighbors /* each nullable where not asked for */, dmi_points_planes_report *r /* nullable */);
int dmi_views_fit_point_planes(dmi_view_set *s, double radius, int32_t min_neighbors, int32_t flags,
                               dmi_points_planes_report *r /* nullable */);
int dmi_views_download_point_plane_rms(dmi_view_set *s, uint64_t first, uint64_t count, float *out);
int dmi_views_get_plane_fit_pass_ms(dmi_view_set *s, double out_ms[6]);

/* ---- One fusion over several MI355X of a node (north star: "depth maps shard across the 8 GPUs of one node with a
 * single RCCL all-reduce of the float TSDF grid over xGMI").  The reference has nothing of the kind (one GPU, default
 * stream, cu:302-386); the seam where this plugs in is the pair of driver calls at
 * Reconstruction/vtkCudaReconstructionFilter.cxx:171-176.
 *
 * A dmi_multi_context is `world` ranks, one per GPU, either all inside this process (dmi_multi_create: one thread
 * drives every device, ncclCommInitAll) or one per process (dmi_multi_create_rank: ncclCommInitRank with a unique id
 * that the launcher distributes -- MPI, torch.distributed, a file).  RCCL (librccl.so.1) is loaded on first use;
 * single-GPU users never need it.
 *
 * Partitions:
 *   DMI_PARTITION_VIEWS    rank r fuses its contiguous share of every batch of views into a private full grid, then
 *                          the grids are summed across ranks (exchange below).  Per-voxel summation order changes:
 *                          |result - single-GPU f64 result| <= 2*world*2^-24*sum|partials| for an f32 grid.
 *   DMI_PARTITION_Z_SLABS  rank r owns the cell layers dmi_multi_z_slab(nz, r, world) and fuses ALL views into them:
 *                          no exchange step at all, bit-identical to one single-GPU fusion.
 * Exchange (VIEWS only):
 *   DMI_EXCHANGE_ALL_REDUCE      the contract: every rank ends with the whole summed grid.  The fusion runs in
 *                                n_slabs z-slabs (dmi_fuse_slab) and the all-reduce of slab i runs on a second stream
 *                                while slab i+1 is fused; the last slab is the thinnest (its exchange is the only part
 *                                nothing hides).
 *   DMI_EXCHANGE_REDUCE_SCATTER  for when only the host consumes the grid: rank r ends with the sum of its own 1/world
 *                                of the grid (half the xGMI traffic) and downloads just that.
 *   DMI_EXCHANGE_PEER_COPY       the all-reduce without RCCL and without a compute unit for the transfers (ranks of ONE
 *                                process, dmi_multi_create; at most 16): behind every slab each rank sends the others their
 *                                1/world chunk of it with peer-to-peer copies (the SDMA engines, all xGMI links at once),
 *                                adds what it received to its own chunk IN RANK ORDER with a small kernel queued behind its
 *                                fusion, and copies the sum back into every grid.  Same contract as ALL_REDUCE (every rank
 *                                ends with the whole summed grid) and the same tolerance; unlike a ring's, the order of the
 *                                additions is fixed: the result is the same bits on every run and on every rank.  Several
 *                                of its ranks may share a device (rehearsals on a one-GPU box). */
typedef struct dmi_multi_context dmi_multi_context;

typedef enum dmi_partition { DMI_PARTITION_VIEWS = 0, DMI_PARTITION_Z_SLABS = 1 } dmi_partition;
typedef enum dmi_exchange { DMI_EXCHANGE_ALL_REDUCE = 0, DMI_EXCHANGE_REDUCE_SCATTER = 1, DMI_EXCHANGE_PEER_COPY = 2 } dmi_exchange;

#define DMI_UNIQUE_ID_BYTES 128 /* = NCCL_UNIQUE_ID_BYTES */

typedef struct dmi_multi_options {
  int32_t grid_dtype;     /* DMI_F32 (the north star's all-reduce type) or DMI_F64 */
  int32_t depth_storage;  /* dmi_depth_storage */
  int32_t kernel_variant; /* as dmi_options */
  int32_t partition;      /* dmi_partition */
  int32_t exchange;       /* dmi_exchange */
  int32_t n_slabs;        /* z-slabs of the overlapped all-reduce; 0 = default (4), 1 = fuse whole grid, then exchange */
} dmi_multi_options;

typedef struct dmi_multi_info {
  int32_t world;          /* ranks of the fusion = GPUs */
  int32_t n_local;        /* ranks driven by this process */
  int32_t first_rank;     /* rank of local device 0 (the others follow consecutively) */
  int32_t rccl_ranks;     /* what ncclCommCount reports for local rank 0's communicator; 0 = no communicator (Z_SLABS) */
  int32_t rccl_version;   /* ncclGetVersion, 0 when RCCL was never loaded */
  int32_t partition, exchange, n_slabs;
  int64_t n_voxels;       /* of the whole grid */
  int64_t n_views_total;  /* views handed to dmi_multi_add_views so far */
  int64_t n_views_local;  /* of those, resident on this process's devices (VIEWS: the shards; Z_SLABS: all, per device) */
} dmi_multi_info;

typedef struct dmi_multi_timings {
  double last_step_ms;        /* hipEvents on local rank 0's compute stream around one dmi_multi_fuse: reset + fusion +
                                 whatever of the exchange the fusion did not hide */
  double last_fuse_kernel_ms; /* of that, the fusion launches of local rank 0 (dmi_timings.last_fuse_kernel_ms summed
                                 over the slabs) */
  double total_step_ms;
  uint64_t steps;
} dmi_multi_timings;

void dmi_multi_default_options(dmi_multi_options *opt); /* f32 grid, AUTO depth storage, VIEWS + ALL_REDUCE, 4 slabs */

/* Pure partition arithmetic (no GPU needed), the same on every rank:
 * contiguous balanced share [*first, *first + *count) of n items for `rank` of `world` (the first n % world ranks
 * get one more) */
int dmi_multi_view_shard(int64_t n, int32_t rank, int32_t world, int64_t *first, int64_t *count);
/* cell layers [*z_first, *z_first + *z_count) owned by `rank` under DMI_PARTITION_Z_SLABS: boundaries are multiples of
 * DMI_Z_SLAB_ALIGNMENT (16, the tallest voxel column of the fusion kernel: each rank's slab is a grid of its own, created
 * with dmi_options.z_first, not a dmi_fuse_slab range -- those need DMI_SLAB_ALIGNMENT) except the top of the grid; a rank
 * may own nothing when nz is small */
#define DMI_Z_SLAB_ALIGNMENT 16
int dmi_multi_z_slab(int32_t nz, int32_t rank, int32_t world, int32_t *z_first, int32_t *z_count);
/* DMI_EXCHANGE_PEER_COPY: the piece [*first, *first + *count) of an n-element slab that rank `c` sums and hands back
 * (pieces are multiples of 256 elements; the last ranks' may be short or empty) */
int dmi_multi_peer_chunk(int64_t n, int32_t world, int32_t c, int64_t *first, int64_t *count);
/* the z-slabs of the overlapped exchange: writes at most max_slabs (z_first, z_count) pairs, returns how many */
int dmi_multi_slab_ranges(int32_t nz, int32_t n_slabs, int32_t *z_first, int32_t *z_count, int32_t max_slabs);

/* All ranks in this process: devices[0..n) are HIP ordinals, rank i runs on devices[i]. */
int dmi_multi_create(const dmi_grid_desc *grid, const dmi_ray_potential *ray, const dmi_multi_options *opt,
                     const int32_t *devices, int32_t n, dmi_multi_context **out);
/* One rank per process.  Rank 0 calls dmi_multi_get_unique_id and the launcher hands the 128 bytes to every rank;
 * all ranks then call dmi_multi_create_rank (collective: returns when every rank has joined). */
int dmi_multi_get_unique_id(uint8_t id[DMI_UNIQUE_ID_BYTES]);
int dmi_multi_create_rank(const dmi_grid_desc *grid, const dmi_ray_potential *ray, const dmi_multi_options *opt,
                          int32_t device, int32_t rank, int32_t world, const uint8_t id[DMI_UNIQUE_ID_BYTES],
                          dmi_multi_context **out);
void dmi_multi_destroy(dmi_multi_context *ctx);
const char *dmi_multi_last_error(const dmi_multi_context *ctx); /* ctx == NULL: the thread's last create failure */

/* Same arguments as dmi_add_views / dmi_add_views_f32, called with the SAME batch on every rank (every process passes
 * the whole batch; each takes what its ranks need: VIEWS -> the rank's share of this batch, Z_SLABS -> all of it). */
int dmi_multi_add_views(dmi_multi_context *ctx, const double *depth, const double *best_cost, double threshold,
                        const double *K4, const double *RT4, int32_t n, int32_t width, int32_t height);
int dmi_multi_add_views_f32(dmi_multi_context *ctx, const float *depth, const double *K4, const double *RT4, int32_t n,
                            int32_t width, int32_t height);
/* Views that belong to local rank `local_index` only, for callers that partition themselves (dmi_multi_view_shard) and
 * never hold the whole batch in one process -- e.g. one process per GPU, each reading its own share of the list files. */
int dmi_multi_add_local_views(dmi_multi_context *ctx, int32_t local_index, const double *depth, const double *best_cost,
                              double threshold, const double *K4, const double *RT4, int32_t n, int32_t width, int32_t height);
int dmi_multi_add_local_views_f32(dmi_multi_context *ctx, int32_t local_index, const float *depth, const double *K4,
                                  const double *RT4, int32_t n, int32_t width, int32_t height);
int dmi_multi_clear_views(dmi_multi_context *ctx);

/* One whole fusion: zero the grids, fuse every resident view, exchange.  Asynchronous; collective across ranks. */
int dmi_multi_fuse(dmi_multi_context *ctx);
int dmi_multi_synchronize(dmi_multi_context *ctx);

/* The fused grid, n_voxels elements, x fastest.  What this process can write, it writes:
 *   ALL_REDUCE: the whole grid (from local rank 0);  REDUCE_SCATTER / Z_SLABS: the parts its ranks own, at their
 *   place in `out` (a single-process context therefore always fills all of `out`).
 * owned_first / owned_count (nullable) receive the contiguous element range this process wrote. */
int dmi_multi_download_grid_f32(dmi_multi_context *ctx, float *out, int64_t *owned_first, int64_t *owned_count);
int dmi_multi_download_grid_f64(dmi_multi_context *ctx, double *out, int64_t *owned_first, int64_t *owned_count);

int dmi_multi_get_info(dmi_multi_context *ctx, dmi_multi_info *out);
int dmi_multi_get_timings(dmi_multi_context *ctx, dmi_multi_timings *out);
/* the single-GPU context of local rank i (views, timings, diagnostics); owned by the multi context */
int dmi_multi_local_context(dmi_multi_context *ctx, int32_t local_index, dmi_context **out);

int dmi_abi_version(void);
int dmi_device_count(void);

#ifdef __cplusplus
}
#endif

#endif /* DMI_H_ */
