// fusion_kernels.h -- device-side records and launchers shared by the C ABI (dmi_capi.hip, dmi_capi_views.hip,
// dmi_capi_fuse.hip) and the kernels (fusion_kernels.hip: general kernel + upload helpers; fusion_tile.hip: the
// register-tiled kernel for axis-aligned grids and pinhole cameras).  gfx950 only.  The per-view records (MapRec, TileMapRec,
// WinRec, FootRec), their constants and the host arithmetic that fills them: view_records.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "fusion_launch_rules.h"  // the variant bits and the thresholds of the launch decisions
#include "point_smooth_rules.h"   // the point smoothing's radius cap and weights
#include "view_records.h"         // the per-view records, the validity maps' and the window column's constants

struct dmi_context;  // include/dmi.h

namespace dmi {

// The grid's device pointer for a writer that stores sums of grids free of -0.0 (dmi_multi.hip's exchanges): unlike
// dmi_grid_device_pointer it leaves the context's "no sum is -0.0" bookkeeping alone (dmi_capi.hip)
int grid_pointer_for_sums(::dmi_context *ctx, void **ptr);

// One tile of a depth table's min/max pyramid (level L: 2^L x 2^L pixels).  dmin/dmax bound every value of
// the tile that is neither the -1 sentinel nor a NaN (rounded outward to f32); flags say what else is there.
struct alignas(16) DepthTile {
  float dmin, dmax;
  uint32_t flags;  // TILE_* bits
  uint32_t pad;
};
// TILE_PART_HOLE_FREE / TILE_PART_NO_VALID: some 8 x 8 tile under this one holds no "no depth" pixel / no valid depth (set at
// the finest level, OR-ed upwards like the others).  With neither over a box's footprint, holes and depths are mingled
// everywhere in it (a depth map after the best-cost threshold): what the coarse classification asks before it lets a box's
// bricks inherit a per-voxel class.
enum TileFlags : uint32_t { TILE_HAS_SENTINEL = 1, TILE_HAS_VALID = 2, TILE_HAS_NAN = 4, TILE_PART_HOLE_FREE = 8, TILE_PART_NO_VALID = 16 };
// coarse class table only: the box's bricks already hold the (BRICK_MIXED) class of the byte's low bits
constexpr uint8_t COARSE_CHILDREN_WRITTEN = 0x80;

constexpr int kPyramidMinLevel = 3;   // finest level kept: 8 x 8 pixel tiles
constexpr int kPyramidMaxLevels = 13; // up to 2^15 pixels per axis

// Geometry of the pyramid, identical for every view of a context (all share W x H).
struct PyramidDesc {
  int32_t n_levels;                       // levels kPyramidMinLevel .. kPyramidMinLevel + n_levels - 1
  int32_t total_tiles;                    // tiles per view over all levels
  int32_t width[kPyramidMaxLevels];       // tiles per row at each level
  int32_t height[kPyramidMaxLevels];
  int32_t offset[kPyramidMaxLevels];      // first tile of each level within a view's pyramid
};

#ifndef DMI_TIER1
#define DMI_TIER1 1  // 0: every instantiation selects its pixels in fp64 only (A/B builds, tools/exp_list*.txt)
#endif
// class byte of a pair of class MIXED_FREE_OR_NODEPTH that has no window (kWindowCols, view_records.h)
constexpr uint8_t CLASS_NO_WINDOW = 0x20;
// Per windowed (brick, view) pair, TileArgs::win_origin[win_pair_index(brick, view, bricks)]: the window's first pixel (padded-image
// coordinates, x0 | y0 << 16) and the fp32 images of hw.x, hw.y and c.z at voxel (0, 0, 0) of the brick
struct alignas(16) WinPair {
  uint32_t origin;
  float ax, ay, acz;
};
static_assert(sizeof(WinPair) == 16, "WinPair layout");

struct FuseArgs {
  int32_t nx, ny, nz;  // voxels (cells) per axis
  int32_t W, H;        // depth-map dims (c_depthMapDims, cu:59)
  int32_t first_map, n_maps;
  int32_t init_from_grid;  // 0: grid is known to be all zero, skip the read
  int32_t kz0, pad1;       // global cell index of this context's first z layer (dmi_options::z_first)
  int32_t k_first, k_count;  // cell layers [k_first, k_first + k_count) of the context's grid to fuse (dmi_fuse_slab)
  double ox, oy, oz;       // c_gridOrig
  double sx, sy, sz;       // c_gridSpacing
  double g[12];            // rows 0..2 of c_gridMatrix
  double thick, delta;     // c_rayPotentialThick / Delta
  double rho_pos, rho_neg, rho_zero;  // rho * (+1, -1, 0): the plateau values rho*sign (cu:117)
  double slope;                       // rho / thick (cu:119), divided on the host in fp64
  double free_space;                  // -eta * rho (cu:115)
  const MapRec *maps;
  void *grid;                    // float or double [nz][ny][nx]
  uint32_t *voxel_hits;          // nullable
  unsigned long long *map_hits;  // nullable, indexed by absolute map id
};

// Kernel argument of the tiled kernel: only what its main loop keeps in SGPRs.  Everything the rare
// exact fallback needs beyond this is read from `full`, a device copy of FuseArgs, inside the branch.
struct TileArgs {
  int32_t nx, ny, nz, W, H, first_map, n_maps, init_from_grid;
  int32_t kpad;                          // row pitch of cz_table (nz rounded up to the column height)
  int32_t bricks_x, bricks_y, bricks_z;  // workgroup bricks per axis
  int32_t super_x, super_y, super_z;     // super-bricks (4 x 4 x 2 bricks) per axis to fuse, XCD-aware ordering
  int32_t sbz_first, pad3;               // first super-brick layer of the slab being fused (dmi_fuse_slab); 0 = whole grid
  int32_t slot_base, slot_count;         // = sbz_first * super_x * super_y * 32, super_x * super_y * super_z * 32
  int32_t depth_bytes;                   // W * H * sizeof(depth element): buffer range of one depth table
  int32_t kz0, pad1;                     // global cell index of the first z layer
  double ox, oy, oz, sx, sy, sz;         // c_gridOrig, c_gridSpacing
  double g[12];                          // rows 0..2 of c_gridMatrix (3x3 part diagonal)
  double thick, delta, rho_pos, rho_neg, slope, free_space;  // as in FuseArgs
  const TileMapRec *tile_maps;           // [n_views]
  const double *cz_table;                // [n_views][kpad]: r22[m] * wz(k), the exact product (cu:92)
  void *grid;
  uint32_t *voxel_hits;
  unsigned long long *map_hits;
  const FuseArgs *full;                  // device memory
  // brick classes (fusion_classify.hip): one byte per (wave brick, map), 16-byte aligned rows of class_pitch
  // bytes; nullptr = every pair takes the full path
  const uint8_t *classes;
  int32_t class_pitch;
  int32_t wbricks_x, wbricks_y;          // wave bricks (8 x 8 x column) per axis, x fastest
  int32_t xcd_run_wg;                    // workgroups dealt to one XCD in a row
  // workgroup order (fusion_classify.hip): brick of the p-th workgroup (pack_brick), heaviest bricks first; nullptr =
  // the enumeration's own order
  const int32_t *order;
  const int32_t *n_order;                // number of entries of `order` (device)
  // 0x0101010101010101 when adding +0.0 cannot change any running sum (the grid starts at +0.0 and there are no hit
  // counters): BRICK_BEHIND is then treated as BRICK_SKIP; 0 otherwise
  unsigned long long behind_mask;
  // Rotated grid (the 3x3 part of the grid matrix is not diagonal): w depends on all of (i, j, k), so c.z cannot
  // be split into a per-lane part and a per-(view, k) table; cz_table then holds [kpad][4] = the k-dependent products
  // (g02, g12, g22) * gz(k) of cu:168, and the kernel forms w and c.z per voxel in the reference's order
  int32_t rotated;
  int32_t flags;                         // TileKernelFlags bits
  const MapRec *maps;                    // RT row 2 in full for the rotated path
  // first entry of each of the four work levels within `order` (device; written by the ordering kernels): with them an
  // XCD takes ONE contiguous eighth of every level instead of runs dealt round-robin (fusion_tile.hip, workgroup -> brick)
  const int32_t *order_levels;
  // free_sums[n] = ((0 + f) + f ...) + f, n times, f = free_space, in fp64: what EVERY voxel of a brick holds after n
  // BRICK_FREE views when nothing else has touched the brick yet (the sums start at +0.0).  The kernel counts such views
  // and fetches the sum when the first view with per-voxel work arrives, instead of adding per view and voxel.
  // nullptr: not available (the grid does not start from zeros, or more views than kFreeSumsMax)
  const double *free_sums;
  // super-brick of the n-th entry of the slot enumeration, n = (slot - slot_base) / 32: sbx | sby << 10 | (sbz - sbz_first)
  // << 20.  Z-order (Morton) over the slab being fused, so that a contiguous share of the enumeration -- an XCD's eighth of
  // a work level -- is a compact region in all three axes and projects onto a small part of every depth map.
  const int32_t *sb_perm;
  // tuning builds (DMI_TUNING) with DMI_DEBUG_WG_TIMES set, u = the brick's position in the order: [2u] = s_memrealtime
  // (100 MHz) when its workgroup has found it, [2u + 1] = just before the sums are stored, [2 * wg_times_n + u] = the
  // XCC_ID it ran on | blockIdx.x << 8; nullptr otherwise (tools/gpu_wg_timeline.py)
  unsigned long long *wg_times;
  int64_t wg_times_n;
  // brick counters of the persistent workgroups, one per XCD at [16 * xcd]; zeroed by the table kernel of every launch
  int32_t *queue_heads;
  // Windows of the FREE column (round 4; WinPair since round 5): for a pair of class MIXED_FREE_OR_NODEPTH,
  // win_origin[win_pair_index(brick, view, n_class_bricks)] holds the first pixel of a kWindowCols x kWindowRows window that holds
  // the reference's pixel of every voxel of the brick, and the window-relative numerators at the brick's first voxel
  // (window_origin_kernel, fusion_classify.hip).  The table is laid out [block of 32 views][brick][32 views]
  // (fusion_launch_rules.h); the fusion kernel gets the brick's number from its class row, (row - classes) / class_pitch.
  // (-DDMI_WINPAIR_BRICK_MAJOR: win_origin[brick * class_pitch + view], the table indexed like the class table)
  WinPair *win_origin;
  int64_t n_class_bricks;  // rows of the class table: wbricks_x * wbricks_y * bricks_z, the bricks of the WHOLE grid
  const WinRec *win_recs;  // [n_views]
  const FootRec *foot_recs;  // [n_views]
  int32_t vb_bytes, vb_rowskip;  // as TileMapRec's (the same for every view of a context)
  int32_t win_cx, win_cy;        // kValidMargin + W / 2, kValidMargin + H / 2: the image centre in padded coordinates
};
constexpr int kFreeSumsMax = 4096;
// an entry of TileArgs::order: the workgroup brick (bx, by, bz), 11 + 11 + 10 bits (checked on the host)
__host__ __device__ inline int32_t pack_brick(int bx, int by, int bz) { return (int32_t)((uint32_t)bx | ((uint32_t)by << 11) | ((uint32_t)bz << 22)); }
// fuse_tile_kernel reads the first sixteen ints as two vectors
static_assert(offsetof(TileArgs, nx) == 0 && offsetof(TileArgs, nz) == 8 && offsetof(TileArgs, kpad) == 32 &&
                  offsetof(TileArgs, bricks_x) == 36 && offsetof(TileArgs, bricks_z) == 44 && offsetof(TileArgs, sbz_first) == 60,
              "TileArgs head layout");
enum TileKernelFlags : int32_t {
  TILE_FLAG_NO_INTERIOR = 1,  // tuning / tests: never take the INTERIOR column variant
  TILE_FLAG_XCD_RUNS = 2,     // deal the ordered bricks to the XCDs in runs of xcd_run_wg (round 1's mapping; with TILE_FLAG_COST_ORDER)
  TILE_FLAG_COST_ORDER = 4,   // the bricks are ordered by their number of mixed views (64 levels; small grids: launch_order_bricks)
  // tuning builds only (DMI_TUNING; results are wrong): what a kind of pair costs -- the window pairs skipped, or every mixed
  // pair but them (DMI_DEBUG_PAIRS=nowin / onlywin; counters per pair: tools/gpu_pair_cost.sh)
  TILE_FLAG_DBG_SKIP_WINDOW_PAIRS = 256,
  TILE_FLAG_DBG_ONLY_WINDOW_PAIRS = 512,
  TILE_FLAG_DBG_NO_WINDOW_LOADS = 1024   // (DMI_DEBUG_PAIRS=nowinloads) the window's two loads dropped: what their latency costs
};

// What the reference does to EVERY voxel of a brick for one map, when that can be proven from the eight
// corner voxels and the depth table's min/max pyramid (fusion_classify.hip):
enum BrickClass : uint8_t {
  BRICK_MIXED = 0,   // not provable: the full per-voxel path runs
  BRICK_FREE = 1,    // every voxel accumulates -eta*rho (far in front of every surface, cu:115)
  BRICK_BEHIND = 2,  // every voxel accumulates 0 (far behind every surface, cu:115)
  BRICK_SKIP = 3     // no voxel reaches cu:211 (behind the camera cu:177, outside the map cu:192, no depth cu:202)
};

// Why a (brick, view) pair could not be proven uniform: stored in bits 2..4 of a BRICK_MIXED class byte (diagnostic)
enum MixedReason : uint8_t {
  MIXED_UNSPECIFIED = 0,
  MIXED_DEGENERATE = 1,          // a non-finite c.z or pixel coordinate at a corner
  MIXED_CAMERA_PLANE = 2,        // c.z changes sign over the brick or comes too close to 0 for the footprint bound
  MIXED_IMAGE_BORDER = 3,        // the footprint is partly outside the depth map
  MIXED_NAN_DEPTH = 4,           // a NaN depth in the footprint's tiles
  MIXED_SENTINEL_AND_DEPTH = 5,  // both "no depth" pixels and depths in the footprint's tiles
  MIXED_NEAR_SURFACE = 6,        // the depths of the footprint's tiles come within delta of the brick's c.z range
  // "No depth" pixels among depths that are ALL far behind the brick (fl(czmax - dmin) < -delta over the valid depths):
  // every voxel either returns at cu:202 or accumulates -eta*rho (cu:115), and which of the two is all that is left to find
  // out per voxel -- the pixel, its load and one compare, no diff and no three-way potential (the FREE column of
  // fuse_tile_kernel).  What a best-cost threshold leaves of free space (RD.cxx:138-167: scattered -1 pixels).
  MIXED_FREE_OR_NODEPTH = 7
};

struct FuseConfig {
  int depth_is_f64;
  int grid_is_f64;
  int k_mode;
  int count_hits;
  int variant;   // tuning variant bits, see launch_fuse / launch_fuse_tiled
  int use_tile;  // host decision: the tiled kernel's preconditions hold
  int general_k; // tiled kernel: some view of the fused range has a K whose third row is not 0 0 1 0 (GENK instantiation)
  int holes;     // tiled kernel: holes scattered all over the resident views (an eighth of their 8-pixel strips hold both a hole
                 // and a depth: maps after a best-cost threshold) -- column height and launch form (fusion_launch_rules.h, launch_shape)
};

// (the tuning-variant bits of dmi_options::kernel_variant, VAR_*: fusion_launch_rules.h)

constexpr int kMaxColumnHeight = 16;  // the tallest column of any tile shape: what z-slab partitions must be multiples of
// Column height (voxels along k owned by one lane) and workgroup shape of tile shape `s`.
struct TileShape {
  int tk, wx, wy;  // column height; waves per workgroup along x and y (a wave is 8 x 8 lanes)
};
TileShape tile_shape(int variant, bool depth_is_f64, bool rotated, bool general_k);  // (rotated: the two default shapes; general K: 16-voxel columns)

// Enqueues the general fusion kernel on `stream`.  Returns hipSuccess or the launch error.
hipError_t launch_fuse(const FuseArgs &args, const FuseConfig &cfg, hipStream_t stream);

// Tiled kernel: fills args.cz_table for maps [first_map, first_map + n_maps) and fuses them.
// args.full must point to a device copy of the matching FuseArgs (read by the exact fallback).
hipError_t launch_fuse_tiled(const TileArgs &args, const MapRec *maps_dev, const FuseConfig &cfg, const PyramidDesc &pyramid,
                             uint8_t *order_scratch, uint8_t *coarse_classes, hipEvent_t before_main_kernel,
                             hipStream_t stream);

// depth upload helpers ------------------------------------------------------------------
hipError_t launch_widen_depth(const float *in, double *out, int64_t n, hipStream_t stream);
// n grid elements f64 -> f32 (in_is_f64) or f32 -> f64, device to device
hipError_t launch_convert_grid(const void *in, int in_is_f64, void *out, int64_t n, hipStream_t stream);

// dmi_fp64_probe: `iters` rounds of eight independent fp64 FMAs per lane; out[thread] keeps the chains alive
hipError_t launch_fp64_probe(double *out, int blocks, int iters, hipStream_t stream);

PyramidDesc make_pyramid_desc(int W, int H);
// The upload pass in one kernel (fusion_classify.hip): n_maps host tables (f64 or f32, vtk row order, optionally with best-cost
// values and their threshold) -> depth tables (top row first, f32 or f64), the finest pyramid level, validity bytes and bits;
// counters[0] += lossy narrowings, [1] += pixels without a depth, [2] += 8-pixel strips with both a hole and a depth.  The upper
// pyramid levels follow with launch_build_pyramid_levels.
hipError_t launch_upload_views(const void *in, int in_is_f64, const double *best_cost, double threshold, void *out, int out_is_f64,
                               int64_t n_maps, int W, int H, const PyramidDesc &desc, DepthTile *pyramids, uint8_t *valid, uint32_t *bits,
                               unsigned long long *counters, hipStream_t stream);
hipError_t launch_build_pyramid_levels(int64_t n_maps, const PyramidDesc &desc, DepthTile *pyramids, hipStream_t stream);
// window origins of the FREE column for the pairs of class MIXED_FREE_OR_NODEPTH of maps [first_map, first_map + n_maps): fills
// args.win_origin and marks the class bytes of those without a window (CLASS_NO_WINDOW); after launch_classify_bricks
hipError_t launch_window_origins(const TileArgs &args, const MapRec *maps_dev, int tk, uint8_t *classes, int general_k,
                                 hipStream_t stream);
// classes[brick][map] for maps [first_map, first_map + n_maps): see BrickClass.  tk = column height.
// general_k: some view of the run has a K with a general third row (the kernels then look at every view's errz)
hipError_t launch_classify_bricks(const TileArgs &args, const MapRec *maps_dev, const PyramidDesc &desc, int tk,
                                  uint8_t *classes, uint8_t *coarse, int general_k, hipStream_t stream);
// bytes of the coarse class table (one row of class_pitch bytes per box of 32^3 voxels of the whole grid)
int64_t coarse_class_bytes(const TileArgs &args, int tk);
// order[p] = slot (super_brick * 32 + brick) of the p-th workgroup, bricks with the most BRICK_MIXED pairs first;
// level: scratch of super_x*super_y*super_z*32 bytes; wx, wy: waves per workgroup
// (kCostOrderMaxSlots, the rule that picks the cost order: fusion_launch_rules.h)
// bytes of the `level` scratch of launch_order_bricks for n_slots workgroup slots (levels + per-chunk counts)
size_t order_scratch_bytes(size_t n_slots);
hipError_t launch_order_bricks(const TileArgs &args, int wx, int wy, uint8_t *level, int *order, int *n_valid,
                               hipStream_t stream);

// vtkCellDataToPointData over the fused grid (Reconstruction/main.cxx:151-155): points[(nz+1)][(ny+1)][(nx+1)] f64
// from cells[nz][ny][nx] (grid_post.hip)
hipError_t launch_cell_to_point(const void *cells, int cells_are_f64, double *points, int nx, int ny, int nz,
                                hipStream_t stream);

// The separable Gaussian over the point data (point_smooth.hip): per axis x, y, z the radius (0: the axis is
// skipped) and the normalised weights k_0..k_r (point_smooth_rules.h: point_smoothing_weights)
struct PointSmoothArgs {
  int32_t r[3];
  double k[3][kPointSmoothMaxRadius + 1];
};
// How many kernels launch_point_smooth runs for these radii.  It reads `first` ((nx+1)(ny+1)(nz+1) f64) and ping-pongs between the
// two buffers: the result is in `first` after an even number of launches and in `second` after an odd one.
int point_smooth_launches(const PointSmoothArgs &a);
hipError_t launch_point_smooth(double *first, double *second, int nx, int ny, int nz, const PointSmoothArgs &a, hipStream_t stream);

// Iso-value pre-pass over the point data (grid_post.hip): blocks of 256 cells of one x-row; counts / bases have
// iso_block_count() + 1 entries (bases' last one receives the total number of active cells)
size_t iso_block_count(int nx, int ny, int nz);
hipError_t launch_iso_count(const double *points, int nx, int ny, int nz, double iso, uint32_t *counts, uint64_t *bases,
                            void *scan_temp, size_t *scan_temp_bytes, hipStream_t stream);
hipError_t launch_iso_write(const double *points, int nx, int ny, int nz, double iso, const uint64_t *bases, int64_t *ids,
                            uint64_t capacity, hipStream_t stream);

// Marching cubes over the point data (isosurface.hip): segments of 256 lattice points of one x-row.
struct MeshGeom {
  int nx, ny, nz, segs_per_row;
  double iso;
  double origin[3], spacing[3];
  double m[12];                      // rows 0..2 of the grid matrix, row-major
  uint64_t n_vertices, n_triangles;  // sizes of the write pass's output buffers
};
// the write pass with normals (dmi_extract_isosurface_normals): the cofactor matrix of the grid matrix's upper-left 3 x 3,
// negated when its determinant is negative, row-major, and the [n_vertices][3] f32 output
struct MeshNormals {
  double nm[9];
  float *normals;
};
int isosurface_max_triangles_per_cell();
size_t isosurface_segment_count(int nx, int ny, int nz);
// counts / bases: 2 (segments + 1) entries, vertices then triangles; counts[segments] and counts[2 segments + 1] are zeros the
// caller keeps there, so bases[segments] and bases[2 segments + 1] receive the totals
hipError_t launch_isosurface_count(const double *points, const MeshGeom &g, uint32_t *counts, uint64_t *bases, void *scan_temp,
                                   size_t *scan_temp_bytes, hipStream_t stream);
// writes the vertices' normals too when `normals` is not null
hipError_t launch_isosurface_write(const double *points, const MeshGeom &g, const uint64_t *bases, double *verts, int64_t *tris,
                                   const MeshNormals *normals, hipStream_t stream);

// Connected components of that mesh (isosurface_components.hip): the mesh to filter and the buffers of the result.
struct ComponentsMesh {
  uint64_t n_vertices, n_triangles;  // both below 2^32 (u32 labels and sizes), n_vertices >= 1
  const double *vertices;            // [n_vertices][3]
  const float *normals;              // [n_vertices][3], or null: the mesh has none
  const int64_t *triangles;          // [n_triangles][3]
  double *out_vertices;              // room for the whole mesh each: how much stays is known only afterwards
  float *out_normals;
  int64_t *out_triangles;
  int64_t *region_id;                // [n_vertices]
  int64_t *region_size;              // [n_vertices]: one per kept component
};
struct ComponentsScratch {
  uint32_t *parent, *size;           // [n_vertices]: after the call, every vertex's label and every label's triangle count
  uint32_t *vmap, *rmap;             // [n_vertices + 1]: kept vertices / kept components before; the totals at [n_vertices]
  uint32_t *tmap;                    // [n_triangles + 1]
  unsigned long long *counters;      // [3]: the largest component's key (size << 32 | ~label), the components found, retried swaps
  void *scan_temp;
  size_t scan_temp_bytes;
};
hipError_t components_scan_temp_bytes(uint64_t n_vertices, uint64_t n_triangles, size_t *bytes);
hipError_t launch_isosurface_components(const ComponentsMesh &m, const ComponentsScratch &s, int largest, uint64_t min_triangles,
                                        hipEvent_t *events, hipStream_t stream);

// Taubin smoothing of that mesh (isosurface_smooth.hip): the mesh to smooth (read only) and where its new normals go.
struct SmoothMesh {
  uint64_t n_vertices, n_triangles;  // n_vertices >= 1 and below 2^32, 6 n_triangles below 2^32 (u32 ids and CSR offsets)
  const double *vertices;            // [n_vertices][3]
  const int64_t *triangles;          // [n_triangles][3]
  float *normals_out;                // [n_vertices][3]: the geometric normals of the result, or null: none wanted
};
struct SmoothScratch {
  uint64_t *keys[2];                 // [6 n_triangles] each: the edge keys and their sort; afterwards the neighbour ids and the incidence
  uint32_t *row_start;               // [n_vertices + 1]
  uint32_t *valence, *offsets;       // [n_vertices + 1]: the CSR offsets, the total at [n_vertices]
  unsigned long long *fixed;         // [(n_vertices + 63) / 64]: one bit per vertex
  double *positions[2];              // [n_vertices][3] each: the steps' two buffers
  void *temp;                        // rocPRIM's
  size_t temp_bytes;
};
hipError_t smooth_temp_bytes(uint64_t n_vertices, uint64_t n_triangles, size_t *bytes);
hipError_t launch_isosurface_smooth(const SmoothMesh &m, const SmoothScratch &s, int iterations, double lambda, double mu,
                                    double **result, hipEvent_t *events, hipStream_t stream);
// The smoother's geometric normals of any mesh (n_vertices >= 1 and below 2^32, n_triangles below 2^32; the decimation's too): the
// vertex -> triangle incidence is built in keys[0] / keys[1] ([3 n_triangles] each) and row_start ([n_vertices + 1]); temp holds
// smooth_temp_bytes(n_vertices, n_triangles).  Triangles naming an id >= n_vertices are skipped.
hipError_t launch_isosurface_geometric_normals(const double *vertices, const int64_t *triangles, uint64_t n_vertices, uint64_t n_triangles,
                                               uint64_t *const keys[2], uint32_t *row_start, void *temp, size_t temp_bytes,
                                               float *normals_out, hipStream_t stream);

// Vertex clustering of that mesh (isosurface_decimate.hip).  Nothing of the input mesh is written.
struct DecimateMesh {
  uint64_t n_vertices, n_triangles;  // n_vertices >= 1, both below 2^32 (u32 ids on the device)
  const double *vertices;            // [n_vertices][3]
  const int64_t *triangles;          // [n_triangles][3]
  double *out_vertices;              // room for the whole mesh each: how much stays is known only afterwards
  int64_t *out_triangles;
};
struct DecimateGrid {                // the bins, from the bounds the first pass found
  double lo[3], h;
  uint64_t n[3];                     // bins per axis, each <= 2^21
};
struct DecimateScratch {
  unsigned long long *bounds;        // [8]: lo[3] and hi[3] as order-preserving integers, the non-finite flag, unused
  uint64_t *keys[2];                 // [max(n_vertices, 2 n_triangles)] each: the vertex keys, then the triangle keys and values;
                                     // [max(that, 3 n_triangles)] for the quadric placement: then the corner pairs, u32
  uint32_t *ids[2];                  // [n_vertices] each: the vertex ids sorted with their keys
  uint32_t *head, *rank;             // [n_vertices + 1]: first of a cluster, and the inclusive scan of that
  uint32_t *cluster_of, *start;      // [n_vertices + 1]: a vertex's cluster; a cluster's first sorted position
  uint32_t *mark, *cmap;             // [n_vertices + 1]: cluster named by a surviving triangle; output vertices before it
  uint32_t *keep, *tmap;             // [n_triangles + 1]: triangle survives; surviving triangles before it
  void *temp;                        // rocPRIM's
  size_t temp_bytes;
};
constexpr int kDecimateMean = 0, kDecimateQuadric = 1;  // DMI_DECIMATE_MEAN, DMI_DECIMATE_QUADRIC
hipError_t decimate_temp_bytes(uint64_t n_vertices, uint64_t n_triangles, int placement, size_t *bytes);
// the bounds pass: s.bounds receives the six bounds (decimate_decode_bound) and the flag; `events`: 2, recorded around it
hipError_t launch_decimate_bounds(const DecimateMesh &m, const DecimateScratch &s, hipEvent_t *events, hipStream_t stream);
double decimate_decode_bound(unsigned long long ordered);
// everything else: `events`: 4, recorded before the keys, after the ranks, after the triangles and after the representatives.
// Afterwards s.cmap[n_vertices] and s.tmap[n_triangles] hold the output's sizes.  `placement` chooses the representative pass
// on the host: the mean's launches are the same whatever else exists; the quadric one needs 3 n_triangles < 2^32.
hipError_t launch_isosurface_decimate(const DecimateMesh &m, const DecimateGrid &g, const DecimateScratch &s, int placement,
                                      hipEvent_t *events, hipStream_t stream);

// The hole filler of that mesh (isosurface_holes.hip).  Nothing of the input mesh is written.
struct HolesMesh {
  uint64_t n_vertices, n_triangles;  // 1 <= n_vertices < 2^31 (an edge key is two ids and a direction bit), 3 n_triangles < 2^32
  const double *vertices;            // [n_vertices][3]
  const int64_t *triangles;          // [n_triangles][3]
  const float *normals;              // [n_vertices][3], or null: the mesh has none
};
struct HolesVertexScratch {          // [n_vertices + 1] each
  uint32_t *out_deg, *in_deg;        // the boundary half-edges that start and end at a vertex
  uint32_t *succ;                    // where the one that starts there ends (read for simple vertices only)
  uint32_t *flag, *rank;             // a boundary vertex; the boundary vertices before it (its slot), the total at [n_vertices]
};
struct HolesLoopScratch {            // [slots + 1] each
  uint32_t *id, *next;               // a slot's vertex; its successor's slot (a complex vertex: itself)
  uint32_t *ptr[2], *label[2];       // the doubling's two buffers
  uint32_t *count;                   // the slots that carry this slot as their label
  uint32_t *new_vertices, *new_triangles, *vertex_offset, *triangle_offset;  // what a head adds, and the scans of that
};
struct HolesOutput {                 // room for the old mesh and what the loops pass counted
  double *vertices;
  int64_t *triangles;
  float *normals;                    // or null
};
hipError_t holes_temp_bytes(uint64_t n_vertices, uint64_t n_triangles, size_t *bytes);
int holes_rounds(uint64_t max_edges, uint64_t n_slots);  // the doubling rounds of launch_holes_loops
// Three passes with a read of the counts between them (dmi_capi_mesh.hip); counters: 4 u64 (boundary edges, filled loops, their
// edges, walks that did not close).  keys: [3 n_triangles] each.
hipError_t launch_holes_boundary(const HolesMesh &m, const HolesVertexScratch &v, uint64_t *const keys[2], void *temp, size_t temp_bytes,
                                 unsigned long long *counters, hipEvent_t *events, hipStream_t stream);
hipError_t launch_holes_loops(const HolesMesh &m, const HolesVertexScratch &v, const HolesLoopScratch &l, uint32_t n_slots, uint64_t max_edges,
                              void *temp, size_t temp_bytes, unsigned long long *counters, hipEvent_t event, hipStream_t stream);
hipError_t launch_holes_fill(const HolesMesh &m, const HolesLoopScratch &l, uint32_t n_slots, const HolesOutput &out,
                             unsigned long long *counters, hipEvent_t event, hipStream_t stream);

// The trim of that mesh by view support (isosurface_support.hip).  Nothing of the input mesh is written.
struct SupportMesh {
  uint64_t n_vertices, n_triangles;  // n_vertices >= 1, both below 2^32 (u32 maps on the device)
  const double *vertices;            // [n_vertices][3]
  const float *normals;              // [n_vertices][3], or null: the mesh has none
  const int64_t *triangles;          // [n_triangles][3]
  double *out_vertices;              // room for the whole mesh each: how much stays is known only afterwards
  float *out_normals;
  int64_t *out_triangles;
};
struct SupportViews {
  const MapRec *maps;                // [n_views], device: K, [R|T] and the depth table the fusion kept of every resident view
  int n_views, W, H;
  int depth_is_f64;
};
struct SupportScratch {
  int32_t *support;                  // [n_vertices]: the counts of the input mesh
  int32_t *out_support;              // [n_vertices]: ... of the compacted one
  uint32_t *mark, *vmap;             // [n_vertices + 1]: named by a surviving triangle; surviving vertices before it
  uint32_t *tmap;                    // [n_triangles + 1]: surviving triangles before it
  void *scan_temp;                   // rocPRIM's
  size_t scan_temp_bytes;
};
hipError_t support_scan_temp_bytes(uint64_t n_vertices, uint64_t n_triangles, size_t *bytes);
// `events`: 4 (or null); the counts run between [0] and [1], the filter's marks and scans between [1] and [2], its compaction
// between [2] and [3].  After the filter s.vmap[n_vertices] and s.tmap[n_triangles] hold the output's sizes.
hipError_t launch_isosurface_support_counts(const SupportMesh &m, const SupportViews &views, double tolerance, int require_facing,
                                            const SupportScratch &s, hipEvent_t *events, hipStream_t stream);
hipError_t launch_isosurface_support_filter(const SupportMesh &m, int32_t min_views, const SupportScratch &s, hipEvent_t *events,
                                            hipStream_t stream);

}  // namespace dmi
