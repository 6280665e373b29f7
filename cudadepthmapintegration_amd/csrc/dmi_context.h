// dmi_context.h -- the context behind the C ABI of include/dmi.h, in groups, and the helpers its translation units share
// (dmi_capi.hip: creation, destruction, grid transfer, info, timings, probes; dmi_capi_views.hip: the resident views;
// dmi_capi_fuse.hip: the fusion launch and the diagnostics that read it; dmi_capi_mesh.hip: point data and the iso-surface).  Every device allocation is a dmi::DeviceBuffer
// (dmi_buffer.h, capacity in bytes) grown by one of two rules, every group has a release().  The mesh's state, the stages' events
// and times and what else the mesh stages share are dmi_mesh_stage.h's.  The colour context
// (dmi_color_context.h, dmi_capi_color.hip) is built from the same parts and exception guard.  Private: never installed.
#pragma once
#include "../../include/dmi.h"
#include "dmi_buffer.h"
#include "dmi_mesh_stage.h"
#include "fusion_kernels.h"

#include <exception>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

namespace dmi {

struct Batch {
  void *d_depth = nullptr;             // n * W * H values of the context's current storage type
  DepthTile *d_pyramid = nullptr;  // n min/max pyramids (fusion_classify.hip), then the n validity maps
  size_t valid_offset = 0;              // byte offset of the validity maps within d_pyramid
  size_t bits_offset = 0;               // ... and of the validity bits (TileMapRec::vbits) behind them
  size_t aux_bytes = 0;                 // size of the d_pyramid allocation
  int32_t n = 0;
  unsigned long long holes = 0;         // pixels without a depth among the n * W * H (counted while the validity maps are built)
  unsigned long long mingled_strips = 0;  // 8-pixel strips (a column of a tile row) with both a hole and a depth
};

struct EventPair {
  hipEvent_t start = nullptr, stop = nullptr;
  hipEvent_t mid = nullptr;  // recorded just before the fusion kernel proper (after cz table, classification, ordering)
  bool has_mid = false;
};
}  // namespace dmi

struct dmi_context {
  dmi_grid_desc grid{};
  dmi_ray_potential ray{};
  dmi_options opt{};
  int64_t n_voxels = 0;

  hipStream_t stream = nullptr;
  bool own_stream = false;
  // dmi_add_views copies, converts and builds pyramids on a stream of its own and waits for that stream only: a fuse
  // still running on `stream` overlaps the upload of the next views (FusionDriver::ProcessDepthMap pipelines on this)
  hipStream_t upload_stream = nullptr;
  hipStream_t download_stream = nullptr;  // dmi_fuse_range_download: the slabs' copies to the host
  std::vector<hipEvent_t> slab_events;    // ... and what each waits for

  bool finite_bounded = true;  // grid descriptor magnitudes allow the K shortcuts

  // ---- fusion (dmi_capi.hip, dmi_capi_views.hip, dmi_capi_fuse.hip): every capacity is in bytes ----
  struct Views {  // the resident views: their store, their records, the staging of an upload
    int32_t W = 0, H = 0;
    bool depth_f64 = false;
    int k_mode = dmi::K_PINHOLE;          // the least structured K among the resident views (dmi_info)
    std::vector<uint8_t> view_k_mode;     // per view: dmi::KMode of its K
    std::vector<uint8_t> view_tile_ok;    // per view: meets the tiled kernel's per-view preconditions (ViewRecords::tile_ok)
    double max_tile_err = 0.0;            // largest TileMapRec::err among the resident views
    dmi::PyramidDesc pyramid{};           // geometry of every view's depth min/max pyramid
    // one per dmi_add_views call; allocated and freed whole by the all-or-nothing upload (upload_batch, promote_to_f64)
    std::vector<dmi::Batch> batches;
    // per view, on the host and -- after sync_maps -- on the device: what the general kernel reads; the tiled kernel (fusion_tile.hip);
    // the window form of its FREE column (one line each); the brick's corners relative to its first voxel (window_origin_kernel).
    // The four device arrays grow as a unit (max(64, 2 n) records each).
    std::vector<dmi::MapRec> h_maps;
    std::vector<dmi::TileMapRec> h_tile_maps;
    std::vector<dmi::WinRec> h_win_recs;
    std::vector<dmi::FootRec> h_foot_recs;
    dmi::DeviceBuffer maps, tile_maps, win_recs, foot_recs;
    bool maps_dirty = false;  // the host records have changed since they were last copied
    dmi::DeviceBuffer stage_depth, stage_cost;  // f64 staging of an upload's depths and best costs (<= 256 MiB of host data at a time)
    dmi::DeviceBuffer lossy;  // 3 u64: lossy narrowings, pixels without a depth, mingled strips of the upload under way
    hipEvent_t up_events[2] = {nullptr, nullptr};  // start, stop around the upload pass's kernels (dmi_get_upload_kernel_ms)
    double last_upload_kernel_ms = 0.0, total_upload_kernel_ms = 0.0;
    void release() {
      for (dmi::Batch &b : batches) {
        (void)hipFree(b.d_depth);
        (void)hipFree(b.d_pyramid);
      }
      batches.clear();
      dmi::free_buffers({&maps, &tile_maps, &win_recs, &foot_recs, &stage_depth, &stage_cost, &lossy});
      dmi::destroy_events(up_events);
    }
  } views;
  struct Hits {  // dmi_options::count_hits
    dmi::DeviceBuffer voxel;  // u32 per voxel
    dmi::DeviceBuffer map;    // u64 per view, max(64, 2 n) of them; keeps its counts when it grows
    void release() { dmi::free_buffers({&voxel, &map}); }
  } hits;
  struct Volume {  // the grid's voxels
    void *d_grid = nullptr;    // owned.ptr, or the caller's dmi_options::external_grid
    dmi::DeviceBuffer owned;
    bool own_grid = false;
    std::vector<uint8_t> layer_is_zero;  // per cell layer: known to hold +0.0 everywhere (reset, not fused since)
    bool zero_fill_pending = false;  // reset requested, memset deferred: the next fuse overwrites every voxel
    // No voxel of the (context-owned) grid is -0.0: true after a reset and preserved by every fusion -- a sum that is not -0.0 never
    // becomes one (x + y is -0.0 only when both are; a non-zero f64 sum does not round to zero) -- so the +0.0 adds of voxels far
    // behind every surface stay unobservable from one dmi_fuse_range to the next, not only in the first (round 4: the chunked
    // fusion of the drop-in filter ran its later chunks at half speed).  False once the caller has uploaded a grid, and for a
    // caller-owned grid (whoever owns it may write anything between two calls).
    bool grid_free_of_negative_zero = false;
    dmi::DeviceBuffer convert;  // staging of the grid up/downloads whose host type is not the grid's (kConvertChunk elements)
    void release() {
      dmi::free_buffers({&owned, &convert});
      d_grid = nullptr;
    }
  } volume;
  // slot enumeration of the tiled kernel (TileArgs::sb_perm), one table per slab geometry seen (the z-slabs of a
  // multi-GPU fusion come round again every step)
  struct SlotPerm {
    int32_t super_x, super_y, super_z, zmajor;
    dmi::DeviceBuffer perm;
  };
  struct LaunchTables {  // what a tiled launch reads beside the views; queued launches may read them: grown by ensure_idle_buffers
    dmi::DeviceBuffer cz_table;   // the r22*wz(k) table, then the sums of n free-space constants; allocated at twice the need
    dmi::DeviceBuffer fuse_args;  // a device copy of FuseArgs
    dmi::DeviceBuffer zero_row;   // one row of BRICK_MIXED bytes: the class table of a fuse without classes
    dmi::DeviceBuffer classes;    // brick classes [wave bricks][class_pitch], then the coarse table [boxes][class_pitch], then the window pairs
    size_t coarse_offset = 0;     // byte offset of the coarse table within classes (last fuse)
    dmi::DeviceBuffer queue_heads;  // TileArgs::queue_heads (128 ints)
    dmi::DeviceBuffer wg_times;     // tuning builds: TileArgs::wg_times of the last tiled fuse
    size_t wg_times_blocks = 0;
    std::vector<SlotPerm> slot_perms;
    dmi::DeviceBuffer order, order_level;  // workgroup order: count and order[]; scratch levels.  Grown as a unit
    void release() {
      for (SlotPerm &sp : slot_perms) dmi::free_buffers({&sp.perm});
      slot_perms.clear();
      dmi::free_buffers({&cz_table, &fuse_args, &zero_row, &classes, &queue_heads, &wg_times, &order, &order_level});
    }
  } tables;
  struct LastLaunch {  // what the diagnostics read (dmi_get_brick_class_histogram ...); filled by fuse_run in one place
    bool tiled = false;
    bool classes = false;
    int64_t class_bricks = 0;  // wave bricks of the last fuse
    int32_t bricks_z = 0, tk = 0;
    const dmi::WinPair *win_origin = nullptr;  // the last tiled launch's pair table (nullptr: it had no windows); only asked whether there was one
    int32_t class_pitch = 0, first = 0, count = 0;
  } last;

  // ---- post-processing (dmi_capi_mesh.hip): every buffer is kept while large enough, every capacity is in bytes ----
  // Every group with events derives from dmi::StageTimes<events, passes> (dmi_mesh_stage.h): the events, created at the first
  // call that needs them, last_kernel_ms and, where the stage has passes, last_pass_ms
  struct CellToPoint : dmi::StageTimes<2> {  // start, stop; the time is timings.last_cell_to_point_ms
    dmi::DeviceBuffer points;  // vtkCellDataToPointData of the grid, (nx+1)(ny+1)(nz+1) f64 (grid_post.hip)
    bool valid = false;        // points matches the grid's current contents
    bool pending = false;
    void release() { dmi::free_buffers({&points}); StageTimes::release(); }
  } c2p;
  // dmi_set_point_smoothing (point_smooth.hip): while `on`, every computation of c2p.points is followed by the smoothing passes
  // and c2p.points holds their result
  struct PointSmoothing : dmi::StageTimes<2> {  // start, stop around the smoothing kernels of the last recomputation; 0 when off
    double sigma[3] = {0.0, 0.0, 0.0}, truncate = 3.0;
    bool on = false;             // some sigma is not 0
    dmi::PointSmoothArgs args{}; // the radii and weights of the setting
    dmi::DeviceBuffer scratch;   // the passes' second buffer, of the point data's size; held only while on
    bool pending = false;
    void release() { dmi::free_buffers({&scratch}); StageTimes::release(); }
  } point_smoothing;
  using Mesh = dmi::MeshState;  // dmi_mesh_stage.h: the mesh, and the one operation that makes a stage's result the mesh
  Mesh mesh;
  struct Extraction : dmi::StageTimes<4> {  // dmi_extract_isosurface (isosurface.hip): around the count pass + scans, and the write pass
    dmi::DeviceBuffer counts, bases, scan_temp;  // per-segment counts (u32) and bases (u64), two arrays of (segments + 1) each
    void release() { dmi::free_buffers({&counts, &bases, &scan_temp}); StageTimes::release(); }
  } extraction;
  // dmi_filter_isosurface_components (isosurface_components.hip); passes: labels (init, hook, flatten), sizes (and largest), scans, compaction
  struct Components : dmi::StageTimes<5, 4> {
    dmi::DeviceBuffer vertex_scratch;  // dmi::kComponentsLanes u32 arrays of (vertices + 1)
    dmi::DeviceBuffer triangle_scratch, counters, scan_temp;
    uint64_t last_cas_retries = 0;  // compare-and-swaps of the last filter's hooking pass that lost a race
    void release() { dmi::free_buffers({&vertex_scratch, &triangle_scratch, &counters, &scan_temp}); StageTimes::release(); }
  } components;
  struct Smoothing : dmi::StageTimes<4, 3> {  // dmi_smooth_isosurface (isosurface_smooth.hip); passes: adjacency (and incidence), steps, normals
    dmi::DeviceBuffer vertices;        // the second position buffer of the steps
    dmi::DeviceBuffer keys;            // two u64 arrays of 6 triangles' keys
    dmi::DeviceBuffer vertex_scratch;  // the fixed bits, then dmi::kSmoothingLanes u32 arrays of (vertices + 1)
    dmi::DeviceBuffer temp;
    void release() { dmi::free_buffers({&vertices, &keys, &vertex_scratch, &temp}); StageTimes::release(); }
  } smoothing;
  // dmi_decimate_isosurface (isosurface_decimate.hip); it also uses smoothing.keys and smoothing.temp.  Events: around the bounds
  // pass; before the keys, after the ranks, the triangles, the representatives; around the normals.  Passes: clustering,
  // representatives, triangles, normals
  struct Decimation : dmi::StageTimes<8, 4> {
    dmi::DeviceBuffer vertex_scratch;    // dmi::kDecimationLanes u32 arrays of (vertices + 1)
    dmi::DeviceBuffer triangle_scratch;  // dmi::kDecimationTriangleLanes u32 arrays of (triangles + 1)
    dmi::DeviceBuffer bounds;            // 8 u64
    bool pending = false;         // the events of the last call have not been read yet (its normals may still run)
    bool pending_normals = false;
    void release() { dmi::free_buffers({&vertex_scratch, &triangle_scratch, &bounds}); StageTimes::release(); }
  } decimation;
  // dmi_fill_isosurface_holes (isosurface_holes.hip); it also uses smoothing.keys and smoothing.temp; passes: boundary, loops, fill
  struct Holes : dmi::StageTimes<4, 3> {
    dmi::DeviceBuffer vertex_scratch;  // dmi::kHolesLanes u32 arrays of (vertices + 1)
    dmi::DeviceBuffer loop_scratch;    // dmi::kHolesLoopLanes u32 arrays of (slots + 1)
    dmi::DeviceBuffer counters;        // 4 u64
    void release() { dmi::free_buffers({&vertex_scratch, &loop_scratch, &counters}); StageTimes::release(); }
  } holes;
  // dmi_filter_isosurface_support (isosurface_support.hip); passes: counts, marks and scans, compaction
  struct Support : dmi::StageTimes<4, 3> {
    dmi::DeviceBuffer counts;          // [n] int32: the supporting views of every vertex of the mesh, as the last call left it
                                       // (mesh.support_counted: they describe this mesh)
    dmi::DeviceBuffer work, compacted; // the call's own counts, and those of its compacted mesh: whichever holds the result is
                                       // swapped with `counts` last
    dmi::DeviceBuffer maps;            // the resident views' MapRecs as the call found them
    dmi::DeviceBuffer vertex_scratch;  // dmi::kSupportLanes u32 arrays of (vertices + 1)
    dmi::DeviceBuffer triangle_scratch, scan_temp;
    void release() {
      dmi::free_buffers({&counts, &work, &compacted, &maps, &vertex_scratch, &triangle_scratch, &scan_temp});
      StageTimes::release();
    }
  } support;
  // dmi_color_process_isosurface (dmi_capi_color.hip through dmi::color_device_vertices).  The one event, without timing, is what
  // the colour context's stream waits for: the end of this context's queued work
  dmi::StageTimes<1> coloration;

  std::vector<dmi::EventPair> pending, pool;
  dmi_timings timings{};
  uint64_t device_bytes = 0;  // the sum of the capacities held, and the batches' bytes: kept by the growth helpers below
  std::string err;
};

namespace dmi {

int fail(dmi_context *ctx, int code, const std::string &msg);  // records msg (ctx == nullptr: for dmi_last_error(nullptr))
int drain_events(dmi_context *ctx);                            // the pending fusions' timings
int drain_c2p(dmi_context *ctx);                               // ... and the pending cell-to-point pass's
int flush_zero_fill(dmi_context *ctx);
inline size_t grid_elem(const dmi_context *c) { return c->opt.grid_dtype == DMI_F64 ? 8 : 4; }
// Preconditions of the tiled kernel that do not depend on the view (the per-view part: Views::view_tile_ok)
bool tile_eligible(const dmi_context *ctx);
// Views [first, first + count) into the cell layers [z_first, z_first + z_count): what every fusing entry point ends in
// (dmi_capi_fuse.hip)
int fuse_views(dmi_context *ctx, int32_t first, int32_t count, int32_t z_first, int32_t z_count);
// grow_buffer for a buffer of this context: device_bytes follows, a failure is recorded
int ensure_buffer(dmi_context *ctx, DeviceBuffer &buffer, uint64_t bytes);
// The rule for buffers that work queued on the context's stream may read (dmi::grow_idle_buffers): kept while they hold `needed`;
// otherwise the stream is synchronised, all are freed and allocated at `allocate`, as a unit (a failure leaves all of them empty).
// *fresh: they are new and want their fill.  In the steady state -- the same views, the same grid -- no call of the runtime.
int ensure_idle_buffers(dmi_context *ctx, std::initializer_list<BufferGrowth> unit, bool *fresh = nullptr);
inline int ensure_idle_buffer(dmi_context *ctx, DeviceBuffer &buffer, uint64_t needed, uint64_t allocate, bool *fresh = nullptr) {
  return ensure_idle_buffers(ctx, {{&buffer, needed, allocate}}, fresh);
}
void drop_buffers(dmi_context *ctx, std::initializer_list<DeviceBuffer *> buffers);  // freed now, device_bytes follows
struct BufferNeed {
  DeviceBuffer *buffer;
  uint64_t bytes;  // 0: not needed by this call, left as it is
};
int ensure_buffers(dmi_context *ctx, std::initializer_list<BufferNeed> needs);  // in order, up to the first failure

// No C++ exception may cross the C ABI (the caller may be C, or C++ built with another runtime): every entry point
// that can allocate on the host runs its body through this.  `fail` is the context type's failure sink (dmi::fail, or the
// colour context's).
template <typename Ctx, typename Body>
int guarded_by(int (*fail)(Ctx *, int, const std::string &), Ctx *ctx, const char *entry, Body &&body) noexcept {
  auto report = [&](int code, const char *what) noexcept {
    try {
      return fail(ctx, code, std::string(entry) + ": " + what);
    } catch (...) {
      return code;
    }
  };
  try {
    return body();
  } catch (const std::bad_alloc &) {
    return report(DMI_ERR_OUT_OF_MEMORY, "host allocation failed");
  } catch (const std::exception &e) {
    return report(DMI_ERR_STATE, e.what());
  } catch (...) {
    return report(DMI_ERR_STATE, "unexpected C++ exception");
  }
}
template <typename Body>
int guarded(dmi_context *ctx, const char *entry, Body &&body) noexcept {
  return guarded_by(&fail, ctx, entry, static_cast<Body &&>(body));
}


// The colouring of vertices that are on the device already (dmi_capi_color.hip, where dmi_color_context is private): the
// chunk body of dmi_color_process with a chunk being an offset into `points` and into the outputs, no copy in and none out.
struct ColorContextShape {
  int32_t device, W, H;
  int64_t n_views;
  bool depth_test;  // dmi_color_set_depth_test is on
};
ColorContextShape color_context_shape(const dmi_color_context *c);
struct DeviceColoring {
  const double *points;  // [n][3], device
  int64_t n;
  uint8_t *mean, *median;  // [n][3], device
  int32_t *count;          // [n], device
  hipEvent_t after;        // the colour context's stream waits for it before it reads the vertices
  // the fused depth test: per view (host array) the view's [H][W] table in a fusion context's store, top row first, f64 or f32;
  // null: the colour context's own settings decide
  const void *const *fused_tables;
  bool fused_f64;
  double fused_tol;
};
// Synchronises once at its end (and once for the order-of-work sample).  A failure's message is dmi_color_last_error()'s.
int color_device_vertices(dmi_color_context *c, const DeviceColoring &work, double *kernel_ms);
// The rasteriser of dmi_color_render_depths on a mesh that is on the device already (dmi_color_render_isosurface_depths): points
// [n][3] f64, triangles [n][3] int64; the colour context's stream waits for `after` first.  Synchronises.
int color_render_device_mesh(dmi_color_context *c, const double *points, int64_t n_points, const int64_t *triangles, int64_t n_triangles,
                             hipEvent_t after);

}  // namespace dmi

#define DMI_HIP(ctx, call)                                                                              \
  do {                                                                                                  \
    hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess) {                                                                             \
      (void)hipGetLastError();                                                                          \
      return dmi::fail(ctx, e_ == hipErrorOutOfMemory ? DMI_ERR_OUT_OF_MEMORY : DMI_ERR_DEVICE,         \
                  std::string(#call) + ": " + hipGetErrorString(e_));                                   \
    }                                                                                                   \
  } while (0)
