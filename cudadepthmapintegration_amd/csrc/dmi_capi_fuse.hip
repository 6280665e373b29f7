// dmi_capi_fuse.hip -- the fusion launch of the C ABI declared in include/dmi.h: dmi_fuse, dmi_fuse_range, dmi_fuse_slab, and the
// three diagnostics that read the last launch's class table.  What CudaInitialize (cu:269-298) and ProcessDepthMap (cu:302-386)
// do in the reference once the depth maps are resident.  fuse_run is a sequence of steps -- the general kernel's arguments, the
// launch decisions (fusion_launch_rules.h), the tiled launch's geometry, its tables, the tuning hooks, the timed launch, the
// bookkeeping --; every table grows through dmi::ensure_idle_buffers or dmi::ensure_buffer (dmi_context.h), so a fusion of the
// same views into the same grid allocates, frees, fills and waits for nothing.  dmi_capi.hip has the context's life cycle,
// dmi_capi_views.hip the views.
#include "dmi_context.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

using dmi::drain_events;
using dmi::EventPair;
using dmi::fail;
using dmi::flush_zero_fill;
using dmi::FuseArgs;
using dmi::FuseConfig;
using dmi::guarded;
using dmi::MapRec;
using dmi::TileArgs;
using dmi::TileMapRec;

namespace {

// The views' records on the device, and a hit counter for each.  The four record arrays grow as a unit: a later call finds all
// four at one capacity or all four empty.  How much a launch may read of each and how much a growth allocates is the record
// tables' rule (fusion_launch_rules.h: the window column reads one WinRec beyond the last view).
static_assert(dmi::kRecordBytes[dmi::REC_MAP] == sizeof(MapRec) && dmi::kRecordBytes[dmi::REC_TILE_MAP] == sizeof(TileMapRec) &&
              dmi::kRecordBytes[dmi::REC_WIN] == sizeof(dmi::WinRec) && dmi::kRecordBytes[dmi::REC_FOOT] == sizeof(dmi::FootRec) &&
              dmi::kRecordBytes[dmi::REC_HITS] == sizeof(unsigned long long), "the record tables' rule has the records' sizes");
int sync_maps(dmi_context *ctx) {
  dmi_context::Views &v = ctx->views;
  const size_t n = v.h_maps.size();
  auto growth = [n](dmi::DeviceBuffer *b, dmi::RecordTable t) { return dmi::BufferGrowth{b, dmi::record_bytes_read(t, n), dmi::record_bytes_allocated(t, n)}; };
  bool fresh = false;
  int rc = dmi::ensure_idle_buffers(ctx, {growth(&v.maps, dmi::REC_MAP), growth(&v.tile_maps, dmi::REC_TILE_MAP),
                                          growth(&v.win_recs, dmi::REC_WIN), growth(&v.foot_recs, dmi::REC_FOOT)}, &fresh);
  if (rc != DMI_OK) return rc;
  if (fresh) v.maps_dirty = true;
  dmi::DeviceBuffer &hits = ctx->hits.map;
  if (ctx->opt.count_hits && !dmi::holds(hits, dmi::record_bytes_read(dmi::REC_HITS, n))) {
    // grow, keeping the counts gathered so far
    dmi::DeviceBuffer grown;
    rc = dmi::ensure_buffer(ctx, grown, dmi::record_bytes_allocated(dmi::REC_HITS, n));
    if (rc != DMI_OK) return rc;
    hipError_t e = hipMemsetAsync(grown.ptr, 0, grown.capacity, ctx->stream);
    if (e == hipSuccess && hits.ptr) {
      e = hipMemcpyAsync(grown.ptr, hits.ptr, hits.capacity, hipMemcpyDeviceToDevice, ctx->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    if (e != hipSuccess) {
      (void)hipGetLastError();
      dmi::drop_buffers(ctx, {&grown});
      return fail(ctx, DMI_ERR_DEVICE, std::string("growth of the views' hit counters: ") + hipGetErrorString(e));
    }
    std::swap(grown, hits);
    dmi::drop_buffers(ctx, {&grown});
  }
  if (v.maps_dirty) {
    DMI_HIP(ctx, hipMemcpyAsync(v.maps.ptr, v.h_maps.data(), n * sizeof(MapRec), hipMemcpyHostToDevice, ctx->stream));
    DMI_HIP(ctx, hipMemcpyAsync(v.tile_maps.ptr, v.h_tile_maps.data(), n * sizeof(TileMapRec), hipMemcpyHostToDevice, ctx->stream));
    DMI_HIP(ctx, hipMemcpyAsync(v.win_recs.ptr, v.h_win_recs.data(), n * sizeof(dmi::WinRec), hipMemcpyHostToDevice, ctx->stream));
    DMI_HIP(ctx, hipMemcpyAsync(v.foot_recs.ptr, v.h_foot_recs.data(), n * sizeof(dmi::FootRec), hipMemcpyHostToDevice, ctx->stream));
    // h_maps / h_tile_maps are pageable: the copies above are complete for the host when they return
    v.maps_dirty = false;
  }
  return DMI_OK;
}

// TileArgs::sb_perm for a slab of super_x x super_y x super_z super-bricks: the super-bricks sorted by the Morton code of
// their coordinates (z-major order when asked for: the enumeration until r03h).  Built on the host once per geometry.
int slot_permutation(dmi_context *ctx, int32_t super_x, int32_t super_y, int32_t super_z, bool zmajor, const int32_t **out) {
  std::vector<dmi_context::SlotPerm> &perms = ctx->tables.slot_perms;
  for (const auto &sp : perms)
    if (sp.super_x == super_x && sp.super_y == super_y && sp.super_z == super_z && sp.zmajor == (zmajor ? 1 : 0)) {
      *out = sp.perm.as<int32_t>();
      return DMI_OK;
    }
  if (super_x > 1023 || super_y > 1023 || super_z > 1023)
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_fuse: more than 1023 super-bricks along an axis");
  const size_t n = (size_t)super_x * super_y * super_z;
  auto spread = [](uint64_t v) {  // bit i -> bit 3i (10 bits)
    v &= 0x3ff;
    v = (v | (v << 16)) & 0x030000ffull;
    v = (v | (v << 8)) & 0x0300f00full;
    v = (v | (v << 4)) & 0x030c30c3ull;
    v = (v | (v << 2)) & 0x09249249ull;
    return v;
  };
  std::vector<std::pair<uint64_t, int32_t>> keyed(n);
  size_t q = 0;
  for (int32_t z = 0; z < super_z; ++z)
    for (int32_t y = 0; y < super_y; ++y)
      for (int32_t x = 0; x < super_x; ++x, ++q)
        keyed[q] = {zmajor ? (uint64_t)q : (spread(x) | (spread(y) << 1) | (spread(z) << 2)), x | (y << 10) | (z << 20)};
  if (!zmajor) std::sort(keyed.begin(), keyed.end());
  std::vector<int32_t> perm(n);
  for (size_t i = 0; i < n; ++i) perm[i] = keyed[i].second;
  dmi::DeviceBuffer d;  // (new: nothing queued reads it, the plain rule)
  const int rc = dmi::ensure_buffer(ctx, d, n * sizeof(int32_t));
  if (rc != DMI_OK) return rc;
  // pageable source: the copy has left the host buffer when the call returns
  hipError_t e = hipMemcpyAsync(d.ptr, perm.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && perms.size() >= 64) {  // a caller cycling through more slab geometries than that: start over
    e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) {
      for (auto &sp : perms) dmi::drop_buffers(ctx, {&sp.perm});
      perms.clear();
    }
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    dmi::drop_buffers(ctx, {&d});
    return fail(ctx, DMI_ERR_DEVICE, std::string("slot permutation upload: ") + hipGetErrorString(e));
  }
  perms.push_back({super_x, super_y, super_z, zmajor ? 1 : 0, d});
  *out = d.as<int32_t>();
  return DMI_OK;
}

// ---- the steps of fuse_run ------------------------------------------------------------------------------------------

// What the general kernel reads (and the tiled kernel's exact fallback, through a device copy): the grid, the ray potential,
// the views [first, first + count), the layers [z_first, z_first + z_count).
FuseArgs general_args(const dmi_context *ctx, int32_t first, int32_t count, int32_t z_first, int32_t z_count) {
  FuseArgs a;
  std::memset(&a, 0, sizeof(a));
  a.nx = ctx->grid.cell_dims[0];
  a.ny = ctx->grid.cell_dims[1];
  a.nz = ctx->grid.cell_dims[2];
  a.W = ctx->views.W;
  a.H = ctx->views.H;
  a.first_map = first;
  a.n_maps = count;
  // the layers being fused start from the grid's values unless all of them are known to be zero (a slab fuse leaves
  // the other layers as they were, so zero-ness is tracked per layer)
  a.init_from_grid = 0;
  for (int32_t z = z_first; z < z_first + z_count; ++z)
    if (!ctx->volume.layer_is_zero[(size_t)z]) a.init_from_grid = 1;
  a.kz0 = ctx->opt.z_first;
  a.k_first = z_first;
  a.k_count = z_count;
  a.ox = ctx->grid.origin[0];
  a.oy = ctx->grid.origin[1];
  a.oz = ctx->grid.origin[2];
  a.sx = ctx->grid.spacing[0];
  a.sy = ctx->grid.spacing[1];
  a.sz = ctx->grid.spacing[2];
  std::memcpy(a.g, ctx->grid.grid_matrix, 12 * sizeof(double));
  a.thick = ctx->ray.thickness;
  a.delta = ctx->ray.delta;
  a.rho_pos = ctx->ray.rho * 1.0;    // rho * sign, sign = +1 (cu:112,117)
  a.rho_neg = ctx->ray.rho * -1.0;   // sign = -1
  a.rho_zero = ctx->ray.rho * 0.0;   // sign = 0 (diff == 0 on the plateau branch: only if thickness < 0)
  a.slope = ctx->ray.rho / ctx->ray.thickness;  // cu:119
  a.free_space = -ctx->ray.eta * ctx->ray.rho;  // cu:115
  a.maps = ctx->views.maps.as<MapRec>();
  a.grid = ctx->volume.d_grid;
  a.voxel_hits = ctx->hits.voxel.as<uint32_t>();
  a.map_hits = ctx->hits.map.as<unsigned long long>();
  return a;
}

// the holes of ALL resident views, as the uploads counted them (dmi::hole_traits says what they mean for a launch)
dmi::HoleTraits resident_hole_traits(const dmi_context::Views &v) {
  unsigned long long mingled = 0, without = 0, strips = 0, pixels = 0;
  for (const dmi::Batch &bt : v.batches) {
    mingled += bt.mingled_strips;
    without += bt.holes;
    strips += (unsigned long long)bt.n * (unsigned long long)v.W * (unsigned long long)(v.H / 8);
    pixels += (unsigned long long)bt.n * (unsigned long long)v.W * (unsigned long long)v.H;
  }
  return dmi::hole_traits(mingled, without, strips, pixels);
}

// The bricks, super-bricks and workgroup slots of a tiled launch, its slot permutation, and what it copies from the general
// kernel's arguments.
int tile_geometry(dmi_context *ctx, const FuseArgs &a, const FuseConfig &cfg, const dmi::TileShape &sh, bool whole_grid, TileArgs *out) {
  TileArgs &t = *out;
  t.nx = a.nx; t.ny = a.ny; t.nz = a.nz; t.W = a.W; t.H = a.H;
  t.first_map = a.first_map; t.n_maps = a.n_maps; t.init_from_grid = a.init_from_grid;
  t.kpad = (a.nz + sh.tk - 1) / sh.tk * sh.tk;
  t.bricks_x = (a.nx + 8 * sh.wx - 1) / (8 * sh.wx);
  t.bricks_y = (a.ny + 8 * sh.wy - 1) / (8 * sh.wy);
  t.bricks_z = t.kpad / sh.tk;
  t.super_x = (t.bricks_x + 3) / 4;
  t.super_y = (t.bricks_y + 3) / 4;
  t.super_z = (t.bricks_z + 1) / 2;
  if (!whole_grid) {  // slab: super-brick layers [sbz_first, sbz_first + super_z)
    t.sbz_first = a.k_first / (2 * sh.tk);
    t.super_z = (a.k_first + a.k_count + 2 * sh.tk - 1) / (2 * sh.tk) - t.sbz_first;
  }
  if (t.bricks_x > 2047 || t.bricks_y > 2047 || t.bricks_z > 1023)  // pack_brick (fusion_kernels.h)
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_fuse: more bricks along an axis than the tiled kernel's order entries hold");
  t.slot_base = t.sbz_first * t.super_x * t.super_y * 32;
  t.slot_count = t.super_x * t.super_y * t.super_z * 32;
  const int rc = slot_permutation(ctx, t.super_x, t.super_y, t.super_z, (cfg.variant & dmi::VAR_ZMAJOR_SLOTS) != 0, &t.sb_perm);
  if (rc != DMI_OK) return rc;
  // spatial order: one z-layer of super-bricks per XCD and round (long runs keep an XCD on one region of every
  // depth map); heaviest-first order: one super-brick's worth, so that the heavy bricks spread over all XCDs
  t.xcd_run_wg = 32 * std::max(1, t.super_x * t.super_y);
  if (((int64_t)t.super_x * t.super_y * t.super_z * 32 + 16 * (int64_t)t.xcd_run_wg + 64) > (int64_t)0x7fffffff)
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_fuse: grid too large for one launch");
  t.depth_bytes = (int32_t)((int64_t)a.W * a.H * (ctx->views.depth_f64 ? 8 : 4));
  t.kz0 = a.kz0;
  t.ox = a.ox; t.oy = a.oy; t.oz = a.oz; t.sx = a.sx; t.sy = a.sy; t.sz = a.sz;
  std::memcpy(t.g, a.g, sizeof(t.g));
  t.thick = a.thick; t.delta = a.delta; t.rho_pos = a.rho_pos; t.rho_neg = a.rho_neg;
  t.slope = a.slope; t.free_space = a.free_space;
  t.tile_maps = ctx->views.tile_maps.as<TileMapRec>();
  t.grid = a.grid; t.voxel_hits = a.voxel_hits; t.map_hits = a.map_hits;
  t.rotated = dmi::grid_axis_aligned(ctx->grid) ? 0 : 1;
  t.flags = ((cfg.variant & dmi::VAR_NO_INTERIOR) ? dmi::TILE_FLAG_NO_INTERIOR : 0) |
            ((cfg.variant & dmi::VAR_XCD_RUNS) ? dmi::TILE_FLAG_XCD_RUNS : 0);
  t.maps = ctx->views.maps.as<MapRec>();
  // brick classes: one byte per (8 x 8 x column wave brick, resident view)
  t.wbricks_x = (a.nx + 7) / 8;
  t.wbricks_y = (a.ny + 7) / 8;
  return DMI_OK;
}

// r22*wz(k) table, one row of kpad doubles per resident view
// rotated: [kpad][4]; behind the table, the sums of n free-space constants (TileArgs::free_sums)
int cz_table(dmi_context *ctx, const FuseArgs &a, TileArgs *t) {
  const size_t table_doubles = std::max<size_t>(ctx->views.h_maps.size(), 4) * (size_t)t->kpad;
  const size_t need = table_doubles + (size_t)dmi::kFreeSumsMax + 1;
  // views often arrive in chunks: grow geometrically
  const int rc = dmi::ensure_idle_buffer(ctx, ctx->tables.cz_table, need * 8, need * 2 * 8);
  if (rc != DMI_OK) return rc;
  t->cz_table = ctx->tables.cz_table.as<double>();
  // valid while every sum of the launch starts at +0.0 and hits are not counted (counted views are taken one by one)
  if (!a.init_from_grid && !ctx->opt.count_hits && a.n_maps <= dmi::kFreeSumsMax) t->free_sums = t->cz_table + table_doubles;
  return DMI_OK;
}

// classes off: every brick reads the same all-BRICK_MIXED row (pitch 0), so the kernel needs no "have classes?"
// test in its view loop
int zero_row(dmi_context *ctx, TileArgs *t) {
  bool fresh = false;
  const int rc = dmi::ensure_idle_buffer(ctx, ctx->tables.zero_row, (uint64_t)t->class_pitch, (uint64_t)t->class_pitch, &fresh);
  if (rc != DMI_OK) return rc;
  if (fresh) DMI_HIP(ctx, hipMemsetAsync(ctx->tables.zero_row.ptr, dmi::BRICK_MIXED, (size_t)t->class_pitch, ctx->stream));
  t->classes = ctx->tables.zero_row.as<uint8_t>();
  t->class_pitch = 0;
  return DMI_OK;
}

// The brick classes of the launch, the coarse table behind them, and behind that -- for a launch with windows -- the window pairs.
int class_table(dmi_context *ctx, const dmi::TileShape &sh, bool windows, TileArgs *t) {
  const size_t fine_bytes = ((size_t)t->wbricks_x * t->wbricks_y * t->bricks_z * (size_t)t->class_pitch + 255) / 256 * 256;
  // the coarse table (one row per box of 32^3 voxels) lives behind the brick table in the same allocation
  const size_t coarse_end = (fine_bytes + (size_t)dmi::coarse_class_bytes(*t, sh.tk) + 255) / 256 * 256;
  // ... and behind that the window origins of the FREE column (TileArgs::win_origin), one word per class byte
  const size_t cbytes = coarse_end + (windows ? fine_bytes * sizeof(dmi::WinPair) : 0);
  ctx->tables.coarse_offset = fine_bytes;
  bool fresh = false;
  const int rc = dmi::ensure_idle_buffer(ctx, ctx->tables.classes, cbytes, cbytes, &fresh);
  if (rc != DMI_OK) return rc;
  // padding bytes (views beyond the resident ones) read as BRICK_SKIP
  if (fresh) DMI_HIP(ctx, hipMemsetAsync(ctx->tables.classes.ptr, dmi::BRICK_SKIP, cbytes, ctx->stream));
  t->classes = ctx->tables.classes.as<uint8_t>();
  if (windows) {
    t->win_origin = reinterpret_cast<dmi::WinPair *>(ctx->tables.classes.as<uint8_t>() + coarse_end);
    // (win_pair_index: the pair table has the class table's entries, fine_bytes of them at least, in blocks of 32 views)
    t->n_class_bricks = (int64_t)t->wbricks_x * t->wbricks_y * t->bricks_z;
    t->win_recs = ctx->views.win_recs.as<dmi::WinRec>();
    t->foot_recs = ctx->views.foot_recs.as<dmi::FootRec>();
    t->vb_bytes = (int32_t)std::min<int64_t>(dmi::valid_bits_bytes(ctx->views.W, ctx->views.H), 0x7fffffff);
    t->vb_rowskip = (dmi::valid_bits_tiles_x(ctx->views.W) - 1) * 128;
    t->win_cx = dmi::kValidMargin + ctx->views.W / 2;
    t->win_cy = dmi::kValidMargin + ctx->views.H / 2;
  }
  return DMI_OK;
}

// The workgroup order of a launch with classes: the count and order[], the ordering kernels' scratch; the pair grows as a unit.
int order_tables(dmi_context *ctx, const dmi::TileShape &sh, int variant, TileArgs *t) {
  const size_t n_slots = (size_t)t->super_x * t->super_y * t->super_z * 32;
  const size_t order_bytes = (n_slots + 1) * sizeof(int32_t), level_bytes = dmi::order_scratch_bytes(n_slots);
  const int rc = dmi::ensure_idle_buffers(ctx, {{&ctx->tables.order, order_bytes, order_bytes}, {&ctx->tables.order_level, level_bytes, level_bytes}});
  if (rc != DMI_OK) return rc;
  t->order = ctx->tables.order.as<int32_t>() + 1;  // [0] holds the count
  t->n_order = ctx->tables.order.as<int32_t>();
  // the ordering kernels leave the first position of every (level, chunk) behind the level bytes of their scratch
  // (launch_order_bricks): chunk 0's four entries are where the levels start
  t->order_levels = reinterpret_cast<const int32_t *>(ctx->tables.order_level.as<uint8_t>() + (n_slots + 15) / 16 * 16);
  t->xcd_run_wg = 32 * (4 / (sh.wx * sh.wy));  // 32 workgroups of four waves, 128 of one (profiles: 7.73 vs 7.78 ms)
  if (dmi::cost_order(sh.wx * sh.wy, variant, n_slots)) {
    t->flags |= dmi::TILE_FLAG_COST_ORDER | dmi::TILE_FLAG_XCD_RUNS;
    t->xcd_run_wg = 16;
  }
  return DMI_OK;
}

#ifdef DMI_TUNING  // tools/ builds only (DMI_TUNING=1 python -m cudadepthmapintegration_amd.build): never in the shipped library
int tuning_hooks(dmi_context *ctx, TileArgs *out) {
  TileArgs &t = *out;
  // timing experiment (results are wrong): a zero-length buffer makes the range check drop every depth load
  if (std::getenv("DMI_DEBUG_NO_DEPTH_LOADS")) t.depth_bytes = 0;
  if (std::getenv("DMI_DEBUG_WG_TIMES")) {  // per-workgroup start / end / XCC (tools/gpu_wg_timeline.py)
    const size_t per_round = 8 * (size_t)t.xcd_run_wg;
    const size_t blocks = ((size_t)t.super_x * t.super_y * t.super_z * 32 + 32 + per_round - 1) / per_round * per_round;  // launch_shape
    // (+ 2: the launch's window pairs and their redone wave-voxels, dmi_debug_window_counts)
    const size_t bytes = (blocks * 3 + 2) * sizeof(unsigned long long);
    const int rc = dmi::ensure_idle_buffer(ctx, ctx->tables.wg_times, bytes, bytes);
    if (rc != DMI_OK) return rc;
    ctx->tables.wg_times_blocks = blocks;  // of THIS launch (a smaller one after a larger reuses the buffer; a larger one reallocates)
    DMI_HIP(ctx, hipMemsetAsync(ctx->tables.wg_times.ptr, 0, bytes, ctx->stream));
    t.wg_times = ctx->tables.wg_times.as<unsigned long long>();
    t.wg_times_n = (int64_t)blocks;
  }
  if (const char *e = std::getenv("DMI_DEBUG_PAIRS")) {  // tools/gpu_pair_cost.sh (results are wrong)
    if (!std::strcmp(e, "nowin")) t.flags |= dmi::TILE_FLAG_DBG_SKIP_WINDOW_PAIRS;
    if (!std::strcmp(e, "onlywin")) t.flags |= dmi::TILE_FLAG_DBG_ONLY_WINDOW_PAIRS;
    if (!std::strcmp(e, "nowinloads")) t.flags |= dmi::TILE_FLAG_DBG_NO_WINDOW_LOADS;
  }
  if (const char *e = std::getenv("DMI_XCD_RUN_WG")) {  // launch-geometry experiments
    t.xcd_run_wg = std::max(1, std::atoi(e));
    if (((int64_t)t.super_x * t.super_y * t.super_z * 32 + 8 * (int64_t)t.xcd_run_wg) > (int64_t)0x7fffffff)
      return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_fuse: DMI_XCD_RUN_WG makes the launch too large");
  }
  return DMI_OK;
}
#endif

// The tables of a tiled launch, one helper each, and the decisions that size them: classes or not (cfg->variant gains
// VAR_NO_BRICK_CLASSES), windows or not, the behind mask.
int tile_tables(dmi_context *ctx, const FuseArgs &a, FuseConfig *cfg, const dmi::TileShape &sh, const dmi::HoleTraits &traits, TileArgs *out) {
  TileArgs &t = *out;
  int rc = cz_table(ctx, a, &t);
  if (rc == DMI_OK) rc = dmi::ensure_buffer(ctx, ctx->tables.queue_heads, 128 * sizeof(int32_t));
  if (rc != DMI_OK) return rc;
  t.queue_heads = ctx->tables.queue_heads.as<int32_t>();
  if (dmi::fuse_without_classes(cfg->variant, (int64_t)t.wbricks_x * t.wbricks_y * (int64_t)t.bricks_z, a.n_maps))
    cfg->variant |= dmi::VAR_NO_BRICK_CLASSES;
  t.class_pitch = dmi::class_table_pitch((int32_t)ctx->views.h_maps.size());
  const bool zero_free = dmi::zero_free(a.init_from_grid != 0, ctx->volume.grid_free_of_negative_zero, ctx->opt.count_hits != 0, cfg->variant);
  if (cfg->variant & dmi::VAR_NO_BRICK_CLASSES) {
    rc = zero_row(ctx, &t);
  } else {
    bool any_tier1 = false;  // (a launch none of whose views has a window record has no window pair: the plain instantiation serves it)
    for (int32_t m = a.first_map; m < a.first_map + a.n_maps && !any_tier1; ++m) any_tier1 = std::isfinite(ctx->views.h_win_recs[(size_t)m].e_abs);
    dmi::WindowsQuestion q;
    q.tier1 = DMI_TIER1 != 0;
    q.general_k = cfg->general_k != 0;
    q.count_hits = cfg->count_hits != 0;
    q.variant = cfg->variant;
    q.holes = cfg->holes != 0;
    q.many_borders = traits.many_borders;
    q.any_tier1 = any_tier1;
    q.zero_free = zero_free;
    q.depth_f64 = ctx->views.depth_f64;
    const bool windows = dmi::use_windows(q) && dmi::win_pair_pieces_addressable((int64_t)t.wbricks_x * t.wbricks_y * t.bricks_z);
    rc = class_table(ctx, sh, windows, &t);
    if (rc == DMI_OK && !(cfg->variant & dmi::VAR_SPATIAL_ORDER)) rc = order_tables(ctx, sh, cfg->variant, &t);
  }
  if (zero_free) t.behind_mask = 0x0101010101010101ull;
  return rc;
}

// The launch between two events of the pool (a third before the fusion kernel proper), queued for drain_events.
int timed_launch(dmi_context *ctx, const FuseArgs &a, const TileArgs &t, const FuseConfig &cfg) {
  EventPair ev;
  if (!ctx->pool.empty()) {
    ev = ctx->pool.back();
    ctx->pool.pop_back();
  } else {
    DMI_HIP(ctx, hipEventCreate(&ev.start));
    DMI_HIP(ctx, hipEventCreate(&ev.stop));
    DMI_HIP(ctx, hipEventCreate(&ev.mid));
  }
  // (the event between the preparation launches and the fusion kernel costs ~6 us of idle queue: a launch without brick
  // classes -- tiny grids, 50 us in all -- has one 3-us table kernel before its fusion kernel and is timed as a whole)
  ev.has_mid = cfg.use_tile != 0 && !(cfg.variant & dmi::VAR_NO_BRICK_CLASSES);
  DMI_HIP(ctx, hipEventRecord(ev.start, ctx->stream));
  const dmi_context::LaunchTables &tb = ctx->tables;
  hipError_t e = cfg.use_tile ? dmi::launch_fuse_tiled(t, ctx->views.maps.as<MapRec>(), cfg, ctx->views.pyramid, tb.order_level.as<uint8_t>(),
                                                         tb.classes.ptr ? tb.classes.as<uint8_t>() + tb.coarse_offset : nullptr,
                                                         ev.has_mid ? ev.mid : nullptr, ctx->stream) : dmi::launch_fuse(a, cfg, ctx->stream);
  if (e != hipSuccess) {
    ctx->pool.push_back(ev);
    (void)hipGetLastError();
    return fail(ctx, DMI_ERR_DEVICE, std::string("fusion kernel launch: ") + hipGetErrorString(e));
  }
  DMI_HIP(ctx, hipEventRecord(ev.stop, ctx->stream));
  ctx->pending.push_back(ev);
  return DMI_OK;
}

int fuse_run(dmi_context *ctx, int32_t first, int32_t count, int32_t z_first, int32_t z_count, bool tiled, int run_k_mode,
             bool general_k) {
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  int rc = sync_maps(ctx);
  if (rc != DMI_OK) return rc;
  const bool whole_grid = z_first == 0 && z_count == ctx->grid.cell_dims[2];
  if (!whole_grid) {
    // a slab fuse writes only its layers: a deferred zero fill of the rest must happen now
    rc = flush_zero_fill(ctx);
    if (rc != DMI_OK) return rc;
  }
  const FuseArgs a = general_args(ctx, first, count, z_first, z_count);

  // the launch decisions (fusion_launch_rules.h)
  const dmi::HoleTraits traits = resident_hole_traits(ctx->views);
  FuseConfig cfg;
  cfg.depth_is_f64 = ctx->views.depth_f64 ? 1 : 0;
  cfg.grid_is_f64 = ctx->opt.grid_dtype == DMI_F64 ? 1 : 0;
  cfg.k_mode = run_k_mode;
  cfg.count_hits = ctx->opt.count_hits ? 1 : 0;
  cfg.use_tile = tiled ? 1 : 0;
  cfg.general_k = tiled && general_k ? 1 : 0;
  cfg.holes = traits.holes ? 1 : 0;
  cfg.variant = dmi::with_default_tile_shape(ctx->opt.kernel_variant, tiled, traits, a.nx, a.ny, a.nz);

  TileArgs t;
  std::memset(&t, 0, sizeof(t));
  if (cfg.use_tile) {
    const dmi::TileShape sh = dmi::tile_shape(cfg.variant, ctx->views.depth_f64, !dmi::grid_axis_aligned(ctx->grid), cfg.general_k != 0);
    rc = tile_geometry(ctx, a, cfg, sh, whole_grid, &t);
    if (rc == DMI_OK) rc = tile_tables(ctx, a, &cfg, sh, traits, &t);
#ifdef DMI_TUNING
    if (rc == DMI_OK) rc = tuning_hooks(ctx, &t);
#endif
    if (rc == DMI_OK) rc = dmi::ensure_buffer(ctx, ctx->tables.fuse_args, sizeof(FuseArgs));
    if (rc != DMI_OK) return rc;
    // pageable source: the copy has left the host buffer when the call returns
    DMI_HIP(ctx, hipMemcpyAsync(ctx->tables.fuse_args.ptr, &a, sizeof(FuseArgs), hipMemcpyHostToDevice, ctx->stream));
    t.full = ctx->tables.fuse_args.as<FuseArgs>();
  }

  rc = timed_launch(ctx, a, t, cfg);
  if (rc != DMI_OK) return rc;

  dmi_context::LastLaunch &last = ctx->last;
  last.tiled = cfg.use_tile != 0;
  last.classes = cfg.use_tile != 0 && !(cfg.variant & dmi::VAR_NO_BRICK_CLASSES);
  last.class_bricks = (int64_t)t.wbricks_x * t.wbricks_y * t.bricks_z;
  last.bricks_z = t.bricks_z;
  last.tk = t.bricks_z > 0 ? t.kpad / t.bricks_z : 0;
  last.win_origin = t.win_origin;
  last.class_pitch = t.class_pitch;
  last.first = first;
  last.count = count;
  // after a whole-grid fuse every voxel has been written; after a slab fuse the other layers still hold what they
  // held (zeros after a reset): later fuses read the grid, which is correct either way
  for (int32_t z = z_first; z < z_first + z_count; ++z) ctx->volume.layer_is_zero[(size_t)z] = 0;
  ctx->volume.zero_fill_pending = false;
  ctx->c2p.valid = false;
  if (ctx->pending.size() >= 256) return drain_events(ctx);
  return DMI_OK;
}

// The class rows of the last launch, downloaded: visit(brick, class byte) for every (wave brick, view of that launch).  A last
// launch without classes visits nothing.
template <typename Visit>
int visit_last_classes(dmi_context *ctx, Visit &&visit) {
  const dmi_context::LastLaunch &last = ctx->last;
  if (!last.classes) return DMI_OK;
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  const size_t bytes = (size_t)last.class_bricks * last.class_pitch;
  std::vector<uint8_t> host(bytes);
  DMI_HIP(ctx, hipMemcpyAsync(host.data(), ctx->tables.classes.ptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
  DMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int64_t b = 0; b < last.class_bricks; ++b) {
    const uint8_t *row = host.data() + (size_t)b * last.class_pitch + last.first;
    for (int32_t m = 0; m < last.count; ++m) visit(b, row[m]);
  }
  return DMI_OK;
}

}  // namespace

namespace dmi {

// Views [first, first + count) into the cell layers [z_first, z_first + z_count).  The reference handles any 4x4 K at
// one speed (cu:176); here the register-tiled kernel takes every view that meets its per-view preconditions (a K with a
// general third row through its GENK instantiation) and the general kernel the rest: maximal runs of consecutive views
// of one kind, launched in view order, so every voxel still accumulates its views in order (cu:211).  An f32 grid is
// rounded once per launch, i.e. once per run.
int fuse_views(dmi_context *ctx, int32_t first, int32_t count, int32_t z_first, int32_t z_count) {
  const dmi_context::Views &v = ctx->views;
  const int32_t n_views = (int32_t)v.h_maps.size();
  if (n_views == 0) return fail(ctx, DMI_ERR_STATE, "dmi_fuse: no views resident (call dmi_add_views first)");
  if (first < 0 || count < 0 || first > n_views || count > n_views - first)
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_fuse_range: range outside the resident views");
  if (count == 0) return DMI_OK;
  const bool tile_possible = tile_eligible(ctx);
  int32_t m = first;
  while (m < first + count) {
    const bool tiled = tile_possible && v.view_tile_ok[(size_t)m];
    int32_t e = m;
    int km = dmi::K_PINHOLE;
    bool general_k = false;
    while (e < first + count && (tile_possible && v.view_tile_ok[(size_t)e]) == tiled) {
      km = std::min(km, (int)v.view_k_mode[(size_t)e]);
      general_k = general_k || v.view_k_mode[(size_t)e] == dmi::K_GENERAL;
      ++e;
    }
    const int rc = fuse_run(ctx, m, e - m, z_first, z_count, tiled, km, general_k);
    if (rc != DMI_OK) return rc;
    m = e;
  }
  return DMI_OK;
}

}  // namespace dmi

extern "C" {

int dmi_fuse_range(dmi_context *ctx, int32_t first, int32_t count) {
  return guarded(ctx, "dmi_fuse_range", [&]() -> int {
  if (!ctx) return DMI_ERR_INVALID_ARGUMENT;
  return dmi::fuse_views(ctx, first, count, 0, ctx->grid.cell_dims[2]);
  });
}

int dmi_fuse_slab(dmi_context *ctx, int32_t z_first, int32_t z_count) {
  return guarded(ctx, "dmi_fuse_slab", [&]() -> int {
  if (!ctx) return DMI_ERR_INVALID_ARGUMENT;
  const int32_t nz = ctx->grid.cell_dims[2];
  if (z_first < 0 || z_count < 0 || z_first > nz || z_count > nz - z_first)
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_fuse_slab: layers outside the grid");
  if (z_first % DMI_SLAB_ALIGNMENT != 0 || (z_first + z_count != nz && (z_first + z_count) % DMI_SLAB_ALIGNMENT != 0))
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_fuse_slab: slab boundaries must be multiples of DMI_SLAB_ALIGNMENT (32) cells");
  if (z_count == 0) return DMI_OK;
  return dmi::fuse_views(ctx, 0, (int32_t)ctx->views.h_maps.size(), z_first, z_count);
  });
}

int dmi_fuse(dmi_context *ctx) {
  return guarded(ctx, "dmi_fuse", [&]() -> int {
  if (!ctx) return DMI_ERR_INVALID_ARGUMENT;
  return dmi_fuse_range(ctx, 0, (int32_t)ctx->views.h_maps.size());
  });
}

int dmi_get_brick_class_histogram(dmi_context *ctx, uint64_t out[4]) {
  return guarded(ctx, "dmi_get_brick_class_histogram", [&]() -> int {
  if (!ctx || !out) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_get_brick_class_histogram: null argument");
  out[0] = out[1] = out[2] = out[3] = 0;
  return visit_last_classes(ctx, [&](int64_t, uint8_t c) { out[c & 3] += 1; });
  });
}

int dmi_get_mixed_reason_histogram(dmi_context *ctx, uint64_t out[8]) {
  return guarded(ctx, "dmi_get_mixed_reason_histogram", [&]() -> int {
  if (!ctx || !out) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_get_mixed_reason_histogram: null argument");
  for (int i = 0; i < 8; ++i) out[i] = 0;
  return visit_last_classes(ctx, [&](int64_t, uint8_t c) {
    if ((c & 3) == dmi::BRICK_MIXED) out[(c >> 2) & 7] += 1;
  });
  });
}

int dmi_get_window_pair_count(dmi_context *ctx, uint64_t *out) {
  return guarded(ctx, "dmi_get_window_pair_count", [&]() -> int {
  if (!ctx || !out) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_get_window_pair_count: null argument");
  *out = 0;
  const dmi_context::LastLaunch &last = ctx->last;
  if (!last.win_origin) return DMI_OK;
  const int64_t per_layer = last.class_bricks / std::max<int64_t>(1, last.bricks_z);
  return visit_last_classes(ctx, [&](int64_t b, uint8_t c) {
    const int64_t bz = b / std::max<int64_t>(1, per_layer);
    if (bz * last.tk + last.tk > ctx->grid.cell_dims[2]) return;  // a brick that sticks out of the top: no windows
    if ((c & 0x3f) == (dmi::BRICK_MIXED | (dmi::MIXED_FREE_OR_NODEPTH << 2))) *out += 1;  // (no CLASS_NO_WINDOW)
  });
  });
}

}  // extern "C"
