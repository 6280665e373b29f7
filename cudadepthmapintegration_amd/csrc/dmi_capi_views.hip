// dmi_capi_views.hip -- the resident views' part of the C ABI of include/dmi.h: dmi_add_views*, dmi_clear_views,
// dmi_get_upload_kernel_ms and dmi_get_view_paths.  The upload of a batch of depth maps (staging, the upload kernels, the
// promotion of the store to f64), all or nothing, and the records of its views: the arithmetic of those is view_records.h's
// make_view_records, this file sets their device pointers.  The context it works on is dmi_context.h's; dmi_capi.hip has the
// context's life cycle and the shared helpers.
#include "dmi_context.h"
#include "dmi_view_set.h"

#include <chrono>
#include <cstring>

using dmi::Batch;
using dmi::fail;
using dmi::guarded;
using dmi::MapRec;
using dmi::tile_eligible;

namespace {

size_t depth_elem(const dmi_context *c) { return c->views.depth_f64 ? 8 : 4; }

// (the upload stream is idle between two uploads: the plain rule, each staging buffer by what the call needs of it)
int ensure_stage(dmi_context *ctx, size_t elems, bool need_cost) {
  return dmi::ensure_buffers(ctx, {{&ctx->views.stage_depth, elems * 8}, {&ctx->views.stage_cost, need_cost ? elems * 8 : 0}});
}

// Converts the whole store to f64 (AUTO promotion).  f32 -> f64 is exact.  All or nothing: every batch is widened into
// a new buffer first; only when every allocation and kernel has succeeded are the pointers swapped, the old buffers
// freed and the storage type changed.  On failure the new buffers are freed and the f32 store is untouched.
int promote_to_f64(dmi_context *ctx) {
  const size_t npix = (size_t)ctx->views.W * ctx->views.H;
  std::vector<double *> wide(ctx->views.batches.size(), nullptr);
  hipError_t e = hipSuccess;
  for (size_t q = 0; e == hipSuccess && q < ctx->views.batches.size(); ++q) {
    const Batch &b = ctx->views.batches[q];
    e = hipMalloc(&wide[q], npix * b.n * 8);
    if (e == hipSuccess)
      e = dmi::launch_widen_depth(static_cast<const float *>(b.d_depth), wide[q], (int64_t)npix * b.n, ctx->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    for (double *p : wide)
      if (p) (void)hipFree(p);
    return fail(ctx, e == hipErrorOutOfMemory ? DMI_ERR_OUT_OF_MEMORY : DMI_ERR_DEVICE,
                std::string("promotion of the depth store to f64: ") + hipGetErrorString(e));
  }
  size_t map_index = 0;
  for (size_t q = 0; q < ctx->views.batches.size(); ++q) {
    Batch &b = ctx->views.batches[q];
    (void)hipFree(b.d_depth);
    ctx->device_bytes += npix * b.n * 4;
    b.d_depth = wide[q];
    for (int i = 0; i < b.n; ++i) {
      ctx->views.h_maps[map_index + i].depth = wide[q] + npix * i;
      ctx->views.h_tile_maps[map_index + i].depth = wide[q] + npix * i;
    }
    map_index += b.n;
  }
  ctx->views.depth_f64 = true;
  ctx->views.maps_dirty = true;
  return DMI_OK;
}

// Uploads n maps (host f64 or f32) into a new batch buffer of the current storage type.
// Returns the number of lossy f32 conversions through *lossy_out.
// on_device: depth64 is device memory the upload stream may read now (a view set's planes, dmi_add_views_from_set): the upload
// pass reads it where it is, nothing is staged.
int upload_batch(dmi_context *ctx, const double *depth64, const float *depth32, const double *best_cost,
                 double threshold, int32_t n, Batch *out, unsigned long long *lossy_out, bool on_device) {
  const size_t npix = (size_t)ctx->views.W * ctx->views.H;
  const size_t esz = depth_elem(ctx);
  Batch b;
  b.n = n;
  DMI_HIP(ctx, hipMalloc(&b.d_depth, npix * n * esz));
  ctx->device_bytes += npix * n * esz;
  // the pyramids of the batch, and behind them its validity maps (TileMapRec::valid): one allocation
  const size_t pyr_only = ((size_t)ctx->views.pyramid.total_tiles * n * sizeof(dmi::DepthTile) + 255) / 256 * 256;
  const size_t maps_end = (pyr_only + (size_t)dmi::valid_map_bytes(ctx->views.W, ctx->views.H) * n + 255) / 256 * 256;
  const size_t pyr_bytes = maps_end + (size_t)dmi::valid_bits_bytes(ctx->views.W, ctx->views.H) * n;
  b.valid_offset = pyr_only;
  b.bits_offset = maps_end;
  b.aux_bytes = pyr_bytes;
  {
    hipError_t pe = hipMalloc(&b.d_pyramid, pyr_bytes);
    if (pe != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(b.d_depth);
      ctx->device_bytes -= npix * n * esz;
      return fail(ctx, DMI_ERR_OUT_OF_MEMORY, std::string("hipMalloc(pyramid): ") + hipGetErrorString(pe));
    }
  }
  ctx->device_bytes += pyr_bytes;
  *lossy_out = 0;
  int rc = DMI_OK;
  // Every path ends in a device kernel that writes the table top row first (the reference's vtk order is
  // bottom row first, cu:141-149): <= 256 MiB of host data is staged at a time.
  const size_t in_elem = depth32 ? 4 : 8;
  const size_t maps_per_chunk = std::max<size_t>(1, (size_t(256) << 20) / (npix * 8));
  const size_t chunk = std::min<size_t>(maps_per_chunk, (size_t)n);
  if (!on_device) rc = ensure_stage(ctx, chunk * npix, best_cost != nullptr);
  if (rc == DMI_OK) {
    hipError_t e = hipMemsetAsync(ctx->views.lossy.as<unsigned long long>(), 0, 3 * sizeof(unsigned long long), ctx->upload_stream);  // [1], [2]: launch_build_valid_maps' counts
    for (size_t m0 = 0; e == hipSuccess && m0 < (size_t)n; m0 += chunk) {
      const size_t cnt = std::min(chunk, (size_t)n - m0);
      const char *src = depth32 ? reinterpret_cast<const char *>(depth32) : reinterpret_cast<const char *>(depth64);
      const double *staged = on_device ? depth64 + m0 * npix : ctx->views.stage_depth.as<double>();
      if (!on_device)
        e = hipMemcpyAsync(ctx->views.stage_depth.as<double>(), src + m0 * npix * in_elem, cnt * npix * in_elem, hipMemcpyHostToDevice,
                           ctx->upload_stream);
      if (e == hipSuccess && best_cost)
        e = hipMemcpyAsync(ctx->views.stage_cost.as<double>(), best_cost + m0 * npix, cnt * npix * 8, hipMemcpyHostToDevice, ctx->upload_stream);
      void *dst = static_cast<char *>(b.d_depth) + m0 * npix * esz;
      // one pass over the staged tables: threshold, row flip, narrowing, the finest pyramid level, validity bytes and bits
      const bool timed = m0 + cnt >= (size_t)n && ctx->views.up_events[0] && ctx->views.up_events[1];  // (the last chunk of the call: with it, the pyramid levels)
      if (e == hipSuccess && timed) e = hipEventRecord(ctx->views.up_events[0], ctx->upload_stream);
      if (e == hipSuccess)
        e = dmi::launch_upload_views(staged, depth32 ? 0 : 1, (!depth32 && best_cost) ? ctx->views.stage_cost.as<double>() : nullptr, threshold,
                                     dst, ctx->views.depth_f64 ? 1 : 0, (int64_t)cnt, ctx->views.W, ctx->views.H, ctx->views.pyramid,
                                     b.d_pyramid + m0 * (size_t)ctx->views.pyramid.total_tiles,
                                     reinterpret_cast<uint8_t *>(b.d_pyramid) + b.valid_offset + m0 * (size_t)dmi::valid_map_bytes(ctx->views.W, ctx->views.H),
                                     reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(b.d_pyramid) + b.bits_offset +
                                                                  m0 * (size_t)dmi::valid_bits_bytes(ctx->views.W, ctx->views.H)),
                                     ctx->views.lossy.as<unsigned long long>(), ctx->upload_stream);
    }
    // depth bounds per 16 x 16 ... image-sized tile of every table: what the brick classification reads
    if (e == hipSuccess) e = dmi::launch_build_pyramid_levels(n, ctx->views.pyramid, b.d_pyramid, ctx->upload_stream);
    if (e == hipSuccess && ctx->views.up_events[0] && ctx->views.up_events[1]) e = hipEventRecord(ctx->views.up_events[1], ctx->upload_stream);
    unsigned long long counters[3] = {0, 0, 0};
    if (e == hipSuccess)
      e = hipMemcpyAsync(counters, ctx->views.lossy.as<unsigned long long>(), sizeof(counters), hipMemcpyDeviceToHost, ctx->upload_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->upload_stream);
    if (e == hipSuccess && ctx->views.up_events[0] && ctx->views.up_events[1]) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ctx->views.up_events[0], ctx->views.up_events[1]) == hipSuccess) {
        // (a call of several staged chunks times its last one: scaled to the call's views)
        const size_t last_cnt = (size_t)n - ((size_t)n - 1) / chunk * chunk;
        ctx->views.last_upload_kernel_ms = (double)ms * (double)n / (double)last_cnt;
        ctx->views.total_upload_kernel_ms += ctx->views.last_upload_kernel_ms;
      } else {
        (void)hipGetLastError();
      }
    }
    *lossy_out = counters[0];
    b.holes = counters[1];
    b.mingled_strips = counters[2];
    if (e != hipSuccess) rc = fail(ctx, DMI_ERR_DEVICE, std::string("depth upload: ") + hipGetErrorString(e));
  }
  if (rc != DMI_OK) {
    (void)hipFree(b.d_depth);
    (void)hipFree(b.d_pyramid);
    ctx->device_bytes -= npix * n * esz + pyr_bytes;
    return rc;
  }
  *out = b;
  return DMI_OK;
}

int add_views_impl(dmi_context *ctx, const double *depth64, const float *depth32, const double *best_cost,
                   double threshold, const double *K4, const double *RT4, int32_t n, int32_t width, int32_t height,
                   bool on_device = false) {
  if (!ctx) return DMI_ERR_INVALID_ARGUMENT;
  if ((!depth64 && !depth32) || !K4 || !RT4) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_add_views: null pointer");
  if (n <= 0) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_add_views: n must be positive");
  if (width < 1 || height < 1 || width > 32768 || height > 32768)
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_add_views: depth-map dimensions must be in [1, 32768]");
  if (!ctx->views.batches.empty() && (width != ctx->views.W || height != ctx->views.H))
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_add_views: every view of a context must share width and height");
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  const auto t0 = std::chrono::steady_clock::now();
  if (ctx->views.batches.empty()) {
    ctx->views.W = width;
    ctx->views.H = height;
    ctx->views.depth_f64 = ctx->opt.depth_storage == DMI_DEPTH_F64;
    ctx->views.k_mode = ctx->finite_bounded ? (int)dmi::K_PINHOLE : (int)dmi::K_GENERAL;
    ctx->views.max_tile_err = 0.0;
    ctx->views.pyramid = dmi::make_pyramid_desc(width, height);
  }
  const size_t npix = (size_t)width * height;

  Batch b;
  unsigned long long lossy = 0;
  int rc = upload_batch(ctx, depth64, depth32, best_cost, threshold, n, &b, &lossy, on_device);
  if (rc != DMI_OK) return rc;
  if (lossy != 0 && !ctx->views.depth_f64 && ctx->opt.depth_storage == DMI_DEPTH_AUTO) {
    // some depth is not an f32: keep every bit -> promote the whole store and redo this batch in f64
    (void)hipFree(b.d_depth);
    (void)hipFree(b.d_pyramid);
    ctx->device_bytes -= npix * n * 4 + b.aux_bytes;
    rc = promote_to_f64(ctx);
    if (rc != DMI_OK) return rc;
    rc = upload_batch(ctx, depth64, depth32, best_cost, threshold, n, &b, &lossy, on_device);
    if (rc != DMI_OK) return rc;
  }
  ctx->views.batches.push_back(b);
  const size_t esz = depth_elem(ctx);
  const dmi::ViewFrame frame = {ctx->grid, ctx->opt.z_first, ctx->views.W, ctx->views.H};
  for (int32_t m = 0; m < n; ++m) {
    MapRec r;
    std::memset(&r, 0, sizeof(r));
    // rows 0..2 of the row-major 4x4s (cu:220-230 marshals all 16; the kernel reads 12, cu:90-92)
    std::memcpy(r.rt, RT4 + 16 * (size_t)m, 12 * sizeof(double));
    std::memcpy(r.k, K4 + 16 * (size_t)m, 12 * sizeof(double));
    r.depth = static_cast<const char *>(b.d_depth) + (size_t)m * npix * esz;
    r.pyramid = b.d_pyramid + (size_t)m * ctx->views.pyramid.total_tiles;
    ctx->views.h_maps.push_back(r);
    dmi::ViewRecords v = dmi::make_view_records(frame, r.rt, r.k);
    if (v.k_mode < ctx->views.k_mode) ctx->views.k_mode = v.k_mode;
    v.tile.depth = r.depth;
    v.tile.valid = reinterpret_cast<const uint8_t *>(b.d_pyramid) + b.valid_offset + (size_t)m * (size_t)dmi::valid_map_bytes(ctx->views.W, ctx->views.H);
    v.tile.vbits = reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(b.d_pyramid) + b.bits_offset +
                                                      (size_t)m * (size_t)dmi::valid_bits_bytes(ctx->views.W, ctx->views.H));
    v.win.vbits = v.tile.vbits;
    ctx->views.h_tile_maps.push_back(v.tile);
    ctx->views.h_win_recs.push_back(v.win);
    ctx->views.h_foot_recs.push_back(v.foot);
    if (!(v.tile.err <= ctx->views.max_tile_err)) ctx->views.max_tile_err = v.tile.err;  // NaN-propagating max
    ctx->views.view_k_mode.push_back((uint8_t)v.k_mode);
    ctx->views.view_tile_ok.push_back(v.tile_ok ? 1 : 0);
  }
  ctx->views.maps_dirty = true;
  ctx->timings.last_upload_ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return DMI_OK;
}

}  // namespace

extern "C" {

int dmi_get_upload_kernel_ms(dmi_context *ctx, double *last, double *total) {
  if (!ctx) return DMI_ERR_INVALID_ARGUMENT;
  if (last) *last = ctx->views.last_upload_kernel_ms;
  if (total) *total = ctx->views.total_upload_kernel_ms;
  return DMI_OK;
}

int dmi_add_views(dmi_context *ctx, const double *depth, const double *best_cost, double threshold, const double *K4,
                  const double *RT4, int32_t n, int32_t width, int32_t height) {
  return guarded(ctx, "dmi_add_views", [&]() -> int {
  return add_views_impl(ctx, depth, nullptr, best_cost, threshold, K4, RT4, n, width, height);
  });
}

int dmi_add_views_f32(dmi_context *ctx, const float *depth, const double *K4, const double *RT4, int32_t n,
                      int32_t width, int32_t height) {
  return guarded(ctx, "dmi_add_views_f32", [&]() -> int {
  return add_views_impl(ctx, nullptr, depth, nullptr, 0.0, K4, RT4, n, width, height);
  });
}

int dmi_add_views_from_set(dmi_context *ctx, const dmi_view_set *s, int32_t first, int32_t count) {
  return guarded(ctx, "dmi_add_views_from_set", [&]() -> int {
  if (!ctx) return DMI_ERR_INVALID_ARGUMENT;
  auto bad = [&](const char *what) { return fail(ctx, DMI_ERR_INVALID_ARGUMENT, std::string("dmi_add_views_from_set: ") + what); };
  if (!s) return bad("the set is null");
  if (s->n < 1) return bad("the set holds no views");
  if (first < 0 || count < 1 || (int64_t)first + count > s->n) return bad("first and count must name views of the set");
  if (s->device != ctx->opt.device) return bad("the set and the context must be on one device");
  if (!ctx->views.batches.empty() && (s->W != ctx->views.W || s->H != ctx->views.H))
    return bad("every view of a context must share width and height");
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  // the set's queued work first (its calls synchronise, so this costs nothing; it states the order)
  DMI_HIP(ctx, hipEventRecord(s->handed_over, s->stream));
  DMI_HIP(ctx, hipStreamWaitEvent(ctx->upload_stream, s->handed_over, 0));
  const size_t npix = (size_t)s->W * (size_t)s->H;
  return add_views_impl(ctx, s->plane[s->current].as<double>() + (size_t)first * npix, nullptr, nullptr, 0.0,
                        s->K4.data() + 16 * (size_t)first, s->RT4.data() + 16 * (size_t)first, count, s->W, s->H, true);
  });
}

int dmi_clear_views(dmi_context *ctx) {
  return guarded(ctx, "dmi_clear_views", [&]() -> int {
  if (!ctx) return DMI_ERR_INVALID_ARGUMENT;
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  DMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const size_t npix = (size_t)ctx->views.W * ctx->views.H;
  for (Batch &b : ctx->views.batches) {
    (void)hipFree(b.d_depth);
    (void)hipFree(b.d_pyramid);
    ctx->device_bytes -= npix * b.n * depth_elem(ctx) + b.aux_bytes;
  }
  ctx->views.batches.clear();
  ctx->views.h_maps.clear();
  ctx->views.h_tile_maps.clear();
  ctx->views.h_win_recs.clear();
  ctx->views.h_foot_recs.clear();
  ctx->views.view_k_mode.clear();
  ctx->views.view_tile_ok.clear();
  ctx->views.max_tile_err = 0.0;
  ctx->views.maps_dirty = true;
  ctx->views.W = ctx->views.H = 0;
  return DMI_OK;
  });
}

int dmi_get_view_paths(dmi_context *ctx, uint64_t out[6]) {
  return guarded(ctx, "dmi_get_view_paths", [&]() -> int {
  if (!ctx || !out) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_get_view_paths: null argument");
  for (int i = 0; i < 6; ++i) out[i] = 0;
  const bool possible = tile_eligible(ctx);
  for (size_t m = 0; m < ctx->views.h_maps.size(); ++m) {
    bool windows = false;
    out[dmi::view_path(possible, ctx->views.view_tile_ok[m] != 0, ctx->views.view_k_mode[m], ctx->views.h_tile_maps[m], ctx->views.h_win_recs[m], &windows)] += 1;
    if (windows) out[5] += 1;
  }
  return DMI_OK;
  });
}

}  // extern "C"
