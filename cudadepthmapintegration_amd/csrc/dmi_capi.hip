// dmi_capi.hip -- implementation of the C ABI declared in include/dmi.h.
//
// Creation, destruction, grid transfer, info, timings and the hardware probes; the resident views (their upload and their records)
// are in dmi_capi_views.hip, the fusion launch and the diagnostics that read it in dmi_capi_fuse.hip, the point data and the mesh
// entry points in dmi_capi_mesh.hip, the context all four work on in dmi_context.h.  No buffer of the context is allocated, freed
// or counted here but through that header's growth helpers (defined below).
// Host-side driver of the fusion path: what CudaInitialize (cu:269-298) and ProcessDepthMap
// (cu:302-386) do in the reference, minus the disk I/O and the VTK types.  No global state: everything
// lives in the context (the reference keeps __constant__ symbols and ch_gridDims, cu:55-64).
#include "dmi_context.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

using dmi::Batch;
using dmi::bounded;
using dmi::drain_c2p;
using dmi::drain_events;
using dmi::EventPair;
using dmi::fail;
using dmi::flush_zero_fill;
using dmi::fuse_views;
using dmi::tile_eligible;
using dmi::guarded;

namespace {

thread_local std::string g_create_error;

using dmi::grid_elem;
}  // namespace

namespace dmi {  // the helpers dmi_context.h declares

int fail(dmi_context *ctx, int code, const std::string &msg) {
  if (ctx)
    ctx->err = msg;
  else
    g_create_error = msg;
  return code;
}

int drain_events(dmi_context *ctx) {
  for (EventPair &p : ctx->pending) {
    DMI_HIP(ctx, hipEventSynchronize(p.stop));
    float ms = 0.f;
    DMI_HIP(ctx, hipEventElapsedTime(&ms, p.start, p.stop));
    ctx->timings.last_fuse_kernel_ms = ms;
    ctx->timings.total_fuse_kernel_ms += ms;
    ctx->timings.fuse_launches += 1;
    float main_ms = ms;  // the general kernel has no preparation launches
    if (p.has_mid) DMI_HIP(ctx, hipEventElapsedTime(&main_ms, p.mid, p.stop));
    ctx->timings.last_fuse_main_kernel_ms = main_ms;
    ctx->timings.total_fuse_main_kernel_ms += main_ms;
    ctx->pool.push_back(p);
  }
  ctx->pending.clear();
  return DMI_OK;
}

int flush_zero_fill(dmi_context *ctx) {
  if (ctx->volume.zero_fill_pending) {
    DMI_HIP(ctx, hipMemsetAsync(ctx->volume.d_grid, 0, ctx->n_voxels * grid_elem(ctx), ctx->stream));
    ctx->volume.zero_fill_pending = false;
  }
  return DMI_OK;
}

namespace {
int growth_failed(dmi_context *ctx, hipError_t grown) {
  (void)hipGetLastError();
  return fail(ctx, grown == hipErrorOutOfMemory ? DMI_ERR_OUT_OF_MEMORY : DMI_ERR_DEVICE,
              std::string("hipMalloc(&buffer.ptr, (size_t)bytes): ") + hipGetErrorString(grown));  // (the message as it always read)
}
}  // namespace

int ensure_buffer(dmi_context *ctx, DeviceBuffer &buffer, uint64_t bytes) {
  const hipError_t grown = grow_buffer(buffer, bytes, ctx->device_bytes);
  return grown == hipSuccess ? DMI_OK : growth_failed(ctx, grown);
}

int ensure_idle_buffers(dmi_context *ctx, std::initializer_list<BufferGrowth> unit, bool *fresh) {
  const hipError_t grown = grow_idle_buffers(unit, ctx->stream, ctx->device_bytes, fresh);
  return grown == hipSuccess ? DMI_OK : growth_failed(ctx, grown);
}

// Preconditions of the tiled kernel (fusion_tile.hip header); otherwise the general kernel runs.
// The part that does not depend on the view; the per-view part is ViewRecords::tile_ok (view_records.h).
bool tile_eligible(const dmi_context *ctx) {
  if (ctx->opt.kernel_variant & dmi::VAR_FORCE_GENERAL) return false;
  if (!ctx->finite_bounded) return false;  // any grid matrix: axis-aligned or rotated (TileArgs::rotated)
  if (!(ctx->ray.thickness >= 0) || !(ctx->ray.delta >= 0)) return false;
  if ((int64_t)ctx->views.W * ctx->views.H * (int64_t)(ctx->views.depth_f64 ? 8 : 4) >= (int64_t(1) << 31)) return false;
  return true;
}

void drop_buffers(dmi_context *ctx, std::initializer_list<DeviceBuffer *> buffers) { free_buffers(buffers, ctx->device_bytes); }

int ensure_buffers(dmi_context *ctx, std::initializer_list<BufferNeed> needs) {
  for (const BufferNeed &need : needs) {
    const int rc = need.bytes ? ensure_buffer(ctx, *need.buffer, need.bytes) : DMI_OK;
    if (rc != DMI_OK) return rc;
  }
  return DMI_OK;
}

}  // namespace dmi

namespace {

// Host <-> device grid transfers in a type that is not the grid's: the conversion runs on the device, chunk by chunk
// through a 32 Mi-element staging buffer, so the host side is one hipMemcpyAsync per chunk (DMA speed when the caller's
// buffer is pinned, dmi_alloc_pinned) instead of a pageable full-size temporary and a scalar loop over every voxel.
constexpr int64_t kConvertChunk = int64_t(32) << 20;  // elements: 256 MiB as f64

int ensure_convert_stage(dmi_context *ctx) {
  return dmi::ensure_buffer(ctx, ctx->volume.convert, (uint64_t)std::min<int64_t>(kConvertChunk, ctx->n_voxels) * 8);
}

// host (HostT) -> device grid of the other type
template <typename HostT>
int upload_converted(dmi_context *ctx, const HostT *src) {
  int rc = ensure_convert_stage(ctx);
  if (rc != DMI_OK) return rc;
  const size_t gsz = grid_elem(ctx);
  for (int64_t i0 = 0; i0 < ctx->n_voxels; i0 += kConvertChunk) {
    const int64_t n = std::min<int64_t>(kConvertChunk, ctx->n_voxels - i0);
    DMI_HIP(ctx, hipMemcpyAsync(ctx->volume.convert.ptr, src + i0, (size_t)n * sizeof(HostT), hipMemcpyHostToDevice, ctx->stream));
    DMI_HIP(ctx, dmi::launch_convert_grid(ctx->volume.convert.ptr, sizeof(HostT) == 8 ? 1 : 0, static_cast<char *>(ctx->volume.d_grid) + (size_t)i0 * gsz, n,
                                          ctx->stream));
  }
  DMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return DMI_OK;
}

// device grid -> host (HostT) of the other type
template <typename HostT>
int download_converted(dmi_context *ctx, HostT *dst) {
  int rc = ensure_convert_stage(ctx);
  if (rc != DMI_OK) return rc;
  const size_t gsz = grid_elem(ctx);
  for (int64_t i0 = 0; i0 < ctx->n_voxels; i0 += kConvertChunk) {
    const int64_t n = std::min<int64_t>(kConvertChunk, ctx->n_voxels - i0);
    DMI_HIP(ctx, dmi::launch_convert_grid(static_cast<const char *>(ctx->volume.d_grid) + (size_t)i0 * gsz, gsz == 8 ? 1 : 0, ctx->volume.convert.ptr, n,
                                          ctx->stream));
    DMI_HIP(ctx, hipMemcpyAsync(dst + i0, ctx->volume.convert.ptr, (size_t)n * sizeof(HostT), hipMemcpyDeviceToHost, ctx->stream));
  }
  DMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return DMI_OK;
}

}  // namespace

extern "C" {

int dmi_abi_version(void) { return DMI_ABI_VERSION; }
size_t dmi_sizeof_info(void) { return sizeof(dmi_info); }
size_t dmi_sizeof_timings(void) { return sizeof(dmi_timings); }

int dmi_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

void dmi_default_options(dmi_options *opt) {
  if (!opt) return;
  std::memset(opt, 0, sizeof(*opt));
  opt->device = 0;
  opt->grid_dtype = DMI_F64;
  opt->depth_storage = DMI_DEPTH_AUTO;
}

const char *dmi_last_error(const dmi_context *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int dmi_create(const dmi_grid_desc *grid, const dmi_ray_potential *ray, const dmi_options *opt, dmi_context **out) {
  return guarded(nullptr, "dmi_create", [&]() -> int {
  auto bad = [](const char *m) {
    g_create_error = m;
    return (int)DMI_ERR_INVALID_ARGUMENT;
  };
  if (!grid || !ray || !out) return bad("dmi_create: null argument");
  *out = nullptr;
  for (int a = 0; a < 3; ++a)
    if (grid->cell_dims[a] < 1) return bad("dmi_create: cell_dims must be >= 1 (vtk point dims >= 2)");
  dmi_options o;
  dmi_default_options(&o);
  if (opt) o = *opt;
  if (o.grid_dtype != DMI_F32 && o.grid_dtype != DMI_F64) return bad("dmi_create: grid_dtype must be DMI_F32 or DMI_F64");
  if (o.depth_storage < DMI_DEPTH_AUTO || o.depth_storage > DMI_DEPTH_F64) return bad("dmi_create: bad depth_storage");
  if (o.z_first < 0 || (int64_t)o.z_first + grid->cell_dims[2] > (int64_t)0x3fffffff) return bad("dmi_create: z_first out of range");
  // the reference refuses only rho == 0 && thickness == 0 (filt.cxx:138-142); so do we
  if (ray->rho == 0 && ray->thickness == 0) return bad("dmi_create: ray potential rho and thickness are both 0 (filt.cxx:138)");
  if ((int64_t)(grid->cell_dims[1] + 3) / 4 > 65535 || (int64_t)grid->cell_dims[2] > 65535)
    return bad("dmi_create: grid too large for one launch (ny <= 262140, nz <= 65535)");
  int ndev = dmi_device_count();
  if (ndev <= 0) return (g_create_error = "dmi_create: no HIP device available", (int)DMI_ERR_DEVICE);
  if (o.device < 0 || o.device >= ndev) return bad("dmi_create: device ordinal out of range");

  dmi_context *ctx = new (std::nothrow) dmi_context();
  if (!ctx) return (g_create_error = "dmi_create: host allocation failed", (int)DMI_ERR_OUT_OF_MEMORY);
  ctx->grid = *grid;
  ctx->ray = *ray;
  ctx->opt = o;
  ctx->n_voxels = (int64_t)grid->cell_dims[0] * grid->cell_dims[1] * grid->cell_dims[2];
  ctx->finite_bounded = true;
  for (int i = 0; i < 12; ++i) ctx->finite_bounded = ctx->finite_bounded && bounded(grid->grid_matrix[i]);
  for (int a = 0; a < 3; ++a)
    ctx->finite_bounded = ctx->finite_bounded && bounded(grid->origin[a]) &&
                          bounded(grid->spacing[a] * (grid->cell_dims[a] + 1.0 + (a == 2 ? o.z_first : 0)));

  auto hip_fail = [&](hipError_t e, const char *what) {
    (void)hipGetLastError();
    g_create_error = std::string("dmi_create: ") + what + ": " + hipGetErrorString(e);
    int code = e == hipErrorOutOfMemory ? DMI_ERR_OUT_OF_MEMORY : DMI_ERR_DEVICE;
    dmi_destroy(ctx);
    return code;
  };
  hipError_t e = hipSetDevice(o.device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  if (o.stream) {
    ctx->stream = static_cast<hipStream_t>(o.stream);
  } else {
    e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) return hip_fail(e, "hipStreamCreate");
    ctx->own_stream = true;
  }
  {
    // The upload stream outranks the fusion's: its one short kernel per chunk then gets the compute-unit slots that the fusion of the
    // previous chunk frees, instead of queueing behind that fusion's waiting workgroups while the copy engine idles (round 4)
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) {
      (void)hipGetLastError();
      least = greatest = 0;
    }
    e = hipStreamCreateWithPriority(&ctx->upload_stream, hipStreamNonBlocking, greatest);
  }
  if (e != hipSuccess) return hip_fail(e, "hipStreamCreate(upload)");
  int rc = DMI_OK;
  auto own_failed = [&](int code) {  // a step that reports through the context: its message becomes dmi_last_error(nullptr)'s
    rc = code;
    if (rc != DMI_OK) g_create_error = "dmi_create: " + ctx->err;
  };
  if (o.external_grid) {
    hipPointerAttribute_t attr;
    e = hipPointerGetAttributes(&attr, o.external_grid);
    if (e != hipSuccess || attr.type != hipMemoryTypeDevice) {
      (void)hipGetLastError();
      g_create_error = "dmi_create: external_grid is not a device pointer";
      dmi_destroy(ctx);
      return DMI_ERR_INVALID_ARGUMENT;
    }
    ctx->volume.d_grid = o.external_grid;
  } else {
    own_failed(dmi::ensure_buffer(ctx, ctx->volume.owned, ctx->n_voxels * grid_elem(ctx)));
    ctx->volume.d_grid = ctx->volume.owned.ptr;
    ctx->volume.own_grid = true;
  }
  if (rc == DMI_OK && o.count_hits) own_failed(dmi::ensure_buffer(ctx, ctx->hits.voxel, ctx->n_voxels * sizeof(uint32_t)));
  if (rc == DMI_OK) own_failed(dmi::ensure_buffer(ctx, ctx->views.lossy, 3 * sizeof(unsigned long long)));
  if (rc == DMI_OK && (hipEventCreate(&ctx->views.up_events[0]) != hipSuccess || hipEventCreate(&ctx->views.up_events[1]) != hipSuccess)) {
    (void)hipGetLastError();  // (the upload pass is then not timed)
    dmi::destroy_events(ctx->views.up_events);
  }
  if (rc == DMI_OK) own_failed(dmi_reset_grid(ctx));
  if (rc != DMI_OK) {
    dmi_destroy(ctx);
    return rc;
  }
  *out = ctx;
  return DMI_OK;
  });
}

void dmi_destroy(dmi_context *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->opt.device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->upload_stream) {
    (void)hipStreamSynchronize(ctx->upload_stream);
    (void)hipStreamDestroy(ctx->upload_stream);
  }
  for (EventPair &p : ctx->pending) {
    (void)hipEventDestroy(p.start);
    (void)hipEventDestroy(p.stop);
    (void)hipEventDestroy(p.mid);
  }
  for (EventPair &p : ctx->pool) {
    (void)hipEventDestroy(p.start);
    (void)hipEventDestroy(p.stop);
    (void)hipEventDestroy(p.mid);
  }
  ctx->views.release();
  ctx->hits.release();
  ctx->volume.release();
  ctx->tables.release();
  ctx->c2p.release();
  ctx->point_smoothing.release();
  ctx->mesh.release();
  ctx->extraction.release();
  ctx->components.release();
  ctx->smoothing.release();
  ctx->decimation.release();
  ctx->holes.release();
  ctx->support.release();
  ctx->coloration.release();
  for (hipEvent_t e : ctx->slab_events) (void)hipEventDestroy(e);
  if (ctx->download_stream) (void)hipStreamDestroy(ctx->download_stream);
  if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

int dmi_reset_grid(dmi_context *ctx) {
  return guarded(ctx, "dmi_reset_grid", [&]() -> int {
  if (!ctx) return DMI_ERR_INVALID_ARGUMENT;
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  // The fusion kernel writes every voxel and skips the read when the grid is known to be zero, so
  // a context-owned grid is only memset if something reads it before the next fuse.
  if (ctx->volume.own_grid) {
    ctx->volume.zero_fill_pending = true;
  } else {
    DMI_HIP(ctx, hipMemsetAsync(ctx->volume.d_grid, 0, ctx->n_voxels * grid_elem(ctx), ctx->stream));
  }
  if (ctx->hits.voxel.ptr) DMI_HIP(ctx, hipMemsetAsync(ctx->hits.voxel.ptr, 0, ctx->n_voxels * sizeof(uint32_t), ctx->stream));
  if (ctx->hits.map.ptr)
    DMI_HIP(ctx, hipMemsetAsync(ctx->hits.map.ptr, 0, ctx->hits.map.capacity, ctx->stream));
  ctx->volume.layer_is_zero.assign((size_t)ctx->grid.cell_dims[2], 1);
  ctx->volume.grid_free_of_negative_zero = ctx->volume.own_grid;
  ctx->c2p.valid = false;
  return DMI_OK;
  });
}

int dmi_upload_grid(dmi_context *ctx, const double *grid) {
  return guarded(ctx, "dmi_upload_grid", [&]() -> int {
  if (!ctx || !grid) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_upload_grid: null argument");
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  ctx->volume.zero_fill_pending = false;
  if (ctx->opt.grid_dtype == DMI_F64) {
    DMI_HIP(ctx, hipMemcpyAsync(ctx->volume.d_grid, grid, ctx->n_voxels * 8, hipMemcpyHostToDevice, ctx->stream));
    DMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  } else {
    int rc_ = upload_converted<double>(ctx, grid);  // narrowed on the device
    if (rc_ != DMI_OK) return rc_;
  }
  ctx->volume.layer_is_zero.assign((size_t)ctx->grid.cell_dims[2], 0);
  ctx->volume.grid_free_of_negative_zero = false;
  ctx->c2p.valid = false;
  return DMI_OK;
  });
}

int dmi_synchronize(dmi_context *ctx) {
  return guarded(ctx, "dmi_synchronize", [&]() -> int {
  if (!ctx) return DMI_ERR_INVALID_ARGUMENT;
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  DMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return drain_events(ctx);
  });
}

int dmi_download_grid_f64(dmi_context *ctx, double *out) {
  return guarded(ctx, "dmi_download_grid_f64", [&]() -> int {
  if (!ctx || !out) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_download_grid_f64: null argument");
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  { int rc_ = flush_zero_fill(ctx); if (rc_ != DMI_OK) return rc_; }
  const auto t0 = std::chrono::steady_clock::now();
  if (ctx->opt.grid_dtype == DMI_F64) {
    // one bulk copy instead of the reference's per-tuple SetTuple1 loop (cu:256-264)
    DMI_HIP(ctx, hipMemcpyAsync(out, ctx->volume.d_grid, ctx->n_voxels * 8, hipMemcpyDeviceToHost, ctx->stream));
    DMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  } else {
    int rc_ = download_converted<double>(ctx, out);  // widened on the device (exact)
    if (rc_ != DMI_OK) return rc_;
  }
  ctx->timings.last_download_ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return drain_events(ctx);
  });
}

int dmi_download_grid_f32(dmi_context *ctx, float *out) {
  return guarded(ctx, "dmi_download_grid_f32", [&]() -> int {
  if (!ctx || !out) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_download_grid_f32: null argument");
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  { int rc_ = flush_zero_fill(ctx); if (rc_ != DMI_OK) return rc_; }
  const auto t0 = std::chrono::steady_clock::now();
  if (ctx->opt.grid_dtype == DMI_F32) {
    DMI_HIP(ctx, hipMemcpyAsync(out, ctx->volume.d_grid, ctx->n_voxels * 4, hipMemcpyDeviceToHost, ctx->stream));
    DMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  } else {
    int rc_ = download_converted<float>(ctx, out);  // narrowed on the device (round to nearest, as the host cast)
    if (rc_ != DMI_OK) return rc_;
  }
  ctx->timings.last_download_ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return drain_events(ctx);
  });
}

// The last step of a chunked reconstruction (cu:343-371: the last map's kernel, then the copy back): views [first, first +
// count) are fused slab by slab and every slab starts its way to the host the moment its fusion ends, on a stream of its
// own, while the next slabs are being fused.  Slabs fused one after the other give the bits of one fusion (dmi_fuse_slab).
int dmi_fuse_range_download(dmi_context *ctx, int32_t first, int32_t count, void *out, int32_t out_dtype, int32_t n_slabs) {
  return guarded(ctx, "dmi_fuse_range_download", [&]() -> int {
  if (!ctx || !out) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_fuse_range_download: null argument");
  if (out_dtype != DMI_F64 && out_dtype != DMI_F32) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_fuse_range_download: out_dtype must be DMI_F32 or DMI_F64");
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  // the range is checked once, here, for both paths below; count == 0 is a plain download (no view need be resident)
  const int32_t n_views = (int32_t)ctx->views.h_maps.size();
  if (first < 0 || count < 0 || first > n_views || count > n_views - first)
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_fuse_range_download: range outside the resident views");
  const int32_t nz = ctx->grid.cell_dims[2];
  const int32_t max_slabs = std::max(1, (nz + DMI_SLAB_ALIGNMENT - 1) / DMI_SLAB_ALIGNMENT);
  n_slabs = std::min(std::max(n_slabs, 1), max_slabs);
  if (out_dtype != ctx->opt.grid_dtype || n_slabs == 1) {
    // another type than the grid's: converted on the device after the whole fusion (dmi_download_grid_*), nothing overlaps
    if (count > 0) {
      int rc = fuse_views(ctx, first, count, 0, nz);
      if (rc != DMI_OK) return rc;
    }
    return out_dtype == DMI_F64 ? dmi_download_grid_f64(ctx, static_cast<double *>(out)) : dmi_download_grid_f32(ctx, static_cast<float *>(out));
  }
  { int rc_ = flush_zero_fill(ctx); if (rc_ != DMI_OK) return rc_; }
  if (!ctx->download_stream) DMI_HIP(ctx, hipStreamCreateWithFlags(&ctx->download_stream, hipStreamNonBlocking));
  while ((int32_t)ctx->slab_events.size() < n_slabs) {
    hipEvent_t e = nullptr;
    DMI_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ctx->slab_events.push_back(e);
  }
  const auto t0 = std::chrono::steady_clock::now();
  // slabs of whole alignment units, as equal as they come
  const int32_t units = max_slabs, per = units / n_slabs, extra = units % n_slabs;
  const size_t gsz = grid_elem(ctx);
  const size_t layer = (size_t)ctx->grid.cell_dims[0] * ctx->grid.cell_dims[1];
  int32_t z0 = 0;
  for (int32_t i = 0; i < n_slabs; ++i) {
    const int32_t z1 = std::min(nz, z0 + (per + (i < extra ? 1 : 0)) * DMI_SLAB_ALIGNMENT);
    if (count > 0) {
      int rc = fuse_views(ctx, first, count, z0, z1 - z0);
      if (rc != DMI_OK) {
        (void)hipStreamSynchronize(ctx->download_stream);  // the copies already queued end before the caller sees the error
        return rc;
      }
    }
    // (a failure past the first queued copy: the copies in flight end before the caller sees the error, as above)
    hipError_t he = hipEventRecord(ctx->slab_events[(size_t)i], ctx->stream);
    if (he == hipSuccess) he = hipStreamWaitEvent(ctx->download_stream, ctx->slab_events[(size_t)i], 0);
    if (he == hipSuccess)
      he = hipMemcpyAsync(static_cast<char *>(out) + (size_t)z0 * layer * gsz, static_cast<const char *>(ctx->volume.d_grid) + (size_t)z0 * layer * gsz,
                          (size_t)(z1 - z0) * layer * gsz, hipMemcpyDeviceToHost, ctx->download_stream);
    if (he != hipSuccess) {
      (void)hipStreamSynchronize(ctx->download_stream);
      (void)hipGetLastError();
      return fail(ctx, DMI_ERR_DEVICE, std::string("dmi_fuse_range_download: ") + hipGetErrorString(he));
    }
    z0 = z1;
  }
  DMI_HIP(ctx, hipStreamSynchronize(ctx->download_stream));
  DMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  // (this call's wall time: the slabs' fusions AND their copies, which overlap -- include/dmi.h says so)
  ctx->timings.last_download_ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return drain_events(ctx);
  });
}

int dmi_download_hits(dmi_context *ctx, uint32_t *voxel_hits, uint64_t *map_hits) {
  return guarded(ctx, "dmi_download_hits", [&]() -> int {
  if (!ctx) return DMI_ERR_INVALID_ARGUMENT;
  if (!ctx->opt.count_hits) return fail(ctx, DMI_ERR_STATE, "dmi_download_hits: context created without count_hits");
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  if (voxel_hits)
    DMI_HIP(ctx, hipMemcpyAsync(voxel_hits, ctx->hits.voxel.ptr, ctx->n_voxels * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                ctx->stream));
  if (map_hits) {
    // the counters grow at the next fusion (sync_maps): views added since the last one may lie beyond them and have no hit yet,
    // while the views before keep what they have gathered
    const size_t n = ctx->views.h_maps.size();
    const size_t counted = ctx->hits.map.ptr ? std::min<size_t>(n, (size_t)(ctx->hits.map.capacity / sizeof(uint64_t))) : 0;
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "u64");
    if (counted > 0)
      DMI_HIP(ctx, hipMemcpyAsync(map_hits, ctx->hits.map.ptr, counted * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    for (size_t i = counted; i < n; ++i) map_hits[i] = 0;
  }
  DMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return drain_events(ctx);
  });
}

int dmi_grid_device_pointer(dmi_context *ctx, void **ptr) {
  return guarded(ctx, "dmi_grid_device_pointer", [&]() -> int {
  if (!ctx || !ptr) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_grid_device_pointer: null argument");
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  int rc = flush_zero_fill(ctx);
  if (rc != DMI_OK) return rc;
  *ptr = ctx->volume.d_grid;
  // whoever holds the pointer may write anything, a -0.0 included: later fusions keep the +0.0 adds of the pairs far behind
  // every surface until the next dmi_reset_grid
  ctx->volume.grid_free_of_negative_zero = false;
  return DMI_OK;
  });
}

extern "C++" {
namespace dmi {
// dmi_multi's exchanges write SUMS of grids that hold no -0.0 into a context-owned grid ((+0) + (+0) = +0, and x + y = -0.0
// only when both are): the invariant of 4b.6 survives them, so they take the pointer without giving it up.
int grid_pointer_for_sums(dmi_context *ctx, void **ptr) {
  return guarded(ctx, "grid_pointer_for_sums", [&]() -> int {
  if (!ctx || !ptr) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "grid_pointer_for_sums: null argument");
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  int rc = flush_zero_fill(ctx);
  if (rc != DMI_OK) return rc;
  *ptr = ctx->volume.d_grid;
  return DMI_OK;
  });
}
}  // namespace dmi
}  // extern "C++"

int dmi_get_timings(dmi_context *ctx, dmi_timings *out) {
  return guarded(ctx, "dmi_get_timings", [&]() -> int {
  if (!ctx || !out) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_get_timings: null argument");
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  int rc = drain_events(ctx);
  if (rc != DMI_OK) return rc;
  rc = drain_c2p(ctx);
  if (rc != DMI_OK) return rc;
  *out = ctx->timings;
  return DMI_OK;
  });
}

int dmi_get_info(dmi_context *ctx, dmi_info *out) {
  return guarded(ctx, "dmi_get_info", [&]() -> int {
  if (!ctx || !out) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_get_info: null argument");
  std::memset(out, 0, sizeof(*out));
  out->n_voxels = ctx->n_voxels;
  out->n_views = (int32_t)ctx->views.h_maps.size();
  out->depth_width = ctx->views.W;
  out->depth_height = ctx->views.H;
  out->depth_storage_in_use = ctx->views.depth_f64 ? DMI_DEPTH_F64 : DMI_DEPTH_F32;
  out->grid_dtype = ctx->opt.grid_dtype;
  out->k_mode = (ctx->opt.kernel_variant & 2) ? 0 : ctx->views.k_mode;
  out->kernel_variant = ctx->opt.kernel_variant;
  // 1: every resident view takes the register-tiled kernel; 0: at least one run goes through the general kernel
  bool all_tiled = !ctx->views.h_maps.empty() && tile_eligible(ctx);
  for (uint8_t ok : ctx->views.view_tile_ok) all_tiled = all_tiled && ok;
  out->tiled_kernel = all_tiled ? 1 : 0;
  out->device_bytes = ctx->device_bytes;
  for (const Batch &bt : ctx->views.batches) out->pixels_without_depth += bt.holes;
  return DMI_OK;
  });
}

int dmi_alloc_pinned(size_t bytes, void **out) {
  return guarded(nullptr, "dmi_alloc_pinned", [&]() -> int {
  if (!out || bytes == 0) return DMI_ERR_INVALID_ARGUMENT;
  hipError_t e = hipHostMalloc(out, bytes, hipHostMallocDefault);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    g_create_error = std::string("dmi_alloc_pinned: ") + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? DMI_ERR_OUT_OF_MEMORY : DMI_ERR_DEVICE;
  }
  return DMI_OK;
  });
}

int dmi_pcie_probe(int32_t device, size_t bytes, double *h2d_GBps, double *d2h_GBps) {
  return guarded(nullptr, "dmi_pcie_probe", [&]() -> int {
    if (bytes < (size_t(1) << 20) || (!h2d_GBps && !d2h_GBps))
      return fail(nullptr, DMI_ERR_INVALID_ARGUMENT, "dmi_pcie_probe: at least 1 MiB and one output");
    dmi_context *none = nullptr;
    DMI_HIP(none, hipSetDevice(device));
    void *host = nullptr, *dev = nullptr;
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipHostMalloc(&host, bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(&dev, bytes);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    double rate[2] = {0.0, 0.0};
    if (e == hipSuccess) std::memset(host, 0, bytes);  // touch the pages
    for (int dir = 0; e == hipSuccess && dir < 2; ++dir) {
      for (int rep = 0; e == hipSuccess && rep < 3; ++rep) {  // the first pass warms up; the best of the others counts
        e = hipEventRecord(e0, s);
        if (e == hipSuccess)
          e = dir == 0 ? hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, s) : hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipEventRecord(e1, s);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        float ms = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e == hipSuccess && rep > 0 && ms > 0.f) rate[dir] = std::max(rate[dir], (double)bytes / (ms * 1e-3) / 1e9);
      }
    }
    if (e1) (void)hipEventDestroy(e1);
    if (e0) (void)hipEventDestroy(e0);
    if (s) (void)hipStreamDestroy(s);
    if (dev) (void)hipFree(dev);
    if (host) (void)hipHostFree(host);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(nullptr, DMI_ERR_DEVICE, std::string("dmi_pcie_probe: ") + hipGetErrorString(e));
    }
    if (h2d_GBps) *h2d_GBps = rate[0];
    if (d2h_GBps) *d2h_GBps = rate[1];
    return DMI_OK;
  });
}

#ifdef DMI_TUNING
// tuning builds only (not part of the ABI): the TileArgs::wg_times record of the last tiled fuse, 3 * blocks values
extern "C" int dmi_debug_wg_times(dmi_context *ctx, unsigned long long *out, int64_t capacity, int64_t *blocks) {
  if (!ctx || !blocks) return DMI_ERR_INVALID_ARGUMENT;
  *blocks = (int64_t)ctx->tables.wg_times_blocks;
  if (!ctx->tables.wg_times.ptr || !out || capacity < 3 * (int64_t)ctx->tables.wg_times_blocks) return DMI_OK;
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return DMI_ERR_DEVICE;
  if (hipMemcpy(out, ctx->tables.wg_times.ptr, ctx->tables.wg_times_blocks * 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess)
    return DMI_ERR_DEVICE;
  return DMI_OK;
}
// ... and the two counters behind it: out[0] = window pairs executed (per wave), out[1] = wave-voxels redone after a window column
extern "C" int dmi_debug_window_counts(dmi_context *ctx, unsigned long long *out) {
  if (!ctx || !out) return DMI_ERR_INVALID_ARGUMENT;
  out[0] = out[1] = 0;
  if (!ctx->tables.wg_times.ptr) return DMI_OK;
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return DMI_ERR_DEVICE;
  if (hipMemcpy(out, ctx->tables.wg_times.as<unsigned long long>() + 3 * ctx->tables.wg_times_blocks, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess)
    return DMI_ERR_DEVICE;
  return DMI_OK;
}
#endif

int dmi_fp64_probe(int32_t device, double milliseconds, double *tflops) {
  return guarded(nullptr, "dmi_fp64_probe", [&]() -> int {
    if (!tflops || !(milliseconds > 0.0) || milliseconds > 1000.0)
      return fail(nullptr, DMI_ERR_INVALID_ARGUMENT, "dmi_fp64_probe: an output and 0 < milliseconds <= 1000");
    dmi_context *none = nullptr;
    DMI_HIP(none, hipSetDevice(device));
    hipDeviceProp_t prop;
    DMI_HIP(none, hipGetDeviceProperties(&prop, device));
    const int blocks = std::max(1, prop.multiProcessorCount) * 8;  // eight workgroups of four waves per CU
    double *out = nullptr;
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipMalloc(&out, (size_t)blocks * 256 * sizeof(double));
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    double best = 0.0;
    int iters = 4096;  // the first pass sizes the others
    for (int rep = 0; e == hipSuccess && rep < 4; ++rep) {
      e = hipEventRecord(e0, s);
      if (e == hipSuccess) e = dmi::launch_fp64_probe(out, blocks, iters, s);
      if (e == hipSuccess) e = hipEventRecord(e1, s);
      if (e == hipSuccess) e = hipEventSynchronize(e1);
      float ms = 0.f;
      if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
      if (e != hipSuccess || !(ms > 0.f)) break;
      const double flops = 2.0 * 8.0 * (double)iters * (double)blocks * 256.0;
      if (rep > 0) best = std::max(best, flops / (ms * 1e-3) / 1e12);
      if (rep == 0) iters = (int)std::min(4.0e6, std::max(1024.0, iters * milliseconds / ms));
    }
    if (e1) (void)hipEventDestroy(e1);
    if (e0) (void)hipEventDestroy(e0);
    if (s) (void)hipStreamDestroy(s);
    if (out) (void)hipFree(out);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(nullptr, DMI_ERR_DEVICE, std::string("dmi_fp64_probe: ") + hipGetErrorString(e));
    }
    *tflops = best;
    return DMI_OK;
  });
}

int dmi_free_pinned(void *ptr) {
  return guarded(nullptr, "dmi_free_pinned", [&]() -> int {
  if (!ptr) return DMI_OK;
  hipError_t e = hipHostFree(ptr);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return DMI_ERR_DEVICE;
  }
  return DMI_OK;
  });
}

}  // extern "C"
