// dmi_capi.hip -- implementation of the C ABI declared in include/dmi.h.
//
// Creation, destruction, views, grid transfer, info, timings and the hardware probes; the fusion launch and the diagnostics that
// read it are in dmi_capi_fuse.hip, the point data and the mesh entry points in dmi_capi_mesh.hip, the context all three work on
// in dmi_context.h.  No buffer of the context is allocated, freed or counted here but through that header's growth helpers (defined
// below) -- the depth batches excepted, whose upload is all or nothing.
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
using dmi::drain_c2p;
using dmi::drain_events;
using dmi::EventPair;
using dmi::fail;
using dmi::flush_zero_fill;
using dmi::fuse_views;
using dmi::grid_axis_aligned;
using dmi::tile_eligible;
using dmi::FuseArgs;
using dmi::FuseConfig;
using dmi::guarded;
using dmi::MapRec;
using dmi::TileArgs;
using dmi::TileMapRec;

namespace {

thread_local std::string g_create_error;

constexpr double kMagnitudeLimit = 1e60;  // see DESIGN.md "K specialisation": keeps every product finite

using dmi::grid_elem;
size_t depth_elem(const dmi_context *c) { return c->views.depth_f64 ? 8 : 4; }

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

bool grid_axis_aligned(const dmi_grid_desc &g) {
  const double *m = g.grid_matrix;
  return m[1] == 0 && m[2] == 0 && m[4] == 0 && m[6] == 0 && m[8] == 0 && m[9] == 0;
}

// Preconditions of the tiled kernel (fusion_tile.hip header); otherwise the general kernel runs.
// The part that does not depend on the view; the per-view part is view_tile_ok (add_views_impl).
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

bool bounded(double v) { return std::isfinite(v) && std::fabs(v) <= kMagnitudeLimit; }

int classify_k(const double *K, const double *RT) {
  for (int i = 0; i < 12; ++i)
    if (!bounded(K[i]) || !bounded(RT[i])) return dmi::K_GENERAL;
  const bool pinhole = K[3] == 0 && K[7] == 0 && K[11] == 0 && K[4] == 0 && K[8] == 0 && K[9] == 0 && K[10] == 1;
  if (!pinhole) return dmi::K_GENERAL;
  return K[1] == 0 ? dmi::K_PINHOLE : dmi::K_PINHOLE_SKEW;
}

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
int upload_batch(dmi_context *ctx, const double *depth64, const float *depth32, const double *best_cost,
                 double threshold, int32_t n, Batch *out, unsigned long long *lossy_out) {
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
  rc = ensure_stage(ctx, chunk * npix, best_cost != nullptr);
  if (rc == DMI_OK) {
    hipError_t e = hipMemsetAsync(ctx->views.lossy.as<unsigned long long>(), 0, 3 * sizeof(unsigned long long), ctx->upload_stream);  // [1], [2]: launch_build_valid_maps' counts
    for (size_t m0 = 0; e == hipSuccess && m0 < (size_t)n; m0 += chunk) {
      const size_t cnt = std::min(chunk, (size_t)n - m0);
      const char *src = depth32 ? reinterpret_cast<const char *>(depth32) : reinterpret_cast<const char *>(depth64);
      e = hipMemcpyAsync(ctx->views.stage_depth.as<double>(), src + m0 * npix * in_elem, cnt * npix * in_elem, hipMemcpyHostToDevice,
                         ctx->upload_stream);
      if (e == hipSuccess && best_cost)
        e = hipMemcpyAsync(ctx->views.stage_cost.as<double>(), best_cost + m0 * npix, cnt * npix * 8, hipMemcpyHostToDevice, ctx->upload_stream);
      void *dst = static_cast<char *>(b.d_depth) + m0 * npix * esz;
      // one pass over the staged tables: threshold, row flip, narrowing, the finest pyramid level, validity bytes and bits
      const bool timed = m0 + cnt >= (size_t)n && ctx->views.up_events[0] && ctx->views.up_events[1];  // (the last chunk of the call: with it, the pyramid levels)
      if (e == hipSuccess && timed) e = hipEventRecord(ctx->views.up_events[0], ctx->upload_stream);
      if (e == hipSuccess)
        e = dmi::launch_upload_views(ctx->views.stage_depth.as<double>(), depth32 ? 0 : 1, (!depth32 && best_cost) ? ctx->views.stage_cost.as<double>() : nullptr, threshold,
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

// ---- tiled kernel support (fusion_tile.hip) --------------------------------------------------------

constexpr int kMaxColumn = 32;  // tallest voxel column of any tile shape (error bound below uses it)

// rows 0..2 of the grid matrix applied to the centre of voxel (i, j, k): cu:78-83 + cu:168
void voxel_world(const dmi_grid_desc &g, int i, int j, int k, double w[3]) {
  const double p[3] = {g.origin[0] + (i + 0.5) * g.spacing[0], g.origin[1] + (j + 0.5) * g.spacing[1],
                       g.origin[2] + (k + 0.5) * g.spacing[2]};
  for (int r = 0; r < 3; ++r)
    w[r] = ((g.grid_matrix[4 * r] * p[0] + g.grid_matrix[4 * r + 1] * p[1]) + g.grid_matrix[4 * r + 2] * p[2]) +
           g.grid_matrix[4 * r + 3];
}

// Smallest float >= x (x >= 0, finite): the tier-1 margins are rounded up.
float float_not_below(double x) {
  float f = (float)x;
  if ((double)f < x) f = std::nextafterf(f, std::numeric_limits<float>::infinity());
  return f;
}

// The pixel selection of a pinhole view on an axis-aligned grid works in coordinates measured from the image centre
// (TileMapRec::cpx ...), in two tiers (fusion_tile.hip).  P, Q, S: rows 0..2 of K*[R|T]; Sx, Sy: magnitudes of
// the terms of h.x, h.y over the grid; M[2]: of c.z.
void make_centred_rows(const dmi_context *ctx, const MapRec &r, const double P[4], const double Q[4], const double S[4],
                       double Sx, double Sy, const double M[3], double zabs, double zscale, bool general, bool aligned, TileMapRec *out,
                       dmi::WinRec *win, dmi::FootRec *foot) {
  TileMapRec &t = *out;
  std::memset(foot, 0, sizeof(*foot));
  std::memset(win, 0, sizeof(*win));
  win->e_abs = std::numeric_limits<float>::infinity();  // no windows unless everything below holds
  win->c1 = dmi::kWinC1;
  t.t1_ok = 0;
  t.t1_e1 = std::numeric_limits<float>::infinity();
  t.t1_c1 = 0.5f - 0x1p-20f;
  const double cxc = (double)(ctx->views.W / 2), cyc = (double)(ctx->views.H / 2);
  t.t1_cidx = (int32_t)((int64_t)ctx->views.W * (ctx->views.H / 2) + ctx->views.W / 2);
  if (general) return;  // those launches (GENK instantiations) read px .. q0 and errk
  double Pc[4], Qc[4];
  for (int c = 0; c < 4; ++c) {
    Pc[c] = P[c] - cxc * S[c];
    Qc[c] = Q[c] - cyc * S[c];
  }
  t.cpx = Pc[0]; t.cpy = Pc[1]; t.cpz = Pc[2]; t.cp0 = Pc[3];
  t.cqx = Qc[0]; t.cqy = Qc[1]; t.cqz = Qc[2]; t.cq0 = Qc[3];
  const double *g = ctx->grid.grid_matrix;
  const double sz = ctx->grid.spacing[2];
  t.cdhx = (Pc[0] * (g[2] * sz) + Pc[1] * (g[6] * sz)) + Pc[2] * (g[10] * sz);
  t.cdhy = (Qc[0] * (g[2] * sz) + Qc[1] * (g[6] * sz)) + Qc[2] * (g[10] * sz);
  // |hx''_ref - hx''_kernel|: the reference's h.x carries <= 11 ulp(Sx), cxc times its c.z <= 6 ulp(cxc * M[2]); the kernel's
  // affine value the 73 ulp of DESIGN.md 4.2 on the centred magnitudes (+ 2 per coefficient for the subtraction above);
  // 512 ulp of Sx + cxc * M[2] covers the sum five times over
  // Rotated grid: M and Sx are sums of magnitudes that also bound every intermediate of the reference's w (three products and
  // three sums per component instead of one of each); its w at two voxels of a column differs from the real, affine one by
  // <= 6 ulp(|w|) each, which the rows turn into <= 12 ulp of the magnitudes: twice the budget keeps the same margin.
  const double rot = aligned ? 1.0 : 2.0;
  const double Sxc = Sx + cxc * M[2], Syc = Sy + cyc * M[2];
  const double cerr = rot * std::max(Sxc, Syc) * 0x1p-44;
  t.cerrk = cerr + 0x1p-22 * zabs * (1.0 + 0x1p-20);  // (zabs >= |c.z| over the grid: make_tile_rec)
  t.t1_dhx = (float)t.cdhx;
  t.t1_dhy = (float)t.cdhy;
  const double dcz = t.dhz;  // pinhole: row 2 of [R|T] times the step of the world position per voxel along k
  t.t1_dcz = (float)dcz;
  t.t1_dthr = (float)(dcz * (double)t.t1_c1);
  if (!(cerr < 0x1p-12 * zscale)) return;  // (such a view fails the tiled kernel's per-view test anyway)
  // c.z over the voxels of the grid: at least czmin (the real-valued minimum over the box of voxel centres, less the
  // rounding of the computed value)
  // (affine in the voxel indices: the extremes are at the eight corner voxels of the grid, whatever its axes)
  double czmin = std::numeric_limits<double>::infinity(), Scx = 0.0, Scy = 0.0;
  for (int c = 0; c < 8; ++c) {
    double w[3];
    voxel_world(ctx->grid, (c & 1) ? ctx->grid.cell_dims[0] - 1 : 0, (c & 2) ? ctx->grid.cell_dims[1] - 1 : 0,
                ctx->opt.z_first + ((c & 4) ? ctx->grid.cell_dims[2] - 1 : 0), w);
    czmin = std::min(czmin, ((r.rt[8] * w[0] + r.rt[9] * w[1]) + r.rt[10] * w[2]) + r.rt[11]);
    // |hx''|, |hy''| over the grid, from the centred rows themselves (for a principal point at the image centre the cz terms
    // of row 0 cancel: this is what keeps |u''| <= W / 2 instead of W)
    Scx = std::max(Scx, std::fabs(((Pc[0] * w[0] + Pc[1] * w[1]) + Pc[2] * w[2]) + Pc[3]));
    Scy = std::max(Scy, std::fabs(((Qc[0] * w[0] + Qc[1] * w[1]) + Qc[2] * w[2]) + Qc[3]));
  }
  czmin -= rot * 16.0 * 0x1p-52 * M[2];
  const double Sc = (std::max(Scx, Scy) + cerr) * (1.0 + 0x1p-20);               // bounds |hx''|, |hy''| and their fp32 images
  const double D = kMaxColumn * std::max(std::fabs(t.cdhx), std::fabs(t.cdhy));  // their change over a column
  const double Dz = kMaxColumn * std::fabs(dcz);
  const double nl = rot * 32.0 * 0x1p-53 * M[2];  // computed c.z against its affine model along a column (roundings of cu:80-92)
  if (!std::isfinite(czmin)) return;
  // The camera inside (or too near) the grid: no bound of |P| holds for the whole view; the kernel forms one per lane from its
  // column's own c.z (t1_ok = 2).  pmax enters e1 linearly: e1 = (A + B pmax)(1 + 2^-10).
  const bool per_lane = !(czmin > 0.0) || !(Sc / czmin + 1.0 < 0x1p22);
  const double pmax = per_lane ? 0.0 : Sc / czmin + 1.0;  // bounds every accepted tier-1 candidate |P|
  // W*py'' + px'' and the validity map's byte index yt*(8W - 8) + (8 px'' + py'') (|.| <= H*W + 4W + H/2) exact in fp32
  // (of the padded image: every pixel the FREE column may ask for lies within the margin, 4b.9)
  const bool index_exact = ((int64_t)ctx->views.H + 2 * dmi::kValidMargin + 8) * ((int64_t)ctx->views.W + 2 * dmi::kValidMargin) + ctx->views.H +
                               2 * dmi::kValidMargin < (int64_t(1) << 24);
  // e1 = e_abs + e_rel * HB, HB = the lane's bound on |hx''|, |hy''| along its column
  double e1 = cerr + 3.0 * 0x1p-24 * Dz * pmax + 0x1p-22 * Dz + nl * (pmax + 2.0) + 0x1p-53 * std::max(Sx, Sy);
  e1 *= 1.0 + 0x1p-10;
  t.t1_erel = 0x1p-22f * (1.0f + 0x1p-10f);
  t.t1_hspan = float_not_below(D * (1.0 + 0x1p-20));
  if (!(pmax < 0x1p22) || !index_exact || !(e1 > 0x1p-100) || !(Sc < 0x1p60) || !std::isfinite(e1)) return;
  t.t1_e1 = float_not_below(e1);  // (per_lane: the part of e1 that does not depend on pmax)
  t.t1_ok = 1;
  {
    // The window form of the FREE column (WinRec, fusion_kernels.h).  Steps of the centred numerators and of c.z
    // per voxel along i, j, k: the rows times the grid matrix's columns times the spacings (as cdhx above for k).
    const double *sp = ctx->grid.spacing;
    double d[3][2], c[3];
    for (int ax = 0; ax < 3; ++ax) {
      const double wxs = g[ax] * sp[ax], wys = g[4 + ax] * sp[ax], wzs = g[8 + ax] * sp[ax];
      d[ax][0] = (Pc[0] * wxs + Pc[1] * wys) + Pc[2] * wzs;
      d[ax][1] = (Qc[0] * wxs + Qc[1] * wys) + Qc[2] * wzs;
      c[ax] = (S[0] * wxs + S[1] * wys) + S[2] * wzs;
    }
    // |hw_ref - model| <= cerr + Xmax * nl2: the centred numerator within cerr of the affine model anchored at the brick's first
    // voxel (the budget of 4d.1 covers the anchor's FMA chain and seven steps each way: < 100 of its 512 ulp), the reference's
    // c.z within nl2 of ITS model (two computed values, 8 ulp(M[2]) each, rotated grids twice that), times the window's anchor
    // pixel Xc: its first pixel (|.| <= xpix) plus (kWinAnchorX, kWinAnchorY)
    const double xpix = (double)(std::max(ctx->views.W, ctx->views.H) / 2 + dmi::kValidMargin + 1);
    const double xmax = xpix + (double)std::max(dmi::kWinAnchorX, dmi::kWinAnchorY);
    const double nl2 = 2.0 * nl;
    const double pwin = (dmi::kWinReach + 0.5) * dmi::kWinCzRatio + 3.0;  // bounds an accepted candidate: |P| < |h| / z + 1/2
    // the steps as the kernel forms them, fl32(d32 - Xc * c32): each within 2^-23 (|d| + |Xc c|) of the real one; a lane takes up
    // to 7 along i and j and kMaxColumn - 1 along k
    const double steps[3] = {7.0, 7.0, (double)(kMaxColumn - 1)};
    double e_step = 0.0;
    for (int xy = 0; xy < 2; ++xy) {
      double e = 0.0;
      for (int ax = 0; ax < 3; ++ax) e += steps[ax] * (std::fabs(d[ax][xy]) + xmax * std::fabs(c[ax]));
      e_step = std::max(e_step, e * 0x1p-23);
    }
    double ew = (cerr + xmax * nl2) + e_step + pwin * nl2 + 0x1p-53 * std::max(Sx, Sy);
    ew *= 1.0 + 0x1p-10;
    bool ok = std::isfinite(ew) && ew > 0x1p-100 && ew < 0x1p60;
    for (int ax = 0; ax < 3; ++ax) ok = ok && std::fabs(d[ax][0]) < 0x1p60 && std::fabs(d[ax][1]) < 0x1p60 && std::fabs(c[ax]) < 0x1p60;
    if (ok) {
      for (int xy = 0; xy < 2; ++xy) {
        win->di[xy] = (float)d[0][xy];
        win->dj[xy] = (float)d[1][xy];
        win->dk[xy] = (float)d[2][xy];
      }
      win->ci[0] = (float)c[0]; win->ci[1] = (float)(c[0] * (double)dmi::kWinC1);
      win->cj[0] = (float)c[1]; win->cj[1] = (float)(c[1] * (double)dmi::kWinC1);
      win->ck[0] = (float)c[2]; win->ck[1] = (float)(c[2] * (double)dmi::kWinC1);
      win->e_abs = float_not_below(ew);
      // the brick's corner voxels relative to its first one (FootRec), for 8- and 16-voxel columns
      for (int cnr = 0; cnr < 8; ++cnr) {
        const double ni = (cnr & 1) ? 7.0 : 0.0, nj = (cnr & 2) ? 7.0 : 0.0;
        for (int v = 0; v < 2; ++v) {
          const double nk = (cnr & 4) ? (v ? 15.0 : 7.0) : 0.0;
          float *dst = v ? foot->s16[cnr] : foot->s8[cnr];
          dst[0] = (float)((ni * d[0][0] + nj * d[1][0]) + nk * d[2][0]);
          dst[1] = (float)((ni * d[0][1] + nj * d[1][1]) + nk * d[2][1]);
          dst[2] = (float)((ni * c[0] + nj * c[1]) + nk * c[2]);
        }
      }
      foot->ferr = float_not_below(cerr + xpix * nl2);  // (times a pixel's |u''|, not an anchor's)
    }
  }
  if (per_lane) {
    // the coefficient of pmax, rounded up, with one more factor (1 + 2^-10) for the roundings of the lane's own p
    const double B = (3.0 * 0x1p-24 * Dz + nl) * (1.0 + 0x1p-10) * (1.0 + 0x1p-10);
    if (!(B < 0x1p60) || !(B >= 0.0)) {
      t.t1_ok = 0;
      t.t1_e1 = std::numeric_limits<float>::infinity();
      return;
    }
    t.t1_b = float_not_below(B);
    t.t1_ok = 2;
  }
}

// Per-map record of the tiled kernel: row 2 of RT for the exact c.z, rows 0 and 1 of K*[R|T] for the
// pixel selection, and `err`, a bound on the absolute difference between the reference's computed
// h.x / h.y and the kernel's affine evaluation anywhere in the grid (DESIGN.md "Tiled kernel: proof
// obligations" derives the 73-ulp budget this bound covers seven times over).
TileMapRec make_tile_rec(const dmi_context *ctx, const MapRec &r, dmi::WinRec *win, dmi::FootRec *foot, double *zscale_out) {
  TileMapRec t;
  std::memset(&t, 0, sizeof(t));
  const double *rt = r.rt, *k = r.k;
  t.rz0 = rt[8];
  t.rz1 = rt[9];
  t.rz3 = rt[11];
  // rows of K * [R|T]: h.x, h.y (and, for a K whose third row is not 0 0 1 0, h.z) as affine functions of the world
  // position.  A pinhole K keeps the shorter sums it always had (the dropped terms are exact zeros).
  const bool general = classify_k(r.k, r.rt) == dmi::K_GENERAL;
  double P[4], Q[4], S[4];
  for (int c = 0; c < 4; ++c) {
    if (general) {
      P[c] = (k[0] * rt[c] + k[1] * rt[4 + c]) + k[2] * rt[8 + c];
      Q[c] = (k[4] * rt[c] + k[5] * rt[4 + c]) + k[6] * rt[8 + c];
      S[c] = (k[8] * rt[c] + k[9] * rt[4 + c]) + k[10] * rt[8 + c];
    } else {
      P[c] = k[0] * rt[c] + k[1] * rt[4 + c] + k[2] * rt[8 + c];  // row 0 of K (fx s cx0 0) times [R|T]
      Q[c] = k[5] * rt[4 + c] + k[6] * rt[8 + c];                 // row 1 of K (0 fy cy0 0)
      S[c] = rt[8 + c];                                           // row 2 of K (0 0 1 0): h.z == c.z
    }
  }
  if (general) {  // the fourth column of K multiplies the homogeneous 1 (cu:90-92)
    P[3] += k[3];
    Q[3] += k[7];
    S[3] += k[11];
  }
  t.px = P[0]; t.py = P[1]; t.pz = P[2]; t.p0 = P[3];
  t.qx = Q[0]; t.qy = Q[1]; t.qz = Q[2]; t.q0 = Q[3];
  t.sx = S[0]; t.sy = S[1]; t.sz = S[2]; t.s0 = S[3];
  // step of the world position per voxel along k: column 2 of the grid matrix times the spacing (for an axis-aligned
  // grid only its z component is non-zero)
  const double *g = ctx->grid.grid_matrix;
  const double sz = ctx->grid.spacing[2];
  t.dhx = (P[0] * (g[2] * sz) + P[1] * (g[6] * sz)) + P[2] * (g[10] * sz);
  t.dhy = (Q[0] * (g[2] * sz) + Q[1] * (g[6] * sz)) + Q[2] * (g[10] * sz);
  t.dhz = (S[0] * (g[2] * sz) + S[1] * (g[6] * sz)) + S[2] * (g[10] * sz);
  // magnitudes of the world coordinates over the grid (plus one column height)
  double wm[3];
  const bool aligned = grid_axis_aligned(ctx->grid);
  if (aligned) {
    // |w| is largest at a grid corner (each w component is monotone in its own index)
    double lo[3], hi[3];
    voxel_world(ctx->grid, 0, 0, ctx->opt.z_first, lo);
    voxel_world(ctx->grid, ctx->grid.cell_dims[0] - 1, ctx->grid.cell_dims[1] - 1,
                ctx->opt.z_first + ctx->grid.cell_dims[2] - 1 + kMaxColumn, hi);
    for (int a = 0; a < 3; ++a) wm[a] = std::max(std::fabs(lo[a]), std::fabs(hi[a]));
  } else {
    // sum of magnitudes: also bounds every intermediate of the evaluation
    double gm[3];
    for (int a = 0; a < 3; ++a)
      gm[a] = std::fabs(ctx->grid.origin[a]) +
              (ctx->grid.cell_dims[a] + 1.0 + (a == 2 ? ctx->opt.z_first + kMaxColumn : 0)) * std::fabs(ctx->grid.spacing[a]);
    for (int a = 0; a < 3; ++a)
      wm[a] = std::fabs(g[4 * a]) * gm[0] + std::fabs(g[4 * a + 1]) * gm[1] + std::fabs(g[4 * a + 2]) * gm[2] + std::fabs(g[4 * a + 3]);
  }
  double M[3];
  for (int row = 0; row < 3; ++row)
    M[row] = std::fabs(rt[4 * row]) * wm[0] + std::fabs(rt[4 * row + 1]) * wm[1] + std::fabs(rt[4 * row + 2]) * wm[2] +
             std::fabs(rt[4 * row + 3]);
  // magnitudes of the terms of h.x, h.y, h.z: every row of K against (|c.x|, |c.y|, |c.z|, 1)
  const double Sx = std::fabs(k[0]) * M[0] + std::fabs(k[1]) * M[1] + std::fabs(k[2]) * M[2] + (general ? std::fabs(k[3]) : 0.0);
  const double Sy = (general ? std::fabs(k[4]) * M[0] : 0.0) + std::fabs(k[5]) * M[1] + std::fabs(k[6]) * M[2] +
                    (general ? std::fabs(k[7]) : 0.0);
  const double Sz = general ? std::fabs(k[8]) * M[0] + std::fabs(k[9]) * M[1] + std::fabs(k[10]) * M[2] + std::fabs(k[11]) : M[2];
  t.err = std::max(Sx, Sy) * 0x1p-44;  // 512 ulps of the term magnitudes
  // general K: the same bound for the affine h.z.  0 for a pinhole K, where the kernel's h.z is the reference's own c.z
  t.errz = general ? Sz * 0x1p-44 : 0.0;
  // rotated grid: the computed c.z (9 + 6 rounded operations on terms bounded by M[2]) is within 8 ulp(M[2]) of the
  // real, exactly affine one; four times that as the margin of the brick classification
  t.cz_err = aligned ? 0.0 : M[2] * 0x1p-47;
  // The kernel accepts a pixel iff |frac| + errk * r < 1/2 with r = (1 +- 2^-39) / h.z.  errk * r covers
  //   err / h.z                      the error of h.x, h.y,
  //   2^16 * errz / h.z              that of h.z, times |u| < 2^16 (beyond that both are outside any map),
  //   2^-22                          the slack of DESIGN.md 4.4, because Sz bounds |h.z| everywhere in the grid
  //                                  (Sz * r >= 1 - 2^-39).
  // Z >= |h.z| over the grid's voxels (and one column above).  General K: the sum of magnitudes.  Pinhole: c.z is affine in the
  // voxel indices, so its extremes are at the grid's corner voxels -- their computed values, widened by the computed c.z's
  // distance from the real one (16 ulp of the term magnitudes, twice that on a rotated grid).  (Until round 5 the sum of
  // magnitudes served both: in a geo-referenced frame, where |T| ~ 1e6 cancels against R w, it overstates |c.z| a millionfold and
  // the fp64 tier accepted next to nothing.)
  double zabs = Sz, czlo = std::numeric_limits<double>::infinity(), czhi = -czlo;
  if (!general) {
    zabs = 0.0;
    for (int c = 0; c < 8; ++c) {
      double w[3];
      voxel_world(ctx->grid, (c & 1) ? ctx->grid.cell_dims[0] - 1 : 0, (c & 2) ? ctx->grid.cell_dims[1] - 1 : 0,
                  ctx->opt.z_first + ((c & 4) ? ctx->grid.cell_dims[2] - 1 + kMaxColumn : 0), w);
      const double cz = ((rt[8] * w[0] + rt[9] * w[1]) + rt[10] * w[2]) + rt[11];
      zabs = std::max(zabs, std::fabs(cz));
      czlo = std::min(czlo, cz);
      czhi = std::max(czhi, cz);
    }
    zabs = zabs * (1.0 + 0x1p-20) + (aligned ? 1.0 : 2.0) * 32.0 * 0x1p-52 * M[2];
    if (!std::isfinite(zabs)) zabs = Sz;
  }
  // What "far below a pixel" is measured against: the bounds err, cerr are absolute (units of h.x), a voxel's share of a pixel is
  // bound / c.z.  zscale: the depth of most of the grid as the view sees it -- its nearest corner, but no less than a sixteenth
  // of its farthest (a camera inside the volume) and no less than 1.
  double zscale = 1.0;
  if (!general && std::isfinite(czlo) && std::isfinite(czhi)) zscale = std::max(1.0, std::max(czlo, czhi / 16.0));
  t.errk = (t.err + 65536.0 * t.errz) + 0x1p-22 * zabs * (1.0 + 0x1p-20);
  t.depth = r.depth;
  make_centred_rows(ctx, r, P, Q, S, Sx, Sy, M, zabs, zscale, general, aligned, &t, win, foot);
  if (zscale_out) *zscale_out = zscale;
  return t;
}

int add_views_impl(dmi_context *ctx, const double *depth64, const float *depth32, const double *best_cost,
                   double threshold, const double *K4, const double *RT4, int32_t n, int32_t width, int32_t height) {
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
  int rc = upload_batch(ctx, depth64, depth32, best_cost, threshold, n, &b, &lossy);
  if (rc != DMI_OK) return rc;
  if (lossy != 0 && !ctx->views.depth_f64 && ctx->opt.depth_storage == DMI_DEPTH_AUTO) {
    // some depth is not an f32: keep every bit -> promote the whole store and redo this batch in f64
    (void)hipFree(b.d_depth);
    (void)hipFree(b.d_pyramid);
    ctx->device_bytes -= npix * n * 4 + b.aux_bytes;
    rc = promote_to_f64(ctx);
    if (rc != DMI_OK) return rc;
    rc = upload_batch(ctx, depth64, depth32, best_cost, threshold, n, &b, &lossy);
    if (rc != DMI_OK) return rc;
  }
  ctx->views.batches.push_back(b);
  const size_t esz = depth_elem(ctx);
  for (int32_t m = 0; m < n; ++m) {
    MapRec r;
    std::memset(&r, 0, sizeof(r));
    // rows 0..2 of the row-major 4x4s (cu:220-230 marshals all 16; the kernel reads 12, cu:90-92)
    std::memcpy(r.rt, RT4 + 16 * (size_t)m, 12 * sizeof(double));
    std::memcpy(r.k, K4 + 16 * (size_t)m, 12 * sizeof(double));
    r.depth = static_cast<const char *>(b.d_depth) + (size_t)m * npix * esz;
    r.pyramid = b.d_pyramid + (size_t)m * ctx->views.pyramid.total_tiles;
    ctx->views.h_maps.push_back(r);
    bool finite = true;
    for (int q = 0; q < 12; ++q) finite = finite && bounded(r.k[q]) && bounded(r.rt[q]);
    const int km = classify_k(r.k, r.rt);
    if (km < ctx->views.k_mode) ctx->views.k_mode = km;
    dmi::WinRec wrec;
    dmi::FootRec frec;
    double zscale = 1.0;
    TileMapRec t = make_tile_rec(ctx, r, &wrec, &frec, &zscale);
    t.valid = reinterpret_cast<const uint8_t *>(b.d_pyramid) + b.valid_offset + (size_t)m * (size_t)dmi::valid_map_bytes(ctx->views.W, ctx->views.H);
    t.vm_c0 = ((float)(ctx->views.H / 2 + dmi::kValidMargin) - 3.5f) * 0.125f;
    t.vm_w8 = (float)(8 * (ctx->views.W + 2 * dmi::kValidMargin) - 8);
    t.vm_base = 8 * (ctx->views.W / 2 + dmi::kValidMargin) + ctx->views.H / 2 + dmi::kValidMargin;
    t.vm_bytes = (int32_t)std::min<int64_t>(dmi::valid_map_bytes(ctx->views.W, ctx->views.H), 0x7fffffff);
    t.vbits = reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(b.d_pyramid) + b.bits_offset +
                                                 (size_t)m * (size_t)dmi::valid_bits_bytes(ctx->views.W, ctx->views.H));
    t.vb_bytes = (int32_t)std::min<int64_t>(dmi::valid_bits_bytes(ctx->views.W, ctx->views.H), 0x7fffffff);
    t.vb_rowskip = (dmi::valid_bits_tiles_x(ctx->views.W) - 1) * 128;
    t.vb_mx = 0x4B400000 + dmi::kValidMargin + ctx->views.W / 2;
    t.vb_my = 0x4B400000 + dmi::kValidMargin + ctx->views.H / 2;
    ctx->views.h_tile_maps.push_back(t);
    wrec.vbits = t.vbits;
    ctx->views.h_win_recs.push_back(wrec);
    ctx->views.h_foot_recs.push_back(frec);
    if (!(t.err <= ctx->views.max_tile_err)) ctx->views.max_tile_err = t.err;  // NaN-propagating max
    ctx->views.view_k_mode.push_back((uint8_t)km);
    // pixel selection must be provable for nearly every lane: the error bounds over h.z must stay far below one pixel at the
    // depth of most of the grid (zscale, make_tile_rec): err / c.z < 2^-12 pixels sends about a voxel in a thousand to the exact
    // expression -- a few per cent of a wave's voxels redone, against the general kernel's 6 x.  (Until round 5 the test was
    // err < 2^-14 whatever the depth: a survey in a UTM frame with a long lens left the tiled kernel at offsets of 1e5.)
    ctx->views.view_tile_ok.push_back(finite && t.err < 0x1p-12 * zscale && 65536.0 * t.errz < 0x1p-14 && t.cerrk < 0x1p-11 * zscale ? 1 : 0);
  }
  ctx->views.maps_dirty = true;
  ctx->timings.last_upload_ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return DMI_OK;
}

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

int dmi_get_upload_kernel_ms(dmi_context *ctx, double *last, double *total) {
  if (!ctx) return DMI_ERR_INVALID_ARGUMENT;
  if (last) *last = ctx->views.last_upload_kernel_ms;
  if (total) *total = ctx->views.total_upload_kernel_ms;
  return DMI_OK;
}

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
  ctx->mesh.release();
  ctx->extraction.release();
  ctx->components.release();
  ctx->smoothing.release();
  ctx->decimation.release();
  ctx->support.release();
  ctx->coloration.release();
  for (hipEvent_t e : ctx->slab_events) (void)hipEventDestroy(e);
  if (ctx->download_stream) (void)hipStreamDestroy(ctx->download_stream);
  if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
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
    const size_t n = ctx->views.h_maps.size();
    if (n > 0 && dmi::holds(ctx->hits.map, n * sizeof(uint64_t))) {
      static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "u64");
      DMI_HIP(ctx, hipMemcpyAsync(map_hits, ctx->hits.map.ptr, n * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    } else {
      for (size_t i = 0; i < n; ++i) map_hits[i] = 0;
    }
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

int dmi_get_view_paths(dmi_context *ctx, uint64_t out[6]) {
  return guarded(ctx, "dmi_get_view_paths", [&]() -> int {
  if (!ctx || !out) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_get_view_paths: null argument");
  for (int i = 0; i < 6; ++i) out[i] = 0;
  const bool possible = tile_eligible(ctx);
  for (size_t m = 0; m < ctx->views.h_maps.size(); ++m) {
    const TileMapRec &t = ctx->views.h_tile_maps[m];
    if (!possible || !ctx->views.view_tile_ok[m]) {
      out[0] += 1;
    } else if (ctx->views.view_k_mode[m] == dmi::K_GENERAL) {
      out[1] += 1;
    } else {
      out[2 + std::min(std::max(t.t1_ok, 0), 2)] += 1;
      if (t.t1_ok != 0 && std::isfinite(ctx->views.h_win_recs[m].e_abs)) out[5] += 1;
    }
  }
  return DMI_OK;
  });
}

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
