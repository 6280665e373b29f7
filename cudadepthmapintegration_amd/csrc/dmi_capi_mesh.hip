// dmi_capi_mesh.hip -- the post-processing entry points of the C ABI declared in include/dmi.h: the grid's point data
// (vtkCellDataToPointData), the active cells of an iso-value, and the iso-surface mesh -- extraction, downloads, the component
// filter, the smoother, the decimation, the hole fill, the support trim, the coloration and their getters.  All of it works on the
// grouped state of dmi_context.h; what the mesh stages share -- the mesh's state and its commit, the events and times, the sizes
// refused, the scratch carving -- is dmi_mesh_stage.h's, and the helpers below (require_mesh, the getters, download) are the rest
// of their scaffold.  dmi_capi.hip, dmi_capi_views.hip and dmi_capi_fuse.hip have the rest of the C ABI.
#include "dmi_context.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>

using dmi::drain_c2p;
using dmi::drain_events;
using dmi::ensure_buffer;
using dmi::ensure_buffers;
using dmi::fail;
using dmi::flush_zero_fill;
using dmi::guarded;

namespace {
// bytes per vertex (3 f64), per triangle (3 int64 ids) and per normal (3 f32) of the mesh buffers
constexpr uint64_t kVertexBytes = 3 * sizeof(double), kTriangleBytes = 3 * sizeof(int64_t), kNormalBytes = 3 * sizeof(float);

int64_t n_points(const dmi_context *c) {
  return (int64_t)(c->grid.cell_dims[0] + 1) * (c->grid.cell_dims[1] + 1) * (c->grid.cell_dims[2] + 1);
}

// every entry point that works on the mesh: `since` is what the message says has not happened
int require_mesh(dmi_context *ctx, const std::string &entry, const char *since = "no extraction has succeeded") {
  if (ctx->mesh.valid) return DMI_OK;
  return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": no mesh (" + since + ")");
}

// a size the stage cannot hold (dmi_mesh_stage.h: the text, empty when accepted)
int refuse_size(dmi_context *ctx, const std::string &entry, const std::string &refusal) {
  return refusal.empty() ? DMI_OK : fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": " + refusal);
}

// The getters: behind the null check and, for the stages whose events are read late, the drain, one number of the context (a
// time, a counter; `field` picks it) or a stage's passes
using Drain = int (*)(dmi_context *);
template <typename T, typename Read>
int get(dmi_context *ctx, const char *entry, T *out, Drain drain, Read read) {
  return guarded(ctx, entry, [&]() -> int {
    if (!ctx || !out) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, std::string(entry) + ": null argument");
    const int rc = drain ? drain(ctx) : DMI_OK;
    if (rc == DMI_OK) read();
    return rc;
  });
}
template <typename T, typename Field>
int get_value(dmi_context *ctx, const char *entry, T *out, Field field, Drain drain = nullptr) {
  return get(ctx, entry, out, drain, [&] { *out = field(*ctx); });
}
template <typename Stage>
int get_passes(dmi_context *ctx, const char *entry, double *out, Stage dmi_context::*stage, Drain drain = nullptr) {
  return get(ctx, entry, out, drain, [&] { std::copy((ctx->*stage).last_pass_ms.begin(), (ctx->*stage).last_pass_ms.end(), out); });
}

// The downloads, behind their checks of the state: the copies whose destination is not null and that have bytes, one wait
struct Download {
  void *to;
  const dmi::DeviceBuffer &from;
  uint64_t bytes;
};
int download(dmi_context *ctx, std::initializer_list<Download> copies) {
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  for (const Download &c : copies)
    if (c.to && c.bytes) DMI_HIP(ctx, hipMemcpyAsync(c.to, c.from.ptr, (size_t)c.bytes, hipMemcpyDeviceToHost, ctx->stream));
  DMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return DMI_OK;
}
}  // namespace

int dmi::drain_c2p(dmi_context *ctx) {
  if (ctx->c2p.pending) {
    DMI_HIP(ctx, hipEventSynchronize(ctx->c2p.events[1]));
    DMI_HIP(ctx, ctx->c2p.elapsed(0, 1, &ctx->timings.last_cell_to_point_ms));
    ctx->c2p.pending = false;
  }
  dmi_context::PointSmoothing &ps = ctx->point_smoothing;
  if (ps.pending) {  // the smoothing passes that followed it (dmi_set_point_smoothing)
    DMI_HIP(ctx, hipEventSynchronize(ps.events[1]));
    DMI_HIP(ctx, ps.elapsed(0, 1, &ps.last_kernel_ms));
    ps.pending = false;
  }
  return DMI_OK;
}

extern "C" {

int dmi_cell_to_point(dmi_context *ctx) {
  return guarded(ctx, "dmi_cell_to_point", [&]() -> int {
  if (!ctx) return DMI_ERR_INVALID_ARGUMENT;
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  // an external grid can be changed by its owner (e.g. an all-reduce) without the context knowing: always recompute
  if (ctx->c2p.valid && ctx->volume.own_grid) return DMI_OK;
  int rc = flush_zero_fill(ctx);
  if (rc != DMI_OK) return rc;
  rc = drain_c2p(ctx);
  if (rc != DMI_OK) return rc;
  rc = ensure_buffer(ctx, ctx->c2p.points, (uint64_t)n_points(ctx) * 8);
  if (rc != DMI_OK) return rc;
  // dmi_set_point_smoothing: the passes ping-pong between the point buffer and a second one of its size and must end in the
  // former, so after an odd number of them the cell -> point pass writes into the second
  dmi_context::PointSmoothing &ps = ctx->point_smoothing;
  const int passes = ps.on ? dmi::point_smooth_launches(ps.args) : 0;
  if (ps.on) {
    rc = ensure_buffer(ctx, ps.scratch, (uint64_t)n_points(ctx) * 8);
    if (rc != DMI_OK) return rc;
    DMI_HIP(ctx, ps.create());
  }
  double *first = passes % 2 ? ps.scratch.as<double>() : ctx->c2p.points.as<double>();
  double *second = passes % 2 ? ctx->c2p.points.as<double>() : ps.scratch.as<double>();
  DMI_HIP(ctx, ctx->c2p.create());
  DMI_HIP(ctx, hipEventRecord(ctx->c2p.events[0], ctx->stream));
  DMI_HIP(ctx, dmi::launch_cell_to_point(ctx->volume.d_grid, ctx->opt.grid_dtype == DMI_F64 ? 1 : 0, first,
                                         ctx->grid.cell_dims[0], ctx->grid.cell_dims[1], ctx->grid.cell_dims[2], ctx->stream));
  DMI_HIP(ctx, hipEventRecord(ctx->c2p.events[1], ctx->stream));
  if (ps.on) {
    DMI_HIP(ctx, hipEventRecord(ps.events[0], ctx->stream));
    DMI_HIP(ctx, dmi::launch_point_smooth(first, second, ctx->grid.cell_dims[0], ctx->grid.cell_dims[1], ctx->grid.cell_dims[2], ps.args,
                                          ctx->stream));
    DMI_HIP(ctx, hipEventRecord(ps.events[1], ctx->stream));
    ps.pending = true;
  }
  ctx->c2p.pending = true;
  ctx->c2p.valid = true;
  return DMI_OK;
  });
}

int dmi_download_point_data_f64(dmi_context *ctx, double *out) {
  return guarded(ctx, "dmi_download_point_data_f64", [&]() -> int {
  if (!ctx || !out) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_download_point_data_f64: null argument");
  int rc = dmi_cell_to_point(ctx);
  if (rc != DMI_OK) return rc;
  DMI_HIP(ctx, hipMemcpyAsync(out, ctx->c2p.points.ptr, (size_t)n_points(ctx) * 8, hipMemcpyDeviceToHost, ctx->stream));
  DMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  rc = drain_c2p(ctx);
  if (rc != DMI_OK) return rc;
  return drain_events(ctx);
  });
}

int dmi_point_data_device_pointer(dmi_context *ctx, void **ptr) {
  return guarded(ctx, "dmi_point_data_device_pointer", [&]() -> int {
  if (!ctx || !ptr) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_point_data_device_pointer: null argument");
  int rc = dmi_cell_to_point(ctx);
  if (rc != DMI_OK) return rc;
  *ptr = ctx->c2p.points.ptr;
  return DMI_OK;
  });
}

int dmi_point_smoothing_weights(double sigma, double truncate, int32_t *radius, double *weights) {
  return guarded(nullptr, "dmi_point_smoothing_weights", [&]() -> int {
  if (dmi::point_smoothing_weights(sigma, truncate, radius, weights) != 0)
    return fail(nullptr, DMI_ERR_INVALID_ARGUMENT,
                "dmi_point_smoothing_weights: sigma must be finite and >= 0, truncate finite and in (0, 4], ceil(truncate * sigma) <= 16, "
                "and the pointers not null");
  return DMI_OK;
  });
}

int dmi_set_point_smoothing(dmi_context *ctx, const double sigma[3], double truncate) {
  return guarded(ctx, "dmi_set_point_smoothing", [&]() -> int {
  if (!ctx || !sigma) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_set_point_smoothing: null argument");
  if (ctx->opt.z_first != 0)
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT,
                "dmi_set_point_smoothing: the context holds a z-slab (z_first != 0); its lattice is not the grid's");
  dmi::PointSmoothArgs args{};
  for (int a = 0; a < 3; ++a)
    if (dmi::point_smoothing_weights(sigma[a], truncate, &args.r[a], args.k[a]) != 0)
      return fail(ctx, DMI_ERR_INVALID_ARGUMENT,
                  "dmi_set_point_smoothing: sigma[" + std::to_string(a) + "] must be finite and >= 0, truncate finite and in (0, 4], and "
                  "the radius ceil(truncate * sigma) at most 16");
  dmi_context::PointSmoothing &ps = ctx->point_smoothing;
  if (sigma[0] == ps.sigma[0] && sigma[1] == ps.sigma[1] && sigma[2] == ps.sigma[2] && truncate == ps.truncate) return DMI_OK;
  const bool on = sigma[0] != 0.0 || sigma[1] != 0.0 || sigma[2] != 0.0;
  for (int a = 0; a < 3; ++a) ps.sigma[a] = sigma[a] + 0.0;  // (a -0.0 is stored as 0)
  ps.truncate = truncate;
  ps.args = args;
  if (!on && !ps.on) return DMI_OK;  // off before and after: the point data is what it was
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  ps.on = on;
  ctx->c2p.valid = false;
  if (!on) {  // the state after dmi_create: no second buffer, no kernel time
    const int rc = drain_c2p(ctx);
    ps.last_kernel_ms = 0.0;
    dmi::drop_buffers(ctx, {&ps.scratch});  // (hipFree waits for the passes that may still read it)
    return rc;
  }
  return DMI_OK;
  });
}

int dmi_get_point_smoothing(dmi_context *ctx, double sigma[3], double *truncate) {
  return guarded(ctx, "dmi_get_point_smoothing", [&]() -> int {
  if (!ctx || !sigma || !truncate) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_get_point_smoothing: null argument");
  for (int a = 0; a < 3; ++a) sigma[a] = ctx->point_smoothing.sigma[a];
  *truncate = ctx->point_smoothing.truncate;
  return DMI_OK;
  });
}

int dmi_get_point_smoothing_kernel_ms(dmi_context *ctx, double *last) {
  return get_value(ctx, "dmi_get_point_smoothing_kernel_ms", last,
                   [](dmi_context &c) { return c.point_smoothing.on ? c.point_smoothing.last_kernel_ms : 0.0; },
                   [](dmi_context *ctx) -> int {
                     DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
                     return drain_c2p(ctx);
                   });
}

int dmi_iso_active_cells(dmi_context *ctx, double iso, uint64_t *count, int64_t *cell_ids, uint64_t capacity) {
  return guarded(ctx, "dmi_iso_active_cells", [&]() -> int {
  if (!ctx || !count) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_iso_active_cells: null argument");
  if (iso != iso) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_iso_active_cells: the iso-value is a NaN");
  *count = 0;
  int rc = dmi_cell_to_point(ctx);  // the contour filter reads the point data (Reconstruction/main.cxx:151-173)
  if (rc != DMI_OK) return rc;
  const int nx = ctx->grid.cell_dims[0], ny = ctx->grid.cell_dims[1], nz = ctx->grid.cell_dims[2];
  const size_t n_blocks = dmi::iso_block_count(nx, ny, nz);
  if (n_blocks >= (size_t(1) << 31)) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_iso_active_cells: grid too large for one launch");
  // scratch for this call: per-block counts (+ a trailing zero), their prefix sums, the scan's own storage, the ids
  struct Scratch {
    uint32_t *counts = nullptr;
    uint64_t *bases = nullptr;
    void *temp = nullptr;
    int64_t *ids = nullptr;
    ~Scratch() {
      (void)hipFree(counts);
      (void)hipFree(bases);
      (void)hipFree(temp);
      (void)hipFree(ids);
    }
  } sc;
  const double *points = ctx->c2p.points.as<double>();
  size_t temp_bytes = 0;
  DMI_HIP(ctx, dmi::launch_iso_count(nullptr, nx, ny, nz, iso, nullptr, nullptr, nullptr, &temp_bytes, ctx->stream));
  DMI_HIP(ctx, hipMalloc(&sc.counts, (n_blocks + 1) * sizeof(uint32_t)));
  DMI_HIP(ctx, hipMalloc(&sc.bases, (n_blocks + 1) * sizeof(uint64_t)));
  DMI_HIP(ctx, hipMalloc(&sc.temp, std::max<size_t>(temp_bytes, 16)));
  DMI_HIP(ctx, hipMemsetAsync(sc.counts + n_blocks, 0, sizeof(uint32_t), ctx->stream));
  DMI_HIP(ctx, dmi::launch_iso_count(points, nx, ny, nz, iso, sc.counts, sc.bases, sc.temp, &temp_bytes, ctx->stream));
  uint64_t total = 0;
  DMI_HIP(ctx, hipMemcpyAsync(&total, sc.bases + n_blocks, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  DMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *count = total;
  const uint64_t n_out = std::min<uint64_t>(total, cell_ids ? capacity : 0);
  if (n_out > 0) {
    DMI_HIP(ctx, hipMalloc(&sc.ids, (size_t)n_out * sizeof(int64_t)));
    DMI_HIP(ctx, dmi::launch_iso_write(points, nx, ny, nz, iso, sc.bases, sc.ids, n_out, ctx->stream));
    DMI_HIP(ctx, hipMemcpyAsync(cell_ids, sc.ids, (size_t)n_out * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    DMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  rc = drain_c2p(ctx);
  if (rc != DMI_OK) return rc;
  return drain_events(ctx);
  });
}

namespace {
// The normals' matrix: the cofactors of the grid matrix's upper-left 3 x 3 A, C[r][c] = A[r+1][c+1] A[r+2][c+2] -
// A[r+1][c+2] A[r+2][c+1] (indices mod 3), negated when det A < 0: inverse(A)^T times |det A|, f64, row-major
void normal_matrix(const double gm[16], double nm[9]) {
  auto a = [&](int r, int c) { return gm[4 * (r % 3) + c % 3]; };
  double cof[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) cof[3 * r + c] = a(r + 1, c + 1) * a(r + 2, c + 2) - a(r + 1, c + 2) * a(r + 2, c + 1);
  const double det = a(0, 0) * cof[0] + a(0, 1) * cof[1] + a(0, 2) * cof[2];
  for (int e = 0; e < 9; ++e) nm[e] = det < 0 ? -cof[e] : cof[e];
}

// dmi_extract_isosurface, and with `normals` dmi_extract_isosurface_normals (`entry` names the call in the errors)
int extract_isosurface(dmi_context *ctx, const std::string &entry, double iso, uint64_t *n_vertices, uint64_t *n_triangles,
                       bool normals) {
  if (!ctx || !n_vertices || !n_triangles) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": null argument");
  if (iso != iso) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": the iso-value is a NaN");
  if (ctx->opt.z_first != 0)
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": the context holds a z-slab (z_first != 0); its lattice is not the grid's");
  *n_vertices = *n_triangles = 0;
  dmi_context::Mesh &mesh = ctx->mesh;
  dmi_context::Extraction &ex = ctx->extraction;
  mesh.valid = false;
  mesh.has_normals = false;
  mesh.filtered = false;
  mesh.support_counted = false;  // the counts of an earlier mesh are not this one's
  const int nx = ctx->grid.cell_dims[0], ny = ctx->grid.cell_dims[1], nz = ctx->grid.cell_dims[2];
  const size_t n_seg = dmi::isosurface_segment_count(nx, ny, nz);
  if (n_seg >= (size_t(1) << 31)) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": grid too large for one launch");
  int rc = dmi_cell_to_point(ctx);  // the contour filter reads the point data (Reconstruction/main.cxx:151-173)
  if (rc != DMI_OK) return rc;
  dmi::MeshGeom g{};
  g.nx = nx;
  g.ny = ny;
  g.nz = nz;
  g.segs_per_row = (int)((nx + 1 + 255) / 256);
  g.iso = iso;
  for (int a = 0; a < 3; ++a) {
    g.origin[a] = ctx->grid.origin[a];
    g.spacing[a] = ctx->grid.spacing[a];
  }
  for (int e = 0; e < 12; ++e) g.m[e] = ctx->grid.grid_matrix[e];
  // two count arrays and two base arrays (vertices, triangles) of n_seg entries and a trailing total each
  rc = ensure_buffers(ctx, {{&ex.counts, (uint64_t)(n_seg + 1) * 2 * sizeof(uint32_t)}, {&ex.bases, (uint64_t)(n_seg + 1) * 2 * sizeof(uint64_t)}});
  if (rc != DMI_OK) return rc;
  uint32_t *counts = ex.counts.as<uint32_t>();
  uint64_t *bases = ex.bases.as<uint64_t>();
  const double *points = ctx->c2p.points.as<double>();
  size_t temp_bytes = 0;
  DMI_HIP(ctx, dmi::launch_isosurface_count(nullptr, g, counts, bases, nullptr, &temp_bytes, ctx->stream));
  temp_bytes = std::max<size_t>(temp_bytes, 16);
  rc = ensure_buffer(ctx, ex.scan_temp, temp_bytes);
  if (rc != DMI_OK) return rc;
  DMI_HIP(ctx, ex.create());
  // the trailing zeros behind each count array: bases[n_seg] and bases[2 n_seg + 1] become the totals
  DMI_HIP(ctx, hipMemsetAsync(counts + n_seg, 0, sizeof(uint32_t), ctx->stream));
  DMI_HIP(ctx, hipMemsetAsync(counts + 2 * n_seg + 1, 0, sizeof(uint32_t), ctx->stream));
  DMI_HIP(ctx, hipEventRecord(ex.events[0], ctx->stream));
  DMI_HIP(ctx, dmi::launch_isosurface_count(points, g, counts, bases, ex.scan_temp.ptr, &temp_bytes, ctx->stream));
  DMI_HIP(ctx, hipEventRecord(ex.events[1], ctx->stream));
  uint64_t totals[2] = {0, 0};
  DMI_HIP(ctx, hipMemcpyAsync(&totals[0], bases + n_seg, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  DMI_HIP(ctx, hipMemcpyAsync(&totals[1], bases + 2 * n_seg + 1, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  DMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  rc = refuse_size(ctx, entry, dmi::extraction_refusal(totals[0], totals[1]));
  if (rc != DMI_OK) return rc;
  g.n_vertices = totals[0];
  g.n_triangles = totals[1];
  double ms_count = 0.0, ms_write = 0.0;
  DMI_HIP(ctx, ex.elapsed(0, 1, &ms_count));
  if (totals[0] > 0) {
    rc = ensure_buffers(ctx, {{&mesh.vertices, totals[0] * kVertexBytes}, {&mesh.triangles, totals[1] * kTriangleBytes},
                              {&mesh.normals, normals ? totals[0] * kNormalBytes : 0}});
    if (rc != DMI_OK) return rc;
    dmi::MeshNormals nrm{};
    if (normals) {
      normal_matrix(ctx->grid.grid_matrix, nrm.nm);
      nrm.normals = mesh.normals.as<float>();
    }
    DMI_HIP(ctx, hipEventRecord(ex.events[2], ctx->stream));
    DMI_HIP(ctx, dmi::launch_isosurface_write(points, g, bases, mesh.vertices.as<double>(), mesh.triangles.as<int64_t>(),
                                              normals ? &nrm : nullptr, ctx->stream));
    DMI_HIP(ctx, hipEventRecord(ex.events[3], ctx->stream));
    DMI_HIP(ctx, hipEventSynchronize(ex.events[3]));
    DMI_HIP(ctx, ex.elapsed(2, 3, &ms_write));
  }
  ex.last_kernel_ms = ms_count + ms_write;
  mesh.n_vertices = totals[0];
  mesh.n_triangles = totals[1];
  mesh.valid = true;
  mesh.has_normals = normals;
  mesh.colored = false;  // the colours of an earlier mesh are not this one's
  *n_vertices = totals[0];
  *n_triangles = totals[1];
  rc = drain_c2p(ctx);
  if (rc != DMI_OK) return rc;
  return drain_events(ctx);
}
}  // namespace

int dmi_extract_isosurface(dmi_context *ctx, double iso, uint64_t *n_vertices, uint64_t *n_triangles) {
  return guarded(ctx, "dmi_extract_isosurface", [&]() -> int {
    return extract_isosurface(ctx, "dmi_extract_isosurface", iso, n_vertices, n_triangles, false);
  });
}

int dmi_extract_isosurface_normals(dmi_context *ctx, double iso, uint64_t *n_vertices, uint64_t *n_triangles) {
  return guarded(ctx, "dmi_extract_isosurface_normals", [&]() -> int {
    return extract_isosurface(ctx, "dmi_extract_isosurface_normals", iso, n_vertices, n_triangles, true);
  });
}

int dmi_download_isosurface(dmi_context *ctx, double *vertices, int64_t *triangles) {
  return guarded(ctx, "dmi_download_isosurface", [&]() -> int {
  if (!ctx || !vertices || !triangles) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_download_isosurface: null argument");
  const dmi_context::Mesh &mesh = ctx->mesh;
  if (int rc = require_mesh(ctx, "dmi_download_isosurface", "dmi_extract_isosurface has not succeeded")) return rc;
  return download(ctx, {{vertices, mesh.vertices, mesh.n_vertices * kVertexBytes}, {triangles, mesh.triangles, mesh.n_triangles * kTriangleBytes}});
  });
}

int dmi_download_isosurface_normals(dmi_context *ctx, float *normals) {
  return guarded(ctx, "dmi_download_isosurface_normals", [&]() -> int {
  if (!ctx || !normals) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_download_isosurface_normals: null argument");
  const dmi_context::Mesh &mesh = ctx->mesh;
  if (int rc = require_mesh(ctx, "dmi_download_isosurface_normals")) return rc;
  if (!mesh.has_normals)
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT,
                "dmi_download_isosurface_normals: the last mesh has no normals (dmi_extract_isosurface, not dmi_extract_isosurface_normals)");
  return download(ctx, {{normals, mesh.normals, mesh.n_vertices * kNormalBytes}});
  });
}

int dmi_get_isosurface_kernel_ms(dmi_context *ctx, double *last) {
  return get_value(ctx, "dmi_get_isosurface_kernel_ms", last, [](dmi_context &c) { return c.extraction.last_kernel_ms; });
}

int dmi_filter_isosurface_components(dmi_context *ctx, int mode, uint64_t min_triangles, uint64_t *n_vertices, uint64_t *n_triangles,
                                     uint64_t *n_components, uint64_t *n_components_kept) {
  return guarded(ctx, "dmi_filter_isosurface_components", [&]() -> int {
  const std::string entry = "dmi_filter_isosurface_components";
  if (!ctx || !n_vertices || !n_triangles || !n_components || !n_components_kept)
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": null argument");
  if (mode != DMI_COMPONENTS_MIN_TRIANGLES && mode != DMI_COMPONENTS_LARGEST)
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": unknown mode " + std::to_string(mode));
  dmi_context::Mesh &mesh = ctx->mesh;
  dmi_context::Components &comp = ctx->components;
  int rc = require_mesh(ctx, entry);
  if (rc != DMI_OK) return rc;
  *n_vertices = *n_triangles = *n_components = *n_components_kept = 0;
  const uint64_t nv = mesh.n_vertices, nt = mesh.n_triangles;
  rc = refuse_size(ctx, entry, dmi::ids_refusal(nv, nt, "32-bit component labels"));  // labels and sizes are u32
  if (rc != DMI_OK) return rc;
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  if (nv == 0) {  // an empty mesh stays empty
    mesh.drop(dmi::drops::kComponents);
    mesh.filtered = true;
    mesh.regions = 0;
    comp.zero();
    comp.last_cas_retries = 0;
    return DMI_OK;
  }
  const bool normals = mesh.has_normals;
  size_t temp_bytes = 0;
  DMI_HIP(ctx, dmi::components_scan_temp_bytes(nv, nt, &temp_bytes));
  temp_bytes = std::max<size_t>(temp_bytes, 16);
  // the compaction's output, the region arrays, the union-find's scratch and the scans'
  dmi::U32Lanes vs{nullptr, nv + 1};
  rc = ensure_buffers(ctx, {{&mesh.alt_vertices, nv * kVertexBytes}, {&mesh.alt_triangles, std::max<uint64_t>(nt, 1) * kTriangleBytes},
                            {&mesh.alt_normals, normals ? nv * kNormalBytes : 0}, {&mesh.region_id, nv * 8}, {&mesh.region_size, nv * 8},
                            {&comp.vertex_scratch, vs.bytes(dmi::kComponentsLanes)}, {&comp.triangle_scratch, (nt + 1) * 4},
                            {&comp.counters, 24}, {&comp.scan_temp, temp_bytes}});
  if (rc != DMI_OK) return rc;
  DMI_HIP(ctx, comp.create());
  dmi::ComponentsMesh m{};
  m.n_vertices = nv;
  m.n_triangles = nt;
  m.vertices = mesh.vertices.as<double>();
  m.normals = normals ? mesh.normals.as<float>() : nullptr;
  m.triangles = mesh.triangles.as<int64_t>();
  m.out_vertices = mesh.alt_vertices.as<double>();
  m.out_normals = mesh.alt_normals.as<float>();
  m.out_triangles = mesh.alt_triangles.as<int64_t>();
  m.region_id = mesh.region_id.as<int64_t>();
  m.region_size = mesh.region_size.as<int64_t>();
  dmi::ComponentsScratch s{};
  vs.base = comp.vertex_scratch.as<uint32_t>();
  s.parent = vs.lane(0);
  s.size = vs.lane(1);
  s.vmap = vs.lane(2);
  s.rmap = vs.lane(3);
  s.tmap = comp.triangle_scratch.as<uint32_t>();
  s.counters = comp.counters.as<unsigned long long>();
  s.scan_temp = comp.scan_temp.ptr;
  s.scan_temp_bytes = temp_bytes;
  // (a failure from here on leaves the context's mesh and its regions as they were: the buffers are swapped only at the end)
  DMI_HIP(ctx, dmi::launch_isosurface_components(m, s, mode == DMI_COMPONENTS_LARGEST ? 1 : 0, min_triangles, comp.events, ctx->stream));
  uint32_t kept[3] = {0, 0, 0};
  unsigned long long counters[3] = {0, 0, 0};
  DMI_HIP(ctx, hipMemcpyAsync(&kept[0], s.vmap + nv, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  DMI_HIP(ctx, hipMemcpyAsync(&kept[1], s.tmap + nt, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  DMI_HIP(ctx, hipMemcpyAsync(&kept[2], s.rmap + nv, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  DMI_HIP(ctx, hipMemcpyAsync(counters, s.counters, sizeof(counters), hipMemcpyDeviceToHost, ctx->stream));
  DMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  DMI_HIP(ctx, comp.read(0, 4));
  mesh.commit_alternates(kept[0], kept[1], dmi::drops::kComponents);  // the colours and support counts were the unfiltered mesh's
  mesh.filtered = true;
  mesh.regions = kept[2];
  comp.last_cas_retries = counters[2];
  *n_vertices = kept[0];
  *n_triangles = kept[1];
  *n_components = counters[1];
  *n_components_kept = kept[2];
  return DMI_OK;
  });
}

int dmi_download_isosurface_regions(dmi_context *ctx, int64_t *region_id, int64_t *region_size) {
  return guarded(ctx, "dmi_download_isosurface_regions", [&]() -> int {
  if (!ctx) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_download_isosurface_regions: null argument");
  const dmi_context::Mesh &mesh = ctx->mesh;
  if (int rc = require_mesh(ctx, "dmi_download_isosurface_regions")) return rc;
  if (!mesh.filtered)
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT,
                "dmi_download_isosurface_regions: no regions (dmi_filter_isosurface_components has not run since the last extraction)");
  return download(ctx, {{region_id, mesh.region_id, mesh.n_vertices * 8}, {region_size, mesh.region_size, mesh.regions * 8}});
  });
}

int dmi_get_isosurface_filter_kernel_ms(dmi_context *ctx, double *last) {
  return get_value(ctx, "dmi_get_isosurface_filter_kernel_ms", last, [](dmi_context &c) { return c.components.last_kernel_ms; });
}

int dmi_get_isosurface_filter_pass_ms(dmi_context *ctx, double out[4]) {
  return get_passes(ctx, "dmi_get_isosurface_filter_pass_ms", out, &dmi_context::components);
}

int dmi_get_isosurface_filter_cas_retries(dmi_context *ctx, uint64_t *last) {
  return get_value(ctx, "dmi_get_isosurface_filter_cas_retries", last, [](dmi_context &c) { return c.components.last_cas_retries; });
}

int dmi_smooth_isosurface(dmi_context *ctx, int32_t iterations, double lambda, double mu) {
  return guarded(ctx, "dmi_smooth_isosurface", [&]() -> int {
  const std::string entry = "dmi_smooth_isosurface";
  if (!ctx) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": null argument");
  if (iterations < 0 || iterations > 1000)
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": iterations " + std::to_string(iterations) + " is not in [0, 1000]");
  if (!(lambda > 0.0 && lambda <= 1.0)) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": lambda is not in (0, 1]");
  if (!(mu <= 0.0) || mu - mu != 0.0) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": mu is not a finite number <= 0");
  dmi_context::Mesh &mesh = ctx->mesh;
  dmi_context::Smoothing &sm = ctx->smoothing;
  const uint64_t nv = mesh.n_vertices, nt = mesh.n_triangles;
  int rc = require_mesh(ctx, entry);
  // ids are u32 on the device, and so are the offsets into the 6 T directed edges
  if (rc == DMI_OK) rc = refuse_size(ctx, entry, dmi::ids_refusal(nv, nt, "32-bit vertex ids"));
  if (rc == DMI_OK) rc = refuse_size(ctx, entry, dmi::product_refusal(6, nt, "32-bit adjacency offsets (6 x triangles >= 2^32)"));
  if (rc != DMI_OK) return rc;
  if (iterations == 0 || nv == 0) {  // nothing to do: the mesh, its normals included, stays as it is
    sm.zero();
    if (iterations > 0) mesh.drop(dmi::drops::kSmoothing);
    return DMI_OK;
  }
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  const bool normals = mesh.has_normals;
  const uint64_t fixed_words = (nv + 63) / 64, n_keys = std::max<uint64_t>(6 * nt, 2);
  size_t temp_bytes = 0;
  DMI_HIP(ctx, dmi::smooth_temp_bytes(nv, nt, &temp_bytes));
  temp_bytes = std::max<size_t>(temp_bytes, 16);
  // the two position buffers of the steps, the new normals, two key arrays, the per-vertex scratch (fixed bits, then the u32
  // arrays) and the sort's and scans' own storage
  dmi::U32Lanes vs{nullptr, nv + 1};
  rc = ensure_buffers(ctx, {{&mesh.alt_vertices, nv * kVertexBytes}, {&sm.vertices, nv * kVertexBytes},
                            {&mesh.alt_normals, normals ? nv * kNormalBytes : 0}, {&sm.keys, 2 * n_keys * 8},
                            {&sm.vertex_scratch, fixed_words * 8 + vs.bytes(dmi::kSmoothingLanes)}, {&sm.temp, temp_bytes}});
  if (rc != DMI_OK) return rc;
  DMI_HIP(ctx, sm.create());
  dmi::SmoothMesh m{};
  m.n_vertices = nv;
  m.n_triangles = nt;
  m.vertices = mesh.vertices.as<double>();
  m.triangles = mesh.triangles.as<int64_t>();
  m.normals_out = normals ? mesh.alt_normals.as<float>() : nullptr;
  dmi::SmoothScratch s{};
  s.keys[0] = sm.keys.as<uint64_t>();
  s.keys[1] = s.keys[0] + n_keys;
  s.fixed = sm.vertex_scratch.as<unsigned long long>();
  vs.base = (uint32_t *)(s.fixed + fixed_words);
  s.row_start = vs.lane(0);
  s.valence = vs.lane(1);
  s.offsets = vs.lane(2);
  s.positions[0] = mesh.alt_vertices.as<double>();
  s.positions[1] = sm.vertices.as<double>();
  s.temp = sm.temp.ptr;
  s.temp_bytes = temp_bytes;
  // (a failure from here on leaves the context's mesh as it was: no kernel writes it, and the buffers are swapped only at the end)
  double *result = nullptr;
  DMI_HIP(ctx, dmi::launch_isosurface_smooth(m, s, iterations, lambda, mu, &result, sm.events, ctx->stream));
  DMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  DMI_HIP(ctx, sm.read(0, 3));
  // the smoothed positions become the context's; the buffer they replace is the next call's scratch
  mesh.commit_positions(result == mesh.alt_vertices.ptr ? mesh.alt_vertices : sm.vertices, dmi::drops::kSmoothing);
  return DMI_OK;
  });
}

int dmi_get_isosurface_smooth_kernel_ms(dmi_context *ctx, double *last) {
  return get_value(ctx, "dmi_get_isosurface_smooth_kernel_ms", last, [](dmi_context &c) { return c.smoothing.last_kernel_ms; });
}

int dmi_get_isosurface_smooth_pass_ms(dmi_context *ctx, double out[3]) {
  return get_passes(ctx, "dmi_get_isosurface_smooth_pass_ms", out, &dmi_context::smoothing);
}

namespace {
// the events of the last decimation become its times (its normals, enqueued behind the call's last synchronisation, may still run)
int drain_decimation(dmi_context *ctx) {
  dmi_context::Decimation &dc = ctx->decimation;
  if (!dc.pending) return DMI_OK;
  DMI_HIP(ctx, hipEventSynchronize(dc.events[dc.pending_normals ? 7 : 5]));
  double bounds = 0.0, ranks = 0.0, triangles = 0.0, representatives = 0.0, normals = 0.0;
  DMI_HIP(ctx, dc.elapsed(0, 1, &bounds));
  DMI_HIP(ctx, dc.elapsed(2, 3, &ranks));
  DMI_HIP(ctx, dc.elapsed(3, 4, &triangles));
  DMI_HIP(ctx, dc.elapsed(4, 5, &representatives));
  if (dc.pending_normals) DMI_HIP(ctx, dc.elapsed(6, 7, &normals));
  dc.last_pass_ms[0] = bounds + ranks;
  dc.last_pass_ms[1] = representatives;
  dc.last_pass_ms[2] = triangles;
  dc.last_pass_ms[3] = normals;
  dc.last_kernel_ms = ((dc.last_pass_ms[0] + dc.last_pass_ms[1]) + dc.last_pass_ms[2]) + dc.last_pass_ms[3];
  dc.pending = false;
  return DMI_OK;
}

// the bins of one axis: floor((hi - lo) / h) + 1, or 0 when that is more than 2^21 (an infinite quotient included)
uint64_t decimate_bins(double lo, double hi, double h) {
  const double q = std::floor((hi - lo) / h);
  return q < 2097152.0 ? (uint64_t)q + 1 : 0;
}

// both entries: `name` is the one the messages speak of
int decimate_isosurface(dmi_context *ctx, const char *name, double cell_size, int32_t placement, uint64_t *n_vertices,
                        uint64_t *n_triangles) {
  return guarded(ctx, name, [&]() -> int {
  const std::string entry = name;
  if (!ctx || !n_vertices || !n_triangles) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": null argument");
  if (!(cell_size > 0.0) || cell_size - cell_size != 0.0)
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": cell_size is not a finite number > 0");
  if (placement != DMI_DECIMATE_MEAN && placement != DMI_DECIMATE_QUADRIC)
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT,
                entry + ": placement " + std::to_string(placement) + " is neither DMI_DECIMATE_MEAN nor DMI_DECIMATE_QUADRIC");
  const bool quadric = placement == DMI_DECIMATE_QUADRIC;
  dmi_context::Mesh &mesh = ctx->mesh;
  dmi_context::Decimation &dc = ctx->decimation;
  dmi_context::Smoothing &sm = ctx->smoothing;
  const uint64_t nv = mesh.n_vertices, nt = mesh.n_triangles;
  int rc = require_mesh(ctx, entry);
  // ids are u32 on the device, and so are the quadric placement's corner indices 3t + e
  if (rc == DMI_OK) rc = refuse_size(ctx, entry, dmi::ids_refusal(nv, nt, "32-bit vertex ids"));
  if (rc == DMI_OK && quadric) rc = refuse_size(ctx, entry, dmi::product_refusal(3, nt, "32-bit corner indices (3 T >= 2^32)"));
  if (rc != DMI_OK) return rc;
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  rc = drain_decimation(ctx);  // (the events are about to be recorded again)
  if (rc != DMI_OK) return rc;
  *n_vertices = *n_triangles = 0;
  if (nv == 0) {  // an empty mesh stays empty (it has no triangles either)
    mesh.drop(dmi::drops::kDecimation);
    dc.zero();
    return DMI_OK;
  }
  const bool normals = mesh.has_normals;
  size_t temp_bytes = 0, normals_temp_bytes = 0;
  DMI_HIP(ctx, dmi::decimate_temp_bytes(nv, nt, quadric ? dmi::kDecimateQuadric : dmi::kDecimateMean, &temp_bytes));
  if (normals) DMI_HIP(ctx, dmi::smooth_temp_bytes(nv, nt, &normals_temp_bytes));  // (the decimated mesh is no larger)
  temp_bytes = std::max<size_t>(std::max(temp_bytes, normals_temp_bytes), 16);
  // the result's buffers (the component filter's alternates), the vertex keys, then the triangle keys and values, then the
  // incidence of the normals (the smoother's key arrays), the per-vertex and per-triangle u32 arrays, rocPRIM's own storage; the
  // quadric placement's corner pairs and their sort's other halves are 3T u64 in each key array too
  const uint64_t n_keys = std::max<uint64_t>(std::max(nv, 2 * nt), normals || quadric ? 3 * nt : 0);
  dmi::U32Lanes vs{nullptr, nv + 1}, ts{nullptr, nt + 1};
  rc = ensure_buffers(ctx, {{&mesh.alt_vertices, nv * kVertexBytes}, {&mesh.alt_triangles, std::max<uint64_t>(nt, 1) * kTriangleBytes},
                            {&mesh.alt_normals, normals ? nv * kNormalBytes : 0}, {&sm.keys, 2 * n_keys * 8},
                            {&dc.vertex_scratch, vs.bytes(dmi::kDecimationLanes)},
                            {&dc.triangle_scratch, ts.bytes(dmi::kDecimationTriangleLanes)}, {&dc.bounds, 64}, {&sm.temp, temp_bytes}});
  if (rc != DMI_OK) return rc;
  DMI_HIP(ctx, dc.create());
  dmi::DecimateMesh m{};
  m.n_vertices = nv;
  m.n_triangles = nt;
  m.vertices = mesh.vertices.as<double>();
  m.triangles = mesh.triangles.as<int64_t>();
  m.out_vertices = mesh.alt_vertices.as<double>();
  m.out_triangles = mesh.alt_triangles.as<int64_t>();
  dmi::DecimateScratch s{};
  s.bounds = dc.bounds.as<unsigned long long>();
  s.keys[0] = sm.keys.as<uint64_t>();
  s.keys[1] = s.keys[0] + n_keys;
  vs.base = dc.vertex_scratch.as<uint32_t>();
  s.ids[0] = vs.lane(0);
  s.ids[1] = vs.lane(1);
  s.head = vs.lane(2);
  s.rank = vs.lane(3);
  s.cluster_of = vs.lane(4);
  s.start = vs.lane(5);
  s.mark = vs.lane(6);
  s.cmap = vs.lane(7);
  ts.base = dc.triangle_scratch.as<uint32_t>();
  s.keep = ts.lane(0);
  s.tmap = ts.lane(1);
  s.temp = sm.temp.ptr;
  s.temp_bytes = temp_bytes;
  // (a failure from here on leaves the context's mesh, its normals and its regions as they were: no kernel writes them, and the
  // buffers are swapped only at the end)
  DMI_HIP(ctx, dmi::launch_decimate_bounds(m, s, dc.events, ctx->stream));
  unsigned long long bounds[7] = {0, 0, 0, 0, 0, 0, 0};
  DMI_HIP(ctx, hipMemcpyAsync(bounds, s.bounds, sizeof(bounds), hipMemcpyDeviceToHost, ctx->stream));
  DMI_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the first of two: the bins, or the refusal
  if (bounds[6]) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": the mesh has a non-finite vertex coordinate");
  dmi::DecimateGrid g{};
  g.h = cell_size;
  double extent = 0.0;
  bool too_many = false;
  for (int d = 0; d < 3; ++d) {
    g.lo[d] = dmi::decimate_decode_bound(bounds[d]);
    const double hi = dmi::decimate_decode_bound(bounds[3 + d]);
    g.n[d] = decimate_bins(g.lo[d], hi, cell_size);
    too_many |= g.n[d] == 0;
    extent = std::max(extent, hi - g.lo[d]);
  }
  if (too_many) {
    // the smallest cell size whose quotient, as rounded, stays below 2^21 on the longest axis
    double least = extent / 2097152.0;
    while (!(std::floor(extent / least) < 2097152.0)) least = std::nextafter(least, std::numeric_limits<double>::infinity());
    char text[64];
    std::snprintf(text, sizeof(text), "%.17g", least);
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT,
                entry + ": more than 2^21 bins on an axis; the smallest acceptable cell size for this mesh is " + text);
  }
  DMI_HIP(ctx, dmi::launch_isosurface_decimate(m, g, s, quadric ? dmi::kDecimateQuadric : dmi::kDecimateMean, dc.events + 2, ctx->stream));
  uint32_t kept[2] = {0, 0};
  DMI_HIP(ctx, hipMemcpyAsync(&kept[0], s.cmap + nv, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  DMI_HIP(ctx, hipMemcpyAsync(&kept[1], s.tmap + nt, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  DMI_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the second: the counts
  const bool new_normals = normals && kept[0] > 0;
  if (new_normals) {  // the smoother's incidence build and kernel on the result; the triangle keys are no longer needed
    uint64_t *const keys[2] = {s.keys[0], s.keys[1]};
    DMI_HIP(ctx, hipEventRecord(dc.events[6], ctx->stream));
    DMI_HIP(ctx, dmi::launch_isosurface_geometric_normals(m.out_vertices, m.out_triangles, kept[0], kept[1], keys, s.head, s.temp, temp_bytes,
                                                          mesh.alt_normals.as<float>(), ctx->stream));
    DMI_HIP(ctx, hipEventRecord(dc.events[7], ctx->stream));
  }
  dc.pending = true;
  dc.pending_normals = new_normals;
  mesh.commit_alternates(kept[0], kept[1], dmi::drops::kDecimation);
  *n_vertices = kept[0];
  *n_triangles = kept[1];
  return DMI_OK;
  });
}
}  // namespace

int dmi_decimate_isosurface(dmi_context *ctx, double cell_size, uint64_t *n_vertices, uint64_t *n_triangles) {
  return decimate_isosurface(ctx, "dmi_decimate_isosurface", cell_size, DMI_DECIMATE_MEAN, n_vertices, n_triangles);
}

int dmi_decimate_isosurface_placed(dmi_context *ctx, double cell_size, int32_t placement, uint64_t *n_vertices,
                                   uint64_t *n_triangles) {
  return decimate_isosurface(ctx, "dmi_decimate_isosurface_placed", cell_size, placement, n_vertices, n_triangles);
}

int dmi_get_isosurface_decimate_kernel_ms(dmi_context *ctx, double *last) {
  return get_value(ctx, "dmi_get_isosurface_decimate_kernel_ms", last, [](dmi_context &c) { return c.decimation.last_kernel_ms; },
                   drain_decimation);
}

int dmi_get_isosurface_decimate_pass_ms(dmi_context *ctx, double out[4]) {
  return get_passes(ctx, "dmi_get_isosurface_decimate_pass_ms", out, &dmi_context::decimation, drain_decimation);
}

int dmi_fill_isosurface_holes(dmi_context *ctx, uint64_t max_edges, uint64_t *n_vertices, uint64_t *n_triangles, uint64_t *n_filled,
                              uint64_t *boundary_edges_left) {
  return guarded(ctx, "dmi_fill_isosurface_holes", [&]() -> int {
  const std::string entry = "dmi_fill_isosurface_holes";
  if (!ctx || !n_vertices || !n_triangles) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": null argument");
  if (max_edges > (uint64_t(1) << 20))
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": max_edges " + std::to_string(max_edges) + " is not in [0, 2^20]");
  dmi_context::Mesh &mesh = ctx->mesh;
  dmi_context::Holes &ho = ctx->holes;
  dmi_context::Smoothing &sm = ctx->smoothing;
  const uint64_t nv = mesh.n_vertices, nt = mesh.n_triangles;
  int rc = require_mesh(ctx, entry);
  // ids are u32 on the device, and so are the positions among the sorted edge keys
  if (rc == DMI_OK) rc = refuse_size(ctx, entry, dmi::ids_refusal(nv, nt, "32-bit vertex ids"));
  if (rc == DMI_OK) rc = refuse_size(ctx, entry, dmi::product_refusal(6, nt, "32-bit edge positions (6 x triangles >= 2^32)"));
  if (rc == DMI_OK) rc = refuse_size(ctx, entry, dmi::direction_bit_refusal(nv));
  if (rc != DMI_OK) return rc;
  auto nothing = [&](uint64_t left) {  // the mesh, its regions, its support counts and its colours stay as they are
    ho.zero();
    *n_vertices = nv;
    *n_triangles = nt;
    if (n_filled) *n_filled = 0;
    if (boundary_edges_left) *boundary_edges_left = left;
    return DMI_OK;
  };
  if (nv == 0) return nothing(0);
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  const bool normals = mesh.has_normals;
  size_t temp_bytes = 0;
  DMI_HIP(ctx, dmi::holes_temp_bytes(nv, nt, &temp_bytes));
  temp_bytes = std::max<size_t>(temp_bytes, 16);
  const uint64_t n_keys = std::max<uint64_t>(3 * nt, 2);
  dmi::U32Lanes vp{nullptr, nv + 1};
  rc = ensure_buffers(ctx, {{&sm.keys, 2 * n_keys * 8}, {&ho.vertex_scratch, vp.bytes(dmi::kHolesLanes)}, {&ho.counters, 32}, {&sm.temp, temp_bytes}});
  if (rc != DMI_OK) return rc;
  DMI_HIP(ctx, ho.create());
  dmi::HolesMesh m{};
  m.n_vertices = nv;
  m.n_triangles = nt;
  m.vertices = mesh.vertices.as<double>();
  m.triangles = mesh.triangles.as<int64_t>();
  m.normals = normals ? mesh.normals.as<float>() : nullptr;
  dmi::HolesVertexScratch vs{};
  vp.base = ho.vertex_scratch.as<uint32_t>();
  vs.out_deg = vp.lane(0);
  vs.in_deg = vp.lane(1);
  vs.succ = vp.lane(2);
  vs.flag = vp.lane(3);
  vs.rank = vp.lane(4);
  uint64_t *const keys[2] = {sm.keys.as<uint64_t>(), sm.keys.as<uint64_t>() + n_keys};
  unsigned long long *counters = ho.counters.as<unsigned long long>();
  // (a failure from here on leaves the context's mesh as it was: no kernel writes it, and the buffers are swapped only at the end)
  DMI_HIP(ctx, dmi::launch_holes_boundary(m, vs, keys, sm.temp.ptr, temp_bytes, counters, ho.events, ctx->stream));
  uint32_t n_slots = 0;
  unsigned long long counts[4] = {0, 0, 0, 0};
  DMI_HIP(ctx, hipMemcpyAsync(&n_slots, vs.rank + nv, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  DMI_HIP(ctx, hipMemcpyAsync(counts, counters, sizeof(counts), hipMemcpyDeviceToHost, ctx->stream));
  DMI_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the first of three: the boundary vertices
  const uint64_t boundary_edges = counts[0];
  if (max_edges < 3 || n_slots == 0) return nothing(boundary_edges);
  dmi::U32Lanes lp{nullptr, (uint64_t)n_slots + 1};
  rc = ensure_buffer(ctx, ho.loop_scratch, lp.bytes(dmi::kHolesLoopLanes));
  if (rc != DMI_OK) return rc;
  dmi::HolesLoopScratch ls{};
  lp.base = ho.loop_scratch.as<uint32_t>();
  ls.id = lp.lane(0);
  ls.next = lp.lane(1);
  ls.ptr[0] = lp.lane(2);
  ls.ptr[1] = lp.lane(3);
  ls.label[0] = lp.lane(4);
  ls.label[1] = lp.lane(5);
  ls.count = lp.lane(6);
  ls.new_vertices = lp.lane(7);
  ls.new_triangles = lp.lane(8);
  ls.vertex_offset = lp.lane(9);
  ls.triangle_offset = lp.lane(10);
  DMI_HIP(ctx, dmi::launch_holes_loops(m, vs, ls, n_slots, max_edges, sm.temp.ptr, temp_bytes, counters, ho.events[2], ctx->stream));
  uint32_t added[2] = {0, 0};
  DMI_HIP(ctx, hipMemcpyAsync(&added[0], ls.vertex_offset + n_slots, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  DMI_HIP(ctx, hipMemcpyAsync(&added[1], ls.triangle_offset + n_slots, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  DMI_HIP(ctx, hipMemcpyAsync(counts, counters, sizeof(counts), hipMemcpyDeviceToHost, ctx->stream));
  DMI_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the second: what the fill adds
  if (counts[1] == 0) return nothing(boundary_edges);
  const uint64_t out_nv = nv + added[0], out_nt = nt + added[1];
  rc = refuse_size(ctx, entry, dmi::filled_refusal(out_nv, out_nt));
  if (rc != DMI_OK) return rc;
  rc = ensure_buffers(ctx, {{&mesh.alt_vertices, out_nv * kVertexBytes}, {&mesh.alt_triangles, out_nt * kTriangleBytes},
                            {&mesh.alt_normals, normals ? out_nv * kNormalBytes : 0}});
  if (rc != DMI_OK) return rc;
  dmi::HolesOutput out{};
  out.vertices = mesh.alt_vertices.as<double>();
  out.triangles = mesh.alt_triangles.as<int64_t>();
  out.normals = normals ? mesh.alt_normals.as<float>() : nullptr;
  DMI_HIP(ctx, dmi::launch_holes_fill(m, ls, n_slots, out, counters, ho.events[3], ctx->stream));
  DMI_HIP(ctx, hipMemcpyAsync(counts, counters, sizeof(counts), hipMemcpyDeviceToHost, ctx->stream));
  DMI_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the third: the filled mesh
  if (counts[3]) return fail(ctx, DMI_ERR_STATE, entry + ": a loop's walk did not close (the mesh is left as it was)");
  DMI_HIP(ctx, ho.read(0, 3));
  mesh.commit_alternates(out_nv, out_nt, dmi::drops::kFill);
  *n_vertices = out_nv;
  *n_triangles = out_nt;
  if (n_filled) *n_filled = counts[1];
  if (boundary_edges_left) *boundary_edges_left = boundary_edges - counts[2];
  return DMI_OK;
  });
}

int dmi_get_isosurface_holes_kernel_ms(dmi_context *ctx, double *last) {
  return get_value(ctx, "dmi_get_isosurface_holes_kernel_ms", last, [](dmi_context &c) { return c.holes.last_kernel_ms; });
}

int dmi_get_isosurface_holes_pass_ms(dmi_context *ctx, double out[3]) {
  return get_passes(ctx, "dmi_get_isosurface_holes_pass_ms", out, &dmi_context::holes);
}

int dmi_filter_isosurface_support(dmi_context *ctx, int32_t min_views, double tolerance, int32_t require_facing, uint64_t *n_vertices,
                                  uint64_t *n_triangles) {
  return guarded(ctx, "dmi_filter_isosurface_support", [&]() -> int {
  const std::string entry = "dmi_filter_isosurface_support";
  if (!ctx || !n_vertices || !n_triangles) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": null argument");
  if (min_views < 0) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": min_views " + std::to_string(min_views) + " is negative");
  if (!(tolerance >= 0.0 && tolerance <= 1.7976931348623157e308))  // NaN, negative, infinite
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": the tolerance must be finite and >= 0");
  dmi_context::Mesh &mesh = ctx->mesh;
  dmi_context::Support &sup = ctx->support;
  int rc = require_mesh(ctx, entry);
  if (rc != DMI_OK) return rc;
  const bool facing = require_facing != 0;
  if (facing && !mesh.has_normals)
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": require_facing needs the mesh's normals (dmi_extract_isosurface_normals)");
  const uint64_t nv = mesh.n_vertices, nt = mesh.n_triangles;
  rc = refuse_size(ctx, entry, dmi::ids_refusal(nv, nt, "32-bit vertex ids"));  // the maps of the compaction are u32
  if (rc != DMI_OK) return rc;
  const size_t n_views = ctx->views.h_maps.size();
  if (n_views == 0) return fail(ctx, DMI_ERR_STATE, entry + ": no views resident (call dmi_add_views first)");
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  if (nv == 0) {  // an empty mesh stays empty, and its counts are empty
    mesh.support_counted = true;
    sup.zero();
    *n_vertices = 0;
    *n_triangles = nt;
    return DMI_OK;
  }
  const bool trim = min_views > 0;  // 0: the counts only
  const bool normals = mesh.has_normals;
  size_t temp_bytes = 0;
  if (trim) {
    DMI_HIP(ctx, dmi::support_scan_temp_bytes(nv, nt, &temp_bytes));
    temp_bytes = std::max<size_t>(temp_bytes, 16);
  }
  // the counts and the views' records; for a trim also the result's buffers (the component filter's alternates), the compacted
  // counts, the per-vertex and per-triangle u32 arrays and the scans' own storage
  dmi::U32Lanes vs{nullptr, nv + 1};
  rc = ensure_buffers(ctx, {{&sup.work, nv * 4}, {&sup.maps, (uint64_t)n_views * sizeof(dmi::MapRec)},
                            {&mesh.alt_vertices, trim ? nv * kVertexBytes : 0},
                            {&mesh.alt_triangles, trim ? std::max<uint64_t>(nt, 1) * kTriangleBytes : 0},
                            {&mesh.alt_normals, trim && normals ? nv * kNormalBytes : 0}, {&sup.compacted, trim ? nv * 4 : 0},
                            {&sup.vertex_scratch, trim ? vs.bytes(dmi::kSupportLanes) : 0}, {&sup.triangle_scratch, trim ? (nt + 1) * 4 : 0},
                            {&sup.scan_temp, trim ? temp_bytes : 0}});
  if (rc != DMI_OK) return rc;
  DMI_HIP(ctx, sup.create());
  dmi::SupportMesh m{};
  m.n_vertices = nv;
  m.n_triangles = nt;
  m.vertices = mesh.vertices.as<double>();
  m.normals = normals ? mesh.normals.as<float>() : nullptr;
  m.triangles = mesh.triangles.as<int64_t>();
  m.out_vertices = mesh.alt_vertices.as<double>();
  m.out_normals = mesh.alt_normals.as<float>();
  m.out_triangles = mesh.alt_triangles.as<int64_t>();
  dmi::SupportViews views{};
  views.maps = sup.maps.as<dmi::MapRec>();
  views.n_views = (int)n_views;
  views.W = ctx->views.W;
  views.H = ctx->views.H;
  views.depth_is_f64 = ctx->views.depth_f64 ? 1 : 0;
  dmi::SupportScratch s{};
  s.support = sup.work.as<int32_t>();
  s.out_support = sup.compacted.as<int32_t>();
  vs.base = sup.vertex_scratch.as<uint32_t>();
  s.mark = vs.lane(0);
  s.vmap = trim ? vs.lane(1) : nullptr;
  s.tmap = sup.triangle_scratch.as<uint32_t>();
  s.scan_temp = sup.scan_temp.ptr;
  s.scan_temp_bytes = temp_bytes;
  // (a failure from here on leaves the context's mesh, its normals, regions, colours and counts as they were: no kernel writes
  // them, and the buffers are swapped only at the end)
  // The records as they are now (h_maps is pageable: the copy is complete for the host when the call returns).  Not ctx->views.maps:
  // that array is brought up to date only by a fusion (sync_maps in dmi_capi_fuse.hip, with the tiled kernel's records and the hit
  // counters), so it lags behind views added since, and bringing it up to date from here would tie this call to the fusion's
  // bookkeeping; 208 B a view per call is the price.
  DMI_HIP(ctx, hipMemcpyAsync(sup.maps.ptr, ctx->views.h_maps.data(), n_views * sizeof(dmi::MapRec), hipMemcpyHostToDevice, ctx->stream));
  DMI_HIP(ctx, dmi::launch_isosurface_support_counts(m, views, tolerance, facing ? 1 : 0, s, sup.events, ctx->stream));
  uint32_t kept[2] = {(uint32_t)nv, (uint32_t)nt};
  if (trim) {
    DMI_HIP(ctx, dmi::launch_isosurface_support_filter(m, min_views, s, sup.events, ctx->stream));
    DMI_HIP(ctx, hipMemcpyAsync(&kept[0], s.vmap + nv, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    DMI_HIP(ctx, hipMemcpyAsync(&kept[1], s.tmap + nt, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  }
  DMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int n_passes = trim ? 3 : 1;
  DMI_HIP(ctx, sup.read(0, n_passes, n_passes));
  if (kept[0] != nv || kept[1] != nt) {  // the compacted mesh becomes the context's, and its counts with it
    mesh.commit_alternates(kept[0], kept[1], dmi::drops::kSupportTrim);
    std::swap(sup.counts, sup.compacted);
  } else {  // nothing went: the mesh, its regions and its colours stay
    std::swap(sup.counts, sup.work);
  }
  mesh.support_counted = true;
  *n_vertices = kept[0];
  *n_triangles = kept[1];
  return DMI_OK;
  });
}

int dmi_download_isosurface_support(dmi_context *ctx, int32_t *support) {
  return guarded(ctx, "dmi_download_isosurface_support", [&]() -> int {
  if (!ctx || !support) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_download_isosurface_support: null argument");
  const dmi_context::Mesh &mesh = ctx->mesh;
  if (int rc = require_mesh(ctx, "dmi_download_isosurface_support")) return rc;
  if (!mesh.support_counted)
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT,
                "dmi_download_isosurface_support: no counts (dmi_filter_isosurface_support has not run since the mesh last changed)");
  return download(ctx, {{support, ctx->support.counts, mesh.n_vertices * 4}});
  });
}

int dmi_get_isosurface_support_kernel_ms(dmi_context *ctx, double *last) {
  return get_value(ctx, "dmi_get_isosurface_support_kernel_ms", last, [](dmi_context &c) { return c.support.last_kernel_ms; });
}

int dmi_get_isosurface_support_pass_ms(dmi_context *ctx, double out[3]) {
  return get_passes(ctx, "dmi_get_isosurface_support_pass_ms", out, &dmi_context::support);
}

int dmi_color_process_isosurface(dmi_color_context *c, dmi_context *ctx, int32_t fused_depth_test, double tolerance, uint64_t *n_vertices) {
  return guarded(ctx, "dmi_color_process_isosurface", [&]() -> int {
  const std::string entry = "dmi_color_process_isosurface";
  if (!c || !ctx || !n_vertices) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": null argument");
  dmi_context::Mesh &mesh = ctx->mesh;
  dmi::StageTimes<1> &col = ctx->coloration;
  if (int rc = require_mesh(ctx, entry)) return rc;
  const dmi::ColorContextShape views = dmi::color_context_shape(c);
  if (views.device != ctx->opt.device)
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": the colour context is on device " + std::to_string(views.device) + ", the mesh on device " +
                                                   std::to_string(ctx->opt.device));
  const bool fused = fused_depth_test != 0;
  if (fused) {
    if (!(tolerance >= 0.0 && tolerance <= 1.7976931348623157e308))  // NaN, negative, infinite
      return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": the tolerance must be finite and >= 0");
    if (views.depth_test)
      return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": the colour context's own depth test is on (dmi_color_set_depth_test); one test at a time");
    if (views.n_views > 0 && ((int64_t)ctx->views.h_maps.size() != views.n_views || ctx->views.W != views.W || ctx->views.H != views.H))
      return fail(ctx, DMI_ERR_INVALID_ARGUMENT,
                  entry + ": the fused test needs the same views in both contexts: " + std::to_string(ctx->views.h_maps.size()) + " of " +
                      std::to_string(ctx->views.W) + " x " + std::to_string(ctx->views.H) + " here, " + std::to_string(views.n_views) + " of " +
                      std::to_string(views.W) + " x " + std::to_string(views.H) + " in the colour context");
  }
  if (views.n_views == 0) return fail(ctx, DMI_ERR_STATE, entry + ": no views resident in the colour context (MC.cxx:102-106)");
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  const uint64_t nv = mesh.n_vertices;
  if (nv > 0) {
    // the results are built in the alternates and swapped in last: a call that fails leaves the previous colours in place
    int rc = ensure_buffers(ctx, {{&mesh.alt_color_mean, nv * 3}, {&mesh.alt_color_median, nv * 3}, {&mesh.alt_color_count, nv * 4}});
    if (rc != DMI_OK) return rc;
    DMI_HIP(ctx, col.create(hipEventDisableTiming));
    // whatever is still queued on this context's stream (a decimation's normals) comes first
    DMI_HIP(ctx, hipEventRecord(col.events[0], ctx->stream));
    std::vector<const void *> tables;
    if (fused)
      for (const dmi::MapRec &r : ctx->views.h_maps) tables.push_back(r.depth);
    dmi::DeviceColoring work{};
    work.points = mesh.vertices.as<double>();
    work.n = (int64_t)nv;
    work.mean = mesh.alt_color_mean.as<uint8_t>();
    work.median = mesh.alt_color_median.as<uint8_t>();
    work.count = mesh.alt_color_count.as<int32_t>();
    work.after = col.events[0];
    work.fused_tables = fused ? tables.data() : nullptr;
    work.fused_f64 = ctx->views.depth_f64;
    work.fused_tol = tolerance;
    double ms = 0.0;
    rc = dmi::color_device_vertices(c, work, &ms);
    if (rc != DMI_OK) return fail(ctx, rc, dmi_color_last_error());
    col.last_kernel_ms = ms;
    std::swap(mesh.color_mean, mesh.alt_color_mean);
    std::swap(mesh.color_median, mesh.alt_color_median);
    std::swap(mesh.color_count, mesh.alt_color_count);
  } else {
    col.last_kernel_ms = 0.0;  // an empty mesh has empty colours
  }
  mesh.colored = true;
  *n_vertices = nv;
  return DMI_OK;
  });
}

int dmi_color_render_isosurface_depths(dmi_color_context *c, dmi_context *ctx) {
  return guarded(ctx, "dmi_color_render_isosurface_depths", [&]() -> int {
  const std::string entry = "dmi_color_render_isosurface_depths";
  if (!c || !ctx) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": null argument");
  dmi_context::Mesh &mesh = ctx->mesh;
  dmi::StageTimes<1> &col = ctx->coloration;
  if (int rc = require_mesh(ctx, entry)) return rc;
  const dmi::ColorContextShape views = dmi::color_context_shape(c);
  if (views.device != ctx->opt.device)
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT, entry + ": the colour context is on device " + std::to_string(views.device) + ", the mesh on device " +
                                                   std::to_string(ctx->opt.device));
  if (views.n_views == 0) return fail(ctx, DMI_ERR_STATE, entry + ": no views resident in the colour context");
  DMI_HIP(ctx, hipSetDevice(ctx->opt.device));
  DMI_HIP(ctx, col.create(hipEventDisableTiming));
  // whatever is still queued on this context's stream (a decimation's normals) comes first
  DMI_HIP(ctx, hipEventRecord(col.events[0], ctx->stream));
  const int rc = dmi::color_render_device_mesh(c, mesh.vertices.as<double>(), (int64_t)mesh.n_vertices, mesh.triangles.as<int64_t>(),
                                               (int64_t)mesh.n_triangles, col.events[0]);
  if (rc != DMI_OK) return fail(ctx, rc, dmi_color_last_error());
  return DMI_OK;
  });
}

int dmi_download_isosurface_colors(dmi_context *ctx, uint8_t *mean, uint8_t *median, int32_t *count) {
  return guarded(ctx, "dmi_download_isosurface_colors", [&]() -> int {
  if (!ctx) return fail(ctx, DMI_ERR_INVALID_ARGUMENT, "dmi_download_isosurface_colors: null argument");
  const dmi_context::Mesh &mesh = ctx->mesh;
  if (int rc = require_mesh(ctx, "dmi_download_isosurface_colors")) return rc;
  if (!mesh.colored)
    return fail(ctx, DMI_ERR_INVALID_ARGUMENT,
                "dmi_download_isosurface_colors: no colours (dmi_color_process_isosurface has not run since the mesh last changed)");
  const uint64_t nv = mesh.n_vertices;
  return download(ctx, {{mean, mesh.color_mean, nv * 3}, {median, mesh.color_median, nv * 3}, {count, mesh.color_count, nv * 4}});
  });
}

int dmi_get_isosurface_color_kernel_ms(dmi_context *ctx, double *last) {
  return get_value(ctx, "dmi_get_isosurface_color_kernel_ms", last, [](dmi_context &c) { return c.coloration.last_kernel_ms; });
}

}  // extern "C"
