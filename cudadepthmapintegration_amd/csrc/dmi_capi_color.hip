// dmi_capi_color.hip -- the dmi_color_* C ABI of include/dmi.h over dmi_color_context (dmi_color_context.h): life cycle, views,
// settings and getters; the host driver of a colouring call (process_vertices: dmi_color_process stages host arrays,
// dmi::color_device_vertices colours device arrays in place); the host driver of the rasteriser that renders the depth planes of
// the visibility test (mesh_depth_render.hip; DESIGN.md 8b'').  The kernels are coloration_kernels.hip's.
#include "dmi_color_context.h"

#include <stdlib.h>

#include <algorithm>
#include <cmath>

using dmi::color_plane_texels;

namespace {

thread_local std::string g_color_error;

int cfail(dmi_color_context *c, int code, const std::string &msg) {
  g_color_error = msg;
  if (c) c->err = msg;
  return code;
}

// no C++ exception may cross the C ABI
template <typename Body>
int guarded(dmi_color_context *c, const char *entry, Body &&body) noexcept {
  return dmi::guarded_by(&cfail, c, entry, static_cast<Body &&>(body));
}

#define DMI_COLOR_HIP(c, call)                                                                               \
  do {                                                                                                       \
    hipError_t e_ = (call);                                                                                  \
    if (e_ != hipSuccess) {                                                                                  \
      (void)hipGetLastError();                                                                               \
      return cfail(c, e_ == hipErrorOutOfMemory ? DMI_ERR_OUT_OF_MEMORY : DMI_ERR_DEVICE,                    \
                   std::string(#call) + ": " + hipGetErrorString(e_));                                       \
    }                                                                                                        \
  } while (0)

// dmi::grow_buffer for buffers of this context, in order up to the first failure: when any of them has to be replaced, the
// streams that may still be using it (`drain`) are synchronised first -- and only then.
hipError_t grow(std::initializer_list<dmi::BufferNeed> needs, std::initializer_list<hipStream_t> drain) {
  auto kept = [](const dmi::BufferNeed &n) { return n.bytes == 0 || dmi::holds(*n.buffer, n.bytes); };
  if (std::all_of(needs.begin(), needs.end(), kept)) return hipSuccess;
  for (hipStream_t st : drain)
    if (const hipError_t e = hipStreamSynchronize(st); e != hipSuccess) return e;
  for (const dmi::BufferNeed &n : needs)
    if (const hipError_t e = kept(n) ? hipSuccess : dmi::grow_buffer(*n.buffer, n.bytes); e != hipSuccess) return e;
  return hipSuccess;
}
int ensure(dmi_color_context *c, std::initializer_list<dmi::BufferNeed> needs, std::initializer_list<hipStream_t> drain) {
  DMI_COLOR_HIP(c, grow(needs, drain));
  return DMI_OK;
}
hipError_t ensure_stage(dmi_color_context *c, size_t bytes) { return grow({{&c->stage.buffer, bytes}}, {c->stream}); }

// n images of the context's size, `per_pixel` Src each in vtk point order -> n tiled planes at dst: at most 256 MiB at a time
// through the stage buffer, packed on the device.  *stage_failed: the error is the stage buffer's growth.
template <typename Src, typename Dst>
hipError_t upload_planes(dmi_color_context *c, const Src *src, size_t per_pixel, Dst *dst, size_t n,
                         hipError_t (*pack)(const Src *, Dst *, int, int, int64_t, hipStream_t), bool *stage_failed) {
  const int W = c->views.W, H = c->views.H;
  const size_t npix = (size_t)W * H, bytes = npix * per_pixel * sizeof(Src), plane = (size_t)color_plane_texels(W, H);
  const size_t chunk = std::min<size_t>(std::max<size_t>(1, (size_t(256) << 20) / bytes), n);
  hipError_t e = ensure_stage(c, chunk * bytes);
  *stage_failed = e != hipSuccess;
  for (size_t m0 = 0; e == hipSuccess && m0 < n; m0 += chunk) {
    const size_t cnt = std::min(chunk, n - m0);
    e = hipMemcpyAsync(c->stage.buffer.ptr, src + m0 * npix * per_pixel, cnt * bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = pack(c->stage.buffer.as<Src>(), dst + m0 * plane, W, H, (int64_t)(cnt * npix), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // the stage buffer is reused by the next chunk
  }
  return e;
}

}  // namespace

extern "C" {

const char *dmi_color_last_error(void) { return g_color_error.c_str(); }

int dmi_color_create(int32_t device, dmi_color_context **out) {
  return guarded(nullptr, "dmi_color_create", [&]() -> int {
  if (!out) return cfail(nullptr, DMI_ERR_INVALID_ARGUMENT, "dmi_color_create: null argument");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return cfail(nullptr, DMI_ERR_DEVICE, "dmi_color_create: no HIP device available");
  }
  if (device < 0 || device >= ndev) return cfail(nullptr, DMI_ERR_INVALID_ARGUMENT, "dmi_color_create: device ordinal out of range");
  dmi_color_context *c = new (std::nothrow) dmi_color_context();
  if (!c) return cfail(nullptr, DMI_ERR_OUT_OF_MEMORY, "dmi_color_create: host allocation failed");
  c->device = device;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->staging.h2d, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->staging.d2h, hipStreamNonBlocking);
  for (int b = 0; b < 2; ++b) {
    if (e == hipSuccess) e = hipEventCreate(&c->work.span[b]);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->staging.up[b], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->staging.down[b], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreate(&c->work.k0[b]);
    if (e == hipSuccess) e = hipEventCreate(&c->work.kdone[b]);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    const std::string msg = std::string("dmi_color_create: ") + hipGetErrorString(e);
    dmi_color_destroy(c);
    return cfail(nullptr, DMI_ERR_DEVICE, msg);
  }
  *out = c;
  return DMI_OK;
  });
}

void dmi_color_destroy(dmi_color_context *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  for (hipStream_t st : {c->staging.h2d, c->stream, c->staging.d2h})
    if (st) (void)hipStreamSynchronize(st);
  c->views.release(), c->visibility.release(), c->work.release(), c->staging.release(), c->order.release(), c->render.release(), c->stage.release();
  for (hipStream_t st : {c->staging.h2d, c->stream, c->staging.d2h})
    if (st) (void)hipStreamDestroy(st);
  delete c;
}

int dmi_color_add_views(dmi_color_context *c, const uint8_t *colors, const double *K4, const double *RT4, int32_t n,
                        int32_t width, int32_t height) {
  return guarded(c, "dmi_color_add_views", [&]() -> int {
  if (!c) return cfail(nullptr, DMI_ERR_INVALID_ARGUMENT, "dmi_color_add_views: null context");
  if (!colors || !K4 || !RT4) return cfail(c, DMI_ERR_INVALID_ARGUMENT, "dmi_color_add_views: null argument");
  if (n < 1 || width < 1 || height < 1 || width > 32768 || height > 32768)
    return cfail(c, DMI_ERR_INVALID_ARGUMENT, "dmi_color_add_views: n >= 1 and image dimensions in [1, 32768] required");
  if (!c->views.batches.empty() && (width != c->views.W || height != c->views.H))
    return cfail(c, DMI_ERR_INVALID_ARGUMENT, "dmi_color_add_views: every view must have the size of view 0 (MC.cxx:111)");
  DMI_COLOR_HIP(c, hipSetDevice(c->device));
  c->views.W = width;
  c->views.H = height;
  dmi_color_context::Batch b;
  b.n = n;
  const size_t plane = (size_t)color_plane_texels(width, height);  // a tiled plane: whole tiles of 8 x 4 texels
  DMI_COLOR_HIP(c, dmi::grow_buffer(b.rgba, plane * (size_t)n * sizeof(uchar4)));
  bool stage_failed = false;
  const hipError_t e = upload_planes(c, colors, 3, b.rgba.as<uchar4>(), (size_t)n, dmi::launch_pack_color, &stage_failed);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    b.release();
    if (stage_failed) return cfail(c, DMI_ERR_OUT_OF_MEMORY, std::string("hipMalloc(stage): ") + hipGetErrorString(e));
    return cfail(c, DMI_ERR_DEVICE, std::string("colour upload: ") + hipGetErrorString(e));
  }
  c->views.batches.push_back(b);
  for (int32_t m = 0; m < n; ++m) {
    dmi::ColorView v;
    for (int i = 0; i < 12; ++i) v.rt[i] = RT4[16 * (size_t)m + i];
    for (int r = 0; r < 3; ++r)
      for (int q = 0; q < 3; ++q) v.k[3 * r + q] = K4[16 * (size_t)m + 4 * r + q];
    v.color = b.rgba.as<uchar4>() + (size_t)m * plane;
    for (int r = 0; r < 3; ++r)
      for (int q = 0; q < 4; ++q) {
        double sum = 0.0, mag = 0.0;
        for (int t = 0; t < 3; ++t) {
          sum += v.k[3 * r + t] * v.rt[4 * t + q];
          mag += std::fabs(v.k[3 * r + t]) * std::fabs(v.rt[4 * t + q]);
        }
        v.p[4 * r + q] = sum;
        v.mag[4 * r + q] = mag;
      }
    c->views.h_views.push_back(v);
    c->views.h_depth_planes.push_back(nullptr);
  }
  c->views.dirty = true;
  return DMI_OK;
  });
}

int dmi_color_clear_views(dmi_color_context *c) {
  return guarded(c, "dmi_color_clear_views", [&]() -> int {
  if (!c) return DMI_ERR_INVALID_ARGUMENT;
  DMI_COLOR_HIP(c, hipSetDevice(c->device));
  DMI_COLOR_HIP(c, hipStreamSynchronize(c->stream));
  c->views.clear();
  dmi::free_buffers({&c->render.planes});  // (the rendered planes go with the views they were rendered for)
  return DMI_OK;
  });
}

int dmi_color_add_views_with_depth(dmi_color_context *c, const uint8_t *colors, const double *depths, const double *K4,
                                   const double *RT4, int32_t n, int32_t width, int32_t height) {
  return guarded(c, "dmi_color_add_views_with_depth", [&]() -> int {
  if (!c) return cfail(nullptr, DMI_ERR_INVALID_ARGUMENT, "dmi_color_add_views_with_depth: null context");
  if (!depths) return cfail(c, DMI_ERR_INVALID_ARGUMENT, "dmi_color_add_views_with_depth: null argument");
  // the colour planes and camera records exactly as dmi_color_add_views (which checks everything else) ...
  const int rc = dmi_color_add_views(c, colors, K4, RT4, n, width, height);
  if (rc != DMI_OK) return rc;
  // ... then the depth planes; on a failure the views just appended go again, so that the call adds all or nothing
  dmi_color_context::Views &v = c->views;
  dmi::DeviceBuffer planes;
  auto undo = [&](const std::string &msg) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(c->stream);
    dmi::free_buffers({&planes});
    v.batches.back().release();
    v.batches.pop_back();
    v.h_views.resize(v.h_views.size() - (size_t)n);
    v.h_depth_planes.resize(v.h_depth_planes.size() - (size_t)n);
    if (v.batches.empty()) v.W = v.H = 0;
    v.dirty = true;
    return cfail(c, DMI_ERR_DEVICE, "dmi_color_add_views_with_depth: " + msg);
  };
  const size_t plane = (size_t)color_plane_texels(width, height);
  hipError_t e = dmi::grow_buffer(planes, plane * (size_t)n * sizeof(double));
  if (e != hipSuccess) return undo(std::string("hipMalloc(depth planes): ") + hipGetErrorString(e));
  e = hipMemsetAsync(planes.ptr, 0, plane * (size_t)n * sizeof(double), c->stream);  // (the tiles' padding: never read)
  bool stage_failed = false;
  if (e == hipSuccess) e = upload_planes(c, depths, 1, planes.as<double>(), (size_t)n, dmi::launch_pack_depth, &stage_failed);
  if (e != hipSuccess) return undo(std::string("depth upload: ") + hipGetErrorString(e));
  v.batches.back().depth = planes;
  const size_t first = v.h_depth_planes.size() - (size_t)n;
  for (int32_t m = 0; m < n; ++m) v.h_depth_planes[first + (size_t)m] = planes.as<double>() + (size_t)m * plane;
  v.dirty = true;
  return DMI_OK;
  });
}

int dmi_color_set_depth_test(dmi_color_context *c, int32_t enable, double tolerance) {
  return guarded(c, "dmi_color_set_depth_test", [&]() -> int {
  if (!c) return cfail(nullptr, DMI_ERR_INVALID_ARGUMENT, "dmi_color_set_depth_test: null context");
  if (!(tolerance >= 0.0 && tolerance <= 1.7976931348623157e308))  // NaN, negative, infinite
    return cfail(c, DMI_ERR_INVALID_ARGUMENT, "dmi_color_set_depth_test: the tolerance must be finite and >= 0");
  c->visibility.depth_test = enable != 0;
  c->visibility.depth_tol = tolerance;
  return DMI_OK;
  });
}

}  // extern "C"

namespace {
// The coherence sample (coloration_kernels.h) judged: coherent when the median step is under a tenth of the median far distance.
// What the answer chooses is a loop form of the projection kernel, never a result.  rows: [samples][3][3].
bool sample_in_coherent_order(const double *rows, int64_t samples) {
  std::vector<double> near_d, far_d;
  near_d.reserve((size_t)samples);
  far_d.reserve((size_t)samples);
  auto dist2 = [&](const double *a, const double *b) {
    double s2 = 0.0;
    for (int q = 0; q < 3; ++q) {
      const double d = a[q] - b[q];
      s2 += d * d;
    }
    return std::isfinite(s2) ? s2 : 1.0e300;  // (a NaN / inf vertex: far from everything -- no NaN reaches the partial sort)
  };
  for (int64_t t = 0; t < samples; ++t) {
    near_d.push_back(dist2(rows + 9 * t, rows + 9 * t + 3));
    far_d.push_back(dist2(rows + 9 * t, rows + 9 * t + 6));
  }
  std::nth_element(near_d.begin(), near_d.begin() + near_d.size() / 2, near_d.end());
  std::nth_element(far_d.begin(), far_d.begin() + far_d.size() / 2, far_d.end());
  return near_d[near_d.size() / 2] < 0.01 * far_d[far_d.size() / 2];  // squared distances: a tenth of the distance
}
bool vertices_in_coherent_order(const double *p, int64_t n) {
  if (n < 64) return true;
  const int64_t samples = dmi::coherence_samples(n);
  std::vector<double> rows((size_t)samples * 9);
  for (int64_t t = 0; t < samples; ++t) {
    const int64_t i = dmi::coherence_row(t, n, samples);
    const int64_t from[3] = {i, i + 1, (i + n / 2) % n};
    for (int r = 0; r < 3; ++r)
      for (int q = 0; q < 3; ++q) rows[(size_t)(9 * t + 3 * r + q)] = p[3 * from[r] + q];
  }
  return sample_in_coherent_order(rows.data(), samples);
}

// One colouring call: where the vertices are and where the results go.  dmi_color_process stages the caller's host arrays chunk
// by chunk through the context's double buffers; dmi::color_device_vertices reads and writes device arrays in place, a chunk being
// an offset into them.  Both run the one chunk body below.
struct ColorJob {
  const char *entry;
  int64_t n;
  const double *h_points;  // staged form: the caller's host arrays
  uint8_t *h_mean, *h_median;
  int32_t *h_count;
  const dmi::DeviceColoring *device;  // in-place form (dmi_context.h): device arrays, the event to wait for, the fused test
  bool in_place() const { return device != nullptr; }
};

// The buffers of a chunk of `chunk` vertices; the three streams are synchronised before one in use is replaced.
int ensure_work_buffers(dmi_color_context *c, size_t chunk, size_t n_views, bool staged) {
  const std::initializer_list<hipStream_t> streams = {c->staging.h2d, c->stream, c->staging.d2h};
  dmi_color_context::Order &o = c->order;
  // the sort's temporary storage is sized for the capacity of perm, the last of the four key buffers to grow
  const bool perm_grows = !dmi::holds(o.perm, chunk * 4);
  int rc = ensure(c, {{&c->work.scratch, chunk * n_views * sizeof(uchar4)}, {&c->work.seeds, chunk * sizeof(dmi::MedianSeed)}, {&o.keys, chunk * 4},
                      {&o.keys_sorted, chunk * 4}, {&o.index, chunk * 4}, {&o.box, 6 * sizeof(unsigned long long)}, {&o.perm, chunk * 4}}, streams);
  if (perm_grows) dmi::free_buffers({&o.sort_temp});
  if (rc == DMI_OK && !o.sort_temp.ptr) {
    DMI_COLOR_HIP(c, dmi::zorder_sort_temp_bytes((size_t)(o.perm.capacity / 4), &o.sort_temp_bytes, c->stream));
    rc = ensure(c, {{&o.sort_temp, std::max<size_t>(o.sort_temp_bytes, 16)}}, {});
  }
  if (rc != DMI_OK || !staged) return rc;
  // the double buffers of the staged form: the in-place form never allocates them
  dmi_color_context::Staging &s = c->staging;
  return ensure(c, {{&s.points[0], chunk * 24}, {&s.mean[0], chunk * 3}, {&s.median[0], chunk * 3}, {&s.count[0], chunk * 4},
                    {&s.points[1], chunk * 24}, {&s.mean[1], chunk * 3}, {&s.median[1], chunk * 3}, {&s.count[1], chunk * 4}}, streams);
}

// What both forms of a colouring call run (the callers have checked their own arguments).
int process_vertices(dmi_color_context *c, const ColorJob &job) {
  const std::string entry = job.entry;
  const int64_t n_points = job.n;
  dmi_color_context::Views &v = c->views;
  dmi_color_context::Work &w = c->work;
  dmi_color_context::Staging &s = c->staging;
  const size_t n_views = v.h_views.size();
  if (n_views == 0) return cfail(c, DMI_ERR_STATE, entry + ": no views resident (MC.cxx:102-106)");
  const dmi::DeviceColoring *const dev = job.device;
  const bool fused = dev && dev->fused_tables;
  const bool own_test = c->visibility.depth_test && !fused;
  if (own_test)
    for (size_t m = 0; m < n_views; ++m)
      if (!v.h_depth_planes[m])
        return cfail(c, DMI_ERR_INVALID_ARGUMENT, entry + ": the depth test is on and view " + std::to_string(m) +
                                                      " was added without depths (dmi_color_add_views_with_depth)");
  w.last_kernel_ms = 0.0;
  if (n_points == 0) return DMI_OK;
  DMI_COLOR_HIP(c, hipSetDevice(c->device));
  // the view tables and what else is per view (no call is in flight: nothing to wait for); a table that is new is copied again
  if (!dmi::holds(v.records, n_views * sizeof(dmi::ColorView)) || !dmi::holds(v.depth_planes, n_views * sizeof(const double *))) v.dirty = true;
  if (const int rc = ensure(c, {{&v.records, n_views * sizeof(dmi::ColorView)}, {&v.depth_planes, n_views * sizeof(const double *)},
                                {&w.margins[0], n_views * sizeof(dmi::ViewMargin)}, {&w.margins[1], n_views * sizeof(dmi::ViewMargin)},
                                {&w.pmax[0], 4 * sizeof(unsigned long long)}, {&w.pmax[1], 4 * sizeof(unsigned long long)}}, {});
      rc != DMI_OK)
    return rc;
  if (v.dirty) {
    DMI_COLOR_HIP(c, hipMemcpyAsync(v.records.ptr, v.h_views.data(), n_views * sizeof(dmi::ColorView), hipMemcpyHostToDevice, c->stream));
    DMI_COLOR_HIP(c, hipMemcpyAsync(v.depth_planes.ptr, v.h_depth_planes.data(), n_views * sizeof(const double *), hipMemcpyHostToDevice,
                                    c->stream));
    DMI_COLOR_HIP(c, hipStreamSynchronize(c->stream));
    v.dirty = false;
  }
  // vertices per chunk: the scratch table [view][vertex] stays within its budget -- and a call of many vertices is cut into at
  // least four chunks, so that a chunk's copy in, its kernels and its copies out run beside its neighbours' (with the caller's
  // arrays in pinned memory, dmi_alloc_pinned, the copies are DMA transfers; from pageable memory they still are correct)
  size_t chunk = std::max<size_t>(256, w.scratch_budget / (n_views * sizeof(uchar4)) / 256 * 256);
  chunk = std::min<size_t>(chunk, ((size_t)n_points + 255) / 256 * 256);
  if ((size_t)n_points >= (size_t(1) << 18)) chunk = std::min<size_t>(chunk, std::max<size_t>(size_t(1) << 16, (((size_t)n_points + 3) / 4 + 255) / 256 * 256));
  if (const int rc = ensure_work_buffers(c, chunk, n_views, !job.in_place()); rc != DMI_OK) return rc;
  // On a failure past the first queued copy nothing may still be writing the caller's arrays when the call returns
  auto bail = [&](hipError_t he, const char *what) {
    for (hipStream_t st : {s.h2d, c->stream, s.d2h}) (void)hipStreamSynchronize(st);
    (void)hipGetLastError();
    return cfail(c, DMI_ERR_DEVICE, entry + ": " + what + ": " + hipGetErrorString(he));
  };
#define DMI_COLOR_TRY(call)                         \
  do {                                              \
    const hipError_t he_ = (call);                  \
    if (he_ != hipSuccess) return bail(he_, #call); \
  } while (0)
  bool coherent = false;
  if (job.in_place()) {
    // the vertices are as whatever is queued on their owner's stream leaves them
    if (dev->after) DMI_COLOR_TRY(hipStreamWaitEvent(c->stream, dev->after, 0));
    if (fused) {  // (only the fused form ever allocates the table)
      DMI_COLOR_TRY(grow({{&c->visibility.fused_tables, n_views * sizeof(const void *)}}, {}));
      c->visibility.h_fused_tables.assign(dev->fused_tables, dev->fused_tables + n_views);
      DMI_COLOR_TRY(hipMemcpyAsync(c->visibility.fused_tables.ptr, c->visibility.h_fused_tables.data(), n_views * sizeof(const void *),
                                   hipMemcpyHostToDevice, c->stream));
    }
    // the order-of-work decision of the staged form from the same sample, brought to the host (36 KB at the most)
    coherent = !c->order.reorder;
    if (coherent && n_points >= 64) {
      const int64_t samples = dmi::coherence_samples(n_points);
      DMI_COLOR_TRY(grow({{&c->order.sample, dmi::kCoherenceSamples * 9 * sizeof(double)}}, {}));
      double *rows = c->order.sample.as<double>();
      std::vector<double> h_rows((size_t)samples * 9);
      DMI_COLOR_TRY(dmi::launch_coherence_sample(dev->points, n_points, samples, rows, c->stream));
      DMI_COLOR_TRY(hipMemcpyAsync(h_rows.data(), rows, h_rows.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      DMI_COLOR_TRY(hipStreamSynchronize(c->stream));
      coherent = sample_in_coherent_order(h_rows.data(), samples);
    }
    DMI_COLOR_TRY(hipEventRecord(w.span[0], c->stream));
  } else {
    coherent = !c->order.reorder && vertices_in_coherent_order(job.h_points, n_points);
  }
  bool timed[2] = {false, false};
  auto collect = [&](int b) {  // the kernel time of the chunk that last used buffer set b (its kernels are known to have ended)
    if (!timed[b]) return;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, w.k0[b], w.kdone[b]) == hipSuccess) w.last_kernel_ms += ms; else (void)hipGetLastError();
    timed[b] = false;
  };
  const dmi::ZOrderBuffers zorder{c->order.box.as<unsigned long long>(), c->order.keys.as<uint32_t>(), c->order.keys_sorted.as<uint32_t>(),
                                  c->order.index.as<uint32_t>(), c->order.perm.as<uint32_t>(), c->order.sort_temp.ptr, c->order.sort_temp_bytes};
  int64_t index = 0;
  for (int64_t v0 = 0; v0 < n_points; v0 += (int64_t)chunk, ++index) {
    const int b = (int)(index & 1);
    const int64_t nv = std::min<int64_t>((int64_t)chunk, n_points - v0);
    // this chunk's vertices and outputs: an offset into the device arrays, or buffer set b
    const double *points = dev ? dev->points + 3 * v0 : s.points[b].as<double>();
    uint8_t *mean = dev ? dev->mean + 3 * v0 : s.mean[b].as<uint8_t>();
    uint8_t *median = dev ? dev->median + 3 * v0 : s.median[b].as<uint8_t>();
    int32_t *count = dev ? dev->count + v0 : s.count[b].as<int32_t>();
    if (!job.in_place()) {
      // copy in, once the kernels of the chunk before last have read this buffer set
      if (index >= 2) {
        DMI_COLOR_TRY(hipStreamWaitEvent(s.h2d, w.kdone[b], 0));
        DMI_COLOR_TRY(hipEventSynchronize(w.kdone[b]));  // (the host reads that chunk's kernel time before the events are re-recorded)
        collect(b);
      }
      DMI_COLOR_TRY(hipMemcpyAsync(s.points[b].ptr, job.h_points + 3 * v0, (size_t)nv * 24, hipMemcpyHostToDevice, s.h2d));
      DMI_COLOR_TRY(hipEventRecord(s.up[b], s.h2d));
      // kernels, once the vertices are there and the outputs of the chunk before last have left this buffer set
      DMI_COLOR_TRY(hipStreamWaitEvent(c->stream, s.up[b], 0));
      if (index >= 2) DMI_COLOR_TRY(hipStreamWaitEvent(c->stream, s.down[b], 0));
      DMI_COLOR_TRY(hipEventRecord(w.k0[b], c->stream));
    }
    DMI_COLOR_TRY(dmi::launch_chunk_margins(points, nv, v.records.as<dmi::ColorView>(), (int)n_views, w.pmax[b].as<unsigned long long>(),
                                            w.margins[b].as<dmi::ViewMargin>(), c->stream));
    const uint32_t *perm = nullptr;
    if (c->order.reorder) {
      DMI_COLOR_TRY(dmi::launch_zorder_sort(points, nv, zorder, c->stream));
      perm = zorder.perm;
    }
    bool histogram_medians = n_views <= 65535;
    // (tuning builds: extra dynamic LDS per workgroup, i.e. FEWER resident waves -- what keeping a vertex's values in LDS
    // instead of the scratch table would cost the view loop: tools/gpu_coloration_occupancy.sh)
    unsigned extra_lds = 0;
#ifdef DMI_TUNING
    if (getenv("DMI_COLOR_BITWISE_MEDIAN")) histogram_medians = false;  // A/B of the two median kernels
    if (const char *env = getenv("DMI_DEBUG_COLOR_EXTRA_LDS")) extra_lds = (unsigned)strtoul(env, nullptr, 0);
#endif
    // the projection pass with the call's depth policy: none, the context's own planes, a fusion context's tables
    dmi::ProjectArgs pa{points, nv, perm, v.records.as<dmi::ColorView>(), (int)n_views, v.W, v.H, w.scratch.as<uchar4>(), mean, count,
                        w.seeds.as<dmi::MedianSeed>(), w.margins[b].as<dmi::ViewMargin>(), histogram_medians, coherent, extra_lds,
                        dmi::ColorDepth::none, nullptr, 0.0};
    if (fused) pa.depth = dev->fused_f64 ? dmi::ColorDepth::fused_f64 : dmi::ColorDepth::fused_f32, pa.depth_tables = c->visibility.fused_tables.ptr, pa.tol = dev->fused_tol;
    else if (own_test) pa.depth = dmi::ColorDepth::planes, pa.depth_tables = v.depth_planes.ptr, pa.tol = c->visibility.depth_tol;
    DMI_COLOR_TRY(dmi::launch_project_color(pa, c->stream));
    DMI_COLOR_TRY(dmi::launch_color_median(pa.scratch, nv, (int)n_views, perm, count, histogram_medians ? pa.seeds : nullptr, median, c->stream));
    if (job.in_place()) continue;
    DMI_COLOR_TRY(hipEventRecord(w.kdone[b], c->stream));
    timed[b] = true;
    // copies out
    DMI_COLOR_TRY(hipStreamWaitEvent(s.d2h, w.kdone[b], 0));
    DMI_COLOR_TRY(hipMemcpyAsync(job.h_mean + 3 * v0, mean, (size_t)nv * 3, hipMemcpyDeviceToHost, s.d2h));
    DMI_COLOR_TRY(hipMemcpyAsync(job.h_median + 3 * v0, median, (size_t)nv * 3, hipMemcpyDeviceToHost, s.d2h));
    DMI_COLOR_TRY(hipMemcpyAsync(job.h_count + v0, count, (size_t)nv * 4, hipMemcpyDeviceToHost, s.d2h));
    DMI_COLOR_TRY(hipEventRecord(s.down[b], s.d2h));
  }
  if (job.in_place()) {
    // nothing but the chunks' kernels is on the stream between the two events: their span is the kernel time
    DMI_COLOR_TRY(hipEventRecord(w.span[1], c->stream));
    DMI_COLOR_TRY(hipStreamSynchronize(c->stream));
    float ms = 0.f;
    DMI_COLOR_TRY(hipEventElapsedTime(&ms, w.span[0], w.span[1]));
    w.last_kernel_ms = (double)ms;
  } else {
    for (hipStream_t st : {s.h2d, c->stream, s.d2h}) DMI_COLOR_TRY(hipStreamSynchronize(st));
    collect(0);
    collect(1);
  }
#undef DMI_COLOR_TRY
  return DMI_OK;
}
}  // namespace

extern "C" {

int dmi_color_process(dmi_color_context *c, const double *points, int64_t n_points, uint8_t *mean, uint8_t *median,
                      int32_t *count) {
  return guarded(c, "dmi_color_process", [&]() -> int {
  if (!c) return cfail(nullptr, DMI_ERR_INVALID_ARGUMENT, "dmi_color_process: null context");
  if (n_points < 0 || (n_points > 0 && (!points || !mean || !median || !count)))
    return cfail(c, DMI_ERR_INVALID_ARGUMENT, "dmi_color_process: null argument");
  return process_vertices(c, ColorJob{"dmi_color_process", n_points, points, mean, median, count, nullptr});
  });
}

int dmi_color_set_scratch_budget(dmi_color_context *c, uint64_t bytes) {
  return guarded(c, "dmi_color_set_scratch_budget", [&]() -> int {
  if (!c) return cfail(nullptr, DMI_ERR_INVALID_ARGUMENT, "dmi_color_set_scratch_budget: null context");
  if (bytes < 1024) return cfail(c, DMI_ERR_INVALID_ARGUMENT, "dmi_color_set_scratch_budget: at least 1024 bytes");
  c->work.scratch_budget = (size_t)bytes;
  return DMI_OK;
  });
}

int dmi_color_set_vertex_reorder(dmi_color_context *c, int32_t enable) {
  if (!c) return cfail(nullptr, DMI_ERR_INVALID_ARGUMENT, "dmi_color_set_vertex_reorder: null context");
  c->order.reorder = enable != 0;
  return DMI_OK;
}

int dmi_color_get_kernel_ms(dmi_color_context *c, double *out) {
  return guarded(c, "dmi_color_get_kernel_ms", [&]() -> int {
  if (!c || !out) return DMI_ERR_INVALID_ARGUMENT;
  *out = c->work.last_kernel_ms;
  return DMI_OK;
  });
}

int dmi_color_mesh(const double *points, int64_t n_points, const uint8_t *colors, const double *K4, const double *RT4,
                   int32_t n_views, int32_t width, int32_t height, int32_t device, uint8_t *mean, uint8_t *median,
                   int32_t *count) {
  return guarded(nullptr, "dmi_color_mesh", [&]() -> int {
  if (!points || !colors || !K4 || !RT4 || !mean || !median || !count)
    return cfail(nullptr, DMI_ERR_INVALID_ARGUMENT, "dmi_color_mesh: null argument");
  if (n_points < 0 || n_views < 1 || width < 1 || height < 1)  // MC.cxx:102-106
    return cfail(nullptr, DMI_ERR_INVALID_ARGUMENT, "dmi_color_mesh: n_points >= 0, n_views >= 1, width >= 1, height >= 1 required");
  if (n_points == 0) return DMI_OK;
  dmi_color_context *c = nullptr;
  int rc = dmi_color_create(device, &c);
  if (rc != DMI_OK) return rc;
  rc = dmi_color_add_views(c, colors, K4, RT4, n_views, width, height);
  if (rc == DMI_OK) rc = dmi_color_process(c, points, n_points, mean, median, count);
  dmi_color_destroy(c);  // g_color_error keeps the message
  return rc;
  });
}

}  // extern "C"

// ---- rendered depth planes (mesh_depth_render.hip; DESIGN.md 8b'') -------------------------------------------------------------
namespace {
// A mesh that is on the device, rendered into NEW planes for every resident view; they replace the old ones (uploaded or rendered)
// only when everything has succeeded.  `after`: an event of the mesh's owner that the context's stream waits for first.
int render_device_mesh(dmi_color_context *c, const std::string &entry, const dmi::RenderMesh &mesh, hipEvent_t after) {
  dmi_color_context::Render &r = c->render;
  const size_t n_views = c->views.h_views.size();
  if (n_views == 0) return cfail(c, DMI_ERR_STATE, entry + ": no views resident");
  DMI_COLOR_HIP(c, hipSetDevice(c->device));
  const int W = c->views.W, H = c->views.H;
  const size_t plane = (size_t)color_plane_texels(W, H);
  const size_t n_groups = (n_views + dmi::kRenderViewGroup - 1) / dmi::kRenderViewGroup;
  auto ensure_queue = [&](size_t entries) { return grow({{&r.queue, entries * sizeof(dmi::RenderPair)}}, {c->stream}); };
  uint32_t capacity = r.queue_capacity;
  DMI_COLOR_HIP(c, grow({{&r.cameras, n_views * sizeof(dmi::RenderView)}, {&r.counters, (n_groups + 1) * sizeof(uint32_t)}}, {c->stream}));
  DMI_COLOR_HIP(c, ensure_queue(capacity));
  while (r.events.size() < 2 + 3 * n_groups) {
    hipEvent_t ev = nullptr;
    DMI_COLOR_HIP(c, hipEventCreate(&ev));
    r.events.push_back(ev);
  }
  hipEvent_t *const pass_events = r.events.data(), *const span = c->work.span;
  std::vector<dmi::RenderView> cameras(n_views);
  for (size_t m = 0; m < n_views; ++m) {
    for (int i = 0; i < 12; ++i) cameras[m].rt[i] = c->views.h_views[m].rt[i];
    for (int i = 0; i < 9; ++i) cameras[m].k[i] = c->views.h_views[m].k[i];
  }
  dmi::DeviceBuffer rendered;
  DMI_COLOR_HIP(c, dmi::grow_buffer(rendered, plane * n_views * sizeof(double)));
  double *const planes = rendered.as<double>();
  // from here on a failure frees the new planes and leaves the context's as they were
  auto bail = [&](int code, const std::string &msg) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(c->stream);
    dmi::free_buffers({&rendered});
    return cfail(c, code, entry + ": " + msg);
  };
#define DMI_RENDER_TRY(call)                                                                                             \
  do {                                                                                                                   \
    const hipError_t he_ = (call);                                                                                       \
    if (he_ != hipSuccess)                                                                                               \
      return bail(he_ == hipErrorOutOfMemory ? DMI_ERR_OUT_OF_MEMORY : DMI_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(he_)); \
  } while (0)
  if (after) DMI_RENDER_TRY(hipStreamWaitEvent(c->stream, after, 0));
  DMI_RENDER_TRY(hipMemcpyAsync(r.cameras.ptr, cameras.data(), n_views * sizeof(dmi::RenderView), hipMemcpyHostToDevice, c->stream));
  // the ids, on the device, before anything is rendered
  uint32_t *const counters = r.counters.as<uint32_t>(), *const flag = counters + n_groups;
  uint32_t h_flag = 0;
  DMI_RENDER_TRY(hipMemsetAsync(flag, 0, sizeof(uint32_t), c->stream));
  DMI_RENDER_TRY(dmi::launch_render_check_ids(mesh, flag, c->stream));
  DMI_RENDER_TRY(hipMemcpyAsync(&h_flag, flag, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  DMI_RENDER_TRY(hipStreamSynchronize(c->stream));
  if (h_flag) return bail(DMI_ERR_INVALID_ARGUMENT, "a triangle names a point outside [0, " + std::to_string(mesh.n_points) + ")");
  std::vector<uint32_t> wanted(n_groups, 0);
  double total_ms = 0.0, pass_ms[3] = {0.0, 0.0, 0.0};
  auto add_span = [&](double &sum, hipEvent_t from, hipEvent_t to) -> hipError_t {
    float ms = 0.f;
    const hipError_t e = hipEventElapsedTime(&ms, from, to);
    if (e == hipSuccess) sum += (double)ms;
    return e;
  };
  bool first_round = true;
  std::vector<size_t> todo(n_groups);
  for (size_t g = 0; g < n_groups; ++g) todo[g] = g;
  while (!todo.empty()) {
    DMI_RENDER_TRY(hipEventRecord(span[0], c->stream));
    if (first_round) {
      DMI_RENDER_TRY(hipEventRecord(pass_events[0], c->stream));
      DMI_RENDER_TRY(dmi::launch_render_init(planes, (int64_t)(plane * n_views), c->stream));
      DMI_RENDER_TRY(hipEventRecord(pass_events[1], c->stream));
    }
    for (size_t g : todo) {
      const int m0 = (int)(g * dmi::kRenderViewGroup), gn = (int)std::min<size_t>(dmi::kRenderViewGroup, n_views - (size_t)m0);
      DMI_RENDER_TRY(hipEventRecord(pass_events[2 + 3 * g], c->stream));
      DMI_RENDER_TRY(dmi::launch_render_group(mesh, r.cameras.as<dmi::RenderView>(), m0, gn, W, H, planes, r.queue.as<dmi::RenderPair>(), capacity,
                                              counters + g, pass_events[3 + 3 * g], c->stream));
      DMI_RENDER_TRY(hipEventRecord(pass_events[4 + 3 * g], c->stream));
    }
    DMI_RENDER_TRY(hipEventRecord(span[1], c->stream));
    DMI_RENDER_TRY(hipMemcpyAsync(wanted.data(), counters, n_groups * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    DMI_RENDER_TRY(hipStreamSynchronize(c->stream));
    DMI_RENDER_TRY(add_span(total_ms, span[0], span[1]));
    if (first_round) DMI_RENDER_TRY(add_span(pass_ms[0], pass_events[0], pass_events[1]));
    for (size_t g : todo) {  // (a group that runs again counts again: that is what the call spent)
      DMI_RENDER_TRY(add_span(pass_ms[1], pass_events[2 + 3 * g], pass_events[3 + 3 * g]));
      DMI_RENDER_TRY(add_span(pass_ms[2], pass_events[3 + 3 * g], pass_events[4 + 3 * g]));
    }
    first_round = false;
    // a group that wanted more entries than the queue had lost pairs: the queue grows to what was counted and the group runs
    // again (a minimum over a superset of what is already in the planes: the same bits as one complete run)
    uint32_t most = 0;
    std::vector<size_t> again;
    for (size_t g : todo)
      if (wanted[g] > capacity) again.push_back(g), most = std::max(most, wanted[g]);
    todo.swap(again);
    if (!todo.empty()) {
      DMI_RENDER_TRY(ensure_queue(most));
      capacity = most;
    }
  }
#undef DMI_RENDER_TRY
  // the new planes become the context's: every view has one, the batches' uploaded planes and the last rendering's go
  for (dmi_color_context::Batch &b : c->views.batches) dmi::free_buffers({&b.depth});
  std::swap(r.planes, rendered);
  dmi::free_buffers({&rendered});
  for (size_t m = 0; m < n_views; ++m) c->views.h_depth_planes[m] = planes + m * plane;
  c->views.dirty = true;
  r.last_ms = total_ms;
  for (int q = 0; q < 3; ++q) r.last_pass_ms[q] = pass_ms[q];
  r.last_queued = 0;
  for (uint32_t n : wanted) r.last_queued += n;  // (every group's last run had room for all it wanted)
  return DMI_OK;
}
}  // namespace

int dmi::color_render_device_mesh(dmi_color_context *c, const double *points, int64_t n_points, const int64_t *triangles, int64_t n_triangles,
                                  hipEvent_t after) {
  return ::guarded(c, "dmi_color_render_isosurface_depths", [&]() -> int {
    return render_device_mesh(c, "dmi_color_render_isosurface_depths", dmi::RenderMesh{points, triangles, n_points, n_triangles}, after);
  });
}

extern "C" {

int dmi_color_render_depths(dmi_color_context *c, const double *points, int64_t n_points, const int64_t *triangles, int64_t n_triangles) {
  return guarded(c, "dmi_color_render_depths", [&]() -> int {
  const std::string entry = "dmi_color_render_depths";
  if (!c) return cfail(nullptr, DMI_ERR_INVALID_ARGUMENT, entry + ": null context");
  if (n_points < 0 || n_triangles < 0 || (n_points > 0 && !points) || (n_triangles > 0 && !triangles))
    return cfail(c, DMI_ERR_INVALID_ARGUMENT, entry + ": null argument or negative count");
  if (c->views.h_views.empty()) return cfail(c, DMI_ERR_STATE, entry + ": no views resident");
  DMI_COLOR_HIP(c, hipSetDevice(c->device));
  dmi::DeviceBuffer d_points, d_triangles;  // of this call only
  auto release = [&]() {
    (void)hipStreamSynchronize(c->stream);
    dmi::free_buffers({&d_points, &d_triangles});
  };
  // the whole mesh has to be resident (a triangle may name any point); it goes up in pieces of at most 64 MiB
  auto upload = [&](void *dst, const void *src, size_t bytes) -> hipError_t {
    const size_t piece = size_t(64) << 20;
    for (size_t off = 0; off < bytes; off += piece) {
      const hipError_t e = hipMemcpyAsync(static_cast<char *>(dst) + off, static_cast<const char *>(src) + off, std::min(piece, bytes - off),
                                          hipMemcpyHostToDevice, c->stream);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  };
  hipError_t e = grow({{&d_points, std::max<size_t>((size_t)n_points * 24, 8)}, {&d_triangles, std::max<size_t>((size_t)n_triangles * 24, 8)}}, {});
  if (e == hipSuccess) e = upload(d_points.ptr, points, (size_t)n_points * 24);
  if (e == hipSuccess) e = upload(d_triangles.ptr, triangles, (size_t)n_triangles * 24);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    release();
    return cfail(c, e == hipErrorOutOfMemory ? DMI_ERR_OUT_OF_MEMORY : DMI_ERR_DEVICE, entry + ": mesh upload: " + hipGetErrorString(e));
  }
  const int rc = render_device_mesh(c, entry, dmi::RenderMesh{d_points.as<double>(), d_triangles.as<int64_t>(), n_points, n_triangles}, nullptr);
  release();
  return rc;
  });
}

int dmi_color_download_depths(dmi_color_context *c, int32_t first, int32_t count, double *out) {
  return guarded(c, "dmi_color_download_depths", [&]() -> int {
  const std::string entry = "dmi_color_download_depths";
  if (!c) return cfail(nullptr, DMI_ERR_INVALID_ARGUMENT, entry + ": null context");
  const std::vector<const double *> &planes = c->views.h_depth_planes;
  if (first < 0 || count < 0 || (size_t)first + (size_t)count > planes.size() || (count > 0 && !out))
    return cfail(c, DMI_ERR_INVALID_ARGUMENT, entry + ": views [" + std::to_string(first) + ", " + std::to_string((int64_t)first + count) + ") of " +
                                                  std::to_string(planes.size()) + " resident, or a null argument");
  for (int32_t m = first; m < first + count; ++m)
    if (!planes[(size_t)m])
      return cfail(c, DMI_ERR_INVALID_ARGUMENT, entry + ": view " + std::to_string(m) + " has no depth plane (dmi_color_add_views_with_depth, dmi_color_render_depths)");
  if (count == 0) return DMI_OK;
  DMI_COLOR_HIP(c, hipSetDevice(c->device));
  const int W = c->views.W, H = c->views.H;
  const size_t npix = (size_t)W * H;
  const size_t chunk = std::min<size_t>(std::max<size_t>(1, (size_t(256) << 20) / (npix * sizeof(double))), (size_t)count);
  DMI_COLOR_HIP(c, ensure_stage(c, chunk * npix * sizeof(double)));
  double *stage = c->stage.buffer.as<double>();
  for (size_t m0 = 0; m0 < (size_t)count; m0 += chunk) {
    const size_t cnt = std::min(chunk, (size_t)count - m0);
    for (size_t q = 0; q < cnt; ++q) DMI_COLOR_HIP(c, dmi::launch_unpack_depth(planes[(size_t)first + m0 + q], stage + q * npix, W, H, c->stream));
    DMI_COLOR_HIP(c, hipMemcpyAsync(out + m0 * npix, stage, cnt * npix * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    DMI_COLOR_HIP(c, hipStreamSynchronize(c->stream));  // the stage buffer is reused by the next chunk
  }
  return DMI_OK;
  });
}

int dmi_color_set_render_queue_capacity(dmi_color_context *c, uint64_t entries) {
  return guarded(c, "dmi_color_set_render_queue_capacity", [&]() -> int {
  if (!c) return cfail(nullptr, DMI_ERR_INVALID_ARGUMENT, "dmi_color_set_render_queue_capacity: null context");
  if (entries < 1 || entries > 0x7fffffffull) return cfail(c, DMI_ERR_INVALID_ARGUMENT, "dmi_color_set_render_queue_capacity: 1 to 2^31 - 1 entries");
  c->render.queue_capacity = (uint32_t)entries;
  return DMI_OK;
  });
}

int dmi_color_get_render_pass_ms(dmi_color_context *c, double out[3]) {
  return guarded(c, "dmi_color_get_render_pass_ms", [&]() -> int {
  if (!c || !out) return cfail(c, DMI_ERR_INVALID_ARGUMENT, "dmi_color_get_render_pass_ms: null argument");
  for (int q = 0; q < 3; ++q) out[q] = c->render.last_pass_ms[q];
  return DMI_OK;
  });
}

int dmi_color_get_render_queued_pairs(dmi_color_context *c, uint64_t *out) {
  return guarded(c, "dmi_color_get_render_queued_pairs", [&]() -> int {
  if (!c || !out) return cfail(c, DMI_ERR_INVALID_ARGUMENT, "dmi_color_get_render_queued_pairs: null argument");
  *out = c->render.last_queued;
  return DMI_OK;
  });
}

int dmi_color_get_render_kernel_ms(dmi_color_context *c, double *last) {
  return guarded(c, "dmi_color_get_render_kernel_ms", [&]() -> int {
  if (!c || !last) return cfail(c, DMI_ERR_INVALID_ARGUMENT, "dmi_color_get_render_kernel_ms: null argument");
  *last = c->render.last_ms;
  return DMI_OK;
  });
}

}  // extern "C"

// ---- the in-place form, for the translation unit that owns the mesh (dmi_capi_mesh.hip; declared in dmi_context.h) ----
dmi::ColorContextShape dmi::color_context_shape(const dmi_color_context *c) {
  return ColorContextShape{c->device, c->views.W, c->views.H, (int64_t)c->views.h_views.size(), c->visibility.depth_test};
}

int dmi::color_device_vertices(dmi_color_context *c, const DeviceColoring &work, double *kernel_ms) {
  return ::guarded(c, "dmi_color_process_isosurface", [&]() -> int {
    const int rc = process_vertices(c, ColorJob{"dmi_color_process_isosurface", work.n, nullptr, nullptr, nullptr, nullptr, &work});
    if (rc == DMI_OK && kernel_ms) *kernel_ms = c->work.last_kernel_ms;
    return rc;
  });
}
