// dmi_capi_points_thin.hip -- dmi_thin_point_cloud of include/dmi.h: the argument checks (all of them before the device is touched),
// the upload of the host arrays in pieces, the thinning, one download of the result.  Context-free, on the scaffold of
// dmi_depth_call.h: everything the call allocates it frees before it returns.  A failure's text is dmi_last_error(NULL)'s.  The thinning itself,
// dmi::run_thin_points, is what dmi_views_thin_points (dmi_capi_viewset.hip) runs on the set's own cloud: one implementation.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>

#include "depth_points_rules.h"
#include "dmi_context.h"
#include "dmi_depth_call.h"
#include "dmi_view_set.h"

namespace dmi {

namespace {

// what a thinning holds beside the cloud; released whatever way it ends
struct ThinHoldings {
  DeviceBuffer counters, keys, ids, start, sorted, queue, temp, result;
  hipEvent_t events[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  hipStream_t stream;
  uint64_t &held;
  ThinHoldings(hipStream_t stream_, uint64_t &held_) : stream(stream_), held(held_) {}
  ~ThinHoldings() {
    (void)hipStreamSynchronize(stream);
    free_buffers({&counters, &keys, &ids, &start, &sorted, &queue, &temp, &result}, held);
    destroy_events(events);
  }
};

}  // namespace

#define THIN_HIP(call)                                                                 \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess) {                                                            \
      (void)hipGetLastError();                                                         \
      *message = entry + ": " + #call + ": " + hipGetErrorString(e_);                  \
      return e_ == hipErrorOutOfMemory ? DMI_ERR_OUT_OF_MEMORY : DMI_ERR_DEVICE;       \
    }                                                                                  \
  } while (0)

int run_thin_points(const std::string &entry, const ThinCloud &cloud, double cell_size, int32_t min_points, uint32_t wave_cell_points,
                    hipStream_t stream, uint64_t &held, ThinOutcome *outcome, std::string *message) {
  namespace tr = thin_rules;
  const uint64_t n = cloud.n;  // in [1, 2^32): the callers have seen to it
  auto refuse = [&](const std::string &what) {
    *message = entry + ": " + what;
    return DMI_ERR_INVALID_ARGUMENT;
  };
  ThinHoldings h(stream, held);
  for (hipEvent_t &e : h.events) THIN_HIP(hipEventCreate(&e));
  size_t temp_bytes = 0;
  THIN_HIP(thin_temp_bytes(n, &temp_bytes));
  const uint64_t queue_capacity = tr::wave_queue_capacity(n, wave_cell_points);
  THIN_HIP(grow_buffer(h.counters, kThinCounters * sizeof(unsigned long long), held));
  THIN_HIP(grow_buffer(h.keys, 2 * (n + 1) * sizeof(uint64_t), held));
  THIN_HIP(grow_buffer(h.ids, 2 * n * sizeof(uint32_t), held));
  THIN_HIP(grow_buffer(h.start, (n + 1) * sizeof(uint32_t), held));
  THIN_HIP(grow_buffer(h.sorted, 40 * n, held));
  THIN_HIP(grow_buffer(h.queue, queue_capacity * sizeof(uint32_t), held));
  THIN_HIP(grow_buffer(h.temp, temp_bytes, held));
  ThinScratch s{};
  s.counters = h.counters.as<unsigned long long>();
  s.keys[0] = h.keys.as<uint64_t>();
  s.keys[1] = s.keys[0] + (n + 1);
  s.ids[0] = h.ids.as<uint32_t>();
  s.ids[1] = s.ids[0] + n;
  s.start = h.start.as<uint32_t>();
  s.sorted_xyz = h.sorted.as<double>();
  s.sorted_normal = reinterpret_cast<float *>(s.sorted_xyz + 3 * n);
  s.sorted_count = reinterpret_cast<int32_t *>(s.sorted_normal + 3 * n);
  s.queue = h.queue.as<uint32_t>();
  s.queue_capacity = queue_capacity;
  s.temp = h.temp.ptr;
  s.temp_bytes = temp_bytes;

  // bounds: the first synchronisation lets the host refuse or derive the bins
  unsigned long long c[kThinCounters];
  THIN_HIP(hipEventRecord(h.events[0], stream));
  THIN_HIP(launch_thin_bounds(cloud, s.counters, stream));
  THIN_HIP(hipEventRecord(h.events[1], stream));
  THIN_HIP(hipMemcpyAsync(c, s.counters, sizeof(c), hipMemcpyDeviceToHost, stream));
  THIN_HIP(hipStreamSynchronize(stream));
  if (c[kThinNonFinite]) return refuse("the cloud has a non-finite coordinate");
  ThinGrid g{};
  g.h = cell_size;
  double extent = 0.0;
  bool too_many = false;
  for (int d = 0; d < 3; ++d) {
    g.lo[d] = thin_decode_bound(c[kThinLo + d]);
    const double hi = thin_decode_bound(c[kThinHi + d]);
    g.n[d] = tr::bins_of_top(std::floor((hi - g.lo[d]) / cell_size));
    too_many |= g.n[d] == 0;
    extent = std::max(extent, hi - g.lo[d]);
  }
  if (too_many) {
    // the smallest cell size whose quotient, as rounded, stays below 2^21 on the longest axis
    double least = extent / 2097152.0;
    while (!(std::floor(extent / least) < 2097152.0)) least = std::nextafter(least, std::numeric_limits<double>::infinity());
    char text[64];
    std::snprintf(text, sizeof(text), "%.17g", least);
    return refuse(std::string("more than 2^21 bins on an axis; the smallest acceptable cell size for this cloud is ") + text);
  }

  // keys, sort, ranks: the counts come down in one read
  ThinRanks ranks{};
  THIN_HIP(launch_thin_cells(cloud, g, (uint32_t)min_points, wave_cell_points, s, h.events + 2, &ranks, stream));
  uint32_t kept = 0;
  THIN_HIP(hipMemcpyAsync(c, s.counters, sizeof(c), hipMemcpyDeviceToHost, stream));
  THIN_HIP(hipMemcpyAsync(&kept, ranks.out_index + n, sizeof(kept), hipMemcpyDeviceToHost, stream));
  THIN_HIP(hipStreamSynchronize(stream));
  const uint64_t cells = c[kThinCells], queued = c[kThinQueued];
  if (cells < 1 || cells > n || kept > cells || queued > queue_capacity) {
    *message = entry + ": the cell counts are inconsistent";
    return DMI_ERR_STATE;
  }

  // the result at exactly the size needed, then the representatives
  tr::Layout layout;
  if (!tr::layout_of(kept, &layout)) return refuse("the points do not fit 64 bits of bytes");
  if (kept) THIN_HIP(grow_buffer(h.result, layout.bytes, held));
  THIN_HIP(hipEventRecord(h.events[6], stream));
  if (kept)
    THIN_HIP(launch_thin_representatives(cloud, s, ranks, cells, queued, wave_cell_points, layout, h.result.as<unsigned char>(), stream));
  THIN_HIP(hipEventRecord(h.events[7], stream));
  THIN_HIP(hipMemcpyAsync(c, s.counters, sizeof(c), hipMemcpyDeviceToHost, stream));
  THIN_HIP(hipStreamSynchronize(stream));

  const int spans[5][2] = {{0, 1}, {2, 3}, {3, 4}, {4, 5}, {6, 7}};
  double kernel_ms = 0.0;
  for (int p = 0; p < 5; ++p) {
    float ms = 0.f;
    THIN_HIP(hipEventElapsedTime(&ms, h.events[spans[p][0]], h.events[spans[p][1]]));
    kernel_ms += (outcome->pass_ms[p] = (double)ms);
  }
  std::swap(outcome->result, h.result);  // the caller's from here on (its bytes stay counted in `held`)
  outcome->n_out = kept;
  outcome->report.points_in = n;
  outcome->report.cells = cells;
  outcome->report.cells_kept = kept;
  outcome->report.multi_view_cells = c[kThinMultiView];
  outcome->report.largest_cell = c[kThinLargest];
  outcome->report.with_normal = c[kThinWithNormal];
  outcome->report.kernel_ms = kernel_ms;
  return DMI_OK;
}

#undef THIN_HIP

}  // namespace dmi

namespace {

using dmi::fail;

constexpr size_t kPieceBytes = size_t(64) << 20;  // host arrays go up, and come down, in pieces of this size

hipError_t copy_in_pieces(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t stream) {
  for (size_t at = 0; at < bytes; at += kPieceBytes) {
    const hipError_t e = hipMemcpyAsync(static_cast<char *>(dst) + at, static_cast<const char *>(src) + at, std::min(kPieceBytes, bytes - at),
                                        kind, stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

int thin(const double *xyz, const float *normal, const int32_t *view, const int32_t *pixel, const int32_t *count, uint64_t n,
         double cell_size, int32_t min_points, int32_t device, double *out_xyz, float *out_normal, int32_t *out_view, int32_t *out_pixel,
         int32_t *out_count, uint32_t *out_members, uint64_t *n_out, dmi_points_thin_report *r) {
  namespace pr = dmi::points_rules;
  const std::string entry = "dmi_thin_point_cloud";
  auto bad = [&](const std::string &what) { return fail(nullptr, DMI_ERR_INVALID_ARGUMENT, entry + ": " + what); };
  if (!n_out) return bad("n_out is null");
  if (!(cell_size > 0.0) || cell_size - cell_size != 0.0) return bad("cell_size is not a finite number > 0");
  if (min_points < 1) return bad("min_points >= 1 required");
  if (n > dmi::thin_rules::kMaxPoints) return bad("P must stay below 2^32");
  if (n == 0) {
    *n_out = 0;
    if (r) *r = dmi_points_thin_report{};
    return DMI_OK;
  }
  if (!xyz) return bad("xyz is null");
  if (!out_xyz || !out_normal || !out_view || !out_pixel || !out_count) return bad("an output array is null");

  struct {
    dmi::DeviceBuffer cloud, result;
  } b;
  dmi::CallHoldings h({&b.cloud, &b.result});  // (the thinning has its own events)
  if (const dmi::CallFailure f = h.open(entry + ": ", device, 0); f.code != DMI_OK) return fail(nullptr, f.code, f.text);
  pr::Layout in;
  if (!pr::layout_of(n, &in)) return bad("the points do not fit 64 bits of bytes");
  DMI_HIP(nullptr, dmi::grow_buffer(b.cloud, in.bytes));
  unsigned char *const base = b.cloud.as<unsigned char>();
  auto up = [&](const void *src, uint64_t offset, uint64_t stride) {  // an absent array is one of zeros
    return src ? copy_in_pieces(base + offset, src, (size_t)(n * stride), hipMemcpyHostToDevice, h.stream)
               : hipMemsetAsync(base + offset, 0, (size_t)(n * stride), h.stream);
  };
  DMI_HIP(nullptr, up(xyz, in.xyz, 24));
  DMI_HIP(nullptr, up(normal, in.normal, 12));
  DMI_HIP(nullptr, up(view, in.view, 4));
  DMI_HIP(nullptr, up(pixel, in.pixel, 4));
  DMI_HIP(nullptr, up(count, in.count, 4));
  DMI_HIP(nullptr, hipStreamSynchronize(h.stream));  // the host arrays may be the outputs: nothing reads them after this

  dmi::ThinCloud cloud{};
  cloud.xyz = reinterpret_cast<const double *>(base + in.xyz);
  cloud.normal = reinterpret_cast<const float *>(base + in.normal);
  cloud.view = reinterpret_cast<const int32_t *>(base + in.view);
  cloud.pixel = reinterpret_cast<const int32_t *>(base + in.pixel);
  cloud.count = reinterpret_cast<const int32_t *>(base + in.count);
  cloud.n = n;
  dmi::ThinOutcome outcome;
  std::string message;
  uint64_t held = 0;
  const int rc = dmi::run_thin_points(entry, cloud, cell_size, min_points, dmi::thin_rules::kDefaultWaveCellPoints, h.stream, held,
                                      &outcome, &message);
  b.result = outcome.result;  // (freed with the rest)
  if (rc != DMI_OK) return fail(nullptr, rc, message);

  const uint64_t q = outcome.n_out;
  dmi::thin_rules::Layout out;
  (void)dmi::thin_rules::layout_of(q, &out);
  const unsigned char *const from = b.result.as<unsigned char>();
  auto down = [&](void *dst, uint64_t offset, uint64_t stride) {
    return dst && q ? copy_in_pieces(dst, from + offset, (size_t)(q * stride), hipMemcpyDeviceToHost, h.stream) : hipSuccess;
  };
  DMI_HIP(nullptr, down(out_xyz, out.xyz, 24));
  DMI_HIP(nullptr, down(out_normal, out.normal, 12));
  DMI_HIP(nullptr, down(out_view, out.view, 4));
  DMI_HIP(nullptr, down(out_pixel, out.pixel, 4));
  DMI_HIP(nullptr, down(out_count, out.count, 4));
  DMI_HIP(nullptr, down(out_members, out.members, 4));
  DMI_HIP(nullptr, hipStreamSynchronize(h.stream));
  *n_out = q;
  if (r) *r = outcome.report;
  return DMI_OK;
}

}  // namespace

extern "C" {

int dmi_thin_point_cloud(const double *xyz, const float *normal, const int32_t *view, const int32_t *pixel, const int32_t *count,
                         uint64_t n_points, double cell_size, int32_t min_points, int32_t device, double *out_xyz, float *out_normal,
                         int32_t *out_view, int32_t *out_pixel, int32_t *out_count, uint32_t *out_members, uint64_t *n_out,
                         dmi_points_thin_report *r) {
  return dmi::guarded(nullptr, "dmi_thin_point_cloud", [&]() -> int {
    return thin(xyz, normal, view, pixel, count, n_points, cell_size, min_points, device, out_xyz, out_normal, out_view, out_pixel,
                out_count, out_members, n_out, r);
  });
}

}  // extern "C"
