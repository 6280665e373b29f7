// dmi_capi_points_radius.hip -- dmi_count_point_neighbors of include/dmi.h: the argument checks (all of them before the device is
// touched), the upload of the coordinates in pieces, the count, one download of the counts.  Context-free, on the scaffold of
// dmi_depth_call.h: everything the call allocates it frees before it returns.  A failure's text is dmi_last_error(NULL)'s.  The
// count itself, dmi::run_radius_points, is what dmi_views_filter_points_radius (dmi_capi_viewset.hip) runs on the set's own cloud,
// with the compaction behind it: one implementation.
#include <algorithm>
#include <cmath>
#include <string>

#include "dmi_context.h"
#include "dmi_depth_call.h"
#include "dmi_view_set.h"

namespace dmi {

namespace {

// what a count holds beside the cloud; released whatever way it ends
struct RadiusHoldings {
  DeviceBuffer counters, keys, ids, start, sorted, neighbors, temp, result;
  hipEvent_t events[11] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  hipStream_t stream;
  uint64_t &held;
  RadiusHoldings(hipStream_t stream_, uint64_t &held_) : stream(stream_), held(held_) {}
  ~RadiusHoldings() {
    (void)hipStreamSynchronize(stream);
    free_buffers({&counters, &keys, &ids, &start, &sorted, &neighbors, &temp, &result}, held);
    destroy_events(events);
  }
};

}  // namespace

const char *radius_refusal(double radius, int32_t min_neighbors) {
  if (!radius_rules::radius_accepted(radius)) return "radius must be finite and > 0, and its square a normal number";
  if (min_neighbors < 0) return "min_neighbors >= 0 required";
  return nullptr;
}

#define RADIUS_HIP(call)                                                               \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess) {                                                            \
      (void)hipGetLastError();                                                         \
      *message = entry + ": " + #call + ": " + hipGetErrorString(e_);                  \
      return e_ == hipErrorOutOfMemory ? DMI_ERR_OUT_OF_MEMORY : DMI_ERR_DEVICE;       \
    }                                                                                  \
  } while (0)

int run_radius_points(const std::string &entry, const RadiusCloud &cloud, double radius, int32_t min_neighbors, uint32_t group_points,
                      uint64_t bytes_per_point, hipStream_t stream, uint64_t &held, RadiusOutcome *outcome, std::string *message) {
  namespace rr = radius_rules;
  const uint64_t n = cloud.n;  // in [1, 2^32): the callers have seen to it
  RadiusHoldings h(stream, held);
  for (hipEvent_t &e : h.events) RADIUS_HIP(hipEventCreate(&e));
  size_t temp_bytes = 0;
  RADIUS_HIP(thin_temp_bytes(n, &temp_bytes));
  RADIUS_HIP(grow_buffer(h.counters, kThinCounters * sizeof(unsigned long long), held));
  RADIUS_HIP(grow_buffer(h.keys, 2 * (n + 1) * sizeof(uint64_t), held));
  RADIUS_HIP(grow_buffer(h.ids, 2 * n * sizeof(uint32_t), held));
  RADIUS_HIP(grow_buffer(h.start, (n + 1) * sizeof(uint32_t), held));
  RADIUS_HIP(grow_buffer(h.sorted, 24 * n, held));
  RADIUS_HIP(grow_buffer(h.neighbors, 4 * n, held));
  RADIUS_HIP(grow_buffer(h.temp, temp_bytes, held));
  RadiusScratch s{};
  s.counters = h.counters.as<unsigned long long>();
  s.keys[0] = h.keys.as<uint64_t>();
  s.keys[1] = s.keys[0] + (n + 1);
  s.ids[0] = h.ids.as<uint32_t>();
  s.ids[1] = s.ids[0] + n;
  s.start = h.start.as<uint32_t>();
  s.sorted_xyz = h.sorted.as<double>();
  s.neighbors = h.neighbors.as<uint32_t>();
  s.temp = h.temp.ptr;
  s.temp_bytes = temp_bytes;

  // bounds: the first synchronisation lets the host refuse or derive the cells
  unsigned long long c[kThinCounters];
  ThinCloud bounds_of{};
  bounds_of.xyz = cloud.xyz;
  bounds_of.n = n;
  RADIUS_HIP(hipEventRecord(h.events[0], stream));
  RADIUS_HIP(launch_thin_bounds(bounds_of, s.counters, stream));
  RADIUS_HIP(hipEventRecord(h.events[1], stream));
  RADIUS_HIP(hipMemcpyAsync(c, s.counters, sizeof(c), hipMemcpyDeviceToHost, stream));
  RADIUS_HIP(hipStreamSynchronize(stream));
  if (c[kThinNonFinite]) {
    *message = entry + ": the cloud has a non-finite coordinate";
    return DMI_ERR_INVALID_ARGUMENT;
  }
  RadiusGrid g{};
  double extent[3];
  for (int d = 0; d < 3; ++d) {
    g.lo[d] = thin_decode_bound(c[kThinLo + d]);
    extent[d] = thin_decode_bound(c[kThinHi + d]) - g.lo[d];
  }
  g.h = rr::cell_size_of(radius, extent);
  for (int d = 0; d < 3; ++d) g.n[d] = rr::bins_of_extent(extent[d], g.h);

  // keys, sort, units, permutation, count, flags: the counts come down in one read
  RadiusKept kept{};
  RADIUS_HIP(launch_radius_counts(cloud.xyz, n, g, radius * radius, (uint32_t)min_neighbors, group_points, s, h.events + 2, &kept, stream));
  uint32_t n_kept = 0;
  RADIUS_HIP(hipMemcpyAsync(c, s.counters, sizeof(c), hipMemcpyDeviceToHost, stream));
  RADIUS_HIP(hipMemcpyAsync(&n_kept, kept.out_index + n, sizeof(n_kept), hipMemcpyDeviceToHost, stream));
  RADIUS_HIP(hipStreamSynchronize(stream));
  if (c[kRadiusUnits] < 1 || c[kRadiusUnits] > n || n_kept > n || c[kRadiusTests] < c[kRadiusSum]) {
    *message = entry + ": the counts are inconsistent";
    return DMI_ERR_STATE;
  }

  // the kept points at exactly the size needed (a caller that compacts for itself passes bytes_per_point == 0)
  RADIUS_HIP(hipEventRecord(h.events[9], stream));
  if (bytes_per_point && n_kept) {
    thin_rules::Layout layout;
    uint64_t neighbors_offset = 0, bytes = 0;
    if (!thin_rules::layout_of(n_kept, &layout) || !rr::filtered_bytes(n_kept, bytes_per_point, &neighbors_offset, &bytes)) {
      *message = entry + ": the points do not fit 64 bits of bytes";
      return DMI_ERR_INVALID_ARGUMENT;
    }
    RADIUS_HIP(grow_buffer(h.result, bytes, held));
    RADIUS_HIP(launch_radius_compaction(cloud, kept, s.neighbors, layout, neighbors_offset, h.result.as<unsigned char>(), stream));
  }
  RADIUS_HIP(hipEventRecord(h.events[10], stream));
  RADIUS_HIP(hipStreamSynchronize(stream));

  // bounds, keys, sort, ranks, permute, count; the compaction is the flags with their scan and the scatter
  const int spans[8][2] = {{0, 1}, {2, 3}, {3, 4}, {4, 5}, {5, 6}, {6, 7}, {7, 8}, {9, 10}};
  double kernel_ms = 0.0;
  for (int p = 0; p < 7; ++p) outcome->pass_ms[p] = 0.0;
  for (int p = 0; p < 8; ++p) {
    float ms = 0.f;
    RADIUS_HIP(hipEventElapsedTime(&ms, h.events[spans[p][0]], h.events[spans[p][1]]));
    outcome->pass_ms[std::min(p, 6)] += (double)ms;
    kernel_ms += (double)ms;
  }
  std::swap(outcome->result, h.result);  // the caller's from here on (their bytes stay counted in `held`)
  if (!bytes_per_point) std::swap(outcome->neighbors, h.neighbors);
  outcome->n_kept = n_kept;
  outcome->report.points_in = n;
  outcome->report.points_kept = n_kept;
  outcome->report.isolated = c[kRadiusIsolated];
  outcome->report.max_neighbors = c[kRadiusMost];
  outcome->report.neighbor_sum = c[kRadiusSum];
  outcome->report.distance_tests = c[kRadiusTests];
  outcome->report.kernel_ms = kernel_ms;
  return DMI_OK;
}

#undef RADIUS_HIP

}  // namespace dmi

namespace {

using dmi::fail;

constexpr size_t kPieceBytes = size_t(64) << 20;  // the coordinates go up, and the counts come down, in pieces of this size

hipError_t copy_in_pieces(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t stream) {
  for (size_t at = 0; at < bytes; at += kPieceBytes) {
    const hipError_t e = hipMemcpyAsync(static_cast<char *>(dst) + at, static_cast<const char *>(src) + at, std::min(kPieceBytes, bytes - at),
                                        kind, stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

int count_neighbors(const double *xyz, uint64_t n, double radius, int32_t min_neighbors, int32_t device, uint32_t *out_neighbors,
                    uint8_t *out_keep, uint64_t *n_kept, dmi_points_radius_report *r) {
  const std::string entry = "dmi_count_point_neighbors";
  auto bad = [&](const std::string &what) { return fail(nullptr, DMI_ERR_INVALID_ARGUMENT, entry + ": " + what); };
  if (!n_kept) return bad("n_kept is null");
  if (const char *what = dmi::radius_refusal(radius, min_neighbors)) return bad(what);
  if (n > dmi::radius_rules::kMaxPoints) return bad("P must stay below 2^32");
  if (n == 0) {
    *n_kept = 0;
    if (r) *r = dmi_points_radius_report{};
    return DMI_OK;
  }
  if (!xyz) return bad("xyz is null");
  if (!out_neighbors) return bad("out_neighbors is null");

  struct {
    dmi::DeviceBuffer cloud, neighbors;
  } b;
  dmi::CallHoldings h({&b.cloud, &b.neighbors});  // (the count has its own events)
  if (const dmi::CallFailure f = h.open(entry + ": ", device, 0); f.code != DMI_OK) return fail(nullptr, f.code, f.text);
  DMI_HIP(nullptr, dmi::grow_buffer(b.cloud, 24 * n));
  DMI_HIP(nullptr, copy_in_pieces(b.cloud.ptr, xyz, (size_t)(24 * n), hipMemcpyHostToDevice, h.stream));
  DMI_HIP(nullptr, hipStreamSynchronize(h.stream));

  dmi::RadiusCloud cloud{};
  cloud.xyz = b.cloud.as<double>();
  cloud.n = n;
  dmi::RadiusOutcome outcome;
  std::string message;
  uint64_t held = 0;
  const int rc = dmi::run_radius_points(entry, cloud, radius, min_neighbors, dmi::radius_rules::kDefaultGroupPoints, 0, h.stream, held,
                                        &outcome, &message);
  b.neighbors = outcome.neighbors;  // (freed with the rest)
  if (rc != DMI_OK) return fail(nullptr, rc, message);
  DMI_HIP(nullptr, copy_in_pieces(out_neighbors, b.neighbors.ptr, (size_t)(4 * n), hipMemcpyDeviceToHost, h.stream));
  DMI_HIP(nullptr, hipStreamSynchronize(h.stream));
  if (out_keep)
    for (uint64_t i = 0; i < n; ++i) out_keep[i] = out_neighbors[i] >= (uint32_t)min_neighbors ? 1 : 0;
  *n_kept = outcome.n_kept;
  if (r) *r = outcome.report;
  return DMI_OK;
}

}  // namespace

extern "C" {

int dmi_count_point_neighbors(const double *xyz, uint64_t n_points, double radius, int32_t min_neighbors, int32_t device,
                              uint32_t *out_neighbors, uint8_t *out_keep, uint64_t *n_kept, dmi_points_radius_report *r) {
  return dmi::guarded(nullptr, "dmi_count_point_neighbors", [&]() -> int {
    return count_neighbors(xyz, n_points, radius, min_neighbors, device, out_neighbors, out_keep, n_kept, r);
  });
}

}  // extern "C"
