// dmi_capi_points_planes.hip -- dmi_fit_point_planes of include/dmi.h: the argument checks (all of them before the device is
// touched), the upload of the coordinates in pieces, the fit, the downloads asked for.  Context-free, on the scaffold of
// dmi_depth_call.h: everything the call allocates it frees before it returns.  A failure's text is dmi_last_error(NULL)'s.  The
// fit itself, dmi::run_plane_fit_points, is what dmi_views_fit_point_planes (dmi_capi_viewset.hip) runs on the set's own cloud:
// one implementation.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "dmi_context.h"
#include "dmi_depth_call.h"
#include "dmi_view_set.h"

namespace dmi {

namespace {

// what a fit holds beside the clouds; released whatever way it ends
struct PlaneFitHoldings {
  DeviceBuffer counters, keys, ids, start, sorted, neighbors, temp, plane_rms;
  hipEvent_t events[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  hipStream_t stream;
  uint64_t &held;
  PlaneFitHoldings(hipStream_t stream_, uint64_t &held_) : stream(stream_), held(held_) {}
  ~PlaneFitHoldings() {
    (void)hipStreamSynchronize(stream);
    free_buffers({&counters, &keys, &ids, &start, &sorted, &neighbors, &temp, &plane_rms}, held);
    destroy_events(events);
  }
};

}  // namespace

const char *plane_fit_refusal(double radius, int32_t min_neighbors, int32_t flags) {
  if (!radius_rules::radius_accepted(radius)) return "radius must be finite and > 0, and its square a normal number";
  planes_rules::Lattice lattice;
  if (!planes_rules::lattice_of(radius, &lattice)) return "radius: 2^15 over its power of two and the inverse must be normal numbers";
  if (min_neighbors < 2) return "min_neighbors >= 2 required";
  if (flags < 1 || flags > (int32_t)(planes_rules::kMove | planes_rules::kNormals))
    return "flags must be DMI_PLANE_FIT_MOVE, DMI_PLANE_FIT_NORMALS or both";
  return nullptr;
}

#define PLANES_HIP(call)                                                               \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess) {                                                            \
      (void)hipGetLastError();                                                         \
      *message = entry + ": " + #call + ": " + hipGetErrorString(e_);                  \
      return e_ == hipErrorOutOfMemory ? DMI_ERR_OUT_OF_MEMORY : DMI_ERR_DEVICE;       \
    }                                                                                  \
  } while (0)

int run_plane_fit_points(const std::string &entry, const double *xyz, const float *normal, uint64_t n, double radius, int32_t min_neighbors,
                         int32_t flags, uint32_t group_points, double *out_xyz, float *out_normal, hipStream_t stream, uint64_t &held,
                         PlaneFitOutcome *outcome, std::string *message) {
  namespace rr = radius_rules;
  namespace pl = planes_rules;
  PlaneFitHoldings h(stream, held);
  for (hipEvent_t &e : h.events) PLANES_HIP(hipEventCreate(&e));
  size_t temp_bytes = 0;
  PLANES_HIP(thin_temp_bytes(n, &temp_bytes));
  PLANES_HIP(grow_buffer(h.counters, kThinCounters * sizeof(unsigned long long), held));
  PLANES_HIP(grow_buffer(h.keys, 2 * (n + 1) * sizeof(uint64_t), held));
  PLANES_HIP(grow_buffer(h.ids, 2 * n * sizeof(uint32_t), held));
  PLANES_HIP(grow_buffer(h.start, (n + 1) * sizeof(uint32_t), held));
  PLANES_HIP(grow_buffer(h.sorted, 24 * n, held));
  PLANES_HIP(grow_buffer(h.neighbors, 4 * n, held));
  PLANES_HIP(grow_buffer(h.plane_rms, 4 * n, held));
  PLANES_HIP(grow_buffer(h.temp, temp_bytes, held));
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

  // bounds: the first synchronisation lets the host refuse or derive the cells, as the radius count does
  unsigned long long c[kThinCounters];
  ThinCloud bounds_of{};
  bounds_of.xyz = xyz;
  bounds_of.n = n;
  PLANES_HIP(hipEventRecord(h.events[0], stream));
  PLANES_HIP(launch_thin_bounds(bounds_of, s.counters, stream));
  PLANES_HIP(hipEventRecord(h.events[1], stream));
  PLANES_HIP(hipMemcpyAsync(c, s.counters, sizeof(c), hipMemcpyDeviceToHost, stream));
  PLANES_HIP(hipStreamSynchronize(stream));
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

  pl::Lattice lattice;
  (void)pl::lattice_of(radius, &lattice);  // (accepted by plane_fit_refusal)
  PlaneFitArgs args{};
  args.r2 = radius * radius;
  args.s = lattice.s;
  args.inv_s = lattice.inv_s;
  args.min_neighbors = (uint32_t)min_neighbors;
  args.flags = (uint32_t)flags;
  args.normal = normal;
  args.out_xyz = (flags & (int32_t)pl::kMove) ? out_xyz : nullptr;
  args.out_normal = (flags & (int32_t)pl::kNormals) ? out_normal : nullptr;
  args.plane_rms = h.plane_rms.as<float>();
  PLANES_HIP(launch_plane_fit(xyz, n, g, args, group_points, s, h.events + 2, stream));
  PLANES_HIP(hipMemcpyAsync(c, s.counters, sizeof(c), hipMemcpyDeviceToHost, stream));
  PLANES_HIP(hipStreamSynchronize(stream));
  if (c[kRadiusUnits] < 1 || c[kRadiusUnits] > n || c[kPlanesFitted] + c[kPlanesCrowded] > n || c[kRadiusTests] < c[kRadiusSum] + n) {
    *message = entry + ": the counts are inconsistent";
    return DMI_ERR_STATE;
  }

  // bounds, keys, sort, ranks, permute, fit
  const int spans[6][2] = {{0, 1}, {2, 3}, {3, 4}, {4, 5}, {5, 6}, {6, 7}};
  double kernel_ms = 0.0;
  for (int p = 0; p < 6; ++p) {
    float ms = 0.f;
    PLANES_HIP(hipEventElapsedTime(&ms, h.events[spans[p][0]], h.events[spans[p][1]]));
    outcome->pass_ms[p] = (double)ms;
    kernel_ms += (double)ms;
  }
  std::swap(outcome->plane_rms, h.plane_rms);  // the caller's from here on (their bytes stay counted in `held`)
  std::swap(outcome->neighbors, h.neighbors);
  dmi_points_planes_report &r = outcome->report;
  r.points_in = n;
  r.fitted = c[kPlanesFitted];
  r.crowded = c[kPlanesCrowded];
  r.unsupported = n - r.fitted - r.crowded;
  r.max_neighbors = c[kRadiusMost];
  r.neighbor_sum = c[kRadiusSum];
  r.distance_tests = c[kRadiusTests];
  const unsigned long long shift_bits = c[kPlanesShift];
  std::memcpy(&r.max_shift, &shift_bits, sizeof(r.max_shift));
  r.kernel_ms = kernel_ms;
  return DMI_OK;
}

#undef PLANES_HIP

}  // namespace dmi

namespace {

using dmi::fail;

constexpr size_t kPieceBytes = size_t(64) << 20;  // the arrays go up and come down in pieces of this size

hipError_t copy_in_pieces(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t stream) {
  for (size_t at = 0; at < bytes; at += kPieceBytes) {
    const hipError_t e = hipMemcpyAsync(static_cast<char *>(dst) + at, static_cast<const char *>(src) + at, std::min(kPieceBytes, bytes - at),
                                        kind, stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

int fit_point_planes(const double *xyz, const float *normal, uint64_t n, double radius, int32_t min_neighbors, int32_t flags, int32_t device,
                     double *out_xyz, float *out_normal, float *out_plane_rms, uint32_t *out_neighbors, dmi_points_planes_report *r) {
  namespace pl = dmi::planes_rules;
  const std::string entry = "dmi_fit_point_planes";
  auto bad = [&](const std::string &what) { return fail(nullptr, DMI_ERR_INVALID_ARGUMENT, entry + ": " + what); };
  if (const char *what = dmi::plane_fit_refusal(radius, min_neighbors, flags)) return bad(what);
  if (n > dmi::radius_rules::kMaxPoints) return bad("P must stay below 2^32");
  const bool move = flags & (int32_t)pl::kMove, normals = flags & (int32_t)pl::kNormals;
  if (n == 0) {
    if (r) *r = dmi_points_planes_report{};
    return DMI_OK;
  }
  if (!xyz) return bad("xyz is null");
  if (move && !out_xyz) return bad("out_xyz is null and DMI_PLANE_FIT_MOVE is set");
  if (normals && !out_normal) return bad("out_normal is null and DMI_PLANE_FIT_NORMALS is set");

  struct {
    dmi::DeviceBuffer cloud, normal, moved, turned, plane_rms, neighbors;
  } b;
  dmi::CallHoldings h({&b.cloud, &b.normal, &b.moved, &b.turned, &b.plane_rms, &b.neighbors});  // (the fit has its own events)
  if (const dmi::CallFailure f = h.open(entry + ": ", device, 0); f.code != DMI_OK) return fail(nullptr, f.code, f.text);
  DMI_HIP(nullptr, dmi::grow_buffer(b.cloud, 24 * n));
  DMI_HIP(nullptr, copy_in_pieces(b.cloud.ptr, xyz, (size_t)(24 * n), hipMemcpyHostToDevice, h.stream));
  if (normal) {
    DMI_HIP(nullptr, dmi::grow_buffer(b.normal, 12 * n));
    DMI_HIP(nullptr, copy_in_pieces(b.normal.ptr, normal, (size_t)(12 * n), hipMemcpyHostToDevice, h.stream));
  }
  // the arrays the kernel writes start as copies of the input: a point without a fit keeps its bits (absent normals are zeros)
  if (move) {
    DMI_HIP(nullptr, dmi::grow_buffer(b.moved, 24 * n));
    DMI_HIP(nullptr, hipMemcpyAsync(b.moved.ptr, b.cloud.ptr, (size_t)(24 * n), hipMemcpyDeviceToDevice, h.stream));
  }
  if (normals) {
    DMI_HIP(nullptr, dmi::grow_buffer(b.turned, 12 * n));
    if (normal) DMI_HIP(nullptr, hipMemcpyAsync(b.turned.ptr, b.normal.ptr, (size_t)(12 * n), hipMemcpyDeviceToDevice, h.stream));
    else DMI_HIP(nullptr, hipMemsetAsync(b.turned.ptr, 0, (size_t)(12 * n), h.stream));
  }
  DMI_HIP(nullptr, hipStreamSynchronize(h.stream));

  dmi::PlaneFitOutcome outcome;
  std::string message;
  uint64_t held = 0;
  const int rc = dmi::run_plane_fit_points(entry, b.cloud.as<double>(), normal ? b.normal.as<float>() : nullptr, n, radius, min_neighbors, flags,
                                           dmi::radius_rules::kDefaultGroupPoints, b.moved.as<double>(), b.turned.as<float>(), h.stream, held,
                                           &outcome, &message);
  b.plane_rms = outcome.plane_rms;  // (freed with the rest)
  b.neighbors = outcome.neighbors;
  if (rc != DMI_OK) return fail(nullptr, rc, message);
  if (move) DMI_HIP(nullptr, copy_in_pieces(out_xyz, b.moved.ptr, (size_t)(24 * n), hipMemcpyDeviceToHost, h.stream));
  if (normals) DMI_HIP(nullptr, copy_in_pieces(out_normal, b.turned.ptr, (size_t)(12 * n), hipMemcpyDeviceToHost, h.stream));
  if (out_plane_rms) DMI_HIP(nullptr, copy_in_pieces(out_plane_rms, b.plane_rms.ptr, (size_t)(4 * n), hipMemcpyDeviceToHost, h.stream));
  if (out_neighbors) DMI_HIP(nullptr, copy_in_pieces(out_neighbors, b.neighbors.ptr, (size_t)(4 * n), hipMemcpyDeviceToHost, h.stream));
  DMI_HIP(nullptr, hipStreamSynchronize(h.stream));
  if (r) *r = outcome.report;
  return DMI_OK;
}

}  // namespace

extern "C" {

int dmi_fit_point_planes(const double *xyz, const float *normal, uint64_t n_points, double radius, int32_t min_neighbors, int32_t flags,
                         int32_t device, double *out_xyz, float *out_normal, float *out_plane_rms, uint32_t *out_neighbors,
                         dmi_points_planes_report *r) {
  return dmi::guarded(nullptr, "dmi_fit_point_planes", [&]() -> int {
    return fit_point_planes(xyz, normal, n_points, radius, min_neighbors, flags, device, out_xyz, out_normal, out_plane_rms, out_neighbors, r);
  });
}

}  // extern "C"
