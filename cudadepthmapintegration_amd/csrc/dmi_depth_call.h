// dmi_depth_call.h -- what every context-free depth-map call of include/dmi.h is built on (dmi_capi_speckle.hip, dmi_capi_holes.hip,
// dmi_capi_smooth.hip, dmi_capi_consistency.hip, dmi_capi_bounds.hip, dmi_thin_point_cloud), each thing once: what a
// call holds on the device and how it is opened and released, how many views it stages at a time, the checks the calls have in
// common, the staged upload into planes in image row order, and the sum of the times between a row of events.  The resident view
// set (dmi_capi_viewset.hip) takes the checks, the camera upload, the flip of a piece and the spans from here.  Like dmi_buffer.h it
// needs nothing but the HIP runtime's names, so it runs on the CPU against the stand-in runtime (tests/cpp/depth_call_host.cpp).
// Private: never installed.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/dmi.h"
#include "depth_consistency.h"
#include "dmi_buffer.h"
#include "view_set_rules.h"

namespace dmi {

// ---- the checks the calls share; every entry point keeps the order of its own ----

inline bool finite_and_not_negative(double v) { return v >= 0.0 && v <= 1.7976931348623157e308; }  // false for NaN
inline const char *side_refusal(int32_t W, int32_t H) {  // what is wrong with the first of them that is, or null
  if (W < 1 || W > view_set_rules::kMaxSide) return "W must lie in [1, 32768]";
  if (H < 1 || H > view_set_rules::kMaxSide) return "H must lie in [1, 32768]";
  return nullptr;
}
inline const char *size_refusal(int32_t n, int32_t W, int32_t H) { return n < 1 ? "n >= 1 required" : side_refusal(W, H); }
inline const char *tolerance_refusal(double abs_tolerance, double rel_tolerance) {
  if (!finite_and_not_negative(abs_tolerance)) return "abs_tolerance must be finite and >= 0";
  if (!finite_and_not_negative(rel_tolerance)) return "rel_tolerance must be finite and >= 0";
  return nullptr;
}

// ---- the staging rule: host data goes up and comes down in pieces of whole views, as many as fit stage_bytes ----

constexpr size_t kStageBytes = (size_t)view_set_rules::kDefaultPieceBytes;  // 256 MiB
inline size_t staged_views(size_t plane_bytes, size_t views, size_t stage_bytes = kStageBytes) {
  return std::min(views, std::max<size_t>(1, stage_bytes / plane_bytes));  // a larger view goes whole
}

// ---- the times between a row of events ----

// ms[p * stride] += the time between events[p] and events[p + 1] for p < spans (stride 0: one sum).  The stream has been
// synchronised behind the last of them.
inline hipError_t add_spans(const hipEvent_t *events, int spans, double *ms, int stride = 1) {
  for (int p = 0; p < spans; ++p) {
    float span = 0.f;
    const hipError_t e = hipEventElapsedTime(&span, events[p], events[p + 1]);
    if (e != hipSuccess) return e;
    ms[p * stride] += (double)span;
  }
  return hipSuccess;
}

// ---- what a call holds ----

struct CallFailure {  // of CallHoldings::open: the entry point hands it to dmi::fail
  int code = DMI_OK;
  std::string text;
};

// The stream of a context-free call, the events that time its kernels, and the buffers it registers -- they are the entry point's
// own, named there, and outlive this object --: released whatever way the call ends.
struct CallHoldings {
  hipStream_t stream = nullptr;
  hipEvent_t events[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int compute_units = 0;  // read by open() where asked for
  explicit CallHoldings(std::initializer_list<DeviceBuffer *> buffers) : buffers_(buffers) {}
  CallHoldings(const CallHoldings &) = delete;
  CallHoldings &operator=(const CallHoldings &) = delete;
  ~CallHoldings() {
    if (stream) (void)hipStreamSynchronize(stream);
    for (DeviceBuffer *b : buffers_) free_buffers({b});
    for (hipEvent_t e : events)
      if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
  }

  // Selects the device (its ordinal checked against the number there is), creates the stream and n_events <= 5 events.  `entry`
  // stands in front of a refusal's text ("dmi_x: ").  A failure leaves what was created to the destructor.
  CallFailure open(const std::string &entry, int32_t device, int n_events, bool read_compute_units = false) {
#define DMI_OPEN_HIP(call)                                                                                                   \
  do {                                                                                                                       \
    const hipError_t e_ = (call);                                                                                            \
    if (e_ != hipSuccess) {                                                                                                  \
      (void)hipGetLastError();                                                                                               \
      return {e_ == hipErrorOutOfMemory ? DMI_ERR_OUT_OF_MEMORY : DMI_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)}; \
    }                                                                                                                        \
  } while (0)
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
      (void)hipGetLastError();
      return {DMI_ERR_DEVICE, entry + "no HIP device available"};
    }
    if (device < 0 || device >= ndev) return {DMI_ERR_INVALID_ARGUMENT, entry + "device ordinal out of range"};
    DMI_OPEN_HIP(hipSetDevice(device));
    if (read_compute_units) DMI_OPEN_HIP(hipDeviceGetAttribute(&compute_units, hipDeviceAttributeMultiprocessorCount, device));
    DMI_OPEN_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (int e = 0; e < n_events; ++e) DMI_OPEN_HIP(hipEventCreate(&events[e]));
#undef DMI_OPEN_HIP
    return {};
  }

 private:
  std::vector<DeviceBuffer *> buffers_;
};

// ---- the staged upload into planes in image row order ----

std::vector<ConsistencyCamera> consistency_cameras(const double *K4, const double *RT4, size_t views);  // dmi_capi_consistency.hip

// the cameras of `views` views into `cameras` (grown by the caller); the stream is synchronised, for the host array goes
inline hipError_t upload_cameras(const DeviceBuffer &cameras, const double *K4, const double *RT4, size_t views, hipStream_t stream) {
  const std::vector<ConsistencyCamera> host = consistency_cameras(K4, RT4, views);
  hipError_t e = hipMemcpyAsync(cameras.ptr, host.data(), views * sizeof(ConsistencyCamera), hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  return e;
}

// `count` views on the device (depth, and cost or null, in vtk point order) into planes[first ...]: threshold, validity, -1 for
// everything else and the row flip in one pass between events[0] and events[1]; waits for it -- the source may be a stage buffer
// the next piece reuses -- and adds its time to *ms
inline hipError_t flip_piece(const double *depth, const double *cost, double threshold, int W, int H, int64_t first, int64_t count,
                             double *planes, hipStream_t stream, const hipEvent_t *events, double *ms) {
  hipError_t e = hipEventRecord(events[0], stream);
  if (e == hipSuccess) e = launch_consistency_upload(depth, cost, threshold, W, H, count, planes, first, stream);
  if (e == hipSuccess) e = hipEventRecord(events[1], stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e == hipSuccess) e = add_spans(events, 1, ms);
  return e;
}

// the host's views (best_cost nullable) through the stage buffers, `chunk` views at a time, into `planes`
inline hipError_t upload_flipped(const double *depth, const double *best_cost, double threshold, int W, int H, size_t views, size_t chunk,
                                 const DeviceBuffer &stage_depth, const DeviceBuffer &stage_cost, double *planes, hipStream_t stream,
                                 const hipEvent_t *events, double *ms) {
  const size_t plane = (size_t)W * H;
  hipError_t e = hipSuccess;
  for (size_t m0 = 0; e == hipSuccess && m0 < views; m0 += chunk) {
    const size_t cnt = std::min(chunk, views - m0);
    e = hipMemcpyAsync(stage_depth.ptr, depth + m0 * plane, cnt * plane * sizeof(double), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && best_cost)
      e = hipMemcpyAsync(stage_cost.ptr, best_cost + m0 * plane, cnt * plane * sizeof(double), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess)
      e = flip_piece(stage_depth.as<double>(), best_cost ? stage_cost.as<double>() : nullptr, threshold, W, H, (int64_t)m0, (int64_t)cnt,
                     planes, stream, events, ms);
  }
  return e;
}

}  // namespace dmi
