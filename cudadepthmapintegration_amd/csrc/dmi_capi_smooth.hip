// dmi_capi_smooth.hip -- dmi_smooth_depths and dmi_depth_smoothing_weights of include/dmi.h: the argument checks (all of them before
// the device is touched), and per piece of whole views the upload, one launch of depth_smooth.hip per iteration between two planes
// and the download.  Context-free, on the scaffold of dmi_depth_call.h: everything the call allocates it frees before it returns; the
// device holds the planes of one piece at a time.  A failure's text is dmi_last_error(NULL)'s.
#include <algorithm>
#include <string>

#include "depth_smooth.h"
#include "dmi_context.h"
#include "dmi_depth_call.h"
#include "dmi_view_set.h"

namespace {

using dmi::fail;

int smooth(const double *depth, const double *best_cost, double threshold, int32_t n, int32_t W, int32_t H, double sigma,
           double truncate, double abs_tolerance, double rel_tolerance, int32_t iterations, int32_t device, double *out_depth,
           int32_t *out_count, double *kernel_ms) {
  const std::string entry = "dmi_smooth_depths: ";
  auto bad = [&](const std::string &what) { return fail(nullptr, DMI_ERR_INVALID_ARGUMENT, entry + what); };
  if (!depth) return bad("depth is null");
  if (!out_depth) return bad("out_depth is null");
  if (const char *what = dmi::size_refusal(n, W, H)) return bad(what);
  if (!dmi::finite_and_not_negative(sigma)) return bad("sigma must be finite and >= 0");
  if (!(truncate > 0.0 && truncate <= 4.0)) return bad("truncate must lie in (0, 4]");
  int32_t radius = 0;
  double s[dmi::kDepthSmoothMaxRadius + 1];
  if (dmi::depth_smoothing_weights(sigma, truncate, &radius, s) != 0)
    return bad("the radius ceil(truncate * sigma) must not exceed " + std::to_string(dmi::kDepthSmoothMaxRadius));
  if (const char *what = dmi::tolerance_refusal(abs_tolerance, rel_tolerance)) return bad(what);
  if (iterations < 1 || iterations > dmi::kDepthSmoothMaxIterations)
    return bad("iterations must lie in [1, " + std::to_string(dmi::kDepthSmoothMaxIterations) + "]");
  if (best_cost && threshold != threshold) return bad("threshold is NaN");

  // what the call holds on the device; the events stand before the first iteration's launch and behind the last one's
  struct {
    dmi::DeviceBuffer plane[2], cost, count;
  } b;
  dmi::CallHoldings h({&b.plane[0], &b.plane[1], &b.cost, &b.count});
  if (const dmi::CallFailure f = h.open(entry, device, 2); f.code != DMI_OK) return fail(nullptr, f.code, f.text);
  const size_t plane = (size_t)W * H, views = (size_t)n;
  const size_t chunk = dmi::staged_views(plane * sizeof(double), views);
  DMI_HIP(nullptr, dmi::grow_buffer(b.plane[0], chunk * plane * sizeof(double)));
  DMI_HIP(nullptr, dmi::grow_buffer(b.plane[1], chunk * plane * sizeof(double)));
  if (best_cost) DMI_HIP(nullptr, dmi::grow_buffer(b.cost, chunk * plane * sizeof(double)));
  if (out_count) DMI_HIP(nullptr, dmi::grow_buffer(b.count, chunk * plane * sizeof(int32_t)));
  const dmi::SmoothArgs args = dmi::smooth_args(s, radius, abs_tolerance, rel_tolerance);

  double total_ms = 0.0;
  for (size_t m0 = 0; m0 < views; m0 += chunk) {
    const size_t cnt = std::min(chunk, views - m0);
    DMI_HIP(nullptr, hipMemcpyAsync(b.plane[0].ptr, depth + m0 * plane, cnt * plane * sizeof(double), hipMemcpyHostToDevice, h.stream));
    if (best_cost)
      DMI_HIP(nullptr, hipMemcpyAsync(b.cost.ptr, best_cost + m0 * plane, cnt * plane * sizeof(double), hipMemcpyHostToDevice, h.stream));
    // iteration k + 1 reads the complete output of iteration k: the two planes take turns
    const double *result = nullptr;
    DMI_HIP(nullptr, dmi::run_smooth_piece(b.plane[0].as<double>(), best_cost ? b.cost.as<double>() : nullptr, threshold, b.plane[1].as<double>(),
                                           b.plane[0].as<double>(), out_count ? b.count.as<int32_t>() : nullptr, (int64_t)cnt, W, H, args,
                                           iterations, h.stream, h.events, &result));
    DMI_HIP(nullptr, hipMemcpyAsync(out_depth + m0 * plane, result, cnt * plane * sizeof(double), hipMemcpyDeviceToHost, h.stream));
    if (out_count)
      DMI_HIP(nullptr, hipMemcpyAsync(out_count + m0 * plane, b.count.ptr, cnt * plane * sizeof(int32_t), hipMemcpyDeviceToHost, h.stream));
    DMI_HIP(nullptr, hipStreamSynchronize(h.stream));  // the planes are reused by the next piece
    DMI_HIP(nullptr, dmi::add_spans(h.events, 1, &total_ms));
  }
  if (kernel_ms) *kernel_ms = total_ms;
  return DMI_OK;
}

}  // namespace

namespace dmi {

// The smoothing on the device planes of one piece: `iterations` launches between an event before the first and one behind the last.
// The first reads src (with cost, nullable, and the threshold) and writes ping, the second reads ping and writes pong, and so on in
// turns; *result is the one the last wrote, count (nullable) the last one's taps.  pong may be src: dmi_smooth_depths alternates
// between its two planes.  The resident view set (dmi_capi_viewset.hip) keeps src as it is.
hipError_t run_smooth_piece(const double *src, const double *cost, double threshold, double *ping, double *pong, int32_t *count,
                            int64_t views, int32_t W, int32_t H, const SmoothArgs &args, int32_t iterations, hipStream_t stream,
                            hipEvent_t events[2], const double **result) {
  hipError_t e = hipEventRecord(events[0], stream);
  const double *from = src;
  for (int32_t k = 0; e == hipSuccess && k < iterations; ++k) {
    const bool first = k == 0, last = k + 1 == iterations;
    double *const to = k % 2 == 0 ? ping : pong;
    e = launch_depth_smooth(from, first ? cost : nullptr, threshold, to, last ? count : nullptr, views, W, H, args, stream);
    from = to;
  }
  if (e == hipSuccess) e = hipEventRecord(events[1], stream);
  *result = from;
  return e;
}

}  // namespace dmi

extern "C" {

int dmi_depth_smoothing_weights(double sigma, double truncate, int32_t *radius, double *weights) {
  return dmi::guarded(nullptr, "dmi_depth_smoothing_weights", [&]() -> int {
    if (dmi::depth_smoothing_weights(sigma, truncate, radius, weights) != 0)
      return fail(nullptr, DMI_ERR_INVALID_ARGUMENT,
                  "dmi_depth_smoothing_weights: sigma must be finite and >= 0, truncate finite and in (0, 4], ceil(truncate * sigma) <= 8, "
                  "and the pointers not null");
    return DMI_OK;
  });
}

int dmi_smooth_depths(const double *depth, const double *best_cost, double threshold, int32_t n, int32_t W, int32_t H, double sigma,
                      double truncate, double abs_tolerance, double rel_tolerance, int32_t iterations, int32_t device,
                      double *out_depth, int32_t *out_count, double *kernel_ms) {
  return dmi::guarded(nullptr, "dmi_smooth_depths", [&]() -> int {
    return smooth(depth, best_cost, threshold, n, W, H, sigma, truncate, abs_tolerance, rel_tolerance, iterations, device, out_depth,
                  out_count, kernel_ms);
  });
}

}  // extern "C"
