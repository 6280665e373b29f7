// dmi_capi_bounds.hip -- dmi_estimate_scene_bounds of include/dmi.h: the argument checks (all of them before the device is touched),
// the staged upload into resident planes (8g's upload pass), the count and select launches of scene_bounds.hip and one download of
// the result.  Context-free, on the scaffold of dmi_depth_call.h: everything the call allocates it frees before it returns.  A
// failure's text is dmi_last_error(NULL)'s.
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "dmi_context.h"
#include "dmi_depth_call.h"
#include "dmi_view_set.h"
#include "scene_bounds.h"

namespace {

using dmi::fail;

#ifdef DMI_TUNING
double g_last_plain_read_ms = 0.0, g_last_select_ms = 0.0;
#endif

int estimate(const double *depth, const double *best_cost, double threshold, const double *K4, const double *RT4, int32_t n, int32_t W,
             int32_t H, const double *axes9, double trim_fraction, int32_t pixel_step, int32_t device, double lo[3], double hi[3],
             uint64_t *n_points, double *kernel_ms) {
  const std::string entry = "dmi_estimate_scene_bounds: ";
  auto bad = [&](const std::string &what) { return fail(nullptr, DMI_ERR_INVALID_ARGUMENT, entry + what); };
  if (!depth) return bad("depth is null");
  if (!K4) return bad("K4 is null");
  if (!RT4) return bad("RT4 is null");
  if (!lo) return bad("lo is null");
  if (!hi) return bad("hi is null");
  if (!n_points) return bad("n_points is null");
  if (const char *what = dmi::size_refusal(n, W, H)) return bad(what);
  if ((uint64_t)n * (uint64_t)W * (uint64_t)H >= (uint64_t(1) << 53)) return bad("n * W * H must stay below 2^53");
  if (!(trim_fraction >= 0.0 && trim_fraction <= 0.5)) return bad("trim_fraction must lie in [0, 0.5]");  // false for NaN
  if (pixel_step < 1) return bad("pixel_step >= 1 required");
  if (best_cost && threshold != threshold) return bad("threshold is NaN");
  dmi::BoundsAxes axes;
  if (!dmi::bounds_axes(axes9, &axes)) return bad("axes9 holds a value that is not finite");
  if (const int32_t m = dmi::first_view_with_other_k(K4, n); m >= 0) return bad(dmi::other_k_message(m));

  // what the call holds on the device; the two events stand around whatever pass is being timed
  struct {
    dmi::DeviceBuffer planes, cameras, stage_depth, stage_cost, state, hist;
  } b;
  dmi::CallHoldings h({&b.planes, &b.cameras, &b.stage_depth, &b.stage_cost, &b.state, &b.hist});
  if (const dmi::CallFailure f = h.open(entry, device, 2, true); f.code != DMI_OK) return fail(nullptr, f.code, f.text);
  const int compute_units = h.compute_units;
  const dmi::BoundsTuning tuning = dmi::bounds_tuning_from_environment();
  const size_t plane = (size_t)W * H, views = (size_t)n;
  const size_t chunk = dmi::staged_views(plane * sizeof(double), views);
  constexpr size_t kHistBytes = sizeof(unsigned long long) * dmi::bounds_rules::kTargets * dmi::bounds_rules::kBins;
  DMI_HIP(nullptr, dmi::grow_buffer(b.planes, views * plane * sizeof(double)));
  DMI_HIP(nullptr, dmi::grow_buffer(b.cameras, views * sizeof(dmi::ConsistencyCamera)));
  DMI_HIP(nullptr, dmi::grow_buffer(b.stage_depth, chunk * plane * sizeof(double)));
  if (best_cost) DMI_HIP(nullptr, dmi::grow_buffer(b.stage_cost, chunk * plane * sizeof(double)));
  DMI_HIP(nullptr, dmi::grow_buffer(b.state, sizeof(dmi::BoundsState)));
  DMI_HIP(nullptr, dmi::grow_buffer(b.hist, kHistBytes));

  double total_ms = 0.0;
  DMI_HIP(nullptr, dmi::upload_cameras(b.cameras, K4, RT4, views, h.stream));
  DMI_HIP(nullptr, hipMemsetAsync(b.state.ptr, 0, sizeof(dmi::BoundsState), h.stream));
  DMI_HIP(nullptr, hipMemsetAsync(b.hist.ptr, 0, kHistBytes, h.stream));
  DMI_HIP(nullptr, dmi::upload_flipped(depth, best_cost, threshold, W, H, views, chunk, b.stage_depth, b.stage_cost, b.planes.as<double>(), h.stream,
                                       h.events, &total_ms));

  // the select: count and select, pass after pass, with no host round trip in between
  dmi::BoundsState result;
  DMI_HIP(nullptr, dmi::run_bounds_select(b.planes.as<double>(), b.cameras.as<dmi::ConsistencyCamera>(), n, W, H, pixel_step, axes, trim_fraction,
                                          b.state.as<dmi::BoundsState>(), b.hist.as<unsigned long long>(), compute_units, tuning, h.stream,
                                          h.events, &result));
  DMI_HIP(nullptr, dmi::add_spans(h.events, 1, &total_ms));
#ifdef DMI_TUNING
  {
    float ms = 0.f;
    DMI_HIP(nullptr, hipEventElapsedTime(&ms, h.events[0], h.events[1]));
    g_last_select_ms = (double)ms;
    // the yardstick: one plain read of the same planes (the stage buffer serves as the sink)
    const unsigned read_blocks = (unsigned)std::min<size_t>((views * plane + 255) / 256, (size_t)std::max(compute_units, 1) * 8);
    for (int round = 0; round < 2; ++round) {  // the second one is the measurement
      DMI_HIP(nullptr, hipEventRecord(h.events[0], h.stream));
      DMI_HIP(nullptr, dmi::launch_bounds_plain_read(b.planes.as<double>(), (int64_t)(views * plane), b.stage_depth.as<double>(), read_blocks,
                                                     h.stream));
      DMI_HIP(nullptr, hipEventRecord(h.events[1], h.stream));
      DMI_HIP(nullptr, hipStreamSynchronize(h.stream));
    }
    DMI_HIP(nullptr, hipEventElapsedTime(&ms, h.events[0], h.events[1]));
    g_last_plain_read_ms = (double)ms;
  }
#endif
  for (int a = 0; a < 3; ++a) {
    lo[a] = result.result[2 * a];
    hi[a] = result.result[2 * a + 1];
  }
  *n_points = result.n;
  if (kernel_ms) *kernel_ms = total_ms;
  return DMI_OK;
}

}  // namespace

namespace dmi {

bool bounds_axes(const double *axes9, BoundsAxes *out) {
  *out = BoundsAxes{{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}};
  if (axes9)
    for (int q = 0; q < 9; ++q) {
      if (!std::isfinite(axes9[q])) return false;
      out->a[q] = axes9[q];
    }
  return true;
}

BoundsTuning bounds_tuning_from_environment() {
  BoundsTuning tuning;
#ifdef DMI_TUNING
  if (const char *v = getenv("DMI_SB_AGGREGATE_ROUNDS")) tuning.aggregate_rounds = atoi(v);
  if (const char *v = getenv("DMI_SB_SHARE_HISTOGRAMS")) tuning.share_histograms = atoi(v);
#endif
  return tuning;
}

// The select on the n resident planes (image row order; state and hist zeroed): count and select, pass after pass, with no host
// round trip in between, between two events; then the state comes down and the stream is synchronised.  What
// dmi_estimate_scene_bounds runs behind its upload passes, and the resident view set (dmi_capi_viewset.hip) on the planes it has
// flipped.
hipError_t run_bounds_select(const double *planes, const ConsistencyCamera *cameras, int32_t n, int32_t W, int32_t H, int32_t pixel_step,
                             const BoundsAxes &axes, double trim_fraction, BoundsState *state, unsigned long long *hist, int compute_units,
                             const BoundsTuning &tuning, hipStream_t stream, hipEvent_t events[2], BoundsState *result) {
  const unsigned blocks = bounds_count_blocks(n, W, H, pixel_step, compute_units);
  hipError_t e = hipEventRecord(events[0], stream);
  for (int pass = 0; e == hipSuccess && pass < bounds_rules::kPasses; ++pass) {
    e = launch_bounds_count(planes, cameras, n, W, H, pixel_step, axes, pass, state, hist, blocks, tuning, stream);
    if (e == hipSuccess) e = launch_bounds_select(state, hist, pass, trim_fraction, stream);
  }
  if (e == hipSuccess) e = hipEventRecord(events[1], stream);
  if (e == hipSuccess) e = hipMemcpyAsync(result, state, sizeof(*result), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  return e;
}

}  // namespace dmi

extern "C" {

int dmi_estimate_scene_bounds(const double *depth, const double *best_cost, double threshold, const double *K4, const double *RT4,
                              int32_t n, int32_t W, int32_t H, const double *axes9, double trim_fraction, int32_t pixel_step,
                              int32_t device, double lo[3], double hi[3], uint64_t *n_points, double *kernel_ms) {
  return dmi::guarded(nullptr, "dmi_estimate_scene_bounds", [&]() -> int {
    return estimate(depth, best_cost, threshold, K4, RT4, n, W, H, axes9, trim_fraction, pixel_step, device, lo, hi, n_points,
                    kernel_ms);
  });
}

#ifdef DMI_TUNING
// tuning builds only (tools/gpu_scene_bounds_time.py): the last call's select passes alone, and a plain read of the same planes
double dmi_tuning_scene_bounds_select_ms(void) { return g_last_select_ms; }
double dmi_tuning_scene_bounds_plain_read_ms(void) { return g_last_plain_read_ms; }
#endif

}  // extern "C"
