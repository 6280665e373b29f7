// dmi_capi_consistency.hip -- dmi_filter_depth_consistency of include/dmi.h: the argument checks (all of them before the device is
// touched), the staged upload, the launches of depth_consistency.hip and the staged download.  Context-free, on the scaffold of
// dmi_depth_call.h: everything the call allocates it frees before it returns.  A failure's text is dmi_last_error(NULL)'s.
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "depth_consistency.h"
#include "dmi_context.h"
#include "dmi_depth_call.h"
#include "dmi_view_set.h"

namespace {

using dmi::fail;

#ifdef DMI_TUNING
unsigned long long g_last_undecided = 0;
#endif

int filter(const double *depth, const double *best_cost, double threshold, const double *K4, const double *RT4, int32_t n, int32_t W,
           int32_t H, double abs_tolerance, double rel_tolerance, int32_t min_views, int32_t device, double *out_depth, int32_t *out_count,
           double *kernel_ms) {
  const std::string entry = "dmi_filter_depth_consistency: ";
  auto bad = [&](const std::string &what) { return fail(nullptr, DMI_ERR_INVALID_ARGUMENT, entry + what); };
  if (!depth) return bad("depth is null");
  if (!K4) return bad("K4 is null");
  if (!RT4) return bad("RT4 is null");
  if (!out_depth) return bad("out_depth is null");
  if (const char *what = dmi::size_refusal(n, W, H)) return bad(what);
  if (min_views < 0) return bad("min_views >= 0 required");
  if (const char *what = dmi::tolerance_refusal(abs_tolerance, rel_tolerance)) return bad(what);
  if (best_cost && threshold != threshold) return bad("threshold is NaN");
  if (const int32_t m = dmi::first_view_with_other_k(K4, n); m >= 0) return bad(dmi::other_k_message(m));

  // what the call holds on the device; the two events stand around whatever pass is being timed
  struct {
    dmi::DeviceBuffer planes, counts, cameras, stage_depth, stage_cost, stage_count, undecided;
  } b;
  dmi::CallHoldings h({&b.planes, &b.counts, &b.cameras, &b.stage_depth, &b.stage_cost, &b.stage_count, &b.undecided});
  if (const dmi::CallFailure f = h.open(entry, device, 2); f.code != DMI_OK) return fail(nullptr, f.code, f.text);
  const dmi::ConsistencyTuning tuning = dmi::consistency_tuning_from_environment();
  const size_t plane = (size_t)W * H, views = (size_t)n;
  const size_t chunk = dmi::staged_views(plane * sizeof(double), views);
  DMI_HIP(nullptr, dmi::grow_buffer(b.planes, views * plane * sizeof(double)));
  DMI_HIP(nullptr, dmi::grow_buffer(b.counts, views * plane * sizeof(int32_t)));
  DMI_HIP(nullptr, dmi::grow_buffer(b.cameras, views * sizeof(dmi::ConsistencyCamera)));
  DMI_HIP(nullptr, dmi::grow_buffer(b.stage_depth, chunk * plane * sizeof(double)));
  if (best_cost) DMI_HIP(nullptr, dmi::grow_buffer(b.stage_cost, chunk * plane * sizeof(double)));
  if (out_count) DMI_HIP(nullptr, dmi::grow_buffer(b.stage_count, chunk * plane * sizeof(int32_t)));
  unsigned long long *undecided = nullptr;
#ifdef DMI_TUNING
  DMI_HIP(nullptr, dmi::grow_buffer(b.undecided, sizeof(unsigned long long)));
  undecided = b.undecided.as<unsigned long long>();
  DMI_HIP(nullptr, hipMemsetAsync(undecided, 0, sizeof(unsigned long long), h.stream));
#endif

  double total_ms = 0.0;
  DMI_HIP(nullptr, dmi::upload_cameras(b.cameras, K4, RT4, views, h.stream));
  DMI_HIP(nullptr, hipMemsetAsync(b.counts.ptr, 0, views * plane * sizeof(int32_t), h.stream));
  DMI_HIP(nullptr, dmi::upload_flipped(depth, best_cost, threshold, W, H, views, chunk, b.stage_depth, b.stage_cost, b.planes.as<double>(), h.stream,
                                       h.events, &total_ms));

  // the counts: every source pixel against the target views, all in one launch or group by group
  if (n > 1) {
    DMI_HIP(nullptr, dmi::run_consistency_count(b.planes.as<double>(), b.cameras.as<dmi::ConsistencyCamera>(), n, W, H, abs_tolerance,
                                                rel_tolerance, tuning, b.counts.as<int32_t>(), undecided, h.stream, h.events));
    DMI_HIP(nullptr, hipStreamSynchronize(h.stream));
    DMI_HIP(nullptr, dmi::add_spans(h.events, 1, &total_ms));
  }

  // down, through the same stage buffers
  for (size_t m0 = 0; m0 < views; m0 += chunk) {
    const size_t cnt = std::min(chunk, views - m0);
    DMI_HIP(nullptr, hipEventRecord(h.events[0], h.stream));
    DMI_HIP(nullptr, dmi::launch_consistency_finish(b.planes.as<double>(), b.counts.as<int32_t>(), W, H, (int64_t)m0, (int64_t)cnt, min_views,
                                                    b.stage_depth.as<double>(), out_count ? b.stage_count.as<int32_t>() : nullptr, h.stream));
    DMI_HIP(nullptr, hipEventRecord(h.events[1], h.stream));
    DMI_HIP(nullptr, hipMemcpyAsync(out_depth + m0 * plane, b.stage_depth.ptr, cnt * plane * sizeof(double), hipMemcpyDeviceToHost, h.stream));
    if (out_count)
      DMI_HIP(nullptr, hipMemcpyAsync(out_count + m0 * plane, b.stage_count.ptr, cnt * plane * sizeof(int32_t), hipMemcpyDeviceToHost, h.stream));
    DMI_HIP(nullptr, hipStreamSynchronize(h.stream));
    DMI_HIP(nullptr, dmi::add_spans(h.events, 1, &total_ms));
  }
#ifdef DMI_TUNING
  DMI_HIP(nullptr, hipMemcpy(&g_last_undecided, undecided, sizeof(unsigned long long), hipMemcpyDeviceToHost));
#endif
  if (kernel_ms) *kernel_ms = total_ms;
  return DMI_OK;
}

}  // namespace

namespace dmi {

int32_t first_view_with_other_k(const double *K4, int32_t n) {
  for (int32_t m = 0; m < n; ++m) {
    const double *K = K4 + 16 * (size_t)m;
    const bool form = K[4] == 0.0 && K[8] == 0.0 && K[9] == 0.0 && K[10] == 1.0 && K[11] == 0.0 && K[0] != 0.0 && K[5] != 0.0 &&
                      K[0] == K[0] && K[5] == K[5];
    if (!form) return m;
  }
  return -1;
}

std::string other_k_message(int32_t m) {
  return "K4 of view " + std::to_string(m) + " is not of the form SetMatrixK produces (K4[1][0] == 0, third row 0 0 1 0, "
         "non-zero K4[0][0] and K4[1][1])";
}

std::vector<ConsistencyCamera> consistency_cameras(const double *K4, const double *RT4, size_t views) {
  std::vector<ConsistencyCamera> cameras(views);
  for (size_t m = 0; m < views; ++m) {
    const double *K = K4 + 16 * m, *RT = RT4 + 16 * m;
    for (int q = 0; q < 12; ++q) cameras[m].rt[q] = RT[q];
    const double k[8] = {K[0], K[1], K[2], K[3], K[5], K[6], K[7], 0.0};
    for (int q = 0; q < 8; ++q) cameras[m].k[q] = k[q];
  }
  return cameras;
}

ConsistencyTuning consistency_tuning_from_environment() {
  ConsistencyTuning tuning;
#ifdef DMI_TUNING
  if (const char *v = getenv("DMI_DC_VIEW_GROUP")) tuning.view_group = atoi(v);
  if (const char *v = getenv("DMI_DC_GATHER_AHEAD")) tuning.gather_ahead = atoi(v);
#endif
  return tuning;
}

// The counts of every source pixel of the n resident planes (image row order, zeroed counts) against the target views, all in one
// launch or group by group, between two events.  What dmi_filter_depth_consistency runs between its upload and its finish passes,
// and the resident view set (dmi_capi_viewset.hip) on the planes it has flipped.  n > 1.
hipError_t run_consistency_count(const double *planes, const ConsistencyCamera *cameras, int32_t n, int32_t W, int32_t H,
                                 double abs_tolerance, double rel_tolerance, const ConsistencyTuning &tuning, int32_t *counts,
                                 unsigned long long *undecided, hipStream_t stream, hipEvent_t events[2]) {
  const int group = tuning.view_group > 0 ? tuning.view_group : n;
  hipError_t e = hipEventRecord(events[0], stream);
  for (int t0 = 0; e == hipSuccess && t0 < n; t0 += group)
    e = launch_consistency_count(planes, cameras, n, W, H, t0, std::min(n, t0 + group), abs_tolerance, rel_tolerance, tuning.gather_ahead,
                                 counts, undecided, stream);
  if (e == hipSuccess) e = hipEventRecord(events[1], stream);
  return e;
}

}  // namespace dmi

extern "C" {

int dmi_filter_depth_consistency(const double *depth, const double *best_cost, double threshold, const double *K4, const double *RT4,
                                 int32_t n, int32_t W, int32_t H, double abs_tolerance, double rel_tolerance, int32_t min_views,
                                 int32_t device, double *out_depth, int32_t *out_count, double *kernel_ms) {
  return dmi::guarded(nullptr, "dmi_filter_depth_consistency", [&]() -> int {
    return filter(depth, best_cost, threshold, K4, RT4, n, W, H, abs_tolerance, rel_tolerance, min_views, device, out_depth, out_count,
                  kernel_ms);
  });
}

#ifdef DMI_TUNING
// tuning builds only (tools/gpu_depth_consistency_time.py): the pairs of the last call that pixel_fast left to pixel_exact
unsigned long long dmi_tuning_depth_consistency_undecided(void) { return g_last_undecided; }
#endif

}  // extern "C"
