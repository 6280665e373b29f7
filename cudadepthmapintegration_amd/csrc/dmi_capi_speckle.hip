// dmi_capi_speckle.hip -- dmi_filter_depth_speckles of include/dmi.h: the argument checks (all of them before the device is touched),
// and per piece of whole views the upload, the four launches of depth_speckle.hip and the download.  Context-free, on the
// scaffold of dmi_depth_call.h: everything the call allocates it frees before it returns; the device holds the planes of one piece
// at a time.  A failure's text is dmi_last_error(NULL)'s.
#include <stdlib.h>

#include <algorithm>
#include <string>

#include "depth_speckle.h"
#include "dmi_context.h"
#include "dmi_depth_call.h"
#include "dmi_view_set.h"

namespace {

using dmi::fail;

#ifdef DMI_TUNING
double g_last_pass_ms[4] = {0.0, 0.0, 0.0, 0.0};
#endif

int filter(const double *depth, const double *best_cost, double threshold, int32_t n, int32_t W, int32_t H, double abs_tolerance,
           double rel_tolerance, int64_t min_pixels, int32_t device, double *out_depth, int32_t *out_size, double *kernel_ms) {
  const std::string entry = "dmi_filter_depth_speckles: ";
  auto bad = [&](const std::string &what) { return fail(nullptr, DMI_ERR_INVALID_ARGUMENT, entry + what); };
  if (!depth) return bad("depth is null");
  if (!out_depth) return bad("out_depth is null");
  if (const char *what = dmi::size_refusal(n, W, H)) return bad(what);
  if (min_pixels < 0) return bad("min_pixels >= 0 required");
  if (const char *what = dmi::tolerance_refusal(abs_tolerance, rel_tolerance)) return bad(what);
  if (best_cost && threshold != threshold) return bad("threshold is NaN");

  // what the call holds on the device; the events stand before the local pass and behind each of the four
  struct {
    dmi::DeviceBuffer depth, cost, label, size, border_down, border_right, out_size;
  } b;
  dmi::CallHoldings h({&b.depth, &b.cost, &b.label, &b.size, &b.border_down, &b.border_right, &b.out_size});
  if (const dmi::CallFailure f = h.open(entry, device, 5); f.code != DMI_OK) return fail(nullptr, f.code, f.text);
  const dmi::SpeckleTuning tuning = dmi::speckle_tuning_from_environment();
  const size_t plane = (size_t)W * H, views = (size_t)n;
  const size_t chunk = dmi::staged_views(plane * sizeof(double), views);
  const size_t tiles = (size_t)dmi::speckle_tiles(W, H, (int64_t)chunk, tuning);
  DMI_HIP(nullptr, dmi::grow_buffer(b.depth, chunk * plane * sizeof(double)));
  if (best_cost) DMI_HIP(nullptr, dmi::grow_buffer(b.cost, chunk * plane * sizeof(double)));
  DMI_HIP(nullptr, dmi::grow_buffer(b.label, chunk * plane * sizeof(uint32_t)));
  DMI_HIP(nullptr, dmi::grow_buffer(b.size, chunk * plane * sizeof(uint32_t)));
  DMI_HIP(nullptr, dmi::grow_buffer(b.border_down, tiles * sizeof(uint64_t)));
  DMI_HIP(nullptr, dmi::grow_buffer(b.border_right, tiles * sizeof(uint64_t)));
  if (out_size) DMI_HIP(nullptr, dmi::grow_buffer(b.out_size, chunk * plane * sizeof(int32_t)));

  double pass_ms[4] = {0.0, 0.0, 0.0, 0.0};
  for (size_t m0 = 0; m0 < views; m0 += chunk) {
    const size_t cnt = std::min(chunk, views - m0);
    const dmi::SpecklePiece piece =
        dmi::speckle_piece(b.depth.as<double>(), best_cost ? b.cost.as<double>() : nullptr, b.label, b.size, b.border_down, b.border_right,
                           out_size ? b.out_size.as<int32_t>() : nullptr, (int64_t)cnt);
    DMI_HIP(nullptr, hipMemcpyAsync(b.depth.ptr, depth + m0 * plane, cnt * plane * sizeof(double), hipMemcpyHostToDevice, h.stream));
    if (best_cost)
      DMI_HIP(nullptr, hipMemcpyAsync(b.cost.ptr, best_cost + m0 * plane, cnt * plane * sizeof(double), hipMemcpyHostToDevice, h.stream));
    DMI_HIP(nullptr, dmi::run_speckle_piece(piece, threshold, W, H, abs_tolerance, rel_tolerance, min_pixels, tuning, h.stream, h.events));
    DMI_HIP(nullptr, hipMemcpyAsync(out_depth + m0 * plane, b.depth.ptr, cnt * plane * sizeof(double), hipMemcpyDeviceToHost, h.stream));
    if (out_size)
      DMI_HIP(nullptr, hipMemcpyAsync(out_size + m0 * plane, b.out_size.ptr, cnt * plane * sizeof(int32_t), hipMemcpyDeviceToHost, h.stream));
    DMI_HIP(nullptr, hipStreamSynchronize(h.stream));  // the planes are reused by the next piece
    DMI_HIP(nullptr, dmi::add_spans(h.events, 4, pass_ms));
  }
#ifdef DMI_TUNING
  for (int p = 0; p < 4; ++p) g_last_pass_ms[p] = pass_ms[p];
#endif
  if (kernel_ms) *kernel_ms = (pass_ms[0] + pass_ms[1]) + (pass_ms[2] + pass_ms[3]);
  return DMI_OK;
}

}  // namespace

namespace dmi {

// The filter on the device planes of one piece: the four passes, an event before the first and one behind each.  What
// dmi_filter_depth_speckles runs between its copies, and the resident view set (dmi_capi_viewset.hip) on its own planes.
hipError_t run_speckle_piece(const SpecklePiece &piece, double threshold, int32_t W, int32_t H, double abs_tolerance, double rel_tolerance,
                             int64_t min_pixels, const SpeckleTuning &tuning, hipStream_t stream, hipEvent_t events[5]) {
  hipError_t e = hipEventRecord(events[0], stream);
  if (e == hipSuccess) e = launch_speckle_local(piece, threshold, W, H, abs_tolerance, rel_tolerance, tuning, stream);
  if (e == hipSuccess) e = hipEventRecord(events[1], stream);
  if (e == hipSuccess) e = launch_speckle_border(piece, W, H, tuning, stream);
  if (e == hipSuccess) e = hipEventRecord(events[2], stream);
  if (e == hipSuccess) e = launch_speckle_sizes(piece, W, H, stream);
  if (e == hipSuccess) e = hipEventRecord(events[3], stream);
  if (e == hipSuccess) e = launch_speckle_output(piece, W, H, min_pixels, stream);
  if (e == hipSuccess) e = hipEventRecord(events[4], stream);
  return e;
}

SpeckleTuning speckle_tuning_from_environment() {
  SpeckleTuning tuning;
#ifdef DMI_TUNING
  if (const char *v = getenv("DMI_DS_TILE_HEIGHT")) tuning.tile_height = atoi(v);
  if (const char *v = getenv("DMI_DS_RUNS")) tuning.runs = atoi(v) != 0;
#endif
  return tuning;
}

}  // namespace dmi

extern "C" {

int dmi_filter_depth_speckles(const double *depth, const double *best_cost, double threshold, int32_t n, int32_t W, int32_t H,
                              double abs_tolerance, double rel_tolerance, int64_t min_pixels, int32_t device, double *out_depth,
                              int32_t *out_size, double *kernel_ms) {
  return dmi::guarded(nullptr, "dmi_filter_depth_speckles", [&]() -> int {
    return filter(depth, best_cost, threshold, n, W, H, abs_tolerance, rel_tolerance, min_pixels, device, out_depth, out_size, kernel_ms);
  });
}

#ifdef DMI_TUNING
// tuning builds only (tools/gpu_depth_speckle_time.py): the last call's hipEvent time per pass -- local, border, sizes, output
void dmi_tuning_depth_speckle_pass_ms(double out[4]) {
  for (int p = 0; p < 4; ++p) out[p] = g_last_pass_ms[p];
}
#endif

}  // extern "C"
