// dmi_capi_speckle.hip -- dmi_filter_depth_speckles of include/dmi.h: the argument checks (all of them before the device is touched),
// and per piece of whole views the upload, the four launches of depth_speckle.hip and the download.  Context-free, like
// dmi_filter_depth_consistency: everything the call allocates it frees before it returns; the device holds the planes of one piece
// at a time.  A failure's text is dmi_last_error(NULL)'s.
#include <stdlib.h>

#include <algorithm>
#include <string>

#include "depth_speckle.h"
#include "dmi_context.h"
#include "dmi_view_set.h"

namespace {

using dmi::fail;

constexpr size_t kStageBytes = size_t(256) << 20;  // host data goes up and comes down in pieces of whole views, as many as fit this

bool finite_and_not_negative(double v) { return v >= 0.0 && v <= 1.7976931348623157e308; }  // false for NaN

#ifdef DMI_TUNING
double g_last_pass_ms[4] = {0.0, 0.0, 0.0, 0.0};
#endif

// what the call holds on the device and the events that time its kernels; released whatever way the call ends
struct Holdings {
  dmi::DeviceBuffer depth, cost, label, size, border_down, border_right, out_size;
  hipStream_t stream = nullptr;
  hipEvent_t events[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // before the local pass and behind each of the four
  ~Holdings() {
    if (stream) (void)hipStreamSynchronize(stream);
    dmi::free_buffers({&depth, &cost, &label, &size, &border_down, &border_right, &out_size});
    for (hipEvent_t e : events)
      if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

#define DMI_DS_HIP(call) DMI_HIP(nullptr, call)

int filter(const double *depth, const double *best_cost, double threshold, int32_t n, int32_t W, int32_t H, double abs_tolerance,
           double rel_tolerance, int64_t min_pixels, int32_t device, double *out_depth, int32_t *out_size, double *kernel_ms) {
  const std::string entry = "dmi_filter_depth_speckles: ";
  auto bad = [&](const std::string &what) { return fail(nullptr, DMI_ERR_INVALID_ARGUMENT, entry + what); };
  if (!depth) return bad("depth is null");
  if (!out_depth) return bad("out_depth is null");
  if (n < 1) return bad("n >= 1 required");
  if (W < 1 || W > 32768) return bad("W must lie in [1, 32768]");
  if (H < 1 || H > 32768) return bad("H must lie in [1, 32768]");
  if (min_pixels < 0) return bad("min_pixels >= 0 required");
  if (!finite_and_not_negative(abs_tolerance)) return bad("abs_tolerance must be finite and >= 0");
  if (!finite_and_not_negative(rel_tolerance)) return bad("rel_tolerance must be finite and >= 0");
  if (best_cost && threshold != threshold) return bad("threshold is NaN");

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return fail(nullptr, DMI_ERR_DEVICE, entry + "no HIP device available");
  }
  if (device < 0 || device >= ndev) return bad("device ordinal out of range");
  DMI_DS_HIP(hipSetDevice(device));

  const dmi::SpeckleTuning tuning = dmi::speckle_tuning_from_environment();

  Holdings h;
  DMI_DS_HIP(hipStreamCreateWithFlags(&h.stream, hipStreamNonBlocking));
  for (hipEvent_t &e : h.events) DMI_DS_HIP(hipEventCreate(&e));
  const size_t plane = (size_t)W * H, views = (size_t)n;
  const size_t chunk = std::min(views, std::max<size_t>(1, kStageBytes / (plane * sizeof(double))));  // a larger view goes whole
  const size_t tiles = (size_t)dmi::speckle_tiles(W, H, (int64_t)chunk, tuning);
  DMI_DS_HIP(dmi::grow_buffer(h.depth, chunk * plane * sizeof(double)));
  if (best_cost) DMI_DS_HIP(dmi::grow_buffer(h.cost, chunk * plane * sizeof(double)));
  DMI_DS_HIP(dmi::grow_buffer(h.label, chunk * plane * sizeof(uint32_t)));
  DMI_DS_HIP(dmi::grow_buffer(h.size, chunk * plane * sizeof(uint32_t)));
  DMI_DS_HIP(dmi::grow_buffer(h.border_down, tiles * sizeof(uint64_t)));
  DMI_DS_HIP(dmi::grow_buffer(h.border_right, tiles * sizeof(uint64_t)));
  if (out_size) DMI_DS_HIP(dmi::grow_buffer(h.out_size, chunk * plane * sizeof(int32_t)));

  double pass_ms[4] = {0.0, 0.0, 0.0, 0.0};
  for (size_t m0 = 0; m0 < views; m0 += chunk) {
    const size_t cnt = std::min(chunk, views - m0);
    dmi::SpecklePiece piece;
    piece.depth = h.depth.as<double>();
    piece.cost = best_cost ? h.cost.as<double>() : nullptr;
    piece.label = h.label.as<uint32_t>();
    piece.size = h.size.as<uint32_t>();
    piece.border_down = h.border_down.as<uint64_t>();
    piece.border_right = h.border_right.as<uint64_t>();
    piece.out_size = out_size ? h.out_size.as<int32_t>() : nullptr;
    piece.count = (int64_t)cnt;
    DMI_DS_HIP(hipMemcpyAsync(h.depth.ptr, depth + m0 * plane, cnt * plane * sizeof(double), hipMemcpyHostToDevice, h.stream));
    if (best_cost)
      DMI_DS_HIP(hipMemcpyAsync(h.cost.ptr, best_cost + m0 * plane, cnt * plane * sizeof(double), hipMemcpyHostToDevice, h.stream));
    DMI_DS_HIP(dmi::run_speckle_piece(piece, threshold, W, H, abs_tolerance, rel_tolerance, min_pixels, tuning, h.stream, h.events));
    DMI_DS_HIP(hipMemcpyAsync(out_depth + m0 * plane, h.depth.ptr, cnt * plane * sizeof(double), hipMemcpyDeviceToHost, h.stream));
    if (out_size)
      DMI_DS_HIP(hipMemcpyAsync(out_size + m0 * plane, h.out_size.ptr, cnt * plane * sizeof(int32_t), hipMemcpyDeviceToHost, h.stream));
    DMI_DS_HIP(hipStreamSynchronize(h.stream));  // the planes are reused by the next piece
    for (int p = 0; p < 4; ++p) {
      float ms = 0.f;
      DMI_DS_HIP(hipEventElapsedTime(&ms, h.events[p], h.events[p + 1]));
      pass_ms[p] += (double)ms;
    }
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
