// depth_consistency.hip -- depth maps filtered by cross-view geometric consistency (dmi_filter_depth_consistency): a depth is kept
// only if enough other views, looking at the same world point, hold a depth that agrees.  What stands between a stereo depth map
// and the fusion besides the best-cost threshold: a wrong depth that is fused bends the iso-surface and carves free space through
// it, and no mesh filter gives that back.
//
// Semantics (include/dmi.h states them in full; tests/depth_consistency_np.py restates them on the CPU and the result is
// identical): f64 throughout, every operation rounded (-ffp-contract=off), the fusion's projection order (row4) and its pixel rule
// (pixel_exact, reached through pixel_fast's checked reciprocal where that provably selects the same pixel).
//
// Passes:
//   upload    one lane per staged pixel: threshold, validity, -1 for everything that is not valid, rows flipped to image order
//   count     one lane per source pixel, a workgroup per 16 x 16 tile of one source view, a wave per 8 x 8 quarter of it (the
//             gathers of neighbouring lanes land a few pixels apart in the target).  The world point is computed once; then a loop
//             over the target views with each camera's 19 numbers arriving through scalar loads (wave-uniform addresses).  The
//             count lives in a register and is added to the view's count plane once per launch.  A wave without a valid lane
//             leaves at once.
//   finish    one lane per output pixel: the filtered depth and the count in vtk point order
#include "depth_consistency.h"
#include "fusion_device.h"

namespace dmi {
namespace {

constexpr int kBlock = 256;

template <typename T>
__device__ __forceinline__ T cload(const T *p) {  // wave-uniform address -> scalar load
  return *reinterpret_cast<const T __attribute__((address_space(4))) *>(reinterpret_cast<uintptr_t>(p));
}

__global__ __launch_bounds__(kBlock) void consistency_upload_kernel(const double *__restrict__ depth, const double *__restrict__ cost,
                                                                    double threshold, int W, int H, int64_t total,
                                                                    double *__restrict__ planes) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= total) return;
  const int64_t plane = (int64_t)W * H, view = i / plane, r = i - view * plane;
  const int row = (int)(r / W), x = (int)(r - (int64_t)row * W);
  double d = depth[i];
  if (cost && cost[i] > threshold) d = -1.0;  // RD.cxx:138-167; a NaN cost keeps the depth
  const bool valid = d > 0.0 && d < __builtin_inf();
  planes[view * plane + (int64_t)(H - 1 - row) * W + x] = valid ? d : -1.0;
}

struct TargetCamera {
  double rt[12], k[7];
  __device__ __forceinline__ explicit TargetCamera(const ConsistencyCamera *__restrict__ c) {
#pragma unroll
    for (int q = 0; q < 12; ++q) rt[q] = cload(&c->rt[q]);
#pragma unroll
    for (int q = 0; q < 7; ++q) k[q] = cload(&c->k[q]);
  }
};

// Step 3 of the definition up to the pixel: true when world point w lies in front of target `cam` and projects into its image;
// then c2 is its camera z and pixel = py * W + px.  h_2 is c'_2 itself and K4[1][0] * c'_0 is left out of h_1: with the K the
// entry point admits, neither changes whether a pixel is selected nor which.
__device__ __forceinline__ bool project(const TargetCamera &cam, double w0, double w1, double w2, int W, int H, double &c2, int &pixel,
                                        unsigned &undecided) {
  const double c0 = row4(cam.rt, w0, w1, w2), c1 = row4(cam.rt + 4, w0, w1, w2);
  c2 = row4(cam.rt + 8, w0, w1, w2);
  if (!(c2 > 0.0)) return false;  // behind the camera, or a NaN (a lane without a valid source pixel carries NaNs)
  const double h0 = ((cam.k[0] * c0 + cam.k[1] * c1) + cam.k[2] * c2) + cam.k[3];
  const double h1 = (cam.k[4] * c1 + cam.k[5] * c2) + cam.k[6];
  int px = 0, py = 0;
  int in = pixel_fast(h0, h1, c2, W, H, px, py);
  if (in < 0) {
    ++undecided;
    in = pixel_exact(h0, h1, c2, W, H, px, py) ? 1 : 0;
  }
  pixel = py * W + px;
  return in != 0;
}

__device__ __forceinline__ bool agrees(double c2, double d, double abs_tol, double rel_tol) {
  const double bound = abs_tol + rel_tol * c2;
  return d > 0.0 && fabs(c2 - d) <= bound;  // -1 (everything the upload found not valid) and a NaN bound reject the pair
}

template <bool AHEAD>
__global__ __launch_bounds__(kBlock) void consistency_count_kernel(const double *__restrict__ planes,
                                                                   const ConsistencyCamera *__restrict__ cameras, int s0, int W, int H,
                                                                   int tiles_x, int t0, int t1, double abs_tol, double rel_tol,
                                                                   int32_t *__restrict__ counts, unsigned long long *undecided_total) {
  const int s = s0 + (int)blockIdx.y;
  const int tile_y = (int)blockIdx.x / tiles_x, tile_x = (int)blockIdx.x - tile_y * tiles_x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int px = tile_x * kConsistencyTile + (wave & 1) * 8 + (lane & 7);
  const int py = tile_y * kConsistencyTile + (wave >> 1) * 8 + (lane >> 3);
  const int64_t plane = (int64_t)W * H;
  const bool inside = px < W && py < H;
  const int64_t self = (int64_t)s * plane + (inside ? (int64_t)py * W + px : 0);
  const double d = inside ? planes[self] : -1.0;
  const bool valid = d > 0.0;  // the planes hold -1 for everything else
  if (__builtin_amdgcn_ballot_w64(valid) == 0) return;

  // step 2: the world point, once per lane
  double w0, w1, w2;
  {
    const ConsistencyCamera *__restrict__ src = cameras + s;
    const double k00 = cload(&src->k[0]), k01 = cload(&src->k[1]), k02 = cload(&src->k[2]), k11 = cload(&src->k[4]),
                 k12 = cload(&src->k[5]);
    const double yn = ((double)py - k12) / k11;
    const double xn = (((double)px - k02) - k01 * yn) / k00;
    const double q0 = xn * d - cload(&src->rt[3]), q1 = yn * d - cload(&src->rt[7]), q2 = d - cload(&src->rt[11]);
    const double nan = __builtin_nan("");
    w0 = valid ? (cload(&src->rt[0]) * q0 + cload(&src->rt[4]) * q1) + cload(&src->rt[8]) * q2 : nan;
    w1 = valid ? (cload(&src->rt[1]) * q0 + cload(&src->rt[5]) * q1) + cload(&src->rt[9]) * q2 : nan;
    w2 = valid ? (cload(&src->rt[2]) * q0 + cload(&src->rt[6]) * q1) + cload(&src->rt[10]) * q2 : nan;
  }

  int32_t count = 0;
  unsigned undecided = 0;
  if constexpr (AHEAD) {
    // the depth of view t is requested in iteration t and compared in iteration t + 1, behind the next view's projection.  A pair
    // without a pixel reads the target's pixel 0 (a valid address) and is rejected by `hit`.
    double c2_pending = 0.0, d_pending = -1.0;
    bool hit_pending = false;
    for (int view = t0; view < t1; ++view) {
      const int t = __builtin_amdgcn_readfirstlane(view);
      if (t == s) continue;
      const TargetCamera cam(cameras + t);
      double c2 = 0.0;
      int pixel = 0;
      const bool hit = project(cam, w0, w1, w2, W, H, c2, pixel, undecided);
      const double dt = planes[(int64_t)t * plane + (hit ? pixel : 0)];
      if (hit_pending && agrees(c2_pending, d_pending, abs_tol, rel_tol)) ++count;
      c2_pending = c2, d_pending = dt, hit_pending = hit;
    }
    if (hit_pending && agrees(c2_pending, d_pending, abs_tol, rel_tol)) ++count;
  } else {
    for (int view = t0; view < t1; ++view) {
      // the loop's bounds are wave-uniform, but lanes leave an iteration at different points: the index is made a scalar by hand,
      // so that the camera's loads stay scalar loads whatever the compiler's uniformity analysis makes of the loop
      const int t = __builtin_amdgcn_readfirstlane(view);
      if (t == s) continue;
      const TargetCamera cam(cameras + t);
      double c2 = 0.0;
      int pixel = 0;
      if (!project(cam, w0, w1, w2, W, H, c2, pixel, undecided)) continue;
      if (agrees(c2, planes[(int64_t)t * plane + pixel], abs_tol, rel_tol)) ++count;
    }
  }
  if (count) counts[self] += count;  // one lane per pixel and launches in stream order: no atomic needed
  if (undecided_total && undecided) atomicAdd(undecided_total, (unsigned long long)undecided);
}

__global__ __launch_bounds__(kBlock) void consistency_finish_kernel(const double *__restrict__ planes, const int32_t *__restrict__ counts,
                                                                    int W, int H, int64_t first_view, int64_t total, int32_t min_views,
                                                                    double *__restrict__ out_depth, int32_t *__restrict__ out_count) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= total) return;
  const int64_t plane = (int64_t)W * H, view = i / plane, r = i - view * plane;
  const int row = (int)(r / W), x = (int)(r - (int64_t)row * W);
  const int64_t at = (first_view + view) * plane + (int64_t)(H - 1 - row) * W + x;
  const double d = planes[at];
  const int32_t c = counts[at];  // 0 wherever the pixel is not valid: such a lane never counts
  out_depth[i] = d > 0.0 && c >= min_views ? d : -1.0;
  if (out_count) out_count[i] = c;
}

unsigned blocks(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

hipError_t launch_consistency_upload(const double *depth, const double *cost, double threshold, int W, int H, int64_t count, double *planes,
                                     int64_t first_view, hipStream_t stream) {
  const int64_t plane = (int64_t)W * H, total = count * plane;
  hipLaunchKernelGGL(consistency_upload_kernel, dim3(blocks(total)), dim3(kBlock), 0, stream, depth, cost, threshold, W, H, total,
                     planes + first_view * plane);
  return hipGetLastError();
}

hipError_t launch_consistency_count(const double *planes, const ConsistencyCamera *cameras, int n, int W, int H, int t0, int t1,
                                    double abs_tolerance, double rel_tolerance, int gather_ahead, int32_t *counts,
                                    unsigned long long *undecided, hipStream_t stream) {
  const int tiles_x = (W + kConsistencyTile - 1) / kConsistencyTile, tiles_y = (H + kConsistencyTile - 1) / kConsistencyTile;
  constexpr int kMaxGridY = 32768;  // source views per launch: the grid's second dimension ends at 65535
  for (int s0 = 0; s0 < n; s0 += kMaxGridY) {
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)(n - s0 < kMaxGridY ? n - s0 : kMaxGridY));
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, stream, planes, cameras, s0, W, H, tiles_x, t0, t1, abs_tolerance, rel_tolerance,
                         counts, undecided);
    };
    if (gather_ahead) launch(consistency_count_kernel<true>); else launch(consistency_count_kernel<false>);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_consistency_finish(const double *planes, const int32_t *counts, int W, int H, int64_t first_view, int64_t count,
                                     int32_t min_views, double *out_depth, int32_t *out_count, hipStream_t stream) {
  const int64_t total = count * (int64_t)W * H;
  hipLaunchKernelGGL(consistency_finish_kernel, dim3(blocks(total)), dim3(kBlock), 0, stream, planes, counts, W, H, first_view, total,
                     min_views, out_depth, out_count);
  return hipGetLastError();
}

}  // namespace dmi
