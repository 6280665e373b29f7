// point_smooth.hip -- a separable Gaussian over the point data, between the cell -> point pass (grid_post.hip) and the contour: what a
// vtkImageGaussianSmooth in front of vtkContourFilter is for (only the intent is shared, not the numbers).  Streaming, HBM/LDS-bound.
//
// Definition (include/dmi.h: dmi_set_point_smoothing), met bit for bit.  Three passes, x then y then z, each over the
// full f64 result of the one before.  On the pass's axis, N points, radius r, weights k_0..k_r, border replicated:
//   v(t) = value at clamp(t, 0, N-1);  acc = k_0 * v(q);  for i = 1..r ascending: acc = acc + k_i * (v(q-i) + v(q+i)).
// f64, every operation rounded (-ffp-contract=off covers this file: no v_fma_f64 in the accumulation).  An axis with sigma == 0 is
// skipped: its pass copies bits (or is not launched), it never multiplies by 1.
//
// Two sweeps of HBM, not three: the x and y passes are fused through LDS (smooth_xy_kernel), z marches columns (smooth_z_kernel).
// Loads are UNCONDITIONAL from clamped (always valid) addresses, as load_quad's are (grid_post.hip); only the stores are guarded.
#include <stdlib.h>

#include "fusion_kernels.h"

namespace dmi {

namespace {

__device__ __forceinline__ int clampi(int t, int hi) { return t < 0 ? 0 : (t > hi ? hi : t); }

// ---- the plain form: one launch per axis, one thread per point, the 2 r + 1 values through the cache.  The A/B partner of the
// tiled form (DMI_TUNING builds, DMI_PSMOOTH_PLAIN=1; tools/gpu_point_smooth_tune.py) ----
template <int AXIS>
__global__ __launch_bounds__(256) void smooth_axis_kernel(const double *__restrict__ src, double *__restrict__ dst, int px, int py,
                                                          int pz, PointSmoothArgs a) {
  const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = blockIdx.z;
  if (i >= px || j >= py) return;
  const int64_t row = px, plane = (int64_t)px * py;
  const int64_t stride = AXIS == 0 ? 1 : (AXIS == 1 ? row : plane);
  const int q = AXIS == 0 ? i : (AXIS == 1 ? j : k), last = (AXIS == 0 ? px : (AXIS == 1 ? py : pz)) - 1;
  const double *line = src + ((int64_t)k * plane + (int64_t)j * row + i) - (int64_t)q * stride;  // the point with index 0 on the axis
  const int r = a.r[AXIS];
  double acc = a.k[AXIS][0] * line[(int64_t)q * stride];
  for (int t = 1; t <= r; ++t) acc = acc + a.k[AXIS][t] * (line[(int64_t)clampi(q - t, last) * stride] + line[(int64_t)clampi(q + t, last) * stride]);
  __builtin_nontemporal_store(acc, &dst[(int64_t)k * plane + (int64_t)j * row + i]);
}

// ---- x and y in one sweep.  A workgroup of 64 x 4 threads produces 64 x BY points of one k-plane.  It stages the
// (64 + 2 rx) x (BY + 2 ry) values around them in LDS (plane A, border replicated by the clamped load addresses), filters every row
// of A along x into plane B (64 x (BY + 2 ry)), then filters B along y and stores.  Lanes read consecutive doubles in every phase:
// no bank conflicts.  Dynamic LDS: ((64 + 2 rx) + 64) (BY + 2 ry) doubles, 60 KB at the radius cap with BY = 16.
// Every phase keeps several independent values per thread in flight: the loads go out eight at a time before the first of them is
// written to LDS, and a thread filters four rows together, tap by tap -- each point still accumulates in the definition's order. ----
constexpr int kLoadsInFlight = 8, kRowsTogether = 4;

template <int BY>
__global__ __launch_bounds__(256) void smooth_xy_kernel(const double *__restrict__ src, double *__restrict__ dst, int px, int py,
                                                        PointSmoothArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int rx = a.r[0], ry = a.r[1];
  const int W = 64 + 2 * rx, H = BY + 2 * ry, n = W * H;
  double *A = lds, *B = lds + n;
  const int tx = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(threadIdx.y);  // (64 lanes in x: a wave shares threadIdx.y)
  const int tid = wave * 64 + tx;
  const int x0 = blockIdx.x * 64, y0 = blockIdx.y * BY;
  const int64_t plane = (int64_t)px * py;
  const double *layer = src + (int64_t)blockIdx.z * plane;
  for (int e0 = tid; e0 < n; e0 += 256 * kLoadsInFlight) {
    double v[kLoadsInFlight];
#pragma unroll
    for (int u = 0; u < kLoadsInFlight; ++u) {
      const int e = min(e0 + 256 * u, n - 1);  // (past the tile's end: its last element once more, not stored)
      const int ly = e / W, lx = e - ly * W;
      v[u] = layer[(int64_t)clampi(y0 - ry + ly, py - 1) * px + clampi(x0 - rx + lx, px - 1)];
    }
#pragma unroll
    for (int u = 0; u < kLoadsInFlight; ++u)
      if (e0 + 256 * u < n) A[e0 + 256 * u] = v[u];
  }
  __syncthreads();
  for (int base = wave; base < H; base += 4 * kRowsTogether) {  // rows base, base + 4, ... of A
    const double *c[kRowsTogether];
    double acc[kRowsTogether];
#pragma unroll
    for (int u = 0; u < kRowsTogether; ++u) {
      c[u] = A + min(base + 4 * u, H - 1) * W + rx + tx;
      acc[u] = rx == 0 ? c[u][0] : a.k[0][0] * c[u][0];
    }
    for (int t = 1; t <= rx; ++t) {
      const double k = a.k[0][t];
#pragma unroll
      for (int u = 0; u < kRowsTogether; ++u)
        if (base + 4 * u < H) acc[u] = acc[u] + k * (c[u][-t] + c[u][t]);
    }
#pragma unroll
    for (int u = 0; u < kRowsTogether; ++u)
      if (base + 4 * u < H) B[(base + 4 * u) * 64 + tx] = acc[u];
  }
  __syncthreads();
  const int i = x0 + tx;
  for (int base = wave; base < BY; base += 4 * kRowsTogether) {  // rows base, base + 4, ... of the output
    const double *c[kRowsTogether];
    double acc[kRowsTogether];
#pragma unroll
    for (int u = 0; u < kRowsTogether; ++u) {
      c[u] = B + (min(base + 4 * u, BY - 1) + ry) * 64 + tx;
      acc[u] = ry == 0 ? c[u][0] : a.k[1][0] * c[u][0];
    }
    for (int t = 1; t <= ry; ++t) {
      const double k = a.k[1][t];
#pragma unroll
      for (int u = 0; u < kRowsTogether; ++u)
        if (base + 4 * u < BY) acc[u] = acc[u] + k * (c[u][-t * 64] + c[u][t * 64]);
    }
#pragma unroll
    for (int u = 0; u < kRowsTogether; ++u) {
      const int j = y0 + base + 4 * u;
      if (base + 4 * u < BY && i < px && j < py) __builtin_nontemporal_store(acc[u], &dst[(int64_t)blockIdx.z * plane + (int64_t)j * px + i]);
    }
  }
}

// ---- z.  A workgroup of one wave, one (i, j) column per lane, produces KZ points along k.  Every lane loads the KZ + 2 rz values of
// its column (clamped k: the border replicated), eight at a time, into a column of LDS that only it reads -- LDS as a register window
// that a run-time radius can index; no barrier -- and filters its KZ points out of it together, tap by tap.  Dynamic LDS:
// 64 (KZ + 2 rz) doubles, 20 KB at the radius cap with KZ = 8. ----
template <int KZ>
__global__ __launch_bounds__(64) void smooth_z_kernel(const double *__restrict__ src, double *__restrict__ dst, int px, int py, int pz,
                                                      PointSmoothArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int rz = a.r[2], n = KZ + 2 * rz;
  const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y, k0 = blockIdx.z * KZ;
  const int64_t plane = (int64_t)px * py;
  const int64_t column = (int64_t)j * px + clampi(i, px - 1);  // a valid column for the tile's tail, whose results are dropped
  double *mine = lds + threadIdx.x;
  for (int t0 = 0; t0 < n; t0 += kLoadsInFlight) {
    double v[kLoadsInFlight];
#pragma unroll
    for (int u = 0; u < kLoadsInFlight; ++u) v[u] = src[(int64_t)clampi(k0 - rz + min(t0 + u, n - 1), pz - 1) * plane + column];
#pragma unroll
    for (int u = 0; u < kLoadsInFlight; ++u)
      if (t0 + u < n) mine[(t0 + u) * 64] = v[u];
  }
  if (i >= px) return;
  const double *c = mine + rz * 64;  // the window's centre for the first point
  double acc[KZ];
#pragma unroll
  for (int kk = 0; kk < KZ; ++kk) acc[kk] = a.k[2][0] * c[kk * 64];
  for (int t = 1; t <= rz; ++t) {
    const double k = a.k[2][t];
#pragma unroll
    for (int kk = 0; kk < KZ; ++kk) acc[kk] = acc[kk] + k * (c[(kk - t) * 64] + c[(kk + t) * 64]);
  }
#pragma unroll
  for (int kk = 0; kk < KZ; ++kk)
    if (k0 + kk < pz) __builtin_nontemporal_store(acc[kk], &dst[(int64_t)(k0 + kk) * plane + (int64_t)j * px + i]);
}

template <int BY>
void launch_xy(const double *src, double *dst, int px, int py, int pz, const PointSmoothArgs &a, hipStream_t stream) {
  const size_t lds = (size_t)((64 + 2 * a.r[0]) + 64) * (BY + 2 * a.r[1]) * sizeof(double);
  const dim3 grid((unsigned)((px + 63) / 64), (unsigned)((py + BY - 1) / BY), (unsigned)pz);
  hipLaunchKernelGGL((smooth_xy_kernel<BY>), grid, dim3(64, 4), lds, stream, src, dst, px, py, a);
}

template <int KZ>
void launch_z(const double *src, double *dst, int px, int py, int pz, const PointSmoothArgs &a, hipStream_t stream) {
  const size_t lds = (size_t)64 * (KZ + 2 * a.r[2]) * sizeof(double);
  const dim3 grid((unsigned)((px + 63) / 64), (unsigned)py, (unsigned)((pz + KZ - 1) / KZ));
  hipLaunchKernelGGL((smooth_z_kernel<KZ>), grid, dim3(64), lds, stream, src, dst, px, py, pz, a);
}

template <int AXIS>
void launch_axis(const double *src, double *dst, int px, int py, int pz, const PointSmoothArgs &a, hipStream_t stream) {
  const dim3 grid((unsigned)((px + 63) / 64), (unsigned)((py + 3) / 4), (unsigned)pz);
  hipLaunchKernelGGL((smooth_axis_kernel<AXIS>), grid, dim3(64, 4), 0, stream, src, dst, px, py, pz, a);
}

bool plain_form() {
#ifdef DMI_TUNING
  const char *e = getenv("DMI_PSMOOTH_PLAIN");
  return e && atoi(e) != 0;
#else
  return false;
#endif
}

}  // namespace

int point_smooth_launches(const PointSmoothArgs &a) {
  if (plain_form()) return (a.r[0] > 0 ? 1 : 0) + (a.r[1] > 0 ? 1 : 0) + (a.r[2] > 0 ? 1 : 0);
  return (a.r[0] > 0 || a.r[1] > 0 ? 1 : 0) + (a.r[2] > 0 ? 1 : 0);
}

hipError_t launch_point_smooth(double *first, double *second, int nx, int ny, int nz, const PointSmoothArgs &a, hipStream_t stream) {
  const int px = nx + 1, py = ny + 1, pz = nz + 1;
  double *src = first, *dst = second;
  auto swap = [&]() {
    double *t = src;
    src = dst;
    dst = t;
  };
  if (plain_form()) {
    if (a.r[0] > 0) launch_axis<0>(src, dst, px, py, pz, a, stream), swap();
    if (a.r[1] > 0) launch_axis<1>(src, dst, px, py, pz, a, stream), swap();
    if (a.r[2] > 0) launch_axis<2>(src, dst, px, py, pz, a, stream), swap();
    return hipGetLastError();
  }
  if (a.r[0] > 0 || a.r[1] > 0) {
#ifdef DMI_TUNING
    const char *e = getenv("DMI_PSMOOTH_BY");  // tuning experiments (tools/gpu_point_smooth_tune.py): the tile's height
    const int by = e ? atoi(e) : 16;
    if (by == 8) launch_xy<8>(src, dst, px, py, pz, a, stream);
    else if (by == 32 && (size_t)((64 + 2 * a.r[0]) + 64) * (32 + 2 * a.r[1]) * 8 <= 64 * 1024) launch_xy<32>(src, dst, px, py, pz, a, stream);
    else
#endif
    launch_xy<16>(src, dst, px, py, pz, a, stream);
    swap();
  }
  if (a.r[2] > 0) {
#ifdef DMI_TUNING
    const char *e = getenv("DMI_PSMOOTH_KZ");  // ... and the column's height
    const int kz = e ? atoi(e) : 8;
    if (kz == 4) launch_z<4>(src, dst, px, py, pz, a, stream);
    else if (kz == 16) launch_z<16>(src, dst, px, py, pz, a, stream);
    else if (kz == 32) launch_z<32>(src, dst, px, py, pz, a, stream);
    else
#endif
    launch_z<8>(src, dst, px, py, pz, a, stream);
    swap();
  }
  return hipGetLastError();
}

}  // namespace dmi
