// scene_bounds.hip -- the bounds of the scene the depth maps see (dmi_estimate_scene_bounds): per grid axis the element of rank k
// and the element of rank N-1-k of the back-projected pixels' coordinates, exact, by a most-significant-digit radix select on an
// order-preserving 64-bit key.  Six targets -- three axes, lo and hi each -- are selected at once.
//
// Semantics (include/dmi.h states them in full; tests/scene_bounds_np.py restates them on the CPU and the result is identical): f64
// throughout, every operation rounded (-ffp-contract=off), 8g's validity and back-projection operation for operation.
//
// Passes, kPasses times, without a host round trip in between:
//   count    a workgroup visits chunks of kBoundsChunk taking-part pixels of one view (the view's camera arrives through scalar
//            loads), recomputes w and s from the resident planes -- the points are never stored -- and counts, per target, the digit
//            of the keys whose higher bits equal the target's prefix, in LDS histograms that are flushed to global u64 counters once
//            per workgroup.  While an axis's lo and hi still carry the same prefix one histogram serves both.  The first passes see
//            nearly every lane of a wave in one bin (sign and exponent agree): the add is aggregated per wave -- a ballot on the
//            leading lane's bin, one add of its popcount -- for kBoundsAggregateRounds rounds (one), then the lanes left add singly.
//   select   one workgroup: per target the bin that holds its rank (scene_bounds_rules.h), the next digit, the rank left; the
//            counters are cleared for the next pass.  Pass 0 takes N and the trimmed ranks first; the last pass writes the result.
#include "scene_bounds.h"

namespace dmi {
namespace {

using namespace bounds_rules;

template <typename T>
__device__ __forceinline__ T cload(const T *p) {  // wave-uniform address -> scalar load
  return *reinterpret_cast<const T __attribute__((address_space(4))) *>(reinterpret_cast<uintptr_t>(p));
}

__device__ __forceinline__ void count_bin(uint32_t *hist, bool active, int bin, int rounds) {
  const int lane = (int)(threadIdx.x & 63);
  unsigned long long rest = __builtin_amdgcn_ballot_w64(active);
  for (int r = 0; r < rounds && rest; ++r) {
    const int leader = __builtin_ctzll(rest);
    const int leading_bin = __builtin_amdgcn_readlane(bin, leader);
    const unsigned long long same = __builtin_amdgcn_ballot_w64(active && bin == leading_bin);
    if (lane == leader) atomicAdd(hist + leading_bin, (uint32_t)__builtin_popcountll(same));
    rest &= ~same;
  }
  if ((rest >> lane) & 1) atomicAdd(hist + bin, 1u);
}

// RUNTIME: the aggregation rounds and the sharing of histograms come from the launch (tuning builds); otherwise they are the
// constants of scene_bounds.h, and the aggregation loop is unrolled
template <bool RUNTIME>
__global__ __launch_bounds__(kBoundsBlock) void bounds_count_kernel(const double *__restrict__ planes,
                                                                    const ConsistencyCamera *__restrict__ cameras, int W, int H, int step,
                                                                    int Ws, int taking_part, int chunks_per_view, int64_t total_chunks,
                                                                    BoundsAxes A, int pass, const BoundsState *__restrict__ state,
                                                                    unsigned long long *__restrict__ hist, int rounds_given,
                                                                    int share_given) {
  const int rounds = RUNTIME ? rounds_given : kBoundsAggregateRounds;
  const bool share = RUNTIME ? share_given != 0 : true;
  __shared__ uint32_t lds[kTargets * kBins];
  if (pass > 0 && cload(&state->done)) return;  // N == 0: nothing left to select (the whole workgroup leaves)
  uint64_t prefix[kTargets];
  bool shared[3];
#pragma unroll
  for (int t = 0; t < kTargets; ++t) prefix[t] = pass > 0 ? cload(&state->prefix[t]) : 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) shared[a] = share && (pass == 0 || cload(&state->shared[a]) != 0);
  for (int i = threadIdx.x; i < kTargets * kBins; i += kBoundsBlock) lds[i] = 0;
  __syncthreads();

  const int64_t plane = (int64_t)W * H;
  for (int64_t chunk = blockIdx.x; chunk < total_chunks; chunk += gridDim.x) {
    const int view = __builtin_amdgcn_readfirstlane((int)(chunk / chunks_per_view));
    const int first = __builtin_amdgcn_readfirstlane((int)(chunk - (int64_t)view * chunks_per_view)) * kBoundsChunk;
    const ConsistencyCamera *__restrict__ src = cameras + view;
    const double k00 = cload(&src->k[0]), k01 = cload(&src->k[1]), k02 = cload(&src->k[2]), k11 = cload(&src->k[4]),
                 k12 = cload(&src->k[5]);
    double rt[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) rt[q] = cload(&src->rt[q]);
    const double *__restrict__ image = planes + (int64_t)view * plane;
#pragma unroll
    for (int item = 0; item < kBoundsItems; ++item) {
      const int j = first + item * kBoundsBlock + (int)threadIdx.x;  // the j-th taking-part pixel of the view
      const bool inside = j < taking_part;
      const int jy = inside ? j / Ws : 0, jx = inside ? j - jy * Ws : 0;
      const int px = jx * step, py = jy * step;
      const double d = inside ? image[(int64_t)py * W + px] : -1.0;
      const bool valid = d > 0.0;  // the planes hold -1 for everything else
      if (__builtin_amdgcn_ballot_w64(valid) == 0) continue;

      // step 2 of 8g, operation for operation
      const double yn = ((double)py - k12) / k11;
      const double xn = (((double)px - k02) - k01 * yn) / k00;
      const double q0 = xn * d - rt[3], q1 = yn * d - rt[7], q2 = d - rt[11];
      const double w0 = (rt[0] * q0 + rt[4] * q1) + rt[8] * q2;
      const double w1 = (rt[1] * q0 + rt[5] * q1) + rt[9] * q2;
      const double w2 = (rt[2] * q0 + rt[6] * q1) + rt[10] * q2;
      double s[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) s[a] = (A.a[3 * a] * w0 + A.a[3 * a + 1] * w1) + A.a[3 * a + 2] * w2;
      const double inf = __builtin_inf();
      const bool counted = valid && __builtin_fabs(s[0]) < inf && __builtin_fabs(s[1]) < inf && __builtin_fabs(s[2]) < inf;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const uint64_t key = key_of_bits((uint64_t)__double_as_longlong(s[a]));
        const int digit = digit_of(key, pass);
        const uint64_t above = prefix_of(key, pass);
        count_bin(lds + (2 * a) * kBins, counted && above == prefix[2 * a], digit, rounds);
        if (!shared[a]) count_bin(lds + (2 * a + 1) * kBins, counted && above == prefix[2 * a + 1], digit, rounds);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kTargets * kBins; i += kBoundsBlock)
    if (const uint32_t c = lds[i]) atomicAdd(hist + i, (unsigned long long)c);
}

__global__ __launch_bounds__(kBoundsBlock) void bounds_select_kernel(BoundsState *state, unsigned long long *hist, int pass,
                                                                     double trim_fraction) {
  __shared__ uint64_t h[kTargets * kBins];
  __shared__ uint64_t first_rank[kTargets];
  __shared__ int digit[kTargets];
  __shared__ int stop;
  if (pass > 0 && state->done) return;  // the count passes left without counting: the counters are still zero
  for (int i = threadIdx.x; i < kTargets * kBins; i += kBoundsBlock) {
    h[i] = hist[i];
    hist[i] = 0;
  }
  if (threadIdx.x == 0) stop = 0;
  __syncthreads();
  if (pass == 0 && threadIdx.x == 0) {
    uint64_t n = 0;  // every counted point is in axis 0's histogram exactly once
    for (int b = 0; b < kBins; ++b) n += h[b];
    state->n = n;
    const uint64_t k = trim_rank(trim_fraction, n);
    for (int a = 0; a < 3; ++a) {
      first_rank[2 * a] = k;
      first_rank[2 * a + 1] = n ? n - 1 - k : 0;
    }
    if (n == 0) {
      for (int t = 0; t < kTargets; ++t) state->result[t] = __builtin_nan("");
      state->done = 1;
      stop = 1;
    }
  }
  __syncthreads();
  if (stop) return;
  const int t = threadIdx.x;
  if (t < kTargets) {
    const int a = t >> 1;
    const bool shared = pass == 0 || state->shared[a] != 0;
    uint64_t left = 0;
    int bin = bin_of_rank(h + (shared ? 2 * a : t) * kBins, kBins, pass == 0 ? first_rank[t] : state->rank[t], &left);
    if (bin < 0) bin = kBins - 1;  // cannot happen: the rank lies inside what the previous pass counted in the chosen bin
    const uint64_t prefix = ((pass == 0 ? 0 : state->prefix[t]) << kDigitBits) | (uint64_t)bin;
    state->prefix[t] = prefix;
    state->rank[t] = left;
    digit[t] = bin;
    if (pass == kPasses - 1) state->result[t] = __longlong_as_double((long long)bits_of_key(prefix));
  }
  __syncthreads();
  if (t < 3) state->shared[t] = (pass == 0 || state->shared[t] != 0) && digit[2 * t] == digit[2 * t + 1] ? 1u : 0u;
}

#ifdef DMI_TUNING
__global__ __launch_bounds__(kBoundsBlock) void bounds_plain_read_kernel(const double *__restrict__ planes, int64_t total, double *sink) {
  double sum = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kBoundsBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBoundsBlock) sum += planes[i];
  if (sum == 12345.678) *sink = sum;  // keeps the loads; practically never true
}
#endif

// the pixels 0, step, 2 step, ... below `size` (size >= 1, step >= 1; no sum that a step near 2^31 could overflow)
int taking_part_along(int size, int step) { return (size - 1) / step + 1; }

int64_t chunks_per_view(int W, int H, int step) {
  const int64_t taking_part = (int64_t)taking_part_along(W, step) * taking_part_along(H, step);
  return (taking_part + kBoundsChunk - 1) / kBoundsChunk;
}

}  // namespace

unsigned bounds_count_blocks(int n, int W, int H, int pixel_step, int compute_units) {
  const int64_t total = chunks_per_view(W, H, pixel_step) * n;
  const int64_t resident = (int64_t)(compute_units > 0 ? compute_units : 256) * 8;
  const int64_t least = (total + kBoundsMaxChunksPerGroup - 1) / kBoundsMaxChunksPerGroup;  // 32-bit LDS counters
  const int64_t blocks = total < resident ? total : (resident > least ? resident : least);
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

hipError_t launch_bounds_count(const double *planes, const ConsistencyCamera *cameras, int n, int W, int H, int pixel_step,
                               const BoundsAxes &axes, int pass, const BoundsState *state, unsigned long long *hist, unsigned blocks,
                               const BoundsTuning &tuning, hipStream_t stream) {
  const int Ws = taking_part_along(W, pixel_step), Hs = taking_part_along(H, pixel_step);
  const int per_view = (int)chunks_per_view(W, H, pixel_step);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBoundsBlock), 0, stream, planes, cameras, W, H, pixel_step, Ws, Ws * Hs, per_view,
                       (int64_t)per_view * n, axes, pass, state, hist, tuning.aggregate_rounds, tuning.share_histograms);
  };
#ifdef DMI_TUNING
  if (tuning.aggregate_rounds != kBoundsAggregateRounds || !tuning.share_histograms) launch(bounds_count_kernel<true>); else
#endif
  launch(bounds_count_kernel<false>);
  return hipGetLastError();
}

hipError_t launch_bounds_select(BoundsState *state, unsigned long long *hist, int pass, double trim_fraction, hipStream_t stream) {
  hipLaunchKernelGGL(bounds_select_kernel, dim3(1), dim3(kBoundsBlock), 0, stream, state, hist, pass, trim_fraction);
  return hipGetLastError();
}

#ifdef DMI_TUNING
hipError_t launch_bounds_plain_read(const double *planes, int64_t total, double *sink, unsigned blocks, hipStream_t stream) {
  hipLaunchKernelGGL(bounds_plain_read_kernel, dim3(blocks), dim3(kBoundsBlock), 0, stream, planes, total, sink);
  return hipGetLastError();
}
#endif

}  // namespace dmi
