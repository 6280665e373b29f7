// view_set_kernels.hip -- the resident view set's own passes (dmi_views_*): the ingest of staged depths into the resident plane and
// the counters of a step's report, computed where the planes are so that a step moves no plane over PCIe.  All of them are
// bandwidth-bound: 16-byte loads and stores per lane, a grid sized from the compute units with the lanes striding over the rest,
// and per workgroup and counter one 64-bit atomic add behind a reduction across the wave (cross-lane) and through LDS.
//
// Semantics (include/dmi.h states them): every counter is a sum of integers, so it is the same whatever order the
// hardware runs in.
//
//   ingest         out = the staged depth where it is valid and its cost passes the threshold, -1 elsewhere: step 1 of the filters'
//                  definitions, once, so that the set holds normalised depths from then on.
//   report         one read of the plane a step started from and of the plane it wrote (and of the tap counts for the smoothing):
//                  valid pixels before and after, pixels that differ, the sum of the counts over the valid ones.
//   segment roots  after the speckle filter's size pass: a pixel whose label is its own index is its segment's final root (a
//                  tile-local root's label entry is its parent, and the size pass left the final root in it), and size[] there is
//                  the segment's; every segment is counted once, at one read of the label plane.
//   hole roots     the same after the hole fill's merge pass, with the FILLABLE predicate of the output pass on the root's record.
//
// A step's piece starts on a 16-byte boundary of the set's planes (view_set_rules.h: piece_views), and the report insists on it.  An
// add does not: views appended behind an odd number of odd-sized views start 8 bytes off.  The ingest peels the element that stands
// before the first boundary off (elements_before_16), takes four elements per lane and step from there as the report does, and
// leaves the up to three behind the last four, with the peeled one, to the first lanes of workgroup 0.
//
// Hang safety: no workgroup waits for another; every loop runs over a range fixed at the launch.
#include "view_set_kernels.h"

#include "view_set_rules.h"

namespace dmi {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

__device__ __forceinline__ bool valid_depth(double d) { return d > 0.0 && d < __builtin_huge_val(); }  // false for NaN

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {  // lane 0 holds the wave's sum
  for (int offset = 32; offset > 0; offset >>= 1) v += __shfl_down(v, offset);
  return v;
}

// counters[first + k] += the workgroup's sum of mine[k].  Every lane of the workgroup calls it, once.
template <int K>
__device__ __forceinline__ void block_add(const unsigned long long (&mine)[K], int first, unsigned long long *counters) {
  __shared__ unsigned long long s_sum[kWaves][K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const unsigned long long v = wave_sum(mine[k]);
    if (lane == 0) s_sum[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    unsigned long long sum = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) sum += s_sum[w][threadIdx.x];
    if (sum != 0) atomicAdd(counters + first + threadIdx.x, sum);
  }
}

// the element a lane of workgroup 0 takes of the edges: [0, head) and [tail, total), at most one and three; `total`: none
__device__ __forceinline__ uint64_t edge_element(uint64_t head, uint64_t tail, uint64_t total) {
  if (blockIdx.x != 0 || threadIdx.x >= 4) return total;
  const uint64_t t = threadIdx.x;
  return t < head ? t : tail + (t - head);
}

__device__ __forceinline__ double ingest_value(double d, double cost, double threshold, bool has_cost) {
  if (!valid_depth(d)) return -1.0;
  if (has_cost && cost > threshold) return -1.0;  // a NaN cost keeps the depth, as in every filter
  return d;
}

template <bool COST>
__global__ __launch_bounds__(kBlock) void view_set_ingest_kernel(const double *__restrict__ depth, const double *__restrict__ cost,
                                                                 double threshold, double *__restrict__ out, uint64_t total, uint64_t head,
                                                                 unsigned long long *counters) {
  const uint64_t quads = (total - head) / 4, tail = head + 4 * quads;
  unsigned long long mine[1] = {0};
  for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < quads; q += (uint64_t)gridDim.x * kBlock) {
    const uint64_t i = head + 4 * q;
    const double2 d0 = *reinterpret_cast<const double2 *>(depth + i), d1 = *reinterpret_cast<const double2 *>(depth + i + 2);
    double2 c0 = make_double2(0.0, 0.0), c1 = c0;
    if (COST) {
      c0 = *reinterpret_cast<const double2 *>(cost + i);
      c1 = *reinterpret_cast<const double2 *>(cost + i + 2);
    }
    const double2 r0 = make_double2(ingest_value(d0.x, c0.x, threshold, COST), ingest_value(d0.y, c0.y, threshold, COST));
    const double2 r1 = make_double2(ingest_value(d1.x, c1.x, threshold, COST), ingest_value(d1.y, c1.y, threshold, COST));
    *reinterpret_cast<double2 *>(out + i) = r0;
    *reinterpret_cast<double2 *>(out + i + 2) = r1;
    mine[0] += (r0.x > 0.0) + (r0.y > 0.0) + (r1.x > 0.0) + (r1.y > 0.0);
  }
  const uint64_t e = edge_element(head, tail, total);
  if (e < total) {
    const double r = ingest_value(depth[e], COST ? cost[e] : 0.0, threshold, COST);
    out[e] = r;
    mine[0] += r > 0.0;
  }
  block_add(mine, kVsIngested, counters);
}

__device__ __forceinline__ void tally(double before, double after, int32_t aux, unsigned long long (&mine)[4]) {
  mine[0] += before > 0.0;
  mine[1] += after > 0.0;
  mine[2] += before != after;
  mine[3] += after > 0.0 ? (unsigned long long)(uint32_t)aux : 0ull;
}

template <bool AUX>
__global__ __launch_bounds__(kBlock) void view_set_report_kernel(const double *__restrict__ before, const double *__restrict__ after,
                                                                 const int32_t *__restrict__ aux, uint64_t total,
                                                                 unsigned long long *counters) {
  const uint64_t quads = total / 4, tail = 4 * quads;  // (the planes and the counts start on 16-byte boundaries: no peel)
  unsigned long long mine[4] = {0, 0, 0, 0};
  for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < quads; q += (uint64_t)gridDim.x * kBlock) {
    const uint64_t i = 4 * q;
    const double2 b0 = *reinterpret_cast<const double2 *>(before + i), b1 = *reinterpret_cast<const double2 *>(before + i + 2);
    const double2 a0 = *reinterpret_cast<const double2 *>(after + i), a1 = *reinterpret_cast<const double2 *>(after + i + 2);
    int4 x = make_int4(0, 0, 0, 0);
    if (AUX) x = *reinterpret_cast<const int4 *>(aux + i);
    tally(b0.x, a0.x, x.x, mine);
    tally(b0.y, a0.y, x.y, mine);
    tally(b1.x, a1.x, x.z, mine);
    tally(b1.y, a1.y, x.w, mine);
  }
  const uint64_t e = edge_element(0, tail, total);
  if (e < total) tally(before[e], after[e], AUX ? aux[e] : 0, mine);
  block_add(mine, kVsValidBefore, counters);
}

__global__ __launch_bounds__(kBlock) void view_set_segment_roots_kernel(SpecklePiece piece, uint64_t plane, int64_t min_pixels,
                                                                        unsigned long long *counters) {
  unsigned long long mine[2] = {0, 0};
  for (int64_t view = blockIdx.y; view < piece.count; view += gridDim.y) {
    const uint64_t base = (uint64_t)view * plane;
    for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p < plane; p += (uint64_t)gridDim.x * kBlock) {
      if (piece.label[base + p] != (uint32_t)p) continue;  // (kNoLabel is no pixel's index: a plane has at most 2^30)
      mine[0] += 1;
      mine[1] += (int64_t)piece.size[base + p] >= min_pixels;
    }
  }
  block_add(mine, kVsRoots, counters);
}

__global__ __launch_bounds__(kBlock) void view_set_hole_roots_kernel(HolesPiece piece, uint64_t plane, double abs_tolerance,
                                                                     double rel_tolerance, int64_t max_pixels, unsigned long long *counters) {
  namespace rules = holes_rules;
  unsigned long long mine[2] = {0, 0};
  for (int64_t view = blockIdx.y; view < piece.count; view += gridDim.y) {
    const uint64_t base = (uint64_t)view * plane;
    for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p < plane; p += (uint64_t)gridDim.x * kBlock) {
      if (piece.label[base + p] != (uint32_t)p) continue;
      mine[0] += 1;
      const uint64_t lo_bits = piece.rim_lo[base + p], hi_bits = piece.rim_hi[base + p];
      mine[1] += rules::fillable(piece.record[base + p], lo_bits != rules::kNoRimLo, __longlong_as_double((long long)lo_bits),
                                 __longlong_as_double((long long)hi_bits), max_pixels, abs_tolerance, rel_tolerance);
    }
  }
  block_add(mine, kVsRoots, counters);
}

inline uint64_t offset_in_16(const void *p) { return (uint64_t)reinterpret_cast<uintptr_t>(p) & 15; }

dim3 roots_grid(uint64_t plane, int64_t count, int compute_units) {
  // (a row of workgroups per view, as many views at a time as the grid's y extent holds; about eight workgroups per compute unit)
  const unsigned views = (unsigned)(count < 65535 ? count : 65535);
  const unsigned all = view_set_blocks(plane * views, compute_units);
  const unsigned need = (unsigned)((plane + kBlock - 1) / kBlock), share = all / views > 0 ? all / views : 1;
  return dim3(need < share ? need : share, views);
}

}  // namespace

unsigned view_set_blocks(uint64_t items, int compute_units) {
  const uint64_t need = (items + kBlock - 1) / kBlock, cap = (uint64_t)(compute_units > 0 ? compute_units : 1) * 8;
  const uint64_t blocks = need < cap ? need : cap;
  return (unsigned)(blocks > 0 ? blocks : 1);
}

hipError_t launch_view_set_ingest(const double *depth, const double *cost, double threshold, double *out, uint64_t total,
                                  unsigned long long *counters, int compute_units, hipStream_t stream) {
  if (total == 0) return hipSuccess;
  if (offset_in_16(depth) != offset_in_16(out) || (cost && offset_in_16(cost) != offset_in_16(out)) || (offset_in_16(out) & 7))
    return hipErrorInvalidValue;
  uint64_t head = view_set_rules::elements_before_16(offset_in_16(out), 8);
  if (head > total) head = total;
  const unsigned blocks = view_set_blocks((total - head) / 4, compute_units);
  if (cost)
    hipLaunchKernelGGL(view_set_ingest_kernel<true>, dim3(blocks), dim3(kBlock), 0, stream, depth, cost, threshold, out, total, head,
                       counters);
  else
    hipLaunchKernelGGL(view_set_ingest_kernel<false>, dim3(blocks), dim3(kBlock), 0, stream, depth, cost, threshold, out, total, head,
                       counters);
  return hipGetLastError();
}

hipError_t launch_view_set_report(const double *before, const double *after, const int32_t *aux, uint64_t total,
                                  unsigned long long *counters, int compute_units, hipStream_t stream) {
  if (total == 0) return hipSuccess;
  if (offset_in_16(before) || offset_in_16(after) || (aux && offset_in_16(aux))) return hipErrorInvalidValue;
  const unsigned blocks = view_set_blocks(total / 4, compute_units);
  if (aux)
    hipLaunchKernelGGL(view_set_report_kernel<true>, dim3(blocks), dim3(kBlock), 0, stream, before, after, aux, total, counters);
  else
    hipLaunchKernelGGL(view_set_report_kernel<false>, dim3(blocks), dim3(kBlock), 0, stream, before, after, aux, total, counters);
  return hipGetLastError();
}

hipError_t launch_view_set_segment_roots(const SpecklePiece &piece, int32_t W, int32_t H, int64_t min_pixels, unsigned long long *counters,
                                         int compute_units, hipStream_t stream) {
  if (piece.count <= 0) return hipSuccess;
  const uint64_t plane = (uint64_t)W * H;
  hipLaunchKernelGGL(view_set_segment_roots_kernel, roots_grid(plane, piece.count, compute_units), dim3(kBlock), 0, stream, piece, plane,
                     min_pixels, counters);
  return hipGetLastError();
}

hipError_t launch_view_set_hole_roots(const HolesPiece &piece, int32_t W, int32_t H, double abs_tolerance, double rel_tolerance,
                                      int64_t max_pixels, unsigned long long *counters, int compute_units, hipStream_t stream) {
  if (piece.count <= 0) return hipSuccess;
  const uint64_t plane = (uint64_t)W * H;
  hipLaunchKernelGGL(view_set_hole_roots_kernel, roots_grid(plane, piece.count, compute_units), dim3(kBlock), 0, stream, piece, plane,
                     abs_tolerance, rel_tolerance, max_pixels, counters);
  return hipGetLastError();
}

}  // namespace dmi
