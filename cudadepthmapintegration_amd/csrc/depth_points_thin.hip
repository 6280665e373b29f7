// depth_points_thin.hip -- a point cloud thinned and merged on a voxel grid (dmi_thin_point_cloud, dmi_views_thin_points): one
// point per occupied cell, at the mean of its members, with a merged normal; what PCL's VoxelGrid or Open3D's voxel_down_sample
// does to a cloud, on the device where the resident view set's cloud already is.
//
// Semantics (include/dmi.h states them in full; tests/depth_points_thin_np.py restates them on the CPU and the result is
// identical): dmi_decimate_isosurface's bounds and bins, a cell per occupied bin in (b_2, b_1, b_0) order, its members in ascending
// input index, every sum made by one lane -- or by the lanes of one wave in step -- in the definition's order.  f64, every operation
// rounded (-ffp-contract=off).  No floating point atomics; the integer atomics are sums, maxima and a queue whose order no result
// depends on.
//
// Passes, each a launch or a few in stream order:
//   bounds   per block the minima and maxima of the coordinates as order-preserving integers (wave shuffles, then LDS), one integer
//            atomic min / max per block and bound; a non-finite coordinate sets a flag.  The host reads them, refuses, or derives
//            the bins
//   keys     a lane per point: (b_2 n_1 + b_1) n_0 + b_0 and its index
//   sort     rocPRIM radix sort of (key, index) over the bits the key needs; stable: a cell's members ascend in index
//   ranks    head flags, their inclusive scan = cell number + 1, every cell's first sorted position; a lane per cell: its size,
//            whether it is kept, the report's maximum and multi-view count (kept per lane, one atomic per workgroup), and the queue
//            of the kept cells above the threshold (one atomic per wave that queues any); the exclusive scan of the kept flags =
//            the output numbering and, at its end, the output's size
//   representatives
//            permute: a lane per sorted position gathers its member's xyz, normal and count (40 bytes from three arrays) and
//            writes them to planes in sorted order, coalesced: a cell's members are then one contiguous run of every plane.
//            lanes: a lane per cell at or below the threshold adds its run in order: neighbouring lanes read neighbouring runs.
//            waves: a wave per queued cell loads 64 members at a time, a lane each, and every lane adds them in order from the
//            wave's registers (v_readlane_b32): the loads are coalesced, the additions are the definition's.
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "depth_points_thin.h"

namespace dmi {
namespace {

using namespace thin_rules;

constexpr int kBoundsBlocks = 1024;  // at most: the bounds pass strides over the points
constexpr unsigned kStrideBlocks = 4096;  // at most, where a pass ends in one atomic per workgroup: it strides over its cells

// doubles as unsigned integers of the same order (-0.0 below +0.0: the bins do not see the difference)
__device__ __forceinline__ unsigned long long ordered_bits(double x) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | (1ull << 63));
}

__device__ __forceinline__ unsigned long long shuffle_xor(unsigned long long x, int mask) {
  const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)x, mask, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(x >> 32), mask, 64);
  return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(kBlock) void thin_bounds_kernel(const double *__restrict__ p, uint64_t n,
                                                             unsigned long long *__restrict__ counters) {
  __shared__ unsigned long long part[kBlock / 64][7];
  unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull}, bad = 0;
  for (uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (uint64_t)gridDim.x * kBlock) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double x = p[3 * v + d];
      if (x - x != 0.0) {  // an infinity or a NaN
        bad = 1;
      } else {
        const unsigned long long o = ordered_bits(x);
        lo[d] = o < lo[d] ? o : lo[d];
        hi[d] = o > hi[d] ? o : hi[d];
      }
    }
  }
  for (int mask = 32; mask >= 1; mask >>= 1) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const unsigned long long a = shuffle_xor(lo[d], mask), b = shuffle_xor(hi[d], mask);
      lo[d] = a < lo[d] ? a : lo[d];
      hi[d] = b > hi[d] ? b : hi[d];
    }
    bad |= shuffle_xor(bad, mask);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      part[wave][d] = lo[d];
      part[wave][3 + d] = hi[d];
    }
    part[wave][6] = bad;
  }
  __syncthreads();
  if (threadIdx.x < 7) {
    const int e = threadIdx.x;
    unsigned long long r = part[0][e];
    for (int w = 1; w < kBlock / 64; ++w) {
      const unsigned long long x = part[w][e];
      r = e < 3 ? (x < r ? x : r) : e < 6 ? (x > r ? x : r) : (r | x);
    }
    if (e < 3) atomicMin(&counters[kThinLo + e], r);
    else if (e < 6) atomicMax(&counters[kThinHi + e - 3], r);
    else if (r) atomicOr(&counters[kThinNonFinite], 1ull);
  }
}

__global__ __launch_bounds__(kBlock) void thin_keys_kernel(const double *__restrict__ p, uint64_t n, ThinGrid g,
                                                           uint64_t *__restrict__ keys, uint32_t *__restrict__ ids) {
  const uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= n) return;
  uint64_t b[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double q = floor((p[3 * v + d] - g.lo[d]) / g.h);  // 0 <= q <= n_d - 1: lo_d <= p <= hi_d and both roundings are monotone
    b[d] = (uint64_t)q;
  }
  keys[v] = key_of(b[0], b[1], b[2], g.n[0], g.n[1]);
  ids[v] = (uint32_t)v;
}

// head[i] = 1 where sorted position i starts a cell
__global__ __launch_bounds__(kBlock) void thin_heads_kernel(const uint64_t *__restrict__ keys, uint64_t n, uint32_t *__restrict__ head) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

// rank[i] = cells up to and including position i: the cell of sorted position i is rank[i] - 1, there are rank[n - 1] cells
__global__ __launch_bounds__(kBlock) void thin_starts_kernel(const uint32_t *__restrict__ head, const uint32_t *__restrict__ rank,
                                                             uint64_t n, uint32_t *__restrict__ start,
                                                             unsigned long long *__restrict__ counters) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = rank[i] - 1;
  if (head[i]) start[c] = (uint32_t)i;
  if (i == n - 1) {
    start[c + 1] = (uint32_t)n;  // the end of the last cell (c + 1 <= n)
    counters[kThinCells] = (unsigned long long)c + 1;
  }
}

__device__ __forceinline__ unsigned wave_max(unsigned x) {
  for (int mask = 32; mask >= 1; mask >>= 1) {
    const unsigned y = (unsigned)__shfl_xor((int)x, mask, 64);
    x = y > x ? y : x;
  }
  return x;
}

__device__ __forceinline__ unsigned long long lane_zero(unsigned long long x) {  // lane 0's value in every lane
  const unsigned lo = (unsigned)__shfl((int)(unsigned)x, 0, 64), hi = (unsigned)__shfl((int)(unsigned)(x >> 32), 0, 64);
  return ((unsigned long long)hi << 32) | lo;
}

// the sum of `x` over the workgroup, in thread 0 (LDS `part`: kBlock / 64 entries; every thread calls it)
__device__ __forceinline__ unsigned long long block_sum(unsigned long long x, unsigned long long *part) {
  for (int mask = 32; mask >= 1; mask >>= 1) x += shuffle_xor(x, mask);
  __syncthreads();  // (part may still be read from an earlier call)
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = x;
  __syncthreads();
  unsigned long long sum = 0;
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) sum += part[w];
  return sum;
}

// The entries c of kept[0 .. n], a lane each, the workgroups striding over them: cells beyond the last one (and entry n, the
// scan's total) are not kept.  The report's maximum and multi-view count are kept per lane and leave the workgroup in one atomic
// each: one per wave cost more than everything else in the pass together.  A wave's queued cells take their slots
// with one atomic; the queue's order decides nothing.
__global__ __launch_bounds__(kBlock) void thin_kept_kernel(const uint32_t *__restrict__ rank_last, const uint32_t *__restrict__ start,
                                                           const uint32_t *__restrict__ ids, const int32_t *__restrict__ view,
                                                           uint64_t n, uint32_t min_points, uint32_t threshold,
                                                           uint32_t *__restrict__ kept, uint32_t *__restrict__ queue,
                                                           uint64_t queue_capacity, unsigned long long *__restrict__ counters) {
  __shared__ unsigned long long part[kBlock / 64];
  __shared__ unsigned wave_largest[kBlock / 64];
  const uint64_t cells = *rank_last;
  const int lane = threadIdx.x & 63;
  unsigned largest = 0;
  unsigned long long multis = 0;
  for (uint64_t first = (uint64_t)blockIdx.x * kBlock; first <= n; first += (uint64_t)gridDim.x * kBlock) {  // (the same trips for the whole workgroup)
    const uint64_t c = first + threadIdx.x;
    uint32_t k = 0;
    bool keep = false, queued = false;
    if (c < n && c < cells) {
      const uint32_t lo = start[c];
      k = start[c + 1] - lo;
      keep = k >= min_points;
      if (keep) {
        multis += view[ids[lo]] != view[ids[lo + k - 1]] ? 1u : 0u;
        queued = wave_cell(k, threshold);
      }
    }
    if (c <= n) kept[c] = keep ? 1u : 0u;
    largest = k > largest ? k : largest;
    const unsigned long long pushing = __builtin_amdgcn_ballot_w64(queued);
    if (pushing) {
      unsigned long long base = 0;
      if (lane == 0) base = atomicAdd(&counters[kThinQueued], (unsigned long long)__builtin_popcountll(pushing));
      base = lane_zero(base);
      const unsigned long long slot = base + (unsigned long long)__builtin_popcountll(pushing & ((1ull << lane) - 1));
      if (queued && slot < queue_capacity) queue[slot] = (uint32_t)c;
    }
  }
  largest = wave_max(largest);
  if (lane == 0) wave_largest[threadIdx.x >> 6] = largest;
  const unsigned long long block_multis = block_sum(multis, part);  // (its barriers order wave_largest too)
  if (threadIdx.x == 0) {
    unsigned most = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) most = wave_largest[w] > most ? wave_largest[w] : most;
    if (most) atomicMax(&counters[kThinLargest], (unsigned long long)most);
    if (block_multis) atomicAdd(&counters[kThinMultiView], block_multis);
  }
}

// sorted position i takes its member's xyz, normal and count: gathered reads, coalesced writes
__global__ __launch_bounds__(kBlock) void thin_permute_kernel(ThinCloud cloud, const uint32_t *__restrict__ ids,
                                                              double *__restrict__ sorted_xyz, float *__restrict__ sorted_normal,
                                                              int32_t *__restrict__ sorted_count) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x, n = cloud.n;
  if (i >= n) return;
  const uint64_t u = ids[i];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    sorted_xyz[(uint64_t)d * n + i] = cloud.xyz[3 * u + d];
    sorted_normal[(uint64_t)d * n + i] = cloud.normal[3 * u + d];
  }
  sorted_count[i] = cloud.count[u];
}

// the running sums of a cell: the first member starts them (no 0.0 + x: a -0.0 stays one), every other is added in order
struct CellSums {
  double s[3], t[3];
  float first_normal[3];
  int32_t count;
  __device__ __forceinline__ void begin(const double x[3], const float nrm[3], int32_t c) {
#pragma unroll
    for (int d = 0; d < 3; ++d) s[d] = x[d], first_normal[d] = nrm[d], t[d] = (double)nrm[d];
    count = c;
  }
  __device__ __forceinline__ void add(const double x[3], const float nrm[3], int32_t c) {
#pragma unroll
    for (int d = 0; d < 3; ++d) s[d] = s[d] + x[d], t[d] = t[d] + (double)nrm[d];
    count = c > count ? c : count;
  }
};

// step 4 for a cell of k members whose sums are complete, stored at output number w; true when its normal is not the zero vector
__device__ __forceinline__ bool write_cell(const CellSums &sums, uint32_t k, uint64_t w, int32_t view, int32_t pixel, const Layout &layout,
                                           unsigned char *__restrict__ out) {
  const double kd = (double)k;
  float nrm[3];
  if (k == 1) {
#pragma unroll
    for (int d = 0; d < 3; ++d) nrm[d] = sums.first_normal[d];
  } else {
    const double length = sqrt((sums.t[0] * sums.t[0] + sums.t[1] * sums.t[1]) + sums.t[2] * sums.t[2]);
    const bool has = length > 0.0 && length < __builtin_inf();
#pragma unroll
    for (int d = 0; d < 3; ++d) nrm[d] = has ? (float)(sums.t[d] / length) : 0.0f;
  }
  double *const xyz = reinterpret_cast<double *>(out + layout.xyz + w * 24);
  float *const normal = reinterpret_cast<float *>(out + layout.normal + w * 12);
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    xyz[d] = sums.s[d] / kd;
    normal[d] = nrm[d];
  }
  *reinterpret_cast<int32_t *>(out + layout.view + w * 4) = view;
  *reinterpret_cast<int32_t *>(out + layout.pixel + w * 4) = pixel;
  *reinterpret_cast<int32_t *>(out + layout.count + w * 4) = sums.count;
  *reinterpret_cast<uint32_t *>(out + layout.members + w * 4) = k;
  return nrm[0] != 0.0f || nrm[1] != 0.0f || nrm[2] != 0.0f;
}

// A lane per cell at or below the threshold: its run of the sorted planes, added in order.
__global__ __launch_bounds__(kBlock) void thin_lane_cells_kernel(ThinCloud cloud, const uint32_t *__restrict__ ids,
                                                                 const uint32_t *__restrict__ start, const uint32_t *__restrict__ kept,
                                                                 const uint32_t *__restrict__ out_index, uint64_t cells, uint32_t threshold,
                                                                 const double *__restrict__ sorted_xyz, const float *__restrict__ sorted_normal,
                                                                 const int32_t *__restrict__ sorted_count, Layout layout,
                                                                 unsigned char *__restrict__ out, unsigned long long *__restrict__ counters) {
  __shared__ unsigned long long part[kBlock / 64];
  const uint64_t n = cloud.n;
  unsigned long long with_normal = 0;  // this lane's: one atomic per workgroup at the end
  for (uint64_t begin = (uint64_t)blockIdx.x * kBlock; begin < cells; begin += (uint64_t)gridDim.x * kBlock) {
    const uint64_t c = begin + threadIdx.x;
    if (c >= cells || !kept[c]) continue;
    const uint32_t lo = start[c], k = start[c + 1] - lo;
    if (wave_cell(k, threshold)) continue;
    CellSums sums;
    for (uint32_t j = 0; j < k; ++j) {
      const uint64_t i = (uint64_t)lo + j;
      const double x[3] = {sorted_xyz[i], sorted_xyz[n + i], sorted_xyz[2 * n + i]};
      const float nrm[3] = {sorted_normal[i], sorted_normal[n + i], sorted_normal[2 * n + i]};
      if (j == 0) sums.begin(x, nrm, sorted_count[i]);
      else sums.add(x, nrm, sorted_count[i]);
    }
    const uint64_t first = ids[lo];
    with_normal += write_cell(sums, k, out_index[c], cloud.view[first], cloud.pixel[first], layout, out) ? 1u : 0u;
  }
  const unsigned long long found = block_sum(with_normal, part);
  if (threadIdx.x == 0 && found) atomicAdd(&counters[kThinWithNormal], found);
}

__device__ __forceinline__ double read_lane(double x, int lane) {  // `lane` is wave-uniform
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane), hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float read_lane(float x, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), lane));
}

// A wave per queued cell: 64 members at a time, a lane each; then every lane adds them in order out of the wave's registers.
__global__ __launch_bounds__(kBlock) void thin_wave_cells_kernel(ThinCloud cloud, const uint32_t *__restrict__ ids,
                                                                 const uint32_t *__restrict__ start, const uint32_t *__restrict__ out_index,
                                                                 const uint32_t *__restrict__ queue, uint64_t queued,
                                                                 const double *__restrict__ sorted_xyz, const float *__restrict__ sorted_normal,
                                                                 const int32_t *__restrict__ sorted_count, Layout layout,
                                                                 unsigned char *__restrict__ out, unsigned long long *__restrict__ counters) {
  __shared__ unsigned long long part[kBlock / 64];
  const uint64_t n = cloud.n, waves = (uint64_t)gridDim.x * (kBlock / 64);
  const int lane = threadIdx.x & 63;
  unsigned long long with_normal = 0;  // lane 0's: the cells of this wave that have a normal
  for (uint64_t q = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); q < queued; q += waves) {  // (the same trips for the whole wave)
    const uint32_t c = __builtin_amdgcn_readfirstlane(queue[q]);
    const uint32_t lo = __builtin_amdgcn_readfirstlane(start[c]), k = __builtin_amdgcn_readfirstlane(start[c + 1]) - lo;
    CellSums sums;
    for (uint32_t base = 0; base < k; base += 64) {
      const uint32_t left = k - base, here = left < 64 ? left : 64;
      const uint64_t i = (uint64_t)lo + base + ((uint32_t)lane < here ? (uint32_t)lane : 0u);  // (a member that is there: unused beyond `here`)
      const double x0 = sorted_xyz[i], x1 = sorted_xyz[n + i], x2 = sorted_xyz[2 * n + i];
      const float n0 = sorted_normal[i], n1 = sorted_normal[n + i], n2 = sorted_normal[2 * n + i];
      const int32_t cnt = sorted_count[i];
      for (uint32_t j = 0; j < here; ++j) {
        const double x[3] = {read_lane(x0, (int)j), read_lane(x1, (int)j), read_lane(x2, (int)j)};
        const float nrm[3] = {read_lane(n0, (int)j), read_lane(n1, (int)j), read_lane(n2, (int)j)};
        const int32_t m = __builtin_amdgcn_readlane(cnt, (int)j);
        if (base + j == 0) sums.begin(x, nrm, m);
        else sums.add(x, nrm, m);
      }
    }
    if (lane == 0) {
      const uint64_t first = ids[lo];
      with_normal += write_cell(sums, k, out_index[c], cloud.view[first], cloud.pixel[first], layout, out) ? 1u : 0u;
    }
  }
  const unsigned long long found = block_sum(with_normal, part);
  if (threadIdx.x == 0 && found) atomicAdd(&counters[kThinWithNormal], found);
}

unsigned blocks(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

hipError_t thin_sort_pairs(void *temp, size_t *temp_bytes, uint64_t *ka, uint64_t *kb, uint32_t *va, uint32_t *vb, uint64_t n, int bits,
                           uint64_t **sorted_keys, uint32_t **sorted_values, hipStream_t stream) {
  rocprim::double_buffer<uint64_t> keys(ka, kb);
  rocprim::double_buffer<uint32_t> values(va, vb);
  size_t bytes = *temp_bytes;
  const hipError_t e = rocprim::radix_sort_pairs(temp, bytes, keys, values, (size_t)n, 0u, (unsigned)bits, stream);
  if (!temp) *temp_bytes = bytes;
  if (sorted_keys) *sorted_keys = keys.current();
  if (sorted_values) *sorted_values = values.current();
  return e;
}

// the storage rocPRIM asks for: the largest of the sort's (all 64 key bits: the bins are not known yet) and the two scans'
hipError_t thin_temp_bytes(uint64_t n, size_t *bytes) {
  size_t a = 0, b = 0, c = 0;
  hipError_t e = thin_sort_pairs(nullptr, &a, nullptr, nullptr, nullptr, nullptr, std::max<uint64_t>(n, 1), 64, nullptr, nullptr, nullptr);
  if (e != hipSuccess) return e;
  e = rocprim::inclusive_scan(nullptr, b, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)(n + 1), rocprim::plus<uint32_t>(), nullptr);
  if (e != hipSuccess) return e;
  e = rocprim::exclusive_scan(nullptr, c, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t)0, (size_t)(n + 1), rocprim::plus<uint32_t>(),
                              nullptr);
  *bytes = std::max<size_t>(std::max(std::max(a, b), c), 16);
  return e;
}

double thin_decode_bound(unsigned long long ordered) {
  const unsigned long long u = (ordered >> 63) ? (ordered & ~(1ull << 63)) : ~ordered;
  double x;
  static_assert(sizeof(x) == sizeof(u), "f64");
  __builtin_memcpy(&x, &u, sizeof(x));
  return x;
}

hipError_t launch_thin_bounds(const ThinCloud &cloud, unsigned long long *counters, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(counters, 0xff, 3 * sizeof(unsigned long long), stream);  // the minima start at the top
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(counters + 3, 0, (kThinCounters - 3) * sizeof(unsigned long long), stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(thin_bounds_kernel, dim3(std::min<unsigned>(blocks(cloud.n), kBoundsBlocks)), dim3(kBlock), 0, stream, cloud.xyz,
                     cloud.n, counters);
  return hipGetLastError();
}

hipError_t launch_thin_cells(const ThinCloud &cloud, const ThinGrid &g, uint32_t min_points, uint32_t wave_cell_points,
                             const ThinScratch &s, hipEvent_t events[4], ThinRanks *ranks, hipStream_t stream) {
  const uint64_t n = cloud.n;
  const int bits = key_bits(g.n[0], g.n[1], g.n[2]);
  hipError_t e = hipEventRecord(events[0], stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(thin_keys_kernel, dim3(blocks(n)), dim3(kBlock), 0, stream, cloud.xyz, n, g, s.keys[0], s.ids[0]);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipEventRecord(events[1], stream)) != hipSuccess) return e;
  uint64_t *sorted_keys = nullptr;
  uint32_t *sorted_ids = nullptr;
  size_t bytes = s.temp_bytes;
  if ((e = thin_sort_pairs(s.temp, &bytes, s.keys[0], s.keys[1], s.ids[0], s.ids[1], n, bits, &sorted_keys, &sorted_ids, stream)) != hipSuccess)
    return e;
  if ((e = hipEventRecord(events[2], stream)) != hipSuccess) return e;
  // the key array the sort did not end in takes the head flags and the ranks ...
  uint64_t *const other_keys = sorted_keys == s.keys[0] ? s.keys[1] : s.keys[0];
  uint32_t *const head = reinterpret_cast<uint32_t *>(other_keys), *const rank = head + (n + 1);
  hipLaunchKernelGGL(thin_heads_kernel, dim3(blocks(n)), dim3(kBlock), 0, stream, sorted_keys, n, head);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  bytes = s.temp_bytes;
  if ((e = rocprim::inclusive_scan(s.temp, bytes, head, rank, (size_t)n, rocprim::plus<uint32_t>(), stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(thin_starts_kernel, dim3(blocks(n)), dim3(kBlock), 0, stream, head, rank, n, s.start, s.counters);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // ... and the sorted keys, read for the last time by the head flags, the kept flags and the output numbers
  uint32_t *const kept = reinterpret_cast<uint32_t *>(sorted_keys), *const out_index = kept + (n + 1);
  hipLaunchKernelGGL(thin_kept_kernel, dim3(std::min<unsigned>(blocks(n + 1), kStrideBlocks)), dim3(kBlock), 0, stream, rank + (n - 1), s.start, sorted_ids, cloud.view, n,
                     min_points, wave_cell_points, kept, s.queue, s.queue_capacity, s.counters);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  bytes = s.temp_bytes;
  if ((e = rocprim::exclusive_scan(s.temp, bytes, kept, out_index, (uint32_t)0, (size_t)(n + 1), rocprim::plus<uint32_t>(), stream)) !=
      hipSuccess)
    return e;
  ranks->sorted_ids = sorted_ids;
  ranks->kept = kept;
  ranks->out_index = out_index;
  return hipEventRecord(events[3], stream);
}

hipError_t launch_thin_representatives(const ThinCloud &cloud, const ThinScratch &s, const ThinRanks &r, uint64_t cells, uint64_t queued,
                                       uint32_t wave_cell_points, const Layout &layout, unsigned char *out, hipStream_t stream) {
  const uint64_t n = cloud.n;
  hipLaunchKernelGGL(thin_permute_kernel, dim3(blocks(n)), dim3(kBlock), 0, stream, cloud, r.sorted_ids, s.sorted_xyz, s.sorted_normal,
                     s.sorted_count);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(thin_lane_cells_kernel, dim3(std::min<unsigned>(blocks(cells), kStrideBlocks)), dim3(kBlock), 0, stream, cloud, r.sorted_ids, s.start, r.kept, r.out_index,
                     cells, wave_cell_points, s.sorted_xyz, s.sorted_normal, s.sorted_count, layout, out, s.counters);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (queued) {
    hipLaunchKernelGGL(thin_wave_cells_kernel, dim3(std::min<unsigned>(blocks(queued * 64), kStrideBlocks)), dim3(kBlock), 0, stream, cloud,
                       r.sorted_ids, s.start, r.out_index, s.queue, queued, s.sorted_xyz, s.sorted_normal, s.sorted_count, layout, out,
                       s.counters);
    e = hipGetLastError();
  }
  return e;
}

}  // namespace dmi
