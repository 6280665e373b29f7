// depth_points_radius.hip -- the neighbours of every point of a cloud within a radius, and the cloud without the points that have
// too few (dmi_count_point_neighbors, dmi_views_filter_points_radius): what PCL's RadiusOutlierRemoval or Open3D's
// remove_radius_outlier does to a cloud, on the device where the resident view set's cloud already is.
//
// Semantics (include/dmi.h states them in full; tests/depth_points_radius_np.py restates them on the CPU over all pairs, without a
// grid, and the result is identical): j is a neighbour of i != j iff (d_0 d_0 + d_1 d_1) + d_2 d_2 <= radius radius in f64, every
// operation rounded (-ffp-contract=off).  The counts are integers: no order of evaluation changes one, and the only atomics are
// integer sums and maxima, one per workgroup and counter.
//
// Passes, each a launch or a few in stream order:
//   bounds   the thinning's (launch_thin_bounds); the host reads them, refuses a non-finite coordinate, and derives the cell size
//            h >= radius (1 + 2^-10) and the bins
//   keys     a lane per point: (b_2 n_1 + b_1) n_0 + b_0 and its index
//   sort     the thinning's stable radix sort of (key, index) over the bits the key needs
//   ranks    the count kernel's work units: runs of at most `group` sorted positions within one (b_1, b_2) row.  Head flags, their
//            inclusive scan, every unit's first sorted position
//   permute  a lane per sorted position gathers its point's xyz and writes it to three planes in sorted order, coalesced
//   count    a wave per unit, a lane per query.  The unit's candidates are nine runs of the sorted planes -- the rows (b_1 + -1,
//            b_2 + -1), each from the unit's lowest b_0 - 1 to its highest b_0 + 1, clamped --, found by eighteen binary searches
//            over the sorted keys that eighteen lanes make side by side.  The wave streams each run 64 candidates at a time: a
//            coalesced load, a lane each, into the wave's own 64 slots of LDS, then every lane reads every slot (a broadcast: one
//            address for the whole wave) and tests it: ten vector instructions a test, nine of them fp64 (eighteen, with six
//            v_readlane_b32, when the candidates were taken out of the wave's registers: DESIGN.md 8p).  The query itself is among its candidates exactly once and always passes; it is taken out of the count
//            afterwards, by position, which is by index.  The count goes to neighbors[index].
//   compaction  flags and the report's sums (a lane per point, one atomic per workgroup and counter), the exclusive scan of the
//            flags = the output numbering, and the stable scatter of every array of the kept points
#include <algorithm>

#include <rocprim/device/device_scan.hpp>

#include "depth_points_radius.h"
#include "depth_points_search_device.h"

namespace dmi {
namespace {

using namespace radius_rules;

__global__ __launch_bounds__(kBlock) void radius_keys_kernel(const double *__restrict__ p, uint64_t n, RadiusGrid g,
                                                             uint64_t *__restrict__ keys, uint32_t *__restrict__ ids) {
  const uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= n) return;
  uint64_t b[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) b[d] = bin_of(p[3 * v + d], g.lo[d], g.h, g.n[d]);
  keys[v] = thin_rules::key_of(b[0], b[1], b[2], g.n[0], g.n[1]);
  ids[v] = (uint32_t)v;
}

// head[i] = 1 where sorted position i starts a unit
__global__ __launch_bounds__(kBlock) void radius_heads_kernel(const uint64_t *__restrict__ keys, uint64_t n, uint64_t n0, uint32_t group,
                                                              uint32_t *__restrict__ head) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  head[i] = unit_head(i, keys[i], i ? keys[i - 1] : 0, n0, group) ? 1u : 0u;
}

// rank[i] = units up to and including position i: the unit of sorted position i is rank[i] - 1, there are rank[n - 1] units
__global__ __launch_bounds__(kBlock) void radius_starts_kernel(const uint32_t *__restrict__ head, const uint32_t *__restrict__ rank,
                                                               uint64_t n, uint32_t *__restrict__ start,
                                                               unsigned long long *__restrict__ counters) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t u = rank[i] - 1;
  if (head[i]) start[u] = (uint32_t)i;
  if (i == n - 1) {
    start[u + 1] = (uint32_t)n;  // the end of the last unit (u + 1 <= n)
    counters[kRadiusUnits] = (unsigned long long)u + 1;
  }
}

// sorted position i takes its point's xyz: gathered reads, coalesced writes
__global__ __launch_bounds__(kBlock) void radius_permute_kernel(const double *__restrict__ xyz, const uint32_t *__restrict__ ids, uint64_t n,
                                                                double *__restrict__ sorted_xyz) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint64_t u = ids[i];
#pragma unroll
  for (int d = 0; d < 3; ++d) sorted_xyz[(uint64_t)d * n + i] = xyz[3 * u + d];
}

// A wave per unit, a lane per query.  Every lane tests every candidate of the unit's nine runs, which hold every point of the 27
// cells round each of its queries (and more: the cells round the others'); a (query, candidate) pair meets once, for the nine key
// ranges are disjoint.
__global__ __launch_bounds__(kBlock) void radius_count_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ ids,
                                                              const uint32_t *__restrict__ start, const double *__restrict__ sorted_xyz,
                                                              uint64_t n, uint64_t n0, uint64_t n1, uint64_t n2, double r2,
                                                              uint32_t *__restrict__ neighbors, unsigned long long *__restrict__ counters) {
  __shared__ unsigned long long part[kBlock / 64];
  __shared__ double staged[kBlock / 64][64][4];  // a wave's batch of candidates: x, y, z and a word of padding (one b128 and one b64 read)
  double(*const mine)[4] = staged[threadIdx.x >> 6];
  const uint64_t units = counters[kRadiusUnits], waves = (uint64_t)gridDim.x * (kBlock / 64);
  const uint32_t lane = threadIdx.x & 63;
  unsigned long long tests = 0;  // this lane's
  for (uint64_t u = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); u < units; u += waves) {  // (the same trips for the whole wave)
    const uint32_t lo = __builtin_amdgcn_readfirstlane(start[u]), k = __builtin_amdgcn_readfirstlane(start[u + 1]) - lo;  // 1 <= k <= 64
    const bool active = lane < k;
    const uint32_t q = lo + (active ? lane : 0u);  // (a query that is there: unused beyond k)
    const double q0 = sorted_xyz[q], q1 = sorted_xyz[n + q], q2 = sorted_xyz[2 * n + q];
    const uint64_t first = keys[lo], last = keys[lo + k - 1];  // the same row: key / n0
    const uint64_t row = first / n0, b0_min = first - row * n0, b0_max = last - row * n0, b2 = row / n1, b1 = row - b2 * n1;
    // lanes 2 t and 2 t + 1 find the run of row t of the nine; an absent row's run is empty
    uint32_t found = 0;
    if (lane < 18) {
      const int t = (int)(lane >> 1);
      uint64_t from = 0, to = 0;
      if (row_key_range(b0_min, b0_max, b1, b2, t % 3 - 1, t / 3 - 1, n0, n1, n2, &from, &to))
        found = lower_bound(keys, n, (lane & 1) ? to + 1 : from);
    }
    uint32_t count = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const uint32_t s = (uint32_t)__builtin_amdgcn_readlane((int)found, 2 * t), e = (uint32_t)__builtin_amdgcn_readlane((int)found, 2 * t + 1);
      for (uint64_t base = s; base < e; base += 64) {
        const uint32_t left = (uint32_t)(e - base);
        const uint32_t here = (uint32_t)__builtin_amdgcn_readfirstlane((int)(left < 64 ? left : 64));  // (uniform: the loop's bound is a scalar)
        const uint64_t c = base + (lane < here ? lane : 0u);  // (a candidate that is there: unused beyond `here`)
        const double c0 = sorted_xyz[c], c1 = sorted_xyz[n + c], c2 = sorted_xyz[2 * n + c];
        // the wave's own 64 slots of LDS: a lane writes its candidate, then every lane reads every slot (one address for the whole
        // wave: a broadcast).  The LDS takes a wave's accesses in order; the fences keep the compiler from moving them.
        wave_fence();  // (the reads of the batch before are done)
        mine[lane][0] = c0, mine[lane][1] = c1, mine[lane][2] = c2;
        wave_fence();
#pragma unroll 8
        for (uint32_t j = 0; j < here; ++j) {
          const double d0 = mine[j][0] - q0, d1 = mine[j][1] - q1, d2 = mine[j][2] - q2;
          const double dd = (d0 * d0 + d1 * d1) + d2 * d2;
          count += dd <= r2 ? 1u : 0u;
        }
        tests += active ? here : 0u;
      }
    }
    // The query itself was among the candidates exactly once -- its own cell lies in the middle row's range, and the nine ranges
    // are disjoint -- and passed the test: x - x is +0 for a finite x, and 0 <= r2.  It is taken out here, by its position, which
    // is by its index; no other candidate at the same place is.
    if (active) neighbors[ids[q]] = count - 1;
  }
  const unsigned long long made = block_sum(tests, part);
  if (threadIdx.x == 0 && made) atomicAdd(&counters[kRadiusTests], made);
}

// The entries i of kept[0 .. n], a lane each, the workgroups striding over them (entry n, the scan's total, is not kept); the
// report's sums stay per lane and leave the workgroup in one atomic each.
__global__ __launch_bounds__(kBlock) void radius_flags_kernel(const uint32_t *__restrict__ neighbors, uint64_t n, uint32_t min_neighbors,
                                                              uint32_t *__restrict__ kept, unsigned long long *__restrict__ counters) {
  __shared__ unsigned long long part[kBlock / 64];
  unsigned long long isolated = 0, most = 0, sum = 0;
  for (uint64_t begin = (uint64_t)blockIdx.x * kBlock; begin <= n; begin += (uint64_t)gridDim.x * kBlock) {
    const uint64_t i = begin + threadIdx.x;
    if (i > n) continue;
    bool keep = false;
    if (i < n) {
      const uint32_t k = neighbors[i];
      keep = k >= min_neighbors;
      isolated += k == 0 ? 1u : 0u;
      most = k > most ? k : most;
      sum += k;
    }
    kept[i] = keep ? 1u : 0u;
  }
  const unsigned long long block_isolated = block_sum(isolated, part), block_total = block_sum(sum, part), block_most = block_max(most, part);
  if (threadIdx.x == 0) {
    if (block_isolated) atomicAdd(&counters[kRadiusIsolated], block_isolated);
    if (block_total) atomicAdd(&counters[kRadiusSum], block_total);
    if (block_most) atomicMax(&counters[kRadiusMost], block_most);
  }
}

// input point i, if kept, goes to output number out_index[i] with every array it has: words are copied, never values
__global__ __launch_bounds__(kBlock) void radius_scatter_kernel(RadiusCloud cloud, const uint32_t *__restrict__ kept,
                                                                const uint32_t *__restrict__ out_index, const uint32_t *__restrict__ neighbors,
                                                                thin_rules::Layout layout, uint64_t neighbors_offset,
                                                                unsigned char *__restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= cloud.n || !kept[i]) return;
  const uint64_t w = out_index[i];
  const unsigned long long *const xyz = reinterpret_cast<const unsigned long long *>(cloud.xyz) + 3 * i;
  const uint32_t *const normal = reinterpret_cast<const uint32_t *>(cloud.normal) + 3 * i;
  unsigned long long *const out_xyz = reinterpret_cast<unsigned long long *>(out + layout.xyz + w * 24);
  uint32_t *const out_normal = reinterpret_cast<uint32_t *>(out + layout.normal + w * 12);
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    out_xyz[d] = xyz[d];
    out_normal[d] = normal[d];
  }
  *reinterpret_cast<int32_t *>(out + layout.view + w * 4) = cloud.view[i];
  *reinterpret_cast<int32_t *>(out + layout.pixel + w * 4) = cloud.pixel[i];
  *reinterpret_cast<int32_t *>(out + layout.count + w * 4) = cloud.count[i];
  if (cloud.members) *reinterpret_cast<uint32_t *>(out + layout.members + w * 4) = cloud.members[i];
  *reinterpret_cast<uint32_t *>(out + neighbors_offset + w * 4) = neighbors[i];
}

unsigned blocks(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

hipError_t launch_radius_front(const double *xyz, uint64_t n, const RadiusGrid &g, uint32_t group_points, const RadiusScratch &s,
                               hipEvent_t events[5], RadiusSorted *out, hipStream_t stream) {
  const int bits = thin_rules::key_bits(g.n[0], g.n[1], g.n[2]);
  hipError_t e = hipEventRecord(events[0], stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(radius_keys_kernel, dim3(blocks(n)), dim3(kBlock), 0, stream, xyz, n, g, s.keys[0], s.ids[0]);
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
  hipLaunchKernelGGL(radius_heads_kernel, dim3(blocks(n)), dim3(kBlock), 0, stream, sorted_keys, n, g.n[0], group_points, head);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  bytes = s.temp_bytes;
  if ((e = rocprim::inclusive_scan(s.temp, bytes, head, rank, (size_t)n, rocprim::plus<uint32_t>(), stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(radius_starts_kernel, dim3(blocks(n)), dim3(kBlock), 0, stream, head, rank, n, s.start, s.counters);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipEventRecord(events[3], stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(radius_permute_kernel, dim3(blocks(n)), dim3(kBlock), 0, stream, xyz, sorted_ids, n, s.sorted_xyz);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  out->keys = sorted_keys;
  out->ids = sorted_ids;
  out->free_words = head;
  return hipEventRecord(events[4], stream);
}

hipError_t launch_radius_counts(const double *xyz, uint64_t n, const RadiusGrid &g, double r2, uint32_t min_neighbors, uint32_t group_points,
                                const RadiusScratch &s, hipEvent_t events[7], RadiusKept *out, hipStream_t stream) {
  RadiusSorted sorted{};
  hipError_t e = launch_radius_front(xyz, n, g, group_points, s, events, &sorted, stream);
  if (e != hipSuccess) return e;
  const uint64_t *const sorted_keys = sorted.keys;
  const uint32_t *const sorted_ids = sorted.ids;
  uint32_t *const head = sorted.free_words, *const rank = head + (n + 1);
  const unsigned count_blocks = (unsigned)std::min<uint64_t>(std::max<uint64_t>((n + 31) / 32, 1), kCountBlocks);
  hipLaunchKernelGGL(radius_count_kernel, dim3(count_blocks), dim3(kBlock), 0, stream, sorted_keys, sorted_ids, s.start, s.sorted_xyz, n,
                     g.n[0], g.n[1], g.n[2], r2, s.neighbors, s.counters);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipEventRecord(events[5], stream)) != hipSuccess) return e;
  // ... and the head flags and ranks, read for the last time by the starts, the kept flags and the output numbers
  uint32_t *const kept = head, *const out_index = rank;
  hipLaunchKernelGGL(radius_flags_kernel, dim3(std::min<unsigned>(blocks(n + 1), kStrideBlocks)), dim3(kBlock), 0, stream, s.neighbors, n,
                     min_neighbors, kept, s.counters);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  size_t bytes = s.temp_bytes;
  if ((e = rocprim::exclusive_scan(s.temp, bytes, kept, out_index, (uint32_t)0, (size_t)(n + 1), rocprim::plus<uint32_t>(), stream)) !=
      hipSuccess)
    return e;
  out->kept = kept;
  out->out_index = out_index;
  return hipEventRecord(events[6], stream);
}

hipError_t launch_radius_compaction(const RadiusCloud &cloud, const RadiusKept &kept, const uint32_t *neighbors,
                                    const thin_rules::Layout &layout, uint64_t neighbors_offset, unsigned char *out, hipStream_t stream) {
  hipLaunchKernelGGL(radius_scatter_kernel, dim3(blocks(cloud.n)), dim3(kBlock), 0, stream, cloud, kept.kept, kept.out_index, neighbors, layout,
                     neighbors_offset, out);
  return hipGetLastError();
}

}  // namespace dmi
