// depth_points_search_device.h -- what the kernels that search a cloud by the radius grid share on the device (depth_points_radius.hip,
// depth_points_planes.hip): the sums and maxima of a workgroup that end in one atomic each, the fence that orders
// a wave's own LDS accesses, and the binary search over the sorted keys.  Private: never installed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "depth_points_radius_rules.h"

namespace dmi {
namespace {

using radius_rules::kBlock;

constexpr unsigned kStrideBlocks = 4096;  // at most, where a pass ends in one atomic per workgroup: it strides over its entries
constexpr unsigned kCountBlocks = 8192;   // at most: the waves of the count kernel stride over the units

__device__ __forceinline__ unsigned long long shuffle_xor(unsigned long long x, int mask) {
  const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)x, mask, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(x >> 32), mask, 64);
  return ((unsigned long long)hi << 32) | lo;
}

// the sum of `x` over the workgroup, in every thread (LDS `part`: kBlock / 64 entries; every thread calls it)
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

__device__ __forceinline__ unsigned long long block_max(unsigned long long x, unsigned long long *part) {
  for (int mask = 32; mask >= 1; mask >>= 1) {
    const unsigned long long y = shuffle_xor(x, mask);
    x = y > x ? y : x;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = x;
  __syncthreads();
  unsigned long long most = 0;
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) most = part[w] > most ? part[w] : most;
  return most;
}

// orders the LDS accesses of one wave among themselves: nothing crosses it, at compile time or at run time
__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// the first sorted position whose key is not below `target` (n when there is none)
__device__ __forceinline__ uint32_t lower_bound(const uint64_t *__restrict__ keys, uint64_t n, uint64_t target) {
  uint64_t a = 0, b = n;
  while (a < b) {
    const uint64_t m = a + ((b - a) >> 1);  // a <= m < b <= n
    if (keys[m] < target) a = m + 1;
    else b = m;
  }
  return (uint32_t)a;
}

}  // namespace
}  // namespace dmi
