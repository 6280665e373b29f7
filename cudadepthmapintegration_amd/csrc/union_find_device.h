// union_find_device.h -- the lock-free union-find over a u32 parent array in global memory that isosurface_components.hip (the
// mesh's vertices) and depth_speckle.hip (the tile-local roots of a depth map's segments) share.  A link always goes from the
// larger root to the smaller, so a finished tree's root is its set's smallest member whatever order the hardware ran in.
//
// Visibility.  parent[] is written by many workgroups, on all eight XCDs, whose L2s are not coherent with each other and whose L1s
// nobody refreshes.  Every access here is an agent-scope atomic (load, store or compare-and-swap: device-coherent, past L1 and the
// XCD's L2).  Correctness needs less than that: (1) parent[v] <= v always, and parent[v] only ever changes to another member of
// v's own set; (2) a LINK -- the only step that merges two sets -- is a device-scope compare-and-swap parent[hi]: hi -> lo with
// lo < hi, which succeeds only if hi is a root at that instant, so no member is ever given two parents and no link is lost; a stale
// view of an ANCESTOR (find_root stopping at a member that has meanwhile been linked further) only makes `lo` a non-root member of
// its set, which is still a correct parent.  Path halving stores an ancestor over a parent: same set, smaller id.  No thread ever
// waits for another: every loop ends because an id strictly decreased.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dmi {
namespace union_find {

__device__ __forceinline__ uint32_t load_parent(const uint32_t *parent, uint32_t v) {
  return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of v's tree as far as this thread can see, halving the path on the way: each step moves to a strictly smaller id
__device__ __forceinline__ uint32_t find_root(uint32_t *parent, uint32_t v) {
  uint32_t p = load_parent(parent, v);
  while (p != v) {
    const uint32_t g = load_parent(parent, p);
    if (g != p) __hip_atomic_store(parent + v, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // an ancestor: same set, smaller
    v = p;
    p = g;
  }
  return v;
}

// the root of v's tree in a forest nobody links any more (a later kernel than the links): no store
__device__ __forceinline__ uint32_t final_root(const uint32_t *parent, uint32_t v) {
  uint32_t p = load_parent(parent, v);
  while (p != v) {
    v = p;
    p = load_parent(parent, v);
  }
  return v;
}

// *retries += 1 for every compare-and-swap that lost its race
__device__ __forceinline__ void unite(uint32_t *parent, uint32_t a, uint32_t b, uint32_t *retries) {
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return;
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    uint32_t seen = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      return;
    // hi was linked by someone else meanwhile: seen < hi is its parent, a member of the same set; go on from there
    ++*retries;
    a = seen;
    b = lo;
  }
}

}  // namespace union_find
}  // namespace dmi
