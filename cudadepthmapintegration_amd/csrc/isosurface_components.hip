// isosurface_components.hip -- connected components of the extracted iso-surface (dmi_filter_isosurface_components): what
// vtkPolyDataConnectivityFilter does after the reference's contour, on the device.  Integer work only; HBM- and atomics-bound.
//
// Semantics (include/dmi.h states them in full; tests/isosurface_components_np.py restates them on the CPU and
// the result is identical): connectivity by vertex id through the triangles, a component's label is its smallest vertex id,
// its size the number of its triangles; the kept components' vertices and triangles keep their order and are renumbered.
//
// Passes, one kernel each unless said otherwise:
//   init      parent[v] = v, size[v] = 0
//   hook      per triangle (a, b, c): unite(a, b), unite(a, c) -- a lock-free union-find; a link always goes from the larger
//             root to the smaller, so a finished tree's root is the definition's label whatever order the hardware ran in
//   flatten   parent[v] = root(v) (a LATER kernel: no link is made while it runs), and the roots are counted
//   sizes     size[label] += 1 per triangle, aggregated: a workgroup counts its 4096-triangle chunk into a (label, count) table in
//             LDS and adds each occupied slot to size[] once
//   largest   (DMI_COMPONENTS_LARGEST only) a 64-bit max over the roots of (size << 32 | ~label): greatest size, ties to the
//             smallest label
//   scans     three rocPRIM exclusive scans over keep flags computed on the fly: vertices, triangles, kept roots (= region ids)
//   compact   vertices (positions, normals, RegionId, and RegionSize by the roots) and triangles (remapped) into a second set of buffers
//
// Visibility.  parent[] is written by many workgroups of the hook kernel, on all eight XCDs, whose L2s are not
// coherent with each other and whose L1s nobody refreshes.  Every access to parent[] in the hook and flatten kernels is an
// agent-scope atomic (load, store or compare-and-swap: device-coherent, past L1 and the XCD's L2).  Correctness needs less than
// that: (1) parent[v] <= v always, and parent[v] only ever changes to another vertex of v's own set; (2) a LINK -- the only step
// that merges two sets -- is a device-scope compare-and-swap parent[hi]: hi -> lo with lo < hi, which succeeds only if hi is a
// root at that instant, so no vertex is ever given two parents and no link is lost; a stale view of an ANCESTOR (find() stopping
// at a vertex that has meanwhile been linked further) only makes `lo` a non-root member of its set, which is still a correct
// parent.  Path halving stores an ancestor over a parent: same set, smaller id.  The flatten pass reads the finished forest in a
// later kernel.  No workgroup ever waits for another: every loop ends because a vertex id strictly decreased.
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "fusion_kernels.h"
#include "union_find_device.h"

namespace dmi {
namespace {

constexpr int kBlock = 256;

// the union-find itself is shared with depth_speckle.hip (union_find_device.h, where the visibility argument above is restated)
using union_find::find_root;
using union_find::load_parent;
using union_find::unite;

__global__ __launch_bounds__(kBlock) void components_init_kernel(uint32_t *__restrict__ parent, uint32_t *__restrict__ size, uint64_t n) {
  const uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v < n) {
    parent[v] = (uint32_t)v;
    size[v] = 0;
  }
}

// counters[2] += the compare-and-swaps that were retried (summed per workgroup in LDS first: millions of adds onto one address
// would cost more than the hooking)
__global__ __launch_bounds__(kBlock) void components_hook_kernel(const int64_t *__restrict__ tris, uint64_t n_triangles,
                                                                 uint64_t n_vertices, uint32_t *parent, unsigned long long *counters) {
  __shared__ uint32_t block_retries;
  if (threadIdx.x == 0) block_retries = 0;
  __syncthreads();
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  uint32_t retries = 0;
  if (t < n_triangles) {
    const uint64_t a = (uint64_t)tris[3 * t], b = (uint64_t)tris[3 * t + 1], c = (uint64_t)tris[3 * t + 2];
    if (a < n_vertices && b < n_vertices && c < n_vertices) {  // (always, for a mesh of this library: no access out of bounds)
      if (a != b) unite(parent, (uint32_t)a, (uint32_t)b, &retries);
      if (a != c) unite(parent, (uint32_t)a, (uint32_t)c, &retries);
    }
  }
  if (retries) atomicAdd(&block_retries, retries);
  __syncthreads();
  if (threadIdx.x == 0 && block_retries) atomicAdd(counters + 2, (unsigned long long)block_retries);
}

// counters[1] += the number of roots
__global__ __launch_bounds__(kBlock) void components_flatten_kernel(uint32_t *parent, uint64_t n, unsigned long long *counters) {
  const uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  bool root = false;
  if (v < n) {
    uint32_t r = (uint32_t)v, p = load_parent(parent, r);
    while (p != r) {
      r = p;
      p = load_parent(parent, r);
    }
    root = r == (uint32_t)v;
    if (!root) __hip_atomic_store(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  const unsigned long long roots = __ballot(root);
  if (roots && (threadIdx.x & 63) == 0) atomicAdd(counters + 1, (unsigned long long)__popcll(roots));  // (no lane has left)
}

// A workgroup counts kSizeChunk consecutive triangles into a small table in LDS -- (label, count) pairs, open addressing,
// LDS atomics -- and adds each occupied slot to size[] once at the end; a label that finds no slot within kSizeProbes adds for
// itself.  Triangles come in cell order: a chunk holds a few large components and some small ones.  One global add per triangle,
// or even per wave, onto the few addresses of the large components serialises in L2 (measured: longer than the union-find).
constexpr int kSizeChunk = 16 * kBlock;
constexpr int kSizeSlots = 256;  // a power of two
constexpr int kSizeProbes = 8;
constexpr uint32_t kNoLabel = 0xffffffffu;  // no vertex has this id: n_vertices < 2^32

__global__ __launch_bounds__(kBlock) void components_size_kernel(const int64_t *__restrict__ tris, uint64_t n_triangles,
                                                                 uint64_t n_vertices, const uint32_t *__restrict__ label,
                                                                 uint32_t *__restrict__ size) {
  __shared__ uint32_t keys[kSizeSlots], counts[kSizeSlots];
  static_assert(kSizeSlots == kBlock, "one slot per thread below");
  keys[threadIdx.x] = kNoLabel;
  counts[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * kSizeChunk;
  auto count = [&](uint32_t l, uint32_t n) {
    const uint32_t h = (l * 2654435761u) >> 24;
    for (int probe = 0; probe < kSizeProbes; ++probe) {
      const uint32_t slot = (h + probe) & (kSizeSlots - 1);
      const uint32_t old = atomicCAS(&keys[slot], kNoLabel, l);
      if (old == kNoLabel || old == l) {
        atomicAdd(&counts[slot], n);
        return;
      }
    }
    atomicAdd(size + l, n);
  };
  for (int it = 0; it < kSizeChunk / kBlock; ++it) {
    const uint64_t t = base + (uint64_t)it * kBlock + threadIdx.x;
    uint32_t l = kNoLabel;
    if (t < n_triangles) {
      const uint64_t a = (uint64_t)tris[3 * t];
      if (a < n_vertices) l = label[a];  // (an id out of range, never for a mesh of this library, is not counted)
    }
    // the lanes that share the wave's first label count together, the others each for themselves
    const unsigned long long live = __ballot(l != kNoLabel);
    if (live) {
      const int first = __ffsll((long long)live) - 1;
      const uint32_t l0 = __shfl(l, first, 64);
      const unsigned long long same = __ballot(l == l0);
      if (l == l0) {
        if ((int)(threadIdx.x & 63) == first) count(l0, (uint32_t)__popcll(same));
      } else if (l != kNoLabel) {
        count(l, 1u);
      }
    }
  }
  __syncthreads();
  if (keys[threadIdx.x] != kNoLabel && counts[threadIdx.x]) atomicAdd(size + keys[threadIdx.x], counts[threadIdx.x]);
}

// which components stay: by size (MIN_TRIANGLES) or the one whose (size << 32 | ~label) is the maximum (LARGEST)
struct Keep {
  const uint32_t *label, *size;
  const unsigned long long *counters;  // [0]: the maximum key of the largest pass
  uint64_t min_triangles;
  int largest;
  __device__ __forceinline__ bool root(uint32_t r) const {
    return largest ? r == ~(uint32_t)counters[0] : (uint64_t)size[r] >= min_triangles;
  }
};

__global__ __launch_bounds__(kBlock) void components_largest_kernel(const uint32_t *__restrict__ label, const uint32_t *__restrict__ size,
                                                                    uint64_t n, unsigned long long *counters) {
  const uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  unsigned long long key = 0;
  if (v < n && label[v] == (uint32_t)v) key = ((unsigned long long)size[v] << 32) | (unsigned long long)(~(uint32_t)v);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long other = __shfl_xor(key, off, 64);
    key = other > key ? other : key;
  }
  if ((threadIdx.x & 63) == 0 && key) atomicMax(counters, key);
}

// the scans' inputs, computed where they are read: index n (one past the end) is 0, so the scans' outputs hold the totals there
struct VertexFlag {
  Keep keep;
  uint64_t n;
  __device__ uint32_t operator()(uint64_t v) const { return v < n && keep.root(keep.label[v]) ? 1u : 0u; }
};
struct RootFlag {
  Keep keep;
  uint64_t n;
  __device__ uint32_t operator()(uint64_t v) const { return v < n && keep.label[v] == (uint32_t)v && keep.root((uint32_t)v) ? 1u : 0u; }
};
struct TriangleFlag {
  Keep keep;
  const int64_t *tris;
  uint64_t n, n_vertices;
  __device__ uint32_t operator()(uint64_t t) const {
    if (t >= n) return 0u;
    const uint64_t a = (uint64_t)tris[3 * t];
    return a < n_vertices && keep.root(keep.label[a]) ? 1u : 0u;
  }
};

template <typename Flag>
hipError_t scan_flags(void *temp, size_t *temp_bytes, const Flag &flag, uint32_t *out, uint64_t n, hipStream_t stream) {
  auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), flag);
  size_t bytes = *temp_bytes;
  const hipError_t e = rocprim::exclusive_scan(temp, bytes, in, out, (uint32_t)0, (size_t)(n + 1), rocprim::plus<uint32_t>(), stream);
  if (!temp) *temp_bytes = bytes;
  return e;
}

__global__ __launch_bounds__(kBlock) void components_compact_vertices_kernel(ComponentsMesh m, Keep keep,
                                                                             const uint32_t *__restrict__ vmap,
                                                                             const uint32_t *__restrict__ rmap) {
  const uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= m.n_vertices) return;
  const uint32_t r = keep.label[v];
  if (!keep.root(r)) return;
  const uint64_t w = vmap[v];
#pragma unroll
  for (int e = 0; e < 3; ++e) m.out_vertices[3 * w + e] = m.vertices[3 * v + e];
  if (m.normals) {
#pragma unroll
    for (int e = 0; e < 3; ++e) m.out_normals[3 * w + e] = m.normals[3 * v + e];
  }
  const uint32_t region = rmap[r];
  m.region_id[w] = (int64_t)region;
  if (r == (uint32_t)v) m.region_size[region] = (int64_t)keep.size[r];
}

__global__ __launch_bounds__(kBlock) void components_compact_triangles_kernel(ComponentsMesh m, Keep keep,
                                                                              const uint32_t *__restrict__ vmap,
                                                                              const uint32_t *__restrict__ tmap) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= m.n_triangles) return;
  const uint64_t a = (uint64_t)m.triangles[3 * t], b = (uint64_t)m.triangles[3 * t + 1], c = (uint64_t)m.triangles[3 * t + 2];
  if (a >= m.n_vertices || b >= m.n_vertices || c >= m.n_vertices || !keep.root(keep.label[a])) return;
  const uint64_t w = tmap[t];
  m.out_triangles[3 * w] = (int64_t)vmap[a];
  m.out_triangles[3 * w + 1] = (int64_t)vmap[b];
  m.out_triangles[3 * w + 2] = (int64_t)vmap[c];
}

unsigned blocks(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

// the three scans' storage (the largest of them)
hipError_t components_scan_temp_bytes(uint64_t n_vertices, uint64_t n_triangles, size_t *bytes) {
  const Keep keep{};
  size_t a = 0, b = 0, c = 0;
  hipError_t e = scan_flags(nullptr, &a, VertexFlag{keep, n_vertices}, (uint32_t *)nullptr, n_vertices, nullptr);
  if (e != hipSuccess) return e;
  e = scan_flags(nullptr, &b, RootFlag{keep, n_vertices}, (uint32_t *)nullptr, n_vertices, nullptr);
  if (e != hipSuccess) return e;
  e = scan_flags(nullptr, &c, TriangleFlag{keep, nullptr, n_triangles, n_vertices}, (uint32_t *)nullptr, n_triangles, nullptr);
  *bytes = a > b ? (a > c ? a : c) : (b > c ? b : c);
  return e;
}

// Labels, sizes, keep flags and the compaction of mesh `m` (n_vertices >= 1, both counts below 2^32).  Afterwards
// s.vmap[n_vertices] / s.tmap[n_triangles] / s.rmap[n_vertices] hold the kept vertices / triangles / components and
// s.counters[1] the components found and s.counters[2] the compare-and-swaps that had to be retried.  `events`: 5 events recorded around the passes (labels, sizes, scans, compaction), or null.
hipError_t launch_isosurface_components(const ComponentsMesh &m, const ComponentsScratch &s, int largest, uint64_t min_triangles,
                                        hipEvent_t *events, hipStream_t stream) {
  const uint64_t nv = m.n_vertices, nt = m.n_triangles;
  hipError_t e = hipMemsetAsync(s.counters, 0, 3 * sizeof(unsigned long long), stream);
  if (e != hipSuccess) return e;
  auto mark = [&](int i) -> hipError_t { return events ? hipEventRecord(events[i], stream) : hipSuccess; };
  if ((e = mark(0)) != hipSuccess) return e;
  hipLaunchKernelGGL(components_init_kernel, dim3(blocks(nv)), dim3(kBlock), 0, stream, s.parent, s.size, nv);
  if (nt) hipLaunchKernelGGL(components_hook_kernel, dim3(blocks(nt)), dim3(kBlock), 0, stream, m.triangles, nt, nv, s.parent, s.counters);
  hipLaunchKernelGGL(components_flatten_kernel, dim3(blocks(nv)), dim3(kBlock), 0, stream, s.parent, nv, s.counters);
  if ((e = mark(1)) != hipSuccess) return e;
  if (nt) hipLaunchKernelGGL(components_size_kernel, dim3((unsigned)((nt + kSizeChunk - 1) / kSizeChunk)), dim3(kBlock), 0, stream, m.triangles, nt, nv, s.parent, s.size);
  if (largest) hipLaunchKernelGGL(components_largest_kernel, dim3(blocks(nv)), dim3(kBlock), 0, stream, s.parent, s.size, nv, s.counters);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = mark(2)) != hipSuccess) return e;
  const Keep keep{s.parent, s.size, s.counters, min_triangles, largest};
  size_t bytes = s.scan_temp_bytes;
  if ((e = scan_flags(s.scan_temp, &bytes, VertexFlag{keep, nv}, s.vmap, nv, stream)) != hipSuccess) return e;
  if ((e = scan_flags(s.scan_temp, &bytes, RootFlag{keep, nv}, s.rmap, nv, stream)) != hipSuccess) return e;
  if ((e = scan_flags(s.scan_temp, &bytes, TriangleFlag{keep, m.triangles, nt, nv}, s.tmap, nt, stream)) != hipSuccess) return e;
  if ((e = mark(3)) != hipSuccess) return e;
  hipLaunchKernelGGL(components_compact_vertices_kernel, dim3(blocks(nv)), dim3(kBlock), 0, stream, m, keep, s.vmap, s.rmap);
  if (nt) hipLaunchKernelGGL(components_compact_triangles_kernel, dim3(blocks(nt)), dim3(kBlock), 0, stream, m, keep, s.vmap, s.tmap);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return mark(4);
}

}  // namespace dmi
