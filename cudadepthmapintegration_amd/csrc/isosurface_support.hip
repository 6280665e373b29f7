// isosurface_support.hip -- the iso-surface trimmed by view support (dmi_filter_isosurface_support): what every TSDF pipeline
// does to the back shell and to the sheets between seen and unseen space that an iso-contour of the summed ray potential carries
// besides the surface.  A vertex is supported by a view that saw it: in front of the camera, inside the image, within a tolerance
// of the depth the fusion kept at its pixel and, optionally, with its normal towards the camera.
//
// Semantics (include/dmi.h states them in full; tests/isosurface_support_np.py restates them on the CPU and the
// result is identical): f64 throughout, every operation rounded (-ffp-contract=off), the fusion's projection order (row4).
//
// Passes:
//   counts    one lane per vertex, a loop over the views: the view's MapRec is wave-uniform and arrives through scalar loads; the
//             count lives in a register and is stored once.  Extraction emits vertices in lattice order, so neighbouring lanes
//             read neighbouring pixels of every depth table.  A small mesh does not fill the chip with one lane per vertex: the
//             views are then split over the grid's second dimension and the partial counts combined with integer atomic adds
//             (integers do not depend on the order).  The two divisions of a pair are replaced by a checked reciprocal where that
//             provably selects the same pixel (rounded_quotient.h, as the coloration does).
//   marks     per surviving triangle (three ids below V, each with at least min_views views): mark[id] = 1 for its three ids;
//             every writer stores the same value, and the readers are later kernels
//   scans     two rocPRIM exclusive scans: the marks (vertices) and the triangle flags computed on the fly
//   compact   vertices (positions, normals and counts, bit for bit) and triangles (remapped) into a second set of buffers
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "fusion_device.h"
#include "rounded_quotient.h"

namespace dmi {
namespace {

constexpr int kBlock = 256;
// the views are split over gridDim.y only while the vertices alone give fewer workgroups than this (four per CU), and never
// into groups of fewer than kMinViewsPerGroup views (the vertex and its normal are loaded once per group).  Both figures are
// reasoned, not tuned: no sweep of either has been run (profiles/NOTEBOOK.md)
constexpr unsigned kFillBlocks = 1024;
constexpr int kMinViewsPerGroup = 8;

template <typename T>
__device__ __forceinline__ T cload(const T *p) {  // wave-uniform address -> scalar load
  return *reinterpret_cast<const T __attribute__((address_space(4))) *>(reinterpret_cast<uintptr_t>(p));
}

// support[v] (+)= the views of [blockIdx.y * views_per_group, ...) that support vertex v.  One group: a plain store.  Several:
// atomic adds onto an array the caller has zeroed.
template <typename DepthT, bool FACING>
__global__ __launch_bounds__(kBlock) void support_count_kernel(const double *__restrict__ vertices, const float *__restrict__ normals,
                                                               uint64_t n_vertices, const MapRec *__restrict__ maps, int n_views,
                                                               int views_per_group, int W, int H, double tolerance,
                                                               int32_t *__restrict__ support) {
  const uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= n_vertices) return;
  const double x = vertices[3 * v], y = vertices[3 * v + 1], z = vertices[3 * v + 2];
  double n0 = 0.0, n1 = 0.0, n2 = 0.0;
  if constexpr (FACING) {
    n0 = (double)normals[3 * v];
    n1 = (double)normals[3 * v + 1];
    n2 = (double)normals[3 * v + 2];
  }
  const int first = (int)blockIdx.y * views_per_group;
  const int last = first + views_per_group < n_views ? first + views_per_group : n_views;
  int32_t count = 0;
  for (int view = first; view < last; ++view) {
    // the loop's bounds are wave-uniform, but lanes leave an iteration at different points: the index is made a scalar by hand, so
    // that the record's loads stay scalar loads whatever the compiler's uniformity analysis makes of the loop
    const int m = __builtin_amdgcn_readfirstlane(view);
    struct {
      double rt[12], k[12];
      const void *depth;
    } rec;
#pragma unroll
    for (int q = 0; q < 12; ++q) {
      rec.rt[q] = cload(&maps[m].rt[q]);
      rec.k[q] = cload(&maps[m].k[q]);
    }
    rec.depth = cload(&maps[m].depth);
    const double c0 = row4(rec.rt, x, y, z), c1 = row4(rec.rt + 4, x, y, z), c2 = row4(rec.rt + 8, x, y, z);
    if (!(c2 > 0.0)) continue;  // behind the camera, or a NaN
    const double h0 = row4(rec.k, c0, c1, c2), h1 = row4(rec.k + 4, c0, c1, c2), h2 = row4(rec.k + 8, c0, c1, c2);
    const FastQuotient by_h2(h2);
    int px = 0, py = 0;
    if (!by_h2.round_to_pixel(h0, h2, px) || !by_h2.round_to_pixel(h1, h2, py)) continue;  // not finite, or beyond 2^31
    if (px < 0 || px >= W || py < 0 || py >= H) continue;
    const double d = (double)static_cast<const DepthT *>(rec.depth)[(int64_t)py * W + px];
    if (!(d > 0.0 && fabs(c2 - d) <= tolerance)) continue;  // -1, NaN and infinite depths reject the pair
    if constexpr (FACING) {
      const double m0 = (rec.rt[0] * n0 + rec.rt[1] * n1) + rec.rt[2] * n2;
      const double m1 = (rec.rt[4] * n0 + rec.rt[5] * n1) + rec.rt[6] * n2;
      const double m2 = (rec.rt[8] * n0 + rec.rt[9] * n1) + rec.rt[10] * n2;
      const double s = (m0 * c0 + m1 * c1) + m2 * c2;
      if (!(s < 0.0)) continue;  // the normal points away from the camera, across its line of sight, or is a NaN
    }
    ++count;
  }
  if (gridDim.y == 1) support[v] = count;
  else if (count) atomicAdd(support + v, count);
}

// which triangles stay: three ids below V, each with at least min_views supporting views
struct Keep {
  const int64_t *tris;
  const int32_t *support;
  uint64_t n_vertices, n_triangles;
  int32_t min_views;
  __device__ __forceinline__ bool triangle(uint64_t t, uint64_t &a, uint64_t &b, uint64_t &c) const {
    a = (uint64_t)tris[3 * t];
    b = (uint64_t)tris[3 * t + 1];
    c = (uint64_t)tris[3 * t + 2];
    if (a >= n_vertices || b >= n_vertices || c >= n_vertices) return false;  // (never for a mesh of this library)
    return support[a] >= min_views && support[b] >= min_views && support[c] >= min_views;
  }
};

__global__ __launch_bounds__(kBlock) void support_mark_kernel(Keep keep, uint32_t *__restrict__ mark) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= keep.n_triangles) return;
  uint64_t a, b, c;
  if (!keep.triangle(t, a, b, c)) return;
  mark[a] = 1u;
  mark[b] = 1u;
  mark[c] = 1u;
}

// the triangle scan's input, computed where it is read: index n (one past the end) is 0, so the scan's output holds the total there
struct TriangleFlag {
  Keep keep;
  __device__ uint32_t operator()(uint64_t t) const {
    uint64_t a, b, c;
    return t < keep.n_triangles && keep.triangle(t, a, b, c) ? 1u : 0u;
  }
};

hipError_t scan_triangles(void *temp, size_t *temp_bytes, const Keep &keep, uint32_t *out, hipStream_t stream) {
  auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), TriangleFlag{keep});
  size_t bytes = *temp_bytes;
  const hipError_t e = rocprim::exclusive_scan(temp, bytes, in, out, (uint32_t)0, (size_t)(keep.n_triangles + 1), rocprim::plus<uint32_t>(), stream);
  if (!temp) *temp_bytes = bytes;
  return e;
}

hipError_t scan_marks(void *temp, size_t *temp_bytes, const uint32_t *mark, uint32_t *out, uint64_t n_vertices, hipStream_t stream) {
  size_t bytes = *temp_bytes;
  const hipError_t e = rocprim::exclusive_scan(temp, bytes, mark, out, (uint32_t)0, (size_t)(n_vertices + 1), rocprim::plus<uint32_t>(), stream);
  if (!temp) *temp_bytes = bytes;
  return e;
}

__global__ __launch_bounds__(kBlock) void support_compact_vertices_kernel(SupportMesh m, const int32_t *__restrict__ support,
                                                                          const uint32_t *__restrict__ mark,
                                                                          const uint32_t *__restrict__ vmap,
                                                                          int32_t *__restrict__ out_support) {
  const uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= m.n_vertices || !mark[v]) return;
  const uint64_t w = vmap[v];
#pragma unroll
  for (int e = 0; e < 3; ++e) m.out_vertices[3 * w + e] = m.vertices[3 * v + e];
  if (m.normals) {
#pragma unroll
    for (int e = 0; e < 3; ++e) m.out_normals[3 * w + e] = m.normals[3 * v + e];
  }
  out_support[w] = support[v];
}

__global__ __launch_bounds__(kBlock) void support_compact_triangles_kernel(SupportMesh m, Keep keep, const uint32_t *__restrict__ vmap,
                                                                           const uint32_t *__restrict__ tmap) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= m.n_triangles) return;
  uint64_t a, b, c;
  if (!keep.triangle(t, a, b, c)) return;
  const uint64_t w = tmap[t];
  m.out_triangles[3 * w] = (int64_t)vmap[a];
  m.out_triangles[3 * w + 1] = (int64_t)vmap[b];
  m.out_triangles[3 * w + 2] = (int64_t)vmap[c];
}

unsigned blocks(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

// the two scans' storage (the larger of them)
hipError_t support_scan_temp_bytes(uint64_t n_vertices, uint64_t n_triangles, size_t *bytes) {
  size_t a = 0, b = 0;
  hipError_t e = scan_marks(nullptr, &a, (const uint32_t *)nullptr, (uint32_t *)nullptr, n_vertices, nullptr);
  if (e != hipSuccess) return e;
  e = scan_triangles(nullptr, &b, Keep{nullptr, nullptr, n_vertices, n_triangles, 0}, (uint32_t *)nullptr, nullptr);
  *bytes = a > b ? a : b;
  return e;
}

// s.support[v] = the views among `views` that support vertex v of mesh `m` (n_vertices >= 1), recorded between events[0] and [1]
hipError_t launch_isosurface_support_counts(const SupportMesh &m, const SupportViews &views, double tolerance, int require_facing,
                                            const SupportScratch &s, hipEvent_t *events, hipStream_t stream) {
  const unsigned vertex_blocks = blocks(m.n_vertices);
  int groups = 1;
  if (vertex_blocks < kFillBlocks) {
    const int by_views = (views.n_views + kMinViewsPerGroup - 1) / kMinViewsPerGroup;
    const int by_fill = (int)((kFillBlocks + vertex_blocks - 1) / vertex_blocks);
    groups = by_views < by_fill ? by_views : by_fill;
    if (groups < 1) groups = 1;
  }
  const int per_group = (views.n_views + groups - 1) / groups;
  groups = (views.n_views + per_group - 1) / per_group;  // no empty group
  hipError_t e = events ? hipEventRecord(events[0], stream) : hipSuccess;
  if (e != hipSuccess) return e;
  if (groups > 1 && (e = hipMemsetAsync(s.support, 0, m.n_vertices * sizeof(int32_t), stream)) != hipSuccess) return e;
  const dim3 grid(vertex_blocks, (unsigned)groups);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, stream, m.vertices, m.normals, m.n_vertices, views.maps, views.n_views, per_group,
                       views.W, views.H, tolerance, s.support);
  };
  if (views.depth_is_f64) {
    if (require_facing) launch(support_count_kernel<double, true>); else launch(support_count_kernel<double, false>);
  } else {
    if (require_facing) launch(support_count_kernel<float, true>); else launch(support_count_kernel<float, false>);
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return events ? hipEventRecord(events[1], stream) : hipSuccess;
}

// The filter by the counts in s.support (min_views >= 1, n_vertices >= 1): marks and scans between events[1] and [2], the
// compaction between [2] and [3].  Afterwards s.vmap[n_vertices] and s.tmap[n_triangles] hold the surviving vertices and triangles,
// m.out_* the compacted mesh and s.out_support its counts.
hipError_t launch_isosurface_support_filter(const SupportMesh &m, int32_t min_views, const SupportScratch &s, hipEvent_t *events,
                                            hipStream_t stream) {
  const uint64_t nv = m.n_vertices, nt = m.n_triangles;
  const Keep keep{m.triangles, s.support, nv, nt, min_views};
  hipError_t e = hipMemsetAsync(s.mark, 0, (nv + 1) * sizeof(uint32_t), stream);  // (the entry one past the end stays 0)
  if (e != hipSuccess) return e;
  if (nt) hipLaunchKernelGGL(support_mark_kernel, dim3(blocks(nt)), dim3(kBlock), 0, stream, keep, s.mark);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  size_t bytes = s.scan_temp_bytes;
  if ((e = scan_marks(s.scan_temp, &bytes, s.mark, s.vmap, nv, stream)) != hipSuccess) return e;
  if ((e = scan_triangles(s.scan_temp, &bytes, keep, s.tmap, stream)) != hipSuccess) return e;
  if (events && (e = hipEventRecord(events[2], stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(support_compact_vertices_kernel, dim3(blocks(nv)), dim3(kBlock), 0, stream, m, s.support, s.mark, s.vmap, s.out_support);
  if (nt) hipLaunchKernelGGL(support_compact_triangles_kernel, dim3(blocks(nt)), dim3(kBlock), 0, stream, m, keep, s.vmap, s.tmap);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return events ? hipEventRecord(events[3], stream) : hipSuccess;
}

}  // namespace dmi
