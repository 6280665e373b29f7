// isosurface_decimate.hip -- decimation of the extracted iso-surface by vertex clustering (dmi_decimate_isosurface;
// Rossignac-Borrel): what a vtkQuadricClustering or, with a tiny cell, a vtkCleanPolyData does after the reference's contour, on
// the device.
//
// Semantics (include/dmi.h states them in full; tests/isosurface_decimate_np.py restates them on the CPU and the
// result is identical): bins of one cell size from the mesh's own lower bounds, a cluster per occupied bin in (b_2, b_1, b_0)
// order, its representative the mean of its members added in ascending id, triangles remapped, degenerate and duplicate ones
// dropped (the lowest original index survives), unreferenced clusters dropped.  No floating point atomics: every sum is made by
// one lane in the definition's order, and no result depends on the order in which atomics arrive.
//
// Passes:
//   bounds      per block the minima and maxima of the coordinates as order-preserving integers (wave shuffles, then LDS), one
//               integer atomic min / max per block and bound; a non-finite coordinate sets a flag.  The host reads them, refuses,
//               or derives the bins (the first of the call's two synchronisations)
//   keys        a lane per vertex: (b_2 n_1 + b_1) n_0 + b_0 and its id
//   sort        rocPRIM radix sort of (key, id) over the bits the key needs; stable: a cluster's members ascend in id
//   ranks       head flags, their inclusive scan = cluster number + 1; every vertex learns its cluster, every cluster its first
//               sorted position (the count of clusters stays on the device)
//   triangles   a lane per triangle: its clusters sorted (min, mid, max); key (min << B | mid), value (max << 32 | index);
//               degenerate triangles and those naming an id >= V get a key above every real one.  One stable sort of the 64-bit
//               keys: triangles sharing (min, mid) are a run, ascending in index.  A lane per sorted position looks back through
//               its run for an equal max: found = duplicate.  Survivors mark their three clusters (plain stores of 1)
//   scans       exclusive scans of the survivor flags and of the marks: the output's numbering and, at their ends, its sizes
//   compaction  a lane per triangle writes the survivor, ids renumbered, stored order kept
//   representatives  a lane per marked cluster walks its members in order (loads batched by four, additions in order) and
//               writes the mean at the cluster's output number
//   quadric     (DMI_DECIMATE_QUADRIC only, in place of the pass above and timed as it) a lane per corner 3t + e writes (cluster of
//               tris[t][e], 3t + e) as u32 pairs; one stable sort over the cluster bits: a cluster's corners are a run, ascending
//               in corner index.  A lane per marked cluster forms the mean as above, finds its run by two binary searches, adds
//               the corners' plane quadrics about the mean in that order, solves the regularised 3x3 system by cofactors, clamps
//               to the cluster's cell and writes at the cluster's output number
//   normals     the smoother's incidence build and kernel on the output (launch_isosurface_geometric_normals), by the caller
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "fusion_kernels.h"

namespace dmi {
namespace {

constexpr int kBlock = 256;
constexpr int kBoundsBlocks = 1024;  // at most: the bounds pass strides over the vertices

__device__ __forceinline__ uint64_t key_limit(int bits) { return bits >= 64 ? ~uint64_t(0) : (uint64_t(1) << bits) - 1; }

// doubles as unsigned integers of the same order (-0.0 below +0.0: the bins do not see the difference)
__device__ __forceinline__ unsigned long long ordered_bits(double x) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | (1ull << 63));
}

__device__ __forceinline__ unsigned long long shuffle_xor(unsigned long long x, int mask) {
  const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)x, mask, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(x >> 32), mask, 64);
  return ((unsigned long long)hi << 32) | lo;
}

// bounds[0..3): minima, [3..6): maxima, [6]: 1 when a coordinate is not finite (such a coordinate takes no part in the bounds)
__global__ __launch_bounds__(kBlock) void decimate_bounds_kernel(const double *__restrict__ p, uint64_t n_vertices,
                                                                 unsigned long long *__restrict__ bounds) {
  __shared__ unsigned long long part[kBlock / 64][7];
  unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull}, bad = 0;
  for (uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x; v < n_vertices; v += (uint64_t)gridDim.x * kBlock) {
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
    if (e < 3) atomicMin(&bounds[e], r);
    else if (e < 6) atomicMax(&bounds[e], r);
    else if (r) atomicOr(&bounds[e], 1ull);
  }
}

__global__ __launch_bounds__(kBlock) void decimate_keys_kernel(const double *__restrict__ p, uint64_t n_vertices, DecimateGrid g,
                                                               uint64_t *__restrict__ keys, uint32_t *__restrict__ ids) {
  const uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= n_vertices) return;
  uint64_t b[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double q = floor((p[3 * v + d] - g.lo[d]) / g.h);  // 0 <= q <= n_d - 1: lo_d <= p <= hi_d and both roundings are monotone
    b[d] = (uint64_t)q;
  }
  keys[v] = (b[2] * g.n[1] + b[1]) * g.n[0] + b[0];
  ids[v] = (uint32_t)v;
}

// head[i] = 1 where sorted position i starts a cluster
__global__ __launch_bounds__(kBlock) void decimate_heads_kernel(const uint64_t *__restrict__ keys, uint64_t n_vertices,
                                                                uint32_t *__restrict__ head) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_vertices) return;
  head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

// rank[i] = clusters up to and including position i: the cluster of sorted position i is rank[i] - 1, there are rank[V - 1]
// clusters.  mark[] is cleared for the triangle pass (all V + 1 entries: the scan reads them all).
__global__ __launch_bounds__(kBlock) void decimate_clusters_kernel(const uint32_t *__restrict__ ids, const uint32_t *__restrict__ head,
                                                                   const uint32_t *__restrict__ rank, uint64_t n_vertices,
                                                                   uint32_t *__restrict__ cluster_of, uint32_t *__restrict__ start,
                                                                   uint32_t *__restrict__ mark) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i > n_vertices) return;
  mark[i] = 0;
  if (i == n_vertices) return;
  const uint32_t c = rank[i] - 1;
  cluster_of[ids[i]] = c;
  if (head[i]) start[c] = (uint32_t)i;
  if (i == n_vertices - 1) start[c + 1] = (uint32_t)n_vertices;  // the end of the last cluster
}

__global__ __launch_bounds__(kBlock) void decimate_triangle_keys_kernel(const int64_t *__restrict__ tris, uint64_t n_triangles,
                                                                        uint64_t n_vertices, const uint32_t *__restrict__ cluster_of,
                                                                        int id_bits, uint64_t *__restrict__ keys,
                                                                        uint64_t *__restrict__ values) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n_triangles) return;
  const uint64_t a = (uint64_t)tris[3 * t], b = (uint64_t)tris[3 * t + 1], c = (uint64_t)tris[3 * t + 2];
  uint64_t key = key_limit(2 * id_bits), value = t;  // (a cluster number is below V < 2^B - 1: no real key has all bits set)
  if (a < n_vertices && b < n_vertices && c < n_vertices) {
    const uint32_t x = cluster_of[a], y = cluster_of[b], z = cluster_of[c];
    if (x != y && y != z && z != x) {
      const uint32_t mn = min(x, min(y, z)), mx = max(x, max(y, z)), md = (uint32_t)((uint64_t)x + y + z - mn - mx);
      key = ((uint64_t)mn << id_bits) | md;
      value = ((uint64_t)mx << 32) | t;
    }
  }
  keys[t] = key;
  values[t] = value;
}

// keep[t] for every triangle (each is at exactly one sorted position); keep[T] = 0 for the scan's total
__global__ __launch_bounds__(kBlock) void decimate_survivors_kernel(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ values,
                                                                    uint64_t n_triangles, int id_bits, uint32_t *__restrict__ keep,
                                                                    uint32_t *__restrict__ mark) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i > n_triangles) return;
  if (i == n_triangles) {
    keep[i] = 0;
    return;
  }
  const uint64_t key = keys[i], value = values[i];
  const uint32_t t = (uint32_t)value, mx = (uint32_t)(value >> 32);
  bool survives = key != key_limit(2 * id_bits);
  if (survives)  // the run is ascending in triangle index (a stable sort): an equal max further back is the one that stays
    for (uint64_t j = i; j > 0 && keys[j - 1] == key; --j)
      if ((uint32_t)(values[j - 1] >> 32) == mx) {
        survives = false;
        break;
      }
  keep[t] = survives ? 1u : 0u;
  if (survives) {
    mark[(uint32_t)(key >> id_bits)] = 1;
    mark[(uint32_t)(key & key_limit(id_bits))] = 1;
    mark[mx] = 1;
  }
}

__global__ __launch_bounds__(kBlock) void decimate_compact_triangles_kernel(const int64_t *__restrict__ tris, uint64_t n_triangles,
                                                                            const uint32_t *__restrict__ keep, const uint32_t *__restrict__ tmap,
                                                                            const uint32_t *__restrict__ cluster_of,
                                                                            const uint32_t *__restrict__ cmap, int64_t *__restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n_triangles || !keep[t]) return;
  const uint64_t w = tmap[t];
#pragma unroll
  for (int e = 0; e < 3; ++e) out[3 * w + e] = (int64_t)cmap[cluster_of[tris[3 * t + e]]];
}

// The mean of the k members of a cluster whose first sorted position is lo: the members' rows are gathered four at a time (the
// loads of a batch are independent of each other, the additions are not) and added in ascending id, the first one starting the sum.
__device__ __forceinline__ void cluster_mean(const double *__restrict__ p, const uint32_t *__restrict__ ids, uint32_t lo, uint32_t k,
                                             double o[3]) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (uint32_t j = 0; j < k; j += 4) {
    double q[4][3];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint64_t u = ids[lo + (j + e < k ? j + e : 0)];  // (the first member again: a row that is there, its values unused)
      q[e][0] = p[3 * u];
      q[e][1] = p[3 * u + 1];
      q[e][2] = p[3 * u + 2];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (j + e == 0) {
        s0 = q[e][0];
        s1 = q[e][1];
        s2 = q[e][2];
      } else if (j + e < k) {
        s0 = s0 + q[e][0];
        s1 = s1 + q[e][1];
        s2 = s2 + q[e][2];
      }
    }
  }
  const double n = (double)k;
  o[0] = s0 / n;
  o[1] = s1 / n;
  o[2] = s2 / n;
}

// A lane per cluster writes the mean of its members.  n_clusters: *rank_last, on the device.
__global__ __launch_bounds__(kBlock) void decimate_representatives_kernel(const double *__restrict__ p, const uint32_t *__restrict__ ids,
                                                                          const uint32_t *__restrict__ start, const uint32_t *__restrict__ mark,
                                                                          const uint32_t *__restrict__ cmap, const uint32_t *__restrict__ rank_last,
                                                                          double *__restrict__ out) {
  const uint64_t c = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (c >= *rank_last || !mark[c]) return;
  const uint32_t lo = start[c];
  double o[3];
  cluster_mean(p, ids, lo, start[c + 1] - lo, o);
  const uint64_t w = cmap[c];
  out[3 * w] = o[0];
  out[3 * w + 1] = o[1];
  out[3 * w + 2] = o[2];
}

// DMI_DECIMATE_QUADRIC.  A lane per corner 3t + e: the cluster of tris[t][e] and the corner's index; a triangle that names an id
// >= V has no corners: theirs get a key above every cluster number (a cluster number is below V < 2^B - 1).
__global__ __launch_bounds__(kBlock) void decimate_corner_keys_kernel(const int64_t *__restrict__ tris, uint64_t n_corners,
                                                                      uint64_t n_vertices, const uint32_t *__restrict__ cluster_of,
                                                                      int id_bits, uint32_t *__restrict__ keys,
                                                                      uint32_t *__restrict__ corners) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_corners) return;
  const uint64_t t = i / 3, e = i - 3 * t;
  const uint64_t a = (uint64_t)tris[3 * t], b = (uint64_t)tris[3 * t + 1], c = (uint64_t)tris[3 * t + 2];
  uint32_t key = (uint32_t)key_limit(id_bits);
  if (a < n_vertices && b < n_vertices && c < n_vertices) key = cluster_of[e == 0 ? a : e == 1 ? b : c];
  keys[i] = key;
  corners[i] = (uint32_t)i;
}

// the first position of the ascending keys[0 .. n) whose key is not below x
__device__ __forceinline__ uint32_t first_not_below(const uint32_t *__restrict__ keys, uint32_t n, uint32_t x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// A lane per cluster: the mean o as above, then the cluster's corners in ascending corner index (its run of the sorted pairs).
// Each adds its triangle's plane n . (x - p_a) = 0, n the unnormalised cross product, as nn^T to A and n d to g with the
// origin at o; the corners of one triangle that follow each other in the run share the gather and the cross product (the same
// values either way).  (A + 2^-10 tr I) x = -g by cofactors, y = o + x clamped to the cluster's cell; the mean wherever the
// definition says so.  f64, every operation rounded (-ffp-contract=off).
__global__ __launch_bounds__(kBlock) void decimate_quadric_representatives_kernel(
    const double *__restrict__ p, const int64_t *__restrict__ tris, const uint32_t *__restrict__ ids, const uint32_t *__restrict__ start,
    const uint32_t *__restrict__ mark, const uint32_t *__restrict__ cmap, const uint32_t *__restrict__ rank_last,
    const uint32_t *__restrict__ corner_keys, const uint32_t *__restrict__ corners, uint32_t n_corners, DecimateGrid grid,
    double *__restrict__ out) {
  const uint64_t c = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (c >= *rank_last || !mark[c]) return;
  const uint32_t lo = start[c];
  double o[3];
  cluster_mean(p, ids, lo, start[c + 1] - lo, o);
  const uint32_t first = first_not_below(corner_keys, n_corners, (uint32_t)c);
  const uint32_t last = first_not_below(corner_keys, n_corners, (uint32_t)c + 1);  // (c + 1 <= V - 1 + 1 < 2^32)
  double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
  double n0 = 0.0, n1 = 0.0, n2 = 0.0, d = 0.0;
  uint32_t held = 0xffffffffu;  // the triangle whose n and d are held (a triangle index is below 2^32 / 3)
  for (uint32_t j = first; j < last; ++j) {
    const uint32_t t = corners[j] / 3;
    if (t != held) {
      const uint64_t ia = (uint64_t)tris[3 * (uint64_t)t], ib = (uint64_t)tris[3 * (uint64_t)t + 1], ic = (uint64_t)tris[3 * (uint64_t)t + 2];
      const double pa0 = p[3 * ia], pa1 = p[3 * ia + 1], pa2 = p[3 * ia + 2];
      const double u0 = p[3 * ib] - pa0, u1 = p[3 * ib + 1] - pa1, u2 = p[3 * ib + 2] - pa2;
      const double v0 = p[3 * ic] - pa0, v1 = p[3 * ic + 1] - pa1, v2 = p[3 * ic + 2] - pa2;
      n0 = u1 * v2 - u2 * v1;
      n1 = u2 * v0 - u0 * v2;
      n2 = u0 * v1 - u1 * v0;
      const double q0 = pa0 - o[0], q1 = pa1 - o[1], q2 = pa2 - o[2];
      d = -((n0 * q0 + n1 * q1) + n2 * q2);
      held = t;
    }
    if (j == first) {
      a00 = n0 * n0, a01 = n0 * n1, a02 = n0 * n2, a11 = n1 * n1, a12 = n1 * n2, a22 = n2 * n2;
      g0 = n0 * d, g1 = n1 * d, g2 = n2 * d;
    } else {
      a00 = a00 + n0 * n0, a01 = a01 + n0 * n1, a02 = a02 + n0 * n2, a11 = a11 + n1 * n1, a12 = a12 + n1 * n2, a22 = a22 + n2 * n2;
      g0 = g0 + n0 * d, g1 = g1 + n1 * d, g2 = g2 + n2 * d;
    }
  }
  double y[3] = {o[0], o[1], o[2]};
  const double tr = (a00 + a11) + a22;
  if (first < last && tr > 0.0 && tr - tr == 0.0) {
    const double mu = 0.0009765625 * tr;  // 2^-10
    const double m00 = a00 + mu, m11 = a11 + mu, m22 = a22 + mu, m01 = a01, m02 = a02, m12 = a12;
    const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
    const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
    const double det = (m00 * c00 + m01 * c01) + m02 * c02;
    if (det > 0.0 && det - det == 0.0) {
      double x[3];
      x[0] = -(((c00 * g0 + c01 * g1) + c02 * g2) / det);
      x[1] = -(((c01 * g0 + c11 * g1) + c12 * g2) / det);
      x[2] = -(((c02 * g0 + c12 * g1) + c22 * g2) / det);
      const uint64_t m = ids[lo];  // any member names the cluster's cell
      double z[3];
      bool nan = false;
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const double b = floor((p[3 * m + e] - grid.lo[e]) / grid.h);  // as the keys pass has it
        const double lower = grid.lo[e] + b * grid.h, upper = grid.lo[e] + (b + 1.0) * grid.h;
        z[e] = o[e] + x[e];
        nan |= z[e] != z[e];
        z[e] = z[e] < lower ? lower : z[e];
        z[e] = z[e] > upper ? upper : z[e];
      }
      if (!nan) y[0] = z[0], y[1] = z[1], y[2] = z[2];
    }
  }
  const uint64_t w = cmap[c];
  out[3 * w] = y[0];
  out[3 * w + 1] = y[1];
  out[3 * w + 2] = y[2];
}

unsigned blocks(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

int bits_for(uint64_t count) {  // the smallest B >= 1 with count < 2^B: every id below count fits, and B set bits are not an id
  int b = 1;
  while (b < 64 && (count >> b) != 0) ++b;
  return b;
}

template <typename Value>
hipError_t sort_pairs(void *temp, size_t *temp_bytes, uint64_t *ka, uint64_t *kb, Value *va, Value *vb, uint64_t n, int bits,
                      uint64_t **sorted_keys, Value **sorted_values, hipStream_t stream) {
  rocprim::double_buffer<uint64_t> keys(ka, kb);
  rocprim::double_buffer<Value> values(va, vb);
  size_t bytes = *temp_bytes;
  const hipError_t e = rocprim::radix_sort_pairs(temp, bytes, keys, values, (size_t)n, 0u, (unsigned)bits, stream);
  if (!temp) *temp_bytes = bytes;
  if (sorted_keys) *sorted_keys = keys.current();
  if (sorted_values) *sorted_values = values.current();
  return e;
}

hipError_t sort_corners(void *temp, size_t *temp_bytes, uint32_t *ka, uint32_t *kb, uint32_t *va, uint32_t *vb, uint64_t n, int bits,
                        uint32_t **sorted_keys, uint32_t **sorted_values, hipStream_t stream) {
  rocprim::double_buffer<uint32_t> keys(ka, kb), values(va, vb);
  size_t bytes = *temp_bytes;
  const hipError_t e = rocprim::radix_sort_pairs(temp, bytes, keys, values, (size_t)n, 0u, (unsigned)bits, stream);
  if (!temp) *temp_bytes = bytes;
  if (sorted_keys) *sorted_keys = keys.current();
  if (sorted_values) *sorted_values = values.current();
  return e;
}

}  // namespace

// the storage rocPRIM asks for: the largest of the two sorts' and the scans' (all 64 key bits: the bins are not known yet), and
// of the corner sort's where the placement is the quadric one
hipError_t decimate_temp_bytes(uint64_t n_vertices, uint64_t n_triangles, int placement, size_t *bytes) {
  size_t a = 0, b = 0, c = 0, d = 0, q = 0;
  hipError_t e = sort_pairs<uint32_t>(nullptr, &a, nullptr, nullptr, nullptr, nullptr, std::max<uint64_t>(n_vertices, 1), 64, nullptr, nullptr, nullptr);
  if (e != hipSuccess) return e;
  e = sort_pairs<uint64_t>(nullptr, &b, nullptr, nullptr, nullptr, nullptr, std::max<uint64_t>(n_triangles, 1), 64, nullptr, nullptr, nullptr);
  if (e != hipSuccess) return e;
  e = rocprim::inclusive_scan(nullptr, c, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)(n_vertices + 1), rocprim::plus<uint32_t>(), nullptr);
  if (e != hipSuccess) return e;
  e = rocprim::exclusive_scan(nullptr, d, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t)0,
                              (size_t)(std::max(n_vertices, n_triangles) + 1), rocprim::plus<uint32_t>(), nullptr);
  if (e != hipSuccess) return e;
  if (placement == kDecimateQuadric)
    e = sort_corners(nullptr, &q, nullptr, nullptr, nullptr, nullptr, std::max<uint64_t>(3 * n_triangles, 1), 32, nullptr, nullptr, nullptr);
  *bytes = std::max(std::max(std::max(a, b), std::max(c, d)), q);
  return e;
}

double decimate_decode_bound(unsigned long long ordered) {
  const unsigned long long u = (ordered >> 63) ? (ordered & ~(1ull << 63)) : ~ordered;
  double x;
  static_assert(sizeof(x) == sizeof(u), "f64");
  __builtin_memcpy(&x, &u, sizeof(x));
  return x;
}

hipError_t launch_decimate_bounds(const DecimateMesh &m, const DecimateScratch &s, hipEvent_t *events, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(s.bounds, 0xff, 3 * sizeof(unsigned long long), stream);  // the minima start at the top
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(s.bounds + 3, 0, 5 * sizeof(unsigned long long), stream)) != hipSuccess) return e;
  if (events && (e = hipEventRecord(events[0], stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(decimate_bounds_kernel, dim3(std::min<unsigned>(blocks(m.n_vertices), kBoundsBlocks)), dim3(kBlock), 0, stream,
                     m.vertices, m.n_vertices, s.bounds);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return events ? hipEventRecord(events[1], stream) : hipSuccess;
}

hipError_t launch_isosurface_decimate(const DecimateMesh &m, const DecimateGrid &g, const DecimateScratch &s, int placement,
                                      hipEvent_t *events, hipStream_t stream) {
  const uint64_t nv = m.n_vertices, nt = m.n_triangles;
  const int id_bits = bits_for(nv);
  // the bits of the largest key, n_0 n_1 n_2 - 1 (the product is at most 2^63)
  const uint64_t last_key = g.n[0] * g.n[1] * g.n[2] - 1;
  const int key_bits = last_key == 0 ? 1 : bits_for(last_key);
  auto mark = [&](int i) -> hipError_t { return events ? hipEventRecord(events[i], stream) : hipSuccess; };
  hipError_t e = mark(0);
  if (e != hipSuccess) return e;
  // clustering
  hipLaunchKernelGGL(decimate_keys_kernel, dim3(blocks(nv)), dim3(kBlock), 0, stream, m.vertices, nv, g, s.keys[0], s.ids[0]);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  uint64_t *sorted_keys = nullptr;
  uint32_t *sorted_ids = nullptr;
  size_t bytes = s.temp_bytes;
  if ((e = sort_pairs<uint32_t>(s.temp, &bytes, s.keys[0], s.keys[1], s.ids[0], s.ids[1], nv, key_bits, &sorted_keys, &sorted_ids, stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(decimate_heads_kernel, dim3(blocks(nv)), dim3(kBlock), 0, stream, sorted_keys, nv, s.head);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  bytes = s.temp_bytes;
  if ((e = rocprim::inclusive_scan(s.temp, bytes, s.head, s.rank, (size_t)nv, rocprim::plus<uint32_t>(), stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(decimate_clusters_kernel, dim3(blocks(nv + 1)), dim3(kBlock), 0, stream, sorted_ids, s.head, s.rank, nv, s.cluster_of, s.start, s.mark);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = mark(1)) != hipSuccess) return e;
  // triangles: the vertex keys are no longer needed, their two arrays hold the triangle keys and values (halves of each)
  if (nt) {
    uint64_t *ka = s.keys[0], *kb = s.keys[0] + nt, *va = s.keys[1], *vb = s.keys[1] + nt, *tk = nullptr, *tv = nullptr;
    hipLaunchKernelGGL(decimate_triangle_keys_kernel, dim3(blocks(nt)), dim3(kBlock), 0, stream, m.triangles, nt, nv, s.cluster_of, id_bits, ka, va);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    bytes = s.temp_bytes;
    if ((e = sort_pairs<uint64_t>(s.temp, &bytes, ka, kb, va, vb, nt, 2 * id_bits, &tk, &tv, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(decimate_survivors_kernel, dim3(blocks(nt + 1)), dim3(kBlock), 0, stream, tk, tv, nt, id_bits, s.keep, s.mark);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  } else if ((e = hipMemsetAsync(s.keep, 0, sizeof(uint32_t), stream)) != hipSuccess) {
    return e;
  }
  bytes = s.temp_bytes;
  if ((e = rocprim::exclusive_scan(s.temp, bytes, s.keep, s.tmap, (uint32_t)0, (size_t)(nt + 1), rocprim::plus<uint32_t>(), stream)) != hipSuccess) return e;
  bytes = s.temp_bytes;
  if ((e = rocprim::exclusive_scan(s.temp, bytes, s.mark, s.cmap, (uint32_t)0, (size_t)(nv + 1), rocprim::plus<uint32_t>(), stream)) != hipSuccess) return e;
  if (nt) {
    hipLaunchKernelGGL(decimate_compact_triangles_kernel, dim3(blocks(nt)), dim3(kBlock), 0, stream, m.triangles, nt, s.keep, s.tmap, s.cluster_of, s.cmap, m.out_triangles);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if ((e = mark(2)) != hipSuccess) return e;
  // representatives (a lane per possible cluster: how many there are is rank[V - 1], on the device)
  if (placement == kDecimateQuadric) {
    // the triangle keys are no longer needed: their arrays hold the corner pairs, u32, two buffers of 3T each in either
    const uint64_t nc = 3 * nt;
    uint32_t *ka = reinterpret_cast<uint32_t *>(s.keys[0]), *va = reinterpret_cast<uint32_t *>(s.keys[1]), *ck = ka, *cv = va;
    if (nc) {
      hipLaunchKernelGGL(decimate_corner_keys_kernel, dim3(blocks(nc)), dim3(kBlock), 0, stream, m.triangles, nc, nv, s.cluster_of, id_bits, ka, va);
      if ((e = hipGetLastError()) != hipSuccess) return e;
      bytes = s.temp_bytes;
      if ((e = sort_corners(s.temp, &bytes, ka, ka + nc, va, va + nc, nc, id_bits, &ck, &cv, stream)) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(decimate_quadric_representatives_kernel, dim3(blocks(nv)), dim3(kBlock), 0, stream, m.vertices, m.triangles, sorted_ids,
                       s.start, s.mark, s.cmap, s.rank + (nv - 1), ck, cv, (uint32_t)nc, g, m.out_vertices);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return mark(3);
  }
  hipLaunchKernelGGL(decimate_representatives_kernel, dim3(blocks(nv)), dim3(kBlock), 0, stream, m.vertices, sorted_ids, s.start, s.mark, s.cmap, s.rank + (nv - 1), m.out_vertices);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return mark(3);
}

}  // namespace dmi
