// isosurface_smooth.hip -- Taubin lambda|mu smoothing of the extracted iso-surface (dmi_smooth_isosurface): what a
// vtkSmoothPolyDataFilter without boundary and feature-edge smoothing does after the reference's contour, on the device.
//
// Semantics (include/dmi.h states them in full; tests/isosurface_smooth_np.py restates them on the CPU and the
// result is identical): neighbours by vertex id in ascending id, the endpoints of the edges one triangle names are fixed, Jacobi
// steps in f64 with the neighbours added left to right, geometric normals from the triangles in ascending index.  No floating
// point atomics: every sum is made by one lane in the definition's order.
//
// Passes:
//   edge keys   per triangle its three undirected edges in both directions as (a << B | b), B = the bits of a vertex id; a
//               triangle that names an id twice gives its one real edge once; unused slots hold a key above every real one
//   sort        rocPRIM radix sort of the 6 T keys over their 2 B bits: row a's keys are together, ascending in b, and an edge
//               named by n triangles is a run of n equal keys -- a run of one is a boundary edge
//   rows        per vertex the start of its row (a binary search), then its distinct neighbours counted and its fixed bit: 64
//               vertices' bits are one ballot, stored by one lane
//   scan, fill  rocPRIM exclusive scan of the valences = the CSR offsets; the distinct neighbours written behind them
//   incidence   (meshes with normals) per triangle the ids it names as (v << Bt | t), sorted: row v's triangles ascending
//   step        the hot path, 2 x iterations launches: a lane per vertex gathers its neighbours' positions ([V][3] f64, the
//               mesh's own layout: one 24-byte row per neighbour) from the previous step's buffer and writes the next one's
//   normals     a lane per vertex over its incident triangles
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "fusion_kernels.h"

namespace dmi {
namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ uint64_t key_limit(int bits) { return bits >= 64 ? ~uint64_t(0) : (uint64_t(1) << bits) - 1; }

// keys[6 t .. 6 t + 6): a key above every real one (all 2 B bits set: its a is not a vertex id) where there is nothing to say
__global__ __launch_bounds__(kBlock) void smooth_edge_keys_kernel(const int64_t *__restrict__ tris, uint64_t n_triangles,
                                                                  uint64_t n_vertices, int id_bits, uint64_t *__restrict__ keys) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n_triangles) return;
  const uint64_t none = key_limit(2 * id_bits);
  const uint64_t a = (uint64_t)tris[3 * t], b = (uint64_t)tris[3 * t + 1], c = (uint64_t)tris[3 * t + 2];
  uint64_t k[6] = {none, none, none, none, none, none};
  if (a < n_vertices && b < n_vertices && c < n_vertices) {  // (always, for a mesh of this library: such a triangle says nothing)
    auto both = [&](int slot, uint64_t x, uint64_t y) {
      k[slot] = (x << id_bits) | y;
      k[slot + 1] = (y << id_bits) | x;
    };
    if (a != b && b != c && c != a) {
      both(0, a, b);
      both(2, b, c);
      both(4, c, a);
    } else if (a != b) {  // two distinct ids: one edge, named once by this triangle
      both(0, a, b);
    } else if (b != c) {
      both(0, b, c);
    }
  }
#pragma unroll
  for (int e = 0; e < 6; ++e) keys[6 * t + e] = k[e];
}

// keys[3 t .. 3 t + 3): (v << triangle_bits | t) for every distinct id v the triangle names
__global__ __launch_bounds__(kBlock) void smooth_incidence_keys_kernel(const int64_t *__restrict__ tris, uint64_t n_triangles,
                                                                       uint64_t n_vertices, int id_bits, int triangle_bits,
                                                                       uint64_t *__restrict__ keys) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n_triangles) return;
  const uint64_t none = key_limit(id_bits + triangle_bits);
  const uint64_t a = (uint64_t)tris[3 * t], b = (uint64_t)tris[3 * t + 1], c = (uint64_t)tris[3 * t + 2];
  uint64_t k[3] = {none, none, none};
  if (a < n_vertices && b < n_vertices && c < n_vertices) {
    k[0] = (a << triangle_bits) | t;
    if (b != a) k[1] = (b << triangle_bits) | t;
    if (c != a && c != b) k[2] = (c << triangle_bits) | t;
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) keys[3 * t + e] = k[e];
}

// row_start[v], v in [0, n_vertices]: the first sorted key that is not below (v << shift)
__global__ __launch_bounds__(kBlock) void smooth_row_start_kernel(const uint64_t *__restrict__ keys, uint32_t n_keys, uint64_t n_vertices,
                                                                  int shift, uint32_t *__restrict__ row_start) {
  const uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v > n_vertices) return;
  const uint64_t want = v << shift;  // (v <= n_vertices < 2^id_bits, shift <= 32: nothing is shifted out)
  uint32_t lo = 0, hi = n_keys;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < want) lo = mid + 1;
    else hi = mid;
  }
  row_start[v] = lo;
}

// valence[v] = the distinct keys of row v (valence[n_vertices] = 0 for the scan's total); fixed: bit (v & 63) of word v / 64
__global__ __launch_bounds__(kBlock) void smooth_valence_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ row_start,
                                                                uint64_t n_vertices, uint32_t *__restrict__ valence,
                                                                unsigned long long *__restrict__ fixed) {
  const uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  uint32_t distinct = 0;
  bool boundary = false;
  if (v < n_vertices) {
    const uint32_t lo = row_start[v], hi = row_start[v + 1];
    uint64_t prev = 0;
    uint32_t run = 0;
    for (uint32_t j = lo; j < hi; ++j) {
      const uint64_t k = keys[j];
      if (j == lo || k != prev) {
        boundary |= run == 1;
        ++distinct;
        run = 0;
      }
      ++run;
      prev = k;
    }
    boundary |= run == 1;
  }
  if (v <= n_vertices) valence[v] = distinct;
  const unsigned long long bits = __ballot(boundary);  // (no lane has left)
  if ((threadIdx.x & 63) == 0 && v < n_vertices) fixed[v >> 6] = bits;
}

__global__ __launch_bounds__(kBlock) void smooth_fill_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ row_start,
                                                             const uint32_t *__restrict__ offsets, uint64_t n_vertices, int id_bits,
                                                             uint32_t *__restrict__ neighbours) {
  const uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= n_vertices) return;
  const uint32_t lo = row_start[v], hi = row_start[v + 1];
  const uint64_t mask = key_limit(id_bits);
  uint32_t w = offsets[v];
  uint64_t prev = 0;
  for (uint32_t j = lo; j < hi; ++j) {
    const uint64_t k = keys[j];
    if (j == lo || k != prev) neighbours[w++] = (uint32_t)(k & mask);
    prev = k;
  }
}

// One Jacobi step.  A lane per vertex; the neighbours' rows are gathered four at a time (the loads of a batch are independent of
// each other, the additions are not) and added in ascending id, the first one starting the sum.
__global__ __launch_bounds__(kBlock) void smooth_step_kernel(const double *__restrict__ in, double *__restrict__ out,
                                                             const uint32_t *__restrict__ offsets, const uint32_t *__restrict__ neighbours,
                                                             const unsigned long long *__restrict__ fixed, uint64_t n_vertices, double f) {
  const uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= n_vertices) return;
  const uint32_t lo = offsets[v], k = offsets[v + 1] - lo;
  const double p0 = in[3 * v], p1 = in[3 * v + 1], p2 = in[3 * v + 2];
  double r0 = p0, r1 = p1, r2 = p2;
  if (k != 0 && !((fixed[v >> 6] >> (v & 63)) & 1ull)) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (uint32_t j = 0; j < k; j += 4) {
      double q[4][3];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint64_t u = j + e < k ? (uint64_t)neighbours[lo + j + e] : v;  // (v: a row that is there, its values unused)
        q[e][0] = in[3 * u];
        q[e][1] = in[3 * u + 1];
        q[e][2] = in[3 * u + 2];
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
    r0 = p0 + f * (s0 / n - p0);
    r1 = p1 + f * (s1 / n - p1);
    r2 = p2 + f * (s2 / n - p2);
  }
  out[3 * v] = r0;
  out[3 * v + 1] = r1;
  out[3 * v + 2] = r2;
}

// the last steps are those of the extraction's normals: the length, the division unless it is 0, the rounding to f32
__global__ __launch_bounds__(kBlock) void smooth_normals_kernel(const double *__restrict__ p, const int64_t *__restrict__ tris,
                                                                const uint64_t *__restrict__ incidence, const uint32_t *__restrict__ row_start,
                                                                uint64_t n_vertices, int triangle_bits, float *__restrict__ normals) {
  const uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= n_vertices) return;
  const uint32_t lo = row_start[v], hi = row_start[v + 1];
  const uint64_t mask = key_limit(triangle_bits);
  double w0 = 0.0, w1 = 0.0, w2 = 0.0;
  for (uint32_t j = lo; j < hi; ++j) {
    const uint64_t t = incidence[j] & mask;
    const uint64_t a = (uint64_t)tris[3 * t], b = (uint64_t)tris[3 * t + 1], c = (uint64_t)tris[3 * t + 2];
    const double a0 = p[3 * a], a1 = p[3 * a + 1], a2 = p[3 * a + 2];
    const double e0 = p[3 * b] - a0, e1 = p[3 * b + 1] - a1, e2 = p[3 * b + 2] - a2;
    const double g0 = p[3 * c] - a0, g1 = p[3 * c + 1] - a1, g2 = p[3 * c + 2] - a2;
    const double x0 = e1 * g2 - e2 * g1, x1 = e2 * g0 - e0 * g2, x2 = e0 * g1 - e1 * g0;
    if (j == lo) {
      w0 = x0;
      w1 = x1;
      w2 = x2;
    } else {
      w0 = w0 + x0;
      w1 = w1 + x1;
      w2 = w2 + x2;
    }
  }
  const double len = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
  if (len != 0.0) {  // (a NaN length too)
    w0 = w0 / len;
    w1 = w1 / len;
    w2 = w2 / len;
  }
  normals[3 * v] = (float)w0;
  normals[3 * v + 1] = (float)w1;
  normals[3 * v + 2] = (float)w2;
}

unsigned blocks(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

int bits_for(uint64_t count) {  // the smallest B >= 1 with count < 2^B: every id below count fits, and B set bits are not an id
  int b = 1;
  while (b < 64 && (count >> b) != 0) ++b;
  return b;
}

hipError_t sort_keys(void *temp, size_t *temp_bytes, uint64_t *a, uint64_t *b, uint64_t n, int bits, uint64_t **sorted,
                     hipStream_t stream) {
  rocprim::double_buffer<uint64_t> keys(a, b);
  size_t bytes = *temp_bytes;
  const hipError_t e = rocprim::radix_sort_keys(temp, bytes, keys, (size_t)n, 0u, (unsigned)bits, stream);
  if (!temp) *temp_bytes = bytes;
  if (sorted) *sorted = keys.current();
  return e;
}

// The vertex -> triangle incidence of the normals: the 3 T keys (v << Bt | t) written to inc_a and sorted into inc_a or inc_b
// (*incidence), row v's triangles ascending in t, and row_start[v], v in [0, V], its rows
hipError_t build_incidence(const int64_t *tris, uint64_t nv, uint64_t nt, uint64_t *inc_a, uint64_t *inc_b, uint32_t *row_start, void *temp,
                           size_t temp_bytes, const uint64_t **incidence, hipStream_t stream) {
  const int id_bits = bits_for(nv), triangle_bits = bits_for(nt);
  hipError_t e = hipSuccess;
  uint64_t *inc_sorted = inc_a;
  if (nt) {
    hipLaunchKernelGGL(smooth_incidence_keys_kernel, dim3(blocks(nt)), dim3(kBlock), 0, stream, tris, nt, nv, id_bits, triangle_bits, inc_a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t bytes = temp_bytes;
    if ((e = sort_keys(temp, &bytes, inc_a, inc_b, 3 * nt, id_bits + triangle_bits, &inc_sorted, stream)) != hipSuccess) return e;
  }
  *incidence = inc_sorted;
  hipLaunchKernelGGL(smooth_row_start_kernel, dim3(blocks(nv + 1)), dim3(kBlock), 0, stream, inc_sorted, (uint32_t)(3 * nt), nv, triangle_bits, row_start);
  return hipGetLastError();
}

}  // namespace

// the storage rocPRIM asks for: the largest of the two sorts' and the scan's
hipError_t smooth_temp_bytes(uint64_t n_vertices, uint64_t n_triangles, size_t *bytes) {
  const int id_bits = bits_for(n_vertices), triangle_bits = bits_for(n_triangles);
  size_t a = 0, b = 0, c = 0;
  hipError_t e = sort_keys(nullptr, &a, nullptr, nullptr, std::max<uint64_t>(6 * n_triangles, 1), 2 * id_bits, nullptr, nullptr);
  if (e != hipSuccess) return e;
  e = sort_keys(nullptr, &b, nullptr, nullptr, std::max<uint64_t>(3 * n_triangles, 1), id_bits + triangle_bits, nullptr, nullptr);
  if (e != hipSuccess) return e;
  e = rocprim::exclusive_scan(nullptr, c, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t)0, (size_t)(n_vertices + 1),
                              rocprim::plus<uint32_t>(), nullptr);
  *bytes = std::max(a, std::max(b, c));
  return e;
}

// Smooths mesh `m` (n_vertices >= 1, 6 n_triangles < 2^32, iterations >= 1): the positions end in *result, which is
// s.positions[0] or s.positions[1]; the normals, when m.normals_out is not null, in m.normals_out.  Nothing of the mesh itself is
// written.  `events`: 4 events recorded around the passes (adjacency, steps, normals), or null.
hipError_t launch_isosurface_smooth(const SmoothMesh &m, const SmoothScratch &s, int iterations, double lambda, double mu,
                                    double **result, hipEvent_t *events, hipStream_t stream) {
  const uint64_t nv = m.n_vertices, nt = m.n_triangles, n_keys = 6 * nt;
  const int id_bits = bits_for(nv), triangle_bits = bits_for(nt);
  auto mark = [&](int i) -> hipError_t { return events ? hipEventRecord(events[i], stream) : hipSuccess; };
  hipError_t e = mark(0);
  if (e != hipSuccess) return e;
  uint64_t *sorted = s.keys[0];
  uint64_t *spare = s.keys[1];
  size_t bytes = s.temp_bytes;
  if (nt) {
    hipLaunchKernelGGL(smooth_edge_keys_kernel, dim3(blocks(nt)), dim3(kBlock), 0, stream, m.triangles, nt, nv, id_bits, s.keys[0]);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = sort_keys(s.temp, &bytes, s.keys[0], s.keys[1], n_keys, 2 * id_bits, &sorted, stream)) != hipSuccess) return e;
    spare = sorted == s.keys[0] ? s.keys[1] : s.keys[0];
  }
  // the neighbour ids (at most 6 T of 4 bytes) go where the unsorted keys were: the first half of the spare buffer
  uint32_t *neighbours = (uint32_t *)spare;
  hipLaunchKernelGGL(smooth_row_start_kernel, dim3(blocks(nv + 1)), dim3(kBlock), 0, stream, sorted, (uint32_t)n_keys, nv, id_bits, s.row_start);
  hipLaunchKernelGGL(smooth_valence_kernel, dim3(blocks(nv + 1)), dim3(kBlock), 0, stream, sorted, s.row_start, nv, s.valence, s.fixed);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  bytes = s.temp_bytes;
  e = rocprim::exclusive_scan(s.temp, bytes, s.valence, s.offsets, (uint32_t)0, (size_t)(nv + 1), rocprim::plus<uint32_t>(), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(smooth_fill_kernel, dim3(blocks(nv)), dim3(kBlock), 0, stream, sorted, s.row_start, s.offsets, nv, id_bits, neighbours);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // the incidence of the normals: its 3 T keys in the second half of the spare buffer, sorted into it or into the first half of
  // the buffer that held the sorted edge keys (read for the last time by the fill kernel above)
  const uint64_t *incidence = nullptr;
  if (m.normals_out && (e = build_incidence(m.triangles, nv, nt, spare + 3 * nt, sorted, s.row_start, s.temp, s.temp_bytes, &incidence, stream)) != hipSuccess)
    return e;
  if ((e = mark(1)) != hipSuccess) return e;
  const double *in = m.vertices;
  int next = 0;
  for (int it = 0; it < iterations; ++it)
    for (int half = 0; half < (mu != 0.0 ? 2 : 1); ++half) {
      hipLaunchKernelGGL(smooth_step_kernel, dim3(blocks(nv)), dim3(kBlock), 0, stream, in, s.positions[next], s.offsets, neighbours, s.fixed, nv,
                         half == 0 ? lambda : mu);
      in = s.positions[next];
      next ^= 1;
    }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  *result = s.positions[next ^ 1];
  if ((e = mark(2)) != hipSuccess) return e;
  if (m.normals_out) {
    hipLaunchKernelGGL(smooth_normals_kernel, dim3(blocks(nv)), dim3(kBlock), 0, stream, in, m.triangles, incidence, s.row_start, nv, triangle_bits, m.normals_out);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return mark(3);
}

hipError_t launch_isosurface_geometric_normals(const double *vertices, const int64_t *triangles, uint64_t n_vertices, uint64_t n_triangles,
                                               uint64_t *const keys[2], uint32_t *row_start, void *temp, size_t temp_bytes,
                                               float *normals_out, hipStream_t stream) {
  const uint64_t *incidence = nullptr;
  const hipError_t e = build_incidence(triangles, n_vertices, n_triangles, keys[0], keys[1], row_start, temp, temp_bytes, &incidence, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(smooth_normals_kernel, dim3(blocks(n_vertices)), dim3(kBlock), 0, stream, vertices, triangles, incidence, row_start, n_vertices,
                     bits_for(n_triangles), normals_out);
  return hipGetLastError();
}

}  // namespace dmi
