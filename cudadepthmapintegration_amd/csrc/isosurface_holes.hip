// isosurface_holes.hip -- small holes of the iso-surface closed on the device (dmi_fill_isosurface_holes): what a
// vtkFillHolesFilter does behind the reference's contour, with a fan round the rim's centroid instead of an ear clipping.
//
// Semantics (include/dmi.h states them in full; tests/isosurface_holes_np.py restates them on the CPU and the
// result is identical): half-edges of the triangles that name three distinct ids, a boundary edge is an undirected edge one
// triangle names, a loop is a cycle of vertices with one boundary half-edge in and one out, its head is its smallest id, a loop
// of 3 .. max_edges edges gets one triangle (3) or a centroid and a fan (4 and more).  No floating point atomics: a loop's
// centroid and its normal are made by one lane in walk order.  The integer atomics are counts, whatever their order.
//
// Passes:
//   boundary   per triangle its three undirected edges as ((lo << B | hi) << 1 | dir), B = the bits of a vertex id, dir = the
//              triangle stores hi -> lo; one rocPRIM radix sort over the 2 B bits above dir; a run of one is a boundary edge:
//              its half-edge counts at its start's out-degree and its end's in-degree and is its start's successor; the vertices
//              with a degree are the boundary vertices, numbered in ascending id by a scan (their "slots")
//   loops      per slot a pointer (a simple vertex: its successor's slot; a complex one: itself) and a label (its own slot; a
//              complex one: poisoned); R rounds of pointer doubling, label = the smaller one, poison = either's, from one buffer
//              into the other: after them a label covers the slot and its next 2^R - 1 successors.  R = ceil(log2(the most edges
//              a loop can have)) + 1, so a loop that may be filled has been seen whole by every one of its vertices.  A label's
//              count is its loop's length.  A head is a slot that is its own label and its successor's: the successor has then
//              seen it, so it is on a cycle no longer than 2^R, seen whole, counted whole.  (The local minima of a longer cycle,
//              and of a chain that ends in a complex vertex further than 2^R away, are their own label but not their
//              successor's.)  Two scans over the heads: the new vertices and the new triangles in front of each
//   fill       the old mesh copied; a lane per head walks its L steps once: it confirms that the walk closes, adds the
//              centroid in walk order and writes the loop's triangles behind the scans' offsets, then reads them back for the
//              new vertex's normal
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "fusion_kernels.h"

namespace dmi {
namespace {

constexpr int kBlock = 256;
constexpr uint32_t kPoison = 0x80000000u;  // (slots are below 2^31: launch_holes_boundary's precondition)

__device__ __forceinline__ uint64_t key_limit(int bits) { return bits >= 64 ? ~uint64_t(0) : (uint64_t(1) << bits) - 1; }

// keys[3 t .. 3 t + 3): a key above every real one (all 2 B + 1 bits set: its lo is not below its hi) for a triangle that names
// an id twice or one that is no vertex
__global__ __launch_bounds__(kBlock) void holes_edge_keys_kernel(const int64_t *__restrict__ tris, uint64_t n_triangles, uint64_t n_vertices,
                                                                 int id_bits, uint64_t *__restrict__ keys) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n_triangles) return;
  const uint64_t none = key_limit(2 * id_bits + 1);
  const uint64_t a = (uint64_t)tris[3 * t], b = (uint64_t)tris[3 * t + 1], c = (uint64_t)tris[3 * t + 2];
  uint64_t k[3] = {none, none, none};
  if (a < n_vertices && b < n_vertices && c < n_vertices && a != b && b != c && c != a) {
    auto key = [&](uint64_t x, uint64_t y) {  // the half-edge x -> y
      return x < y ? ((x << id_bits) | y) << 1 : (((y << id_bits) | x) << 1) | 1;
    };
    k[0] = key(a, b);
    k[1] = key(b, c);
    k[2] = key(c, a);
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) keys[3 * t + e] = k[e];
}

// The runs of one among the sorted keys.  Two half-edges may write one vertex's successor: it has two out then, is complex, and
// its successor is never read.  counters[0]: the boundary edges, one addition per wave.
__global__ __launch_bounds__(kBlock) void holes_runs_kernel(const uint64_t *__restrict__ keys, uint32_t n_keys, int id_bits,
                                                            uint32_t *__restrict__ out_deg, uint32_t *__restrict__ in_deg,
                                                            uint32_t *__restrict__ succ, unsigned long long *__restrict__ counters) {
  const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  bool single = false;
  if (j < n_keys) {
    const uint64_t k = keys[j], edge = k >> 1;
    if (edge != key_limit(2 * id_bits)) {
      single = (j == 0 || (keys[j - 1] >> 1) != edge) && (j + 1 == n_keys || (keys[j + 1] >> 1) != edge);
      if (single) {
        const uint32_t lo = (uint32_t)(edge >> id_bits), hi = (uint32_t)(edge & key_limit(id_bits));
        const uint32_t from = (k & 1) ? hi : lo, to = (k & 1) ? lo : hi;
        atomicAdd(&out_deg[from], 1u);
        atomicAdd(&in_deg[to], 1u);
        succ[from] = to;
      }
    }
  }
  const unsigned long long found = __ballot(single);  // (no lane has left)
  if ((threadIdx.x & 63) == 0 && found) atomicAdd(&counters[0], (unsigned long long)__popcll(found));
}

// flag[v], v in [0, n_vertices]: a boundary half-edge starts or ends at v (flag[n_vertices] = 0 for the scan's total)
__global__ __launch_bounds__(kBlock) void holes_flag_kernel(const uint32_t *__restrict__ out_deg, const uint32_t *__restrict__ in_deg,
                                                            uint64_t n_vertices, uint32_t *__restrict__ flag) {
  const uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v > n_vertices) return;
  flag[v] = v < n_vertices && (out_deg[v] | in_deg[v]) != 0 ? 1u : 0u;
}

// a boundary vertex's slot: its id, its successor's slot, and the doubling's first pointer and label
__global__ __launch_bounds__(kBlock) void holes_slots_kernel(const uint32_t *__restrict__ out_deg, const uint32_t *__restrict__ in_deg,
                                                             const uint32_t *__restrict__ succ, const uint32_t *__restrict__ flag,
                                                             const uint32_t *__restrict__ rank, uint64_t n_vertices, uint32_t *__restrict__ id,
                                                             uint32_t *__restrict__ next, uint32_t *__restrict__ ptr, uint32_t *__restrict__ label,
                                                             uint32_t *__restrict__ count) {
  const uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= n_vertices || !flag[v]) return;
  const uint32_t i = rank[v];
  const bool simple = out_deg[v] == 1 && in_deg[v] == 1;
  const uint32_t to = simple ? rank[succ[v]] : i;  // (the successor ends a boundary half-edge: it has a slot)
  id[i] = (uint32_t)v;
  next[i] = to;
  ptr[i] = to;
  label[i] = simple ? i : (i | kPoison);
  count[i] = 0;
}

__global__ __launch_bounds__(kBlock) void holes_double_kernel(const uint32_t *__restrict__ ptr_in, const uint32_t *__restrict__ label_in,
                                                              uint32_t n_slots, uint32_t *__restrict__ ptr_out, uint32_t *__restrict__ label_out) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_slots) return;
  const uint32_t p = ptr_in[i], a = label_in[i], b = label_in[p];
  label_out[i] = min(a & ~kPoison, b & ~kPoison) | ((a | b) & kPoison);
  ptr_out[i] = ptr_in[p];
}

__global__ __launch_bounds__(kBlock) void holes_count_kernel(const uint32_t *__restrict__ label, uint32_t n_slots, uint32_t *__restrict__ count) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_slots) return;
  const uint32_t l = label[i];
  if (!(l & kPoison)) atomicAdd(&count[l], 1u);
}

// new_vertices[i], new_triangles[i], i in [0, n_slots]: what the loop headed by slot i adds (0 at n_slots for the scans' totals);
// counters[1], counters[2]: the filled loops and their edges, one addition per wave
__global__ __launch_bounds__(kBlock) void holes_heads_kernel(const uint32_t *__restrict__ label, const uint32_t *__restrict__ next,
                                                             const uint32_t *__restrict__ count, uint32_t n_slots, uint32_t max_edges,
                                                             uint32_t *__restrict__ new_vertices, uint32_t *__restrict__ new_triangles,
                                                             unsigned long long *__restrict__ counters) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  uint32_t edges = 0;
  if (i < n_slots && label[i] == i && label[next[i]] == i) {
    const uint32_t L = count[i];
    if (L >= 3 && L <= max_edges) edges = L;
  }
  if (i <= n_slots) {
    new_vertices[i] = edges >= 4 ? 1u : 0u;
    new_triangles[i] = edges >= 4 ? edges : (edges ? 1u : 0u);
  }
  // (no lane has left) a wave's edges: its lanes' added by a butterfly of integer additions
  const unsigned long long heads = __ballot(edges != 0);
  if (heads) {
    uint32_t sum = edges;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if ((threadIdx.x & 63) == 0) {
      atomicAdd(&counters[1], (unsigned long long)__popcll(heads));
      atomicAdd(&counters[2], (unsigned long long)sum);
    }
  }
}

// A lane per head.  The walk that does not come back to its head after exactly L steps (it cannot: see above) is counted in
// counters[3], and the call fails.
__global__ __launch_bounds__(kBlock) void holes_fill_kernel(const uint32_t *__restrict__ id, const uint32_t *__restrict__ next,
                                                            const uint32_t *__restrict__ count, const uint32_t *__restrict__ new_triangles,
                                                            const uint32_t *__restrict__ vertex_offset, const uint32_t *__restrict__ triangle_offset,
                                                            uint32_t n_slots, uint64_t n_vertices, uint64_t n_triangles, double *vertices,
                                                            int64_t *triangles, float *normals, unsigned long long *__restrict__ counters) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_slots || new_triangles[i] == 0) return;
  const uint32_t L = count[i];
  int64_t *tri = triangles + 3 * (n_triangles + triangle_offset[i]);
  const int64_t h0 = (int64_t)id[i];
  if (L == 3) {
    const uint32_t i1 = next[i], i2 = next[i1];
    if (next[i2] != i || i1 == i || i2 == i) atomicAdd(&counters[3], 1ull);
    tri[0] = h0;
    tri[1] = (int64_t)id[i2];
    tri[2] = (int64_t)id[i1];
    return;
  }
  const uint64_t c = n_vertices + vertex_offset[i];
  double s0 = vertices[3 * h0], s1 = vertices[3 * h0 + 1], s2 = vertices[3 * h0 + 2];
  uint32_t cur = i;
  int64_t h = h0;
  bool closed = true;
  for (uint32_t e = 0; e < L; ++e) {  // triangle e = (h_{e+1}, h_e, c)
    cur = next[cur];
    const int64_t to = (int64_t)id[cur];
    if (e + 1 < L) {
      closed &= cur != i;
      s0 = s0 + vertices[3 * to];
      s1 = s1 + vertices[3 * to + 1];
      s2 = s2 + vertices[3 * to + 2];
    }
    tri[3 * e] = to;
    tri[3 * e + 1] = h;
    tri[3 * e + 2] = (int64_t)c;
    h = to;
  }
  if (!closed || cur != i) atomicAdd(&counters[3], 1ull);
  const double n = (double)L;
  const double c0 = s0 / n, c1 = s1 / n, c2 = s2 / n;
  vertices[3 * c] = c0;
  vertices[3 * c + 1] = c1;
  vertices[3 * c + 2] = c2;
  if (!normals) return;
  // the smoother's geometric normal over the L triangles just written, in ascending index
  double w0 = 0.0, w1 = 0.0, w2 = 0.0;
  for (uint32_t e = 0; e < L; ++e) {
    const int64_t a = tri[3 * e], b = tri[3 * e + 1];
    const double a0 = vertices[3 * a], a1 = vertices[3 * a + 1], a2 = vertices[3 * a + 2];
    const double e0 = vertices[3 * b] - a0, e1 = vertices[3 * b + 1] - a1, e2 = vertices[3 * b + 2] - a2;
    const double g0 = c0 - a0, g1 = c1 - a1, g2 = c2 - a2;
    const double x0 = e1 * g2 - e2 * g1, x1 = e2 * g0 - e0 * g2, x2 = e0 * g1 - e1 * g0;
    if (e == 0) {
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
  normals[3 * c] = (float)w0;
  normals[3 * c + 1] = (float)w1;
  normals[3 * c + 2] = (float)w2;
}

unsigned blocks(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

int bits_for(uint64_t count) {  // the smallest B >= 1 with count < 2^B
  int b = 1;
  while (b < 64 && (count >> b) != 0) ++b;
  return b;
}

int ceil_log2(uint64_t n) {  // the smallest k with 2^k >= n
  int k = 0;
  while (k < 63 && (uint64_t(1) << k) < n) ++k;
  return k;
}

// the keys' bits above the direction bit
hipError_t sort_edges(void *temp, size_t *temp_bytes, uint64_t *a, uint64_t *b, uint64_t n, int id_bits, uint64_t **sorted, hipStream_t stream) {
  rocprim::double_buffer<uint64_t> keys(a, b);
  size_t bytes = *temp_bytes;
  const hipError_t e = rocprim::radix_sort_keys(temp, bytes, keys, (size_t)n, 1u, (unsigned)(2 * id_bits + 1), stream);
  if (!temp) *temp_bytes = bytes;
  if (sorted) *sorted = keys.current();
  return e;
}

hipError_t scan(void *temp, size_t temp_bytes, uint32_t *in, uint32_t *out, uint64_t n, hipStream_t stream) {
  return rocprim::exclusive_scan(temp, temp_bytes, in, out, (uint32_t)0, (size_t)n, rocprim::plus<uint32_t>(), stream);
}

}  // namespace

// the storage rocPRIM asks for: the larger of the sort's and the largest scan's (over the vertices; the slots are no more)
hipError_t holes_temp_bytes(uint64_t n_vertices, uint64_t n_triangles, size_t *bytes) {
  size_t a = 0, b = 0;
  hipError_t e = sort_edges(nullptr, &a, nullptr, nullptr, std::max<uint64_t>(3 * n_triangles, 1), bits_for(n_vertices), nullptr, nullptr);
  if (e != hipSuccess) return e;
  e = rocprim::exclusive_scan(nullptr, b, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t)0, (size_t)(n_vertices + 1),
                              rocprim::plus<uint32_t>(), nullptr);
  *bytes = std::max(a, b);
  return e;
}

int holes_rounds(uint64_t max_edges, uint64_t n_slots) { return ceil_log2(std::max<uint64_t>(std::min(max_edges, n_slots), 1)) + 1; }

// The boundary of mesh `m` (1 <= n_vertices < 2^31, 3 n_triangles < 2^32).  Afterwards v.rank[n_vertices] is the number of
// boundary vertices and counters[0] the number of boundary edges.  `events`: 2, recorded around the pass.
hipError_t launch_holes_boundary(const HolesMesh &m, const HolesVertexScratch &v, uint64_t *const keys[2], void *temp, size_t temp_bytes,
                                 unsigned long long *counters, hipEvent_t *events, hipStream_t stream) {
  const uint64_t nv = m.n_vertices, nt = m.n_triangles, n_keys = 3 * nt;
  const int id_bits = bits_for(nv);
  hipError_t e = hipEventRecord(events[0], stream);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(counters, 0, 4 * sizeof(unsigned long long), stream)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(v.out_deg, 0, (nv + 1) * sizeof(uint32_t), stream)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(v.in_deg, 0, (nv + 1) * sizeof(uint32_t), stream)) != hipSuccess) return e;
  if (nt) {
    uint64_t *sorted = keys[0];
    hipLaunchKernelGGL(holes_edge_keys_kernel, dim3(blocks(nt)), dim3(kBlock), 0, stream, m.triangles, nt, nv, id_bits, keys[0]);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t bytes = temp_bytes;
    if ((e = sort_edges(temp, &bytes, keys[0], keys[1], n_keys, id_bits, &sorted, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(holes_runs_kernel, dim3(blocks(n_keys)), dim3(kBlock), 0, stream, sorted, (uint32_t)n_keys, id_bits, v.out_deg, v.in_deg,
                       v.succ, counters);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(holes_flag_kernel, dim3(blocks(nv + 1)), dim3(kBlock), 0, stream, v.out_deg, v.in_deg, nv, v.flag);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = scan(temp, temp_bytes, v.flag, v.rank, nv + 1, stream)) != hipSuccess) return e;
  return hipEventRecord(events[1], stream);
}

// The loops among the n_slots >= 1 boundary vertices of that pass, max_edges >= 3.  Afterwards l.vertex_offset[n_slots] and
// l.triangle_offset[n_slots] are what the fill adds, counters[1] and [2] the loops it fills and their edges.  `event`: recorded
// behind the pass.
hipError_t launch_holes_loops(const HolesMesh &m, const HolesVertexScratch &v, const HolesLoopScratch &l, uint32_t n_slots, uint64_t max_edges,
                              void *temp, size_t temp_bytes, unsigned long long *counters, hipEvent_t event, hipStream_t stream) {
  hipError_t e = hipSuccess;
  hipLaunchKernelGGL(holes_slots_kernel, dim3(blocks(m.n_vertices)), dim3(kBlock), 0, stream, v.out_deg, v.in_deg, v.succ, v.flag, v.rank,
                     m.n_vertices, l.id, l.next, l.ptr[0], l.label[0], l.count);
  const int rounds = holes_rounds(max_edges, n_slots);
  for (int r = 0; r < rounds; ++r)
    hipLaunchKernelGGL(holes_double_kernel, dim3(blocks(n_slots)), dim3(kBlock), 0, stream, l.ptr[r & 1], l.label[r & 1], n_slots,
                       l.ptr[(r & 1) ^ 1], l.label[(r & 1) ^ 1]);
  const uint32_t *label = l.label[rounds & 1];
  hipLaunchKernelGGL(holes_count_kernel, dim3(blocks(n_slots)), dim3(kBlock), 0, stream, label, n_slots, l.count);
  hipLaunchKernelGGL(holes_heads_kernel, dim3(blocks((uint64_t)n_slots + 1)), dim3(kBlock), 0, stream, label, l.next, l.count, n_slots,
                     (uint32_t)std::min<uint64_t>(max_edges, 0xffffffffu), l.new_vertices, l.new_triangles, counters);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = scan(temp, temp_bytes, l.new_vertices, l.vertex_offset, (uint64_t)n_slots + 1, stream)) != hipSuccess) return e;
  if ((e = scan(temp, temp_bytes, l.new_triangles, l.triangle_offset, (uint64_t)n_slots + 1, stream)) != hipSuccess) return e;
  return hipEventRecord(event, stream);
}

// The filled mesh into `out`, which has room for the old mesh and what launch_holes_loops counted: the old mesh copied, the new
// vertices, triangles and (out.normals not null) normals behind it.  counters[3] stays 0.  `event`: recorded behind the pass.
hipError_t launch_holes_fill(const HolesMesh &m, const HolesLoopScratch &l, uint32_t n_slots, const HolesOutput &out,
                             unsigned long long *counters, hipEvent_t event, hipStream_t stream) {
  hipError_t e = hipMemcpyAsync(out.vertices, m.vertices, m.n_vertices * 3 * sizeof(double), hipMemcpyDeviceToDevice, stream);
  if (e != hipSuccess) return e;
  if (m.n_triangles &&
      (e = hipMemcpyAsync(out.triangles, m.triangles, m.n_triangles * 3 * sizeof(int64_t), hipMemcpyDeviceToDevice, stream)) != hipSuccess)
    return e;
  if (out.normals && (e = hipMemcpyAsync(out.normals, m.normals, m.n_vertices * 3 * sizeof(float), hipMemcpyDeviceToDevice, stream)) != hipSuccess)
    return e;
  hipLaunchKernelGGL(holes_fill_kernel, dim3(blocks(n_slots)), dim3(kBlock), 0, stream, l.id, l.next, l.count, l.new_triangles, l.vertex_offset,
                     l.triangle_offset, n_slots, m.n_vertices, m.n_triangles, out.vertices, out.triangles, out.normals, counters);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return hipEventRecord(event, stream);
}

}  // namespace dmi
