// isosurface.hip -- the contour step of the reference's CLI (Reconstruction/main.cxx:166-182: vtkContourFilter on the
// point data, then vtkTransformFilter with the grid matrix) as marching cubes on the device.  Streaming, HBM-bound.
//
// Semantics (tests/isosurface_np.py restates them on the CPU and the result is bit-identical):
//   * a lattice point is inside when value >= iso (a NaN is outside: the iso_cell_active test of grid_post.hip);
//   * one vertex per crossed lattice edge (exactly one inside endpoint), owned by its lower endpoint; vertices are
//     numbered by (owner point's linear id, axis x < y < z);
//   * t = (iso - v_a) / (v_b - v_a) (0 / 1 when a NaN endpoint makes a / b the inside one), the corner coordinates
//     origin + idx * spacing, x_d = c_a[d] + t * (c_b[d] - c_a[d]), then the grid matrix, every operation rounded;
//   * triangles from the generated case table (isosurface_table.inc), by ascending cell id, then table order.
//
// Two passes over segments of 256 lattice points of one row (j, k): a segment owns the edges of its points and the
// cells whose lower corner is one of them.  The count pass stores (vertices, triangles) per segment, two rocPRIM scans
// give each segment its bases, and the write pass recomputes its masks and writes at base + rank within the segment.
// The triangles of a segment's cells name vertices of the rows (j, k), (j+1, k), (j, k+1), (j+1, k+1) and of one point
// past the segment: the write pass rebuilds those rows' in-segment prefix counts in LDS and adds the scanned bases, so
// no per-point index array exists (device scratch is O(segments)).
// The write pass with normals (NORMALS) also writes each vertex's normal (tests/isosurface_normals_np.py):
// the negated central-difference gradient at both endpoints of its edge, interpolated at t, through the cofactor matrix of
// the grid matrix and normalised, f32.  The gradient's neighbours in rows j - 1 and k - 1 are not among the 8 rows in LDS:
// every lattice value it needs is read from global memory, where L2 and the MALL serve the rows the workgroup just loaded.
#include <rocprim/device/device_scan.hpp>

#include "fusion_kernels.h"

namespace dmi {
namespace {

#include "isosurface_table.inc"

constexpr int kSeg = 256;

// lattice rows a workgroup reads, as (dj, dk) offsets from its own row: rows 0..3 are those whose vertices the cells
// name (row r = dj + 2 dk, the y / z bits of the corner index), 4..7 their +y / +z neighbours that decide y / z crossings
#define DMI_ROW_DJ {0, 1, 0, 1, 2, 2, 0, 1}
#define DMI_ROW_DK {0, 0, 1, 1, 0, 1, 2, 2}
#define DMI_ROW_PLUS_Y {1, 4, 3, 5}  // the row one step along y from row r
#define DMI_ROW_PLUS_Z {2, 3, 6, 7}  // ... along z

// the generated table in device memory (indexed by the case at run time)
template <typename T, int N>
struct Table {
  T v[N];
};
constexpr Table<int, 48> make_edges() {
  Table<int, 48> t{};
  for (int e = 0; e < 12; ++e)
    for (int c = 0; c < 4; ++c) t.v[e * 4 + c] = kMcEdges[e][c];
  return t;
}
constexpr Table<unsigned char, 256> make_count_table() {
  Table<unsigned char, 256> t{};
  for (int c = 0; c < 256; ++c) t.v[c] = kMcTriCount[c];
  return t;
}
constexpr Table<unsigned char, 256 * 3 * kMcMaxTris> make_edge_table() {
  Table<unsigned char, 256 * 3 * kMcMaxTris> t{};
  for (int c = 0; c < 256; ++c)
    for (int e = 0; e < 3 * kMcMaxTris; ++e) t.v[c * 3 * kMcMaxTris + e] = kMcTriEdges[c][e];
  return t;
}
__constant__ Table<int, 48> kEdges = make_edges();
__constant__ Table<unsigned char, 256> kTriCount = make_count_table();
__constant__ Table<unsigned char, 256 * 3 * kMcMaxTris> kTriEdges = make_edge_table();

// Exclusive prefix sum over the workgroup; *total = the sum of all.  Fields packed side by side in x never carry into each
// other (each field's workgroup sum stays below its width).
__device__ __forceinline__ uint64_t block_exclusive_scan(uint64_t x, uint64_t *wave_tot, uint64_t *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t s = x;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint64_t y = __shfl_up(s, off, 64);
    if (lane >= off) s += y;
  }
  if (lane == 63) wave_tot[wave] = s;
  __syncthreads();
  uint64_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kSeg / 64; ++w) {
    before += w < wave ? wave_tot[w] : 0;
    all += wave_tot[w];
  }
  *total = all;
  return before + s - x;
}

constexpr int kField = 12;  // bits per packed count: a segment has at most 257 * 3 vertices per row and 256 * 5 triangles
constexpr uint64_t kFieldMask = (1u << kField) - 1;

// minus the gradient of the point data at lattice point (i, j, k), p = &P[i, j, k]: one-sided at the lattice's borders,
// central inside, every operation rounded.  The contexts have cell_dims >= 1, so no axis has a single point.
__device__ __forceinline__ void neg_gradient(const double *p, int i, int j, int k, const MeshGeom &g, int64_t prow, int64_t pplane,
                                             double out[3]) {
  const int q[3] = {i, j, k}, n[3] = {g.nx, g.ny, g.nz};
  const int64_t stride[3] = {1, prow, pplane};
  const double c = p[0];
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const bool lo = q[e] == 0, hi = q[e] == n[e];
    const double below = lo ? c : p[-stride[e]], above = hi ? c : p[stride[e]];
    // (0.5 * (below - above)) inside, (below - above) at a border: 1.0 * x is x, bit for bit
    out[e] = ((lo || hi ? 1.0 : 0.5) * (below - above)) / g.spacing[e];
  }
}

// Normals: empty for the count pass and the plain write pass, whose kernel arguments and code stay what they were without
// normals; one MeshNormals for the write pass that writes them (NORMALS).
template <bool WRITE, typename... Normals>
__global__ __launch_bounds__(kSeg) void isosurface_kernel(const double *__restrict__ points, MeshGeom g,
                                                          uint32_t *__restrict__ vcounts, uint32_t *__restrict__ tcounts,
                                                          const uint64_t *__restrict__ vbases, const uint64_t *__restrict__ tbases,
                                                          double *__restrict__ verts, int64_t *__restrict__ tris, Normals... normals) {
  constexpr bool NORMALS = sizeof...(Normals) != 0;
  static_assert(sizeof...(Normals) <= 1, "one MeshNormals at most");
  static_assert(WRITE || !NORMALS, "normals are written by the write pass");
  const MeshNormals nrm{normals...};  // (unused without normals)
  constexpr int kRows = WRITE ? 8 : 4;  // the count pass needs the cells' corner rows and the own row's +y / +z only
  __shared__ uint8_t inb[kSeg + 2];     // bit r: point (i0 + q) of row r is inside
  __shared__ uint8_t msk[4][kSeg + 1];  // crossed edges (bit = axis) of the points of rows 0..3
  __shared__ uint32_t pref[4][kSeg + 1];  // their vertices before the point within the segment
  __shared__ uint64_t wave_tot[kSeg / 64];
  const int nx = g.nx, ny = g.ny, nz = g.nz;
  const int64_t prow = (int64_t)nx + 1, pplane = prow * (ny + 1);
  const int64_t seg = blockIdx.x;
  const int64_t row = seg / g.segs_per_row;  // = k * (ny + 1) + j
  const int sx = (int)(seg - row * g.segs_per_row);
  const int k = (int)(row / (ny + 1)), j = (int)(row - (int64_t)k * (ny + 1));
  const int i0 = sx * kSeg, t = threadIdx.x;
  const double iso = g.iso;

  for (int q = t; q < kSeg + 2; q += kSeg) {
    const int i = i0 + q;
    unsigned b = 0;
    if (i <= nx) {
#pragma unroll
      for (int r = 0; r < kRows; ++r) {
        constexpr int dj[8] = DMI_ROW_DJ, dk[8] = DMI_ROW_DK;
        const int jj = j + dj[r], kk = k + dk[r];
        if (jj <= ny && kk <= nz) b |= (points[kk * pplane + jj * prow + i] >= iso ? 1u : 0u) << r;
      }
    }
    inb[q] = (uint8_t)b;
  }
  __syncthreads();

  // crossed edges owned by point q of row r (0..3)
  auto point_mask = [&](int q, int r) -> unsigned {
    const int i = i0 + q, jj = j + (r & 1), kk = k + (r >> 1);
    if (i > nx || jj > ny || kk > nz) return 0u;
    constexpr int plus_y[4] = DMI_ROW_PLUS_Y, plus_z[4] = DMI_ROW_PLUS_Z;
    const unsigned b = inb[q], self = (b >> r) & 1u;
    unsigned m = 0;
    if (i < nx) m |= self ^ ((inb[q + 1] >> r) & 1u);
    if (jj < ny) m |= (self ^ ((b >> plus_y[r]) & 1u)) << 1;
    if (kk < nz) m |= (self ^ ((b >> plus_z[r]) & 1u)) << 2;
    return m;
  };

  const int i = i0 + t;
  unsigned ccase = 0, ntri = 0;
  if (i < nx && j < ny && k < nz) {
#pragma unroll
    for (int c = 0; c < 8; ++c) ccase |= ((inb[t + (c & 1)] >> (c >> 1)) & 1u) << c;
    ntri = kTriCount.v[ccase];
  }

  if constexpr (!WRITE) {
    const unsigned m0 = point_mask(t, 0);
    uint64_t total = 0;
    (void)block_exclusive_scan((uint64_t)__popc(m0) | ((uint64_t)ntri << 32), wave_tot, &total);
    if (t == 0) {
      vcounts[seg] = (uint32_t)(total & 0xffffffffu);
      tcounts[seg] = (uint32_t)(total >> 32);
    }
  } else {
    unsigned m[4];
    uint64_t packed = (uint64_t)ntri << (4 * kField);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      m[r] = point_mask(t, r);
      packed |= (uint64_t)__popc(m[r]) << (r * kField);
    }
    uint64_t total = 0;
    const uint64_t excl = block_exclusive_scan(packed, wave_tot, &total);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      msk[r][t] = (uint8_t)m[r];
      pref[r][t] = (uint32_t)((excl >> (r * kField)) & kFieldMask);
      if (t == 0) {  // the first point of the next segment: its prefix within this one is this segment's total
        msk[r][kSeg] = (uint8_t)point_mask(kSeg, r);
        pref[r][kSeg] = (uint32_t)((total >> (r * kField)) & kFieldMask);
      }
    }
    __syncthreads();

    // the vertices this point owns
    if (m[0]) {
      const uint64_t base = vbases[seg] + pref[0][t];
      const double *p = points + (int64_t)k * pplane + (int64_t)j * prow + i;
      const int idx[3] = {i, j, k};
      const int64_t stride[3] = {1, prow, pplane};
      const double ca[3] = {g.origin[0] + idx[0] * g.spacing[0], g.origin[1] + idx[1] * g.spacing[1],
                            g.origin[2] + idx[2] * g.spacing[2]};
      double ga[3];  // G(a), shared by the point's vertices
      if constexpr (NORMALS) neg_gradient(p, i, j, k, g, prow, pplane, ga);
      unsigned before = 0;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        if (!((m[0] >> d) & 1u)) continue;
        const double va = p[0], vb = p[stride[d]];
        double s = (iso - va) / (vb - va);
        if (va != va || vb != vb) s = va >= iso ? 0.0 : 1.0;
        double x[3] = {ca[0], ca[1], ca[2]};
        const double cb = g.origin[d] + (idx[d] + 1) * g.spacing[d];
        x[d] = ca[d] + s * (cb - ca[d]);
        const uint64_t id = base + before++;
        if (id < g.n_vertices) {
#pragma unroll
          for (int r = 0; r < 3; ++r)
            verts[id * 3 + r] = g.m[4 * r + 0] * x[0] + g.m[4 * r + 1] * x[1] + g.m[4 * r + 2] * x[2] + g.m[4 * r + 3];
          if constexpr (NORMALS) {
            double gb[3], gv[3], w[3];
            neg_gradient(p + stride[d], i + (d == 0), j + (d == 1), k + (d == 2), g, prow, pplane, gb);
#pragma unroll
            for (int r = 0; r < 3; ++r) gv[r] = ga[r] + s * (gb[r] - ga[r]);
#pragma unroll
            for (int r = 0; r < 3; ++r) w[r] = nrm.nm[3 * r + 0] * gv[0] + nrm.nm[3 * r + 1] * gv[1] + nrm.nm[3 * r + 2] * gv[2];
            const double len = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
#pragma unroll
            for (int r = 0; r < 3; ++r) nrm.normals[id * 3 + r] = (float)(len != 0.0 ? w[r] / len : w[r]);  // a NaN len divides
          }
        }
      }
    }

    // the triangles of this point's cell
    if (ntri) {
      const uint64_t tbase = tbases[seg] + ((excl >> (4 * kField)) & kFieldMask);
      uint64_t rb[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) rb[r] = vbases[(((int64_t)k + (r >> 1)) * (ny + 1) + j + (r & 1)) * g.segs_per_row + sx];
      const unsigned char *edges = kTriEdges.v + ccase * 3 * kMcMaxTris;
      for (unsigned s = 0; s < ntri; ++s) {
        const uint64_t tid = tbase + s;
        if (tid >= g.n_triangles) break;
#pragma unroll
        for (int v = 0; v < 3; ++v) {
          const int e = edges[3 * s + v];
          const int *ed = kEdges.v + 4 * e;
          const int d = ed[0], q = t + ed[1], r = ed[2] + 2 * ed[3];
          tris[tid * 3 + v] = (int64_t)(rb[r] + pref[r][q] + (uint64_t)__popc(msk[r][q] & ((1u << d) - 1u)));
        }
      }
    }
  }
}

}  // namespace

int isosurface_max_triangles_per_cell() { return kMcMaxTris; }

size_t isosurface_segment_count(int nx, int ny, int nz) {
  return (size_t)((nx + 1 + kSeg - 1) / kSeg) * (size_t)(ny + 1) * (size_t)(nz + 1);
}

// counts[0 .. n] vertices and counts[n + 1 .. 2n + 1] triangles per segment (the two trailing entries zeros the caller
// keeps there), bases likewise: bases[n] and bases[2n + 1] are the totals
hipError_t launch_isosurface_count(const double *points, const MeshGeom &g, uint32_t *counts, uint64_t *bases, void *scan_temp,
                                   size_t *scan_temp_bytes, hipStream_t stream) {
  const size_t n = isosurface_segment_count(g.nx, g.ny, g.nz);
  if (!scan_temp)
    return rocprim::exclusive_scan(nullptr, *scan_temp_bytes, counts, bases, (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), stream);
  hipLaunchKernelGGL((isosurface_kernel<false>), dim3((unsigned)n), dim3(kSeg), 0, stream, points, g, counts, counts + n + 1,
                     (const uint64_t *)nullptr, (const uint64_t *)nullptr, (double *)nullptr, (int64_t *)nullptr);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  size_t bytes = *scan_temp_bytes;
  e = rocprim::exclusive_scan(scan_temp, bytes, counts, bases, (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), stream);
  if (e != hipSuccess) return e;
  bytes = *scan_temp_bytes;
  return rocprim::exclusive_scan(scan_temp, bytes, counts + n + 1, bases + n + 1, (uint64_t)0, n + 1, rocprim::plus<uint64_t>(),
                                 stream);
}

hipError_t launch_isosurface_write(const double *points, const MeshGeom &g, const uint64_t *bases, double *verts, int64_t *tris,
                                   const MeshNormals *normals, hipStream_t stream) {
  const size_t n = isosurface_segment_count(g.nx, g.ny, g.nz);
  if (normals)
    hipLaunchKernelGGL((isosurface_kernel<true, MeshNormals>), dim3((unsigned)n), dim3(kSeg), 0, stream, points, g, (uint32_t *)nullptr,
                       (uint32_t *)nullptr, bases, bases + n + 1, verts, tris, *normals);
  else
    hipLaunchKernelGGL((isosurface_kernel<true>), dim3((unsigned)n), dim3(kSeg), 0, stream, points, g, (uint32_t *)nullptr,
                       (uint32_t *)nullptr, bases, bases + n + 1, verts, tris);
  return hipGetLastError();
}

}  // namespace dmi
