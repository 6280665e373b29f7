// coloration_kernels.hip -- the MeshColoration pass on the GPU (BASELINE config 5).
//
// Reference (Coloration/MeshColoration.cxx:98-199, CPU only): for every mesh vertex and every view, project the
// vertex (ReconstructionData::TransformWorldToDepthMapPosition, RD.cxx:169-182: RT as a point transform, K as a
// vector transform, divide, std::round; NO test of the sign of z, NO depth test), keep the views whose pixel is
// inside the image, fetch that pixel's RGB (GetColorValue, RD.cxx:92-116: row flip) and store per vertex the mean
// (integer accumulation, MC.cxx:176-180), the median (Helper.h:174-187) and the number of views.
//
// Here: one lane per vertex, colour planes and camera records resident in HBM (dmi_color_context).  The planes are
// repacked at upload to RGBA dwords, top image row first, so a vertex-view pair costs one dword gather.  Kernel 1
// loops over the views (camera records through scalar loads), projects with the reference's expression in fp64 -- the
// two divisions replaced by a checked reciprocal where that provably selects the same pixel (FastQuotient) --
// accumulates count and integer sums, writes the fetched colour of every (view, vertex) pair to a scratch table
// [view][vertex] (uchar4, alpha = valid) and, per lane in LDS, 16-bin histograms of the upper nibbles, from which it
// leaves the upper nibble of each median and the rank inside that bin.  Kernel 2 reads the table once and finds the
// lower nibbles the same way (more than 65 535 views: a bit-by-bit radix selection, eight reads).  Vertices are
// processed in chunks that bound the scratch table.  Everything after the pixel selection is integer arithmetic, so the
// three outputs are bit-identical to the reference's.
//
// Opt-in and not in the reference: the visibility test (dmi_color_set_depth_test, DESIGN.md 8b'): with resident depth planes a
// pair counts only if the vertex's camera z is > 0 and within a tolerance of the view's depth (> 0) at the pixel.
//
// The vertices may also be on the device already (dmi::color_device_vertices, for dmi_color_process_isosurface: the mesh of a
// fusion context): the same chunk body with a chunk being an offset into the caller's device arrays, and the depth
// of the visibility test optionally read from the fusion context's own tables (FusedDepth).
// This file: the device code and its launches (coloration_kernels.h).  The context, the C ABI and the host drivers: dmi_capi_color.hip.
#include "coloration_kernels.h"
#include "mesh_depth_render.h"
#include "rounded_quotient.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace {

using dmi::ColorView, dmi::ViewMargin, dmi::MedianSeed, dmi::FastQuotient, dmi::to_pixel;

template <typename T>
__device__ __forceinline__ T cload(const T *p) {  // wave-uniform address -> scalar load
  return *reinterpret_cast<const T __attribute__((address_space(4))) *>(reinterpret_cast<uintptr_t>(p));
}

// A colour plane in HBM: RGBA texels, top image row first, in TILES of 8 x 4 texels = one 128-byte line (texel (x, y) at
// ((y >> 2) * tiles_x + (x >> 3)) * 32 + (y & 3) * 8 + (x & 7)).  The vertices of a wave are neighbours on the surface, their
// pixels a patch of a few pixels each way: in rows of texels such a patch touches a line per image row, in tiles about half as
// many (profiles/r17t_*).
// (the layout itself: mesh_depth_render.h, shared with the rasteriser that fills depth planes)
using dmi::kTexLogW, dmi::kTexLogH, dmi::kTexTileW, dmi::kTexTileH, dmi::kTexTile, dmi::color_plane_texels, dmi::texel_index;

// [n][H][W] f64 depths in vtk point order -> [n] tiled f64 planes in the colour planes' layout (the same texel index serves
// both gathers of a pair: dmi_color_add_views_with_depth)
__global__ __launch_bounds__(256) void pack_depth_kernel(const double *__restrict__ src, double *__restrict__ dst, int W, int H,
                                                         int64_t n_pixels_total) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= n_pixels_total) return;
  const int64_t npix = (int64_t)W * H;
  const int64_t m = id / npix, r = id % npix;
  const int y = (int)(r / W), x = (int)(r % W);
  dst[m * color_plane_texels(W, H) + texel_index(x, y, (W + kTexTileW - 1) / kTexTileW)] = src[m * npix + (int64_t)(H - 1 - y) * W + x];
}

// [n][H][W][3] in vtk point order (row 0 = bottom, RD.cxx:106-108) -> [n] tiled RGBA planes, top row first
__global__ __launch_bounds__(256) void pack_color_kernel(const uint8_t *__restrict__ rgb, uchar4 *__restrict__ rgba, int W,
                                                         int H, int64_t n_pixels_total) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= n_pixels_total) return;
  const int64_t npix = (int64_t)W * H;
  const int64_t m = id / npix, r = id % npix;
  const int y = (int)(r / W), x = (int)(r % W);
  const uint8_t *c = rgb + (m * npix + (int64_t)(H - 1 - y) * W + x) * 3;
  rgba[m * color_plane_texels(W, H) + texel_index(x, y, (W + kTexTileW - 1) / kTexTileW)] = make_uchar4(c[0], c[1], c[2], 255);
}

// ---- processing order ---------------------------------------------------------------------------------------------
// A vertex's result depends on that vertex alone, so the order in which lanes take vertices is free -- and it decides
// how the colour gathers behave: neighbouring lanes that hold neighbouring vertices read neighbouring texels of every
// view (same cache lines), random ones read one sector each from all over an 8 MB plane.  So a chunk's vertices are
// taken along a Z-order curve of the chunk's bounding box: 30-bit keys, rocPRIM's radix sort of (key, index) pairs,
// and `perm[lane position] = vertex`.  Inputs and outputs stay in the caller's order.  Optional
// (dmi_color_set_vertex_reorder): it pays for vertices in no particular order (1 M x 512 views of 1920x1080: 8.8
// instead of 11.7 ms) and costs for a mesh whose vertices already come in a spatially coherent order, as a
// marching-cubes sweep emits them (8.3 instead of 7.5 ms: the sort, indirect vertex reads, scattered result writes).
__device__ __forceinline__ unsigned long long ordered_bits(double d) {  // monotone map double -> u64 (NaN sorts last)
  const unsigned long long b = (unsigned long long)__double_as_longlong(d);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double from_ordered_bits(unsigned long long u) {
  return __longlong_as_double((long long)((u >> 63) ? (u & 0x7fffffffffffffffull) : ~u));
}

// pmax[a] = max |p_a| over the chunk's vertices as the bits of a double (non-negative doubles order like their bits; a NaN or
// an infinity counts as +inf); zeroed by the caller.  With view_margins_kernel this replaces a host loop over every vertex
// (2 M vertices: 3-4 ms of a 5-6 ms call, round 4) and lets a chunk's kernels start without a trip through the host.
__global__ __launch_bounds__(256) void chunk_magnitude_kernel(const double *__restrict__ points, int64_t nv, unsigned long long *__restrict__ pmax) {
  const unsigned long long kInf = 0x7ff0000000000000ull;
  unsigned long long hi[3] = {0ull, 0ull, 0ull};
  for (int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; id < nv; id += (int64_t)gridDim.x * blockDim.x)
    for (int a = 0; a < 3; ++a) {
      const double m = fabs(points[3 * id + a]);
      unsigned long long u = (unsigned long long)__double_as_longlong(m);
      if (!(m <= 1.7976931348623157e308)) u = kInf;  // NaN, inf
      hi[a] = u > hi[a] ? u : hi[a];
    }
  for (int a = 0; a < 3; ++a)
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long h2 = __shfl_xor(hi[a], off, 64);
      hi[a] = h2 > hi[a] ? h2 : hi[a];
    }
  __shared__ unsigned long long wave_hi[4][3];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
    for (int a = 0; a < 3; ++a) wave_hi[wave][a] = hi[a];
  __syncthreads();
  if (threadIdx.x < 3) {
    const int a = threadIdx.x;
    unsigned long long h = wave_hi[0][a];
    for (int w = 1; w < 4; ++w) h = wave_hi[w][a] > h ? wave_hi[w][a] : h;
    if (h) atomicMax(&pmax[a], h);
  }
}

// ViewMargin of every view for the chunk whose coordinate magnitudes are pmax (the formula of the struct's comment, the host's
// operation order)
__global__ __launch_bounds__(256) void view_margins_kernel(const ColorView *__restrict__ views, int n_views, const unsigned long long *__restrict__ pmax,
                                                           ViewMargin *__restrict__ out) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n_views) return;
  const double pm[4] = {__longlong_as_double((long long)pmax[0]), __longlong_as_double((long long)pmax[1]), __longlong_as_double((long long)pmax[2]), 1.0};
  double e[3];
  for (int r = 0; r < 3; ++r) {
    double sum = 0.0;
    for (int q = 0; q < 4; ++q) sum += views[m].mag[4 * r + q] * pm[q];
    e[r] = sum * 0x1p-47 * (1.0 + 0x1p-20);
  }
  out[m].ex = e[0] + 65537.0 * e[2];
  out[m].ey = e[1] + 65537.0 * e[2];
}

// box[0..2] = min, box[3..5] = max of the finite coordinates, as ordered bits (initialised to ~0 / 0 by the caller)
__global__ __launch_bounds__(256) void bbox_kernel(const double *__restrict__ points, int64_t nv, unsigned long long *__restrict__ box) {
  unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull};
  for (int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; id < nv; id += (int64_t)gridDim.x * blockDim.x)
    for (int a = 0; a < 3; ++a) {
      const double v = points[3 * id + a];
      if (!(fabs(v) <= 1.0e300)) continue;  // NaN / inf: no part in the box
      const unsigned long long u = ordered_bits(v);
      lo[a] = u < lo[a] ? u : lo[a];
      hi[a] = u > hi[a] ? u : hi[a];
    }
  for (int a = 0; a < 3; ++a) {
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long l2 = __shfl_xor(lo[a], off, 64), h2 = __shfl_xor(hi[a], off, 64);
      lo[a] = l2 < lo[a] ? l2 : lo[a];
      hi[a] = h2 > hi[a] ? h2 : hi[a];
    }
  }
  // one pair of atomics per axis and WORKGROUP (they all hit the same six words: per wave, 1024 workgroups' 24 576 atomics took
  // 0.28 ms for a million vertices -- profiles/r17o_coloration_cfg5_kernel_stats.csv)
  __shared__ unsigned long long wave_lo[4][3], wave_hi[4][3];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
    for (int a = 0; a < 3; ++a) wave_lo[wave][a] = lo[a], wave_hi[wave][a] = hi[a];
  __syncthreads();
  if (threadIdx.x < 3) {
    const int a = threadIdx.x;
    unsigned long long l = wave_lo[0][a], h = wave_hi[0][a];
    for (int w = 1; w < 4; ++w) {
      l = wave_lo[w][a] < l ? wave_lo[w][a] : l;
      h = wave_hi[w][a] > h ? wave_hi[w][a] : h;
    }
    atomicMin(&box[a], l);
    atomicMax(&box[3 + a], h);
  }
}

__device__ __forceinline__ uint32_t spread10(uint32_t v) {  // 10 bits -> every third bit
  v &= 0x3ffu;
  v = (v | (v << 16)) & 0x030000ffu;
  v = (v | (v << 8)) & 0x0300f00fu;
  v = (v | (v << 4)) & 0x030c30c3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

__global__ __launch_bounds__(256) void morton_key_kernel(const double *__restrict__ points, int64_t nv,
                                                         const unsigned long long *__restrict__ box, uint32_t *__restrict__ keys,
                                                         uint32_t *__restrict__ index) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= nv) return;
  uint32_t q[3];
  for (int a = 0; a < 3; ++a) {
    const double lo = from_ordered_bits(box[a]), hi = from_ordered_bits(box[3 + a]);
    const double t = (points[3 * id + a] - lo) / (hi - lo) * 1023.0;   // any value will do: only the order of work depends on it
    q[a] = t >= 0.0 && t <= 1023.0 ? (uint32_t)t : (t > 1023.0 ? 1023u : 0u);  // NaN, empty boxes: cell 0
  }
  keys[id] = spread10(q[0]) | (spread10(q[1]) << 1) | (spread10(q[2]) << 2);
  index[id] = (uint32_t)id;
}

constexpr int kHistWords = 8;   // 16 bins of 16 bits, two to a 32-bit word

// The visibility test (dmi_color_set_depth_test): per view a tiled f64 depth plane, and the tolerance.  Passed
// as a trailing parameter pack that is empty with the test off, so those instantiations are the plain pass instruction for
// instruction.
struct DepthTest {
  const double *const *planes;  // [view] -> tiled plane (pack_depth_kernel)
  double tol;
  __device__ __forceinline__ double depth_at(int m, int px, int py, int tiles_x, int) const {
    return cload(&planes[m])[texel_index(px, py, tiles_x)];
  }
};
// The same test with the depth taken from a fusion context's resident tables (dmi_color_process_isosurface): per view
// a plain [H][W] table of T = float or double, top image row first (what dmi_add_views* left: thresholded, flipped, narrowed when
// the store is f32), widened to f64 where it is compared.
template <typename T>
struct FusedDepth {
  const T *const *tables;  // [view] -> that view's table inside its Batch::d_depth
  double tol;
  __device__ __forceinline__ double depth_at(int m, int px, int py, int, int W) const {
    return (double)cload(&tables[m])[(int64_t)py * W + px];
  }
};
template <typename... T>
__device__ __forceinline__ auto depth_test_of(T... t) {
  if constexpr (sizeof...(T) == 0) return DepthTest{nullptr, 0.0};
  else return (t, ...);
}

// HIST: also fill, per lane, 16-bin histograms of the upper nibbles of the three channels in LDS (every lane owns a
// column of counters: no barrier, no conflict) and leave the MedianSeed of the vertex: the first of the two passes of
// the histogram medians costs no read of the scratch table.
// Depth (one DepthTest, one FusedDepth<float / double> or nothing): a pair counts only if, besides the bounds test, the vertex's
// camera z cz (the reference's TransformPoint row 2, every operation rounded) is > 0, the view's depth d at the pixel is > 0 and
// fabs(cz - d) <= tol.  The depth is gathered in the same step as the texel and the test is made where the texel is consumed.
template <bool HIST, bool PIPE, typename... Depth>
__global__ __launch_bounds__(256) void project_color_kernel(const double *__restrict__ points, int64_t nv,
                                                            const uint32_t *__restrict__ perm,
                                                            const ColorView *__restrict__ views, int n, int W, int H,
                                                            uchar4 *__restrict__ scratch, uint8_t *__restrict__ mean,
                                                            int32_t *__restrict__ count, MedianSeed *__restrict__ seeds,
                                                            const ViewMargin *__restrict__ margins, Depth... depth) {
  constexpr bool DEPTH = sizeof...(Depth) > 0;
  const auto dt = depth_test_of(depth...);
  __shared__ uint32_t hist[HIST ? 3 * kHistWords * 256 : 1];  // [channel][word][lane]: 24 KB
  const int lane = threadIdx.x;
  const int tiles_x = (W + kTexTileW - 1) / kTexTileW;
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // position along the Z-order curve
  if (id >= nv) return;
  const int64_t vtx = perm ? (int64_t)perm[id] : id;                  // the vertex this lane colours
  const double x = points[3 * vtx], y = points[3 * vtx + 1], z = points[3 * vtx + 2];
  int cnt = 0, s0 = 0, s1 = 0, s2 = 0;
  auto bump = [&](int table, int b) {
    __hip_atomic_fetch_add(&hist[(table * kHistWords + (b & 7)) * 256 + lane], 1u << (16 * (b >> 3)), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
  };
  if constexpr (HIST)
    for (int q = 0; q < 3 * kHistWords; ++q) hist[q * 256 + lane] = 0;
  // what happens to a view's texel once it has arrived: count, integer sums, histogram, the scratch table's entry
  auto consume = [&](int mq, uchar4 c, bool ok, double d, double cz) {
    if constexpr (DEPTH) ok = ok && d > 0.0 && __builtin_fabs(cz - d) <= dt.tol;  // (cz > 0 was part of ok; NaN: false)
    uchar4 out = make_uchar4(0, 0, 0, 0);
    if (ok) {
      out = make_uchar4(c.x, c.y, c.z, 1);
      cnt += 1;
      s0 += c.x;  // std::accumulate(..., 0): integer running sums (MC.cxx:176-178)
      s1 += c.y;
      s2 += c.z;
      if constexpr (HIST) {
        bump(0, c.x >> 4);
        bump(1, c.y >> 4);
        bump(2, c.z >> 4);
      }
    }
    scratch[(int64_t)mq * nv + id] = out;
  };
  // the view's pixel for this vertex and the request for its texel
  auto project = [&](int m, uchar4 &c, bool &ok, double &d, double &cz) __attribute__((always_inline)) {
    const ColorView *v = views + m;  // wave-uniform
    // The pixel only has to be the reference's pixel: the homogeneous coordinates come from the rows of K3*[R|T] (nine
    // FMAs instead of the reference's 33 operations), and the pixel they select is taken when it provably is the
    // reference's (round_to_pixel_near with this view's margin for this chunk of vertices); whatever is not decided
    // that way goes through the reference's own expression below.
    const double ax = __builtin_fma(cload(&v->p[0]), x, __builtin_fma(cload(&v->p[1]), y, __builtin_fma(cload(&v->p[2]), z, cload(&v->p[3]))));
    const double ay = __builtin_fma(cload(&v->p[4]), x, __builtin_fma(cload(&v->p[5]), y, __builtin_fma(cload(&v->p[6]), z, cload(&v->p[7]))));
    const double az = __builtin_fma(cload(&v->p[8]), x, __builtin_fma(cload(&v->p[9]), y, __builtin_fma(cload(&v->p[10]), z, cload(&v->p[11]))));
    int px = 0, py = 0;
    const FastQuotient by_az(az);
    bool have_pixel = by_az.round_to_pixel_near(ax, cload(&margins[m].ex), px) && by_az.round_to_pixel_near(ay, cload(&margins[m].ey), py);
    bool is_pixel = have_pixel;
    if (!have_pixel) {
      // vtkTransform::TransformPoint with MatrixTR (RD.cxx:173): M[i][0]*x + M[i][1]*y + M[i][2]*z + M[i][3], left to right
      const double cx = ((cload(&v->rt[0]) * x + cload(&v->rt[1]) * y) + cload(&v->rt[2]) * z) + cload(&v->rt[3]);
      const double cy = ((cload(&v->rt[4]) * x + cload(&v->rt[5]) * y) + cload(&v->rt[6]) * z) + cload(&v->rt[7]);
      const double cz = ((cload(&v->rt[8]) * x + cload(&v->rt[9]) * y) + cload(&v->rt[10]) * z) + cload(&v->rt[11]);
      // vtkTransform::TransformVector with Matrix4K (RD.cxx:175): no translation
      const double dx = (cload(&v->k[0]) * cx + cload(&v->k[1]) * cy) + cload(&v->k[2]) * cz;
      const double dy = (cload(&v->k[3]) * cx + cload(&v->k[4]) * cy) + cload(&v->k[5]) * cz;
      const double dz = (cload(&v->k[6]) * cx + cload(&v->k[7]) * cy) + cload(&v->k[8]) * cz;
      const FastQuotient by_dz(dz);
      is_pixel = by_dz.round_to_pixel(dx, dz, px) && by_dz.round_to_pixel(dy, dz, py);   // RD.cxx:177-181
    }
    ok = is_pixel && px >= 0 && py >= 0 && px < W && py < H;                             // MC.cxx:158-163
    if constexpr (DEPTH) {
      // the camera z of TransformPoint (RD.cxx:173), not the shortcut's az
      cz = ((cload(&v->rt[8]) * x + cload(&v->rt[9]) * y) + cload(&v->rt[10]) * z) + cload(&v->rt[11]);
      ok = ok && cz > 0.0;
      d = 0.0;
    }
    c = make_uchar4(0, 0, 0, 0);
    if (ok) {
      c = cload(&v->color)[texel_index(px, py, tiles_x)];     // RD.cxx:106-108 (row flip and tiling done at upload)
      if constexpr (DEPTH) d = dt.depth_at(m, px, py, tiles_x, W);
    }
  };
  if constexpr (PIPE) {
    // Vertices in the caller's order (a mesh: neighbours in neighbouring lanes): the loop software-pipelined.  View m's texel is
    // requested in its own step and consumed K steps later, behind the projections of the K views in between -- consumed at
    // once, a gather that misses every cache stalled the wave once per view (2.9 us per view and wave at 512 views,
    // profiles/r17o_*).  Integer sums, histogram counts, distinct table entries: the order of consumption changes no result
    // bit.  K slots, the loop unrolled by K: a slot is a register the load writes and nothing copies.
    // (mesh order at cfg 5's scale: 4.96 ms plain, 4.51 with K = 2, 4.37 with 4, 4.2 with 8, 4.3 with 16, 4.4 with 32; with
    // scattered vertices -- random order 7.7 -> 9.2 ms at K = 2 -- the gathers are bound by the lines they drag in and more of
    // them in flight evict each other: those keep the plain loop; the device-reordered pass lost 5 % at K = 2 on row-major
    // planes and gains 4 % at K = 8 on tiled ones; profiles/r17q_*, r17s_*, r17t_*)
#ifndef DMI_COLOR_AHEAD
#define DMI_COLOR_AHEAD 8
#endif
    constexpr int K = DMI_COLOR_AHEAD;  // views between a texel's request and its use
    uchar4 slot_c[K];
    bool slot_ok[K];
    double slot_d[K] = {}, slot_cz[K] = {};  // (the depth test's: the gathered depth and the camera z; unused without it)
    int m = 0;
    if (n >= K) {
#pragma unroll
      for (int q = 0; q < K; ++q) project(q, slot_c[q], slot_ok[q], slot_d[q], slot_cz[q]);
      for (m = K; m + K <= n; m += K) {
#pragma unroll
        for (int q = 0; q < K; ++q) {
          uchar4 c;
          bool ok;
          double d = 0.0, cz = 0.0;
          project(m + q, c, ok, d, cz);
          consume(m + q - K, slot_c[q], slot_ok[q], slot_d[q], slot_cz[q]);  // the view this slot held
          slot_c[q] = c;
          slot_ok[q] = ok;
          slot_d[q] = d;
          slot_cz[q] = cz;
        }
      }
#pragma unroll
      for (int q = 0; q < K; ++q) consume(m - K + q, slot_c[q], slot_ok[q], slot_d[q], slot_cz[q]);
    }
    for (; m < n; ++m) {  // the views a whole round of K does not cover
      uchar4 c;
      bool ok;
      double d = 0.0, cz = 0.0;
      project(m, c, ok, d, cz);
      consume(m, c, ok, d, cz);
    }
  } else {
    for (int m = 0; m < n; ++m) {
      uchar4 c;
      bool ok;
      double d = 0.0, cz = 0.0;
      project(m, c, ok, d, cz);
      consume(m, c, ok, d, cz);
    }
  }
  count[vtx] = cnt;  // MC.cxx:186 (0 when no view sees the vertex, MC.cxx:130)
  // sum / nbVal in double, then static_cast<unsigned char> (MC.cxx:179-180): exactly the integer quotient
  mean[3 * vtx + 0] = cnt ? (uint8_t)(s0 / cnt) : 0;
  mean[3 * vtx + 1] = cnt ? (uint8_t)(s1 / cnt) : 0;
  mean[3 * vtx + 2] = cnt ? (uint8_t)(s2 / cnt) : 0;
  if constexpr (HIST) {
    // rank (0-based) of the upper and of the lower middle element (Helper.h:174-187; the same element for an odd count)
    const int want[2] = {cnt / 2, (cnt & 1) == 0 ? cnt / 2 - 1 : cnt / 2};
    uint32_t hi = 0, rest[6] = {0, 0, 0, 0, 0, 0};
    if (cnt > 0) {
      for (int c = 0; c < 3; ++c)
        for (int t = 0; t < 2; ++t) {
          int k = want[t], b = 0;
          for (; b < 15; ++b) {
            const int here = (int)((hist[(c * kHistWords + (b & 7)) * 256 + lane] >> (16 * (b >> 3))) & 0xffffu);
            if (k < here) break;
            k -= here;
          }
          hi |= (uint32_t)b << (4 * (2 * c + t));
          rest[2 * c + t] = (uint32_t)k;
        }
    }
    seeds[id] = MedianSeed{hi, rest[0] | (rest[1] << 16), rest[2] | (rest[3] << 16), rest[4] | (rest[5] << 16)};
  }
}

// Medians of the valid entries of the three channels (Helper.h:174-187: sorted[cnt/2], or the mean of sorted[cnt/2]
// and sorted[cnt/2 - 1] for an even count).  Radix selection from the top bit down; one pass over the vertex's column
// of the scratch table per bit serves all six (channel, middle element) selections.
__global__ __launch_bounds__(256) void median_kernel(const uchar4 *__restrict__ scratch, int64_t nv, int n,
                                                     const uint32_t *__restrict__ perm, const int32_t *__restrict__ count,
                                                     uint8_t *__restrict__ median) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // scratch column = position along the curve
  if (id >= nv) return;
  const int64_t vtx = perm ? (int64_t)perm[id] : id;
  const int cnt = count[vtx];
  int prefix[3][2] = {{0, 0}, {0, 0}, {0, 0}};
  int k[3][2];
  for (int c = 0; c < 3; ++c) {
    k[c][0] = cnt / 2;                                // 0-based rank of the upper middle element
    k[c][1] = (cnt & 1) == 0 ? cnt / 2 - 1 : cnt / 2;  // the lower one (the same element for an odd count)
  }
  if (cnt > 0) {
    for (int bit = 7; bit >= 0; --bit) {
      int zeros[3][2] = {{0, 0}, {0, 0}, {0, 0}};  // valid entries matching the prefix above `bit` with a 0 at `bit`
      for (int m = 0; m < n; ++m) {
        const uchar4 e = scratch[(int64_t)m * nv + id];
        const int val[3] = {e.x, e.y, e.z};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int high = val[c] >> (bit + 1), is_zero = ((val[c] >> bit) & 1) == 0;
#pragma unroll
          for (int t = 0; t < 2; ++t) zeros[c][t] += (e.w != 0 && high == prefix[c][t] && is_zero) ? 1 : 0;
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          if (k[c][t] < zeros[c][t]) {
            prefix[c][t] = prefix[c][t] << 1;
          } else {
            k[c][t] -= zeros[c][t];
            prefix[c][t] = (prefix[c][t] << 1) | 1;
          }
        }
    }
  }
  // (a + b) / 2 in double, then static_cast<unsigned char> (MC.cxx:185): the integer (a + b) >> 1; a == b for odd counts
  for (int c = 0; c < 3; ++c) median[3 * vtx + c] = cnt > 0 ? (uint8_t)((prefix[c][0] + prefix[c][1]) >> 1) : 0;
}

// The same medians from nibble histograms: the projection pass has already found, per channel and middle rank, the
// upper nibble of the median and the rank left inside that nibble's bin (MedianSeed); this pass reads the scratch column
// ONCE.  Per channel ONE 16-bin histogram of the lower nibbles of the entries in the upper middle element's bin, in LDS --
// every lane owns a column of counters, two 16-bit counters to a word (so at most 65 535 views; more take the bit-by-bit
// kernel above, eight reads of the column).  The lower middle element (even counts) is in the same bin, at the rank
// before -- or, when the two middle elements straddle a bin boundary, it is the LARGEST entry of its own bin and the upper
// one the SMALLEST of its: two running extremes per channel, no second table.  24 KB of LDS per 256 lanes instead of 48.
__global__ __launch_bounds__(256) void median_low_nibble_kernel(const uchar4 *__restrict__ scratch, int64_t nv, int n,
                                                                const uint32_t *__restrict__ perm, const int32_t *__restrict__ count,
                                                                const MedianSeed *__restrict__ seeds, uint8_t *__restrict__ median) {
  __shared__ uint32_t hist[3 * kHistWords * 256];  // [channel][word][lane]
  const int lane = threadIdx.x;
  const int64_t id = (int64_t)blockIdx.x * 256 + lane;  // scratch column = position along the curve
  if (id >= nv) return;                                 // (no barrier below)
  const int64_t vtx = perm ? (int64_t)perm[id] : id;
  const int cnt = count[vtx];
  const MedianSeed seed = seeds[id];
  // [2c] = upper middle element of channel c, [2c + 1] = lower one
  int hi[6], rest[6] = {(int)(seed.rest01 & 0xffffu), (int)(seed.rest01 >> 16), (int)(seed.rest23 & 0xffffu),
                        (int)(seed.rest23 >> 16), (int)(seed.rest45 & 0xffffu), (int)(seed.rest45 >> 16)};
  for (int q = 0; q < 6; ++q) hi[q] = (int)((seed.hi >> (4 * q)) & 15u);
  int smallest[3] = {15, 15, 15};  // of the entries in the upper element's bin
  int largest[3] = {0, 0, 0};      // of the entries in the lower element's bin
  for (int q = 0; q < 3 * kHistWords; ++q) hist[q * 256 + lane] = 0;
  if (cnt > 0) {
    auto take = [&](uchar4 e) {
      const int val[3] = {e.x, e.y, e.z};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int up = val[c] >> 4, low = val[c] & 15;
        const bool in_upper = e.w != 0 && up == hi[2 * c], in_lower = e.w != 0 && up == hi[2 * c + 1];
        if (in_upper) {
          __hip_atomic_fetch_add(&hist[(c * kHistWords + (low & 7)) * 256 + lane], 1u << (16 * (low >> 3)), __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WORKGROUP);
          smallest[c] = min(smallest[c], low);
        }
        if (in_lower) largest[c] = max(largest[c], low);
      }
    };
    // eight table entries requested before the first is looked at: the kernel is this table's read and nothing else, and one
    // entry per trip to HBM left it at 4 TB/s (profiles/r17o_*: 0.5 ms per 2 GB)
    constexpr int kBatch = 8;
    int m = 0;
    for (; m + kBatch <= n; m += kBatch) {
      uchar4 e[kBatch];
#pragma unroll
      for (int q = 0; q < kBatch; ++q) e[q] = scratch[(int64_t)(m + q) * nv + id];
#pragma unroll
      for (int q = 0; q < kBatch; ++q) take(e[q]);
    }
    for (; m < n; ++m) take(scratch[(int64_t)m * nv + id]);
  }
  uint8_t out[3] = {0, 0, 0};
  if (cnt > 0) {
    for (int c = 0; c < 3; ++c) {
      auto at_rank = [&](int k) {
        int b = 0;
        for (; b < 15; ++b) {
          const int here = (int)((hist[(c * kHistWords + (b & 7)) * 256 + lane] >> (16 * (b >> 3))) & 0xffffu);
          if (k < here) break;
          k -= here;
        }
        return b;
      };
      int upper_low, lower_low;
      if (hi[2 * c] == hi[2 * c + 1]) {  // both middle elements in one bin (always so for an odd count: the same element)
        upper_low = at_rank(rest[2 * c]);
        lower_low = rest[2 * c + 1] == rest[2 * c] ? upper_low : at_rank(rest[2 * c + 1]);
      } else {                            // they straddle a bin boundary: first of its bin, last of the bin before
        upper_low = smallest[c];
        lower_low = largest[c];
      }
      // (a + b) / 2 in double, then static_cast<unsigned char> (MC.cxx:185): the integer (a + b) >> 1
      out[c] = (uint8_t)((((hi[2 * c] << 4) | upper_low) + ((hi[2 * c + 1] << 4) | lower_low)) >> 1);
    }
  }
  for (int c = 0; c < 3; ++c) median[3 * vtx + c] = out[c];
}

// the coherence sample (coloration_kernels.h) of vertices that are on the device
__global__ __launch_bounds__(256) void coherence_sample_kernel(const double *__restrict__ points, int64_t n, int64_t samples,
                                                               double *__restrict__ rows) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= samples) return;
  const int64_t i = dmi::coherence_row(t, n, samples);
  const int64_t from[3] = {i, i + 1, (i + n / 2) % n};
  for (int r = 0; r < 3; ++r)
    for (int q = 0; q < 3; ++q) rows[9 * t + 3 * r + q] = points[3 * from[r] + q];
}

inline dim3 blocks_of(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

// ---- the launches (coloration_kernels.h) ---------------------------------------------------------------------------
namespace dmi {

hipError_t launch_coherence_sample(const double *points, int64_t n, int64_t samples, double *rows, hipStream_t stream) {
  hipLaunchKernelGGL(coherence_sample_kernel, blocks_of(samples), dim3(256), 0, stream, points, n, samples, rows);
  return hipGetLastError();
}
hipError_t launch_pack_color(const uint8_t *rgb, uchar4 *rgba, int W, int H, int64_t n_pixels_total, hipStream_t stream) {
  hipLaunchKernelGGL(pack_color_kernel, blocks_of(n_pixels_total), dim3(256), 0, stream, rgb, rgba, W, H, n_pixels_total);
  return hipGetLastError();
}
hipError_t launch_pack_depth(const double *src, double *dst, int W, int H, int64_t n_pixels_total, hipStream_t stream) {
  hipLaunchKernelGGL(pack_depth_kernel, blocks_of(n_pixels_total), dim3(256), 0, stream, src, dst, W, H, n_pixels_total);
  return hipGetLastError();
}

// (a coordinate that is not finite makes the margins infinite: every pair then takes the reference's expression)
hipError_t launch_chunk_margins(const double *points, int64_t nv, const ColorView *views, int n_views, unsigned long long *pmax,
                                ViewMargin *margins, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(pmax, 0, 4 * sizeof(unsigned long long), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(chunk_magnitude_kernel, dim3(std::min<unsigned>(blocks_of(nv).x, 512u)), dim3(256), 0, stream, points, nv, pmax);
  hipLaunchKernelGGL(view_margins_kernel, blocks_of(n_views), dim3(256), 0, stream, views, n_views, pmax, margins);
  return hipGetLastError();
}

// rocPRIM tells how much temporary storage a sort of `capacity` pairs needs when called without any
hipError_t zorder_sort_temp_bytes(size_t capacity, size_t *bytes, hipStream_t stream) {
  uint32_t *const none = nullptr;
  return rocprim::radix_sort_pairs(nullptr, *bytes, none, none, none, none, capacity, 0, 30, stream);
}

hipError_t launch_zorder_sort(const double *points, int64_t nv, const ZOrderBuffers &o, hipStream_t stream) {
  static const unsigned long long kEmptyBox[6] = {~0ull, ~0ull, ~0ull, 0ull, 0ull, 0ull};
  hipError_t e = hipMemcpyAsync(o.box, kEmptyBox, sizeof(kEmptyBox), hipMemcpyHostToDevice, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(bbox_kernel, dim3(std::min<unsigned>(blocks_of(nv).x, 256u)), dim3(256), 0, stream, points, nv, o.box);
  hipLaunchKernelGGL(morton_key_kernel, blocks_of(nv), dim3(256), 0, stream, points, nv, o.box, o.keys, o.index);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  size_t temp = o.temp_bytes;
  return rocprim::radix_sort_pairs(o.temp, temp, o.keys, o.keys_sorted, o.index, o.perm, (size_t)nv, 0, 30, stream);
}

hipError_t launch_project_color(const ProjectArgs &a, hipStream_t stream) {
  auto project = [&](auto... policy) {
    if (a.histogram_medians && !a.perm && !a.coherent)
      hipLaunchKernelGGL((project_color_kernel<true, false, decltype(policy)...>), blocks_of(a.nv), dim3(256), a.extra_lds, stream, a.points, a.nv,
                         a.perm, a.views, a.n_views, a.W, a.H, a.scratch, a.mean, a.count, a.seeds, a.margins, policy...);
    else if (a.histogram_medians)
      hipLaunchKernelGGL((project_color_kernel<true, true, decltype(policy)...>), blocks_of(a.nv), dim3(256), a.extra_lds, stream, a.points, a.nv,
                         a.perm, a.views, a.n_views, a.W, a.H, a.scratch, a.mean, a.count, a.seeds, a.margins, policy...);
    else
      hipLaunchKernelGGL((project_color_kernel<false, false, decltype(policy)...>), blocks_of(a.nv), dim3(256), 0, stream, a.points, a.nv,
                         a.perm, a.views, a.n_views, a.W, a.H, a.scratch, a.mean, a.count, a.seeds, a.margins, policy...);
  };
  switch (a.depth) {
    case ColorDepth::fused_f64: project(FusedDepth<double>{static_cast<const double *const *>(a.depth_tables), a.tol}); break;
    case ColorDepth::fused_f32: project(FusedDepth<float>{static_cast<const float *const *>(a.depth_tables), a.tol}); break;
    case ColorDepth::planes: project(DepthTest{static_cast<const double *const *>(a.depth_tables), a.tol}); break;
    case ColorDepth::none: project(); break;
  }
  return hipGetLastError();
}

hipError_t launch_color_median(const uchar4 *scratch, int64_t nv, int n_views, const uint32_t *perm, const int32_t *count,
                               const MedianSeed *seeds, uint8_t *median, hipStream_t stream) {
  if (seeds)
    hipLaunchKernelGGL(median_low_nibble_kernel, blocks_of(nv), dim3(256), 0, stream, scratch, nv, n_views, perm, count, seeds, median);
  else
    hipLaunchKernelGGL(median_kernel, blocks_of(nv), dim3(256), 0, stream, scratch, nv, n_views, perm, count, median);
  return hipGetLastError();
}

}  // namespace dmi
