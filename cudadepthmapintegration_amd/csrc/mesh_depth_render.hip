// mesh_depth_render.hip -- a software z-buffer rasteriser: a triangle mesh rendered into the depth planes of the views resident in
// a colour context (dmi_color_render_depths, dmi_color_render_isosurface_depths; DESIGN.md 8b'').  What the visibility test of the
// colouring (project_color_kernel's DepthTest) then compares against is the surface being coloured, not the noisy depth maps it
// was fused from.  Not in the reference, whose colouring has no visibility test at all.
//
// Definition (every operation f64, rounded, nothing contracted; met bit for bit by tests/mesh_depth_np.py):
//   projection  (cx, cy, cz) = TransformPoint by [R|T], left to right; (dx, dy, dz) = K3 (cx, cy, cz), no translation -- the exact
//               branch of project_color_kernel --; u = dx / dz, v = dy / dz, correctly rounded.  A triangle is skipped for a view
//               unless all three vertices have cz > 0, dz > 0 and finite u, v: NO NEAR-PLANE CLIPPING, a triangle that crosses the
//               camera plane does not occlude.
//   pixels      centres at integer coordinates; x in [max(0, ceil(min u)), min(W - 1, floor(max u))], likewise y.
//   coverage    e0 = (u2-u1)*(y-v1) - (v2-v1)*(x-u1), e1 = (u0-u2)*(y-v2) - (v0-v2)*(x-u2), e2 = (u1-u0)*(y-v0) - (v1-v0)*(x-u0);
//               covered iff all three >= 0 or all three <= 0, and s = (e0 + e1) + e2 != 0.  Both windings, inclusive edges.
//   depth       q = (e0/cz0 + e1/cz1) + e2/cz2, d = s / q, kept iff finite and > 0: the perspective-correct camera z (exact for a K
//               whose last row is 0 0 1, all that SetMatrixK produces; for a general K it interpolates 1/cz linearly in a plane
//               where 1/dz is what is linear -- an approximation of the same order as the triangle's depth range over its depth).
//   plane       the minimum of d over the covering triangles, +inf where nothing covers: order-independent, the same bits whatever
//               order the triangles or the atomics arrive in.
//
// Kernels: a fill with the bits of +inf; the SMALL pass, one lane per triangle, a loop over a group of views (camera records
// through scalar loads), the lane walking the clipped range itself when it holds at most kRenderLaneCap pixels; the LARGE pass,
// one wave per (triangle, view) pair the small pass queued, its lanes striding the range in 8 x 8 blocks aligned to the planes'
// tiles.  A covered pixel reads the plane first and issues a 64-bit unsigned atomic minimum on the bits of d only when d is
// smaller (positive finite doubles order as their bit patterns; a stale read can only be LARGER than the present value, so it
// never skips a minimum that was needed).
#include "mesh_depth_render.h"

#include <algorithm>

namespace dmi {
namespace {

template <typename T>
__device__ __forceinline__ T cload(const T *p) {  // wave-uniform address -> scalar load
  return *reinterpret_cast<const T __attribute__((address_space(4))) *>(reinterpret_cast<uintptr_t>(p));
}

constexpr unsigned long long kInfBits = 0x7ff0000000000000ull;

// a view's camera in registers (scalar ones: every lane of the wave has the same view)
struct Camera {
  double r0, r1, r2, r3, r4, r5, r6, r7, r8, r9, r10, r11;
  double k0, k1, k2, k3, k4, k5, k6, k7, k8;
};
__device__ __forceinline__ Camera load_camera(const RenderView *v) {
  Camera c;
  c.r0 = cload(&v->rt[0]); c.r1 = cload(&v->rt[1]); c.r2 = cload(&v->rt[2]); c.r3 = cload(&v->rt[3]);
  c.r4 = cload(&v->rt[4]); c.r5 = cload(&v->rt[5]); c.r6 = cload(&v->rt[6]); c.r7 = cload(&v->rt[7]);
  c.r8 = cload(&v->rt[8]); c.r9 = cload(&v->rt[9]); c.r10 = cload(&v->rt[10]); c.r11 = cload(&v->rt[11]);
  c.k0 = cload(&v->k[0]); c.k1 = cload(&v->k[1]); c.k2 = cload(&v->k[2]);
  c.k3 = cload(&v->k[3]); c.k4 = cload(&v->k[4]); c.k5 = cload(&v->k[5]);
  c.k6 = cload(&v->k[6]); c.k7 = cload(&v->k[7]); c.k8 = cload(&v->k[8]);
  return c;
}

// (u, v, cz) of one vertex; false unless cz > 0, dz > 0 and u, v finite (a NaN fails every comparison)
__device__ __forceinline__ bool project_vertex(const Camera &c, double x, double y, double z, double &u, double &v, double &cz) {
  const double cx = ((c.r0 * x + c.r1 * y) + c.r2 * z) + c.r3;
  const double cy = ((c.r4 * x + c.r5 * y) + c.r6 * z) + c.r7;
  cz = ((c.r8 * x + c.r9 * y) + c.r10 * z) + c.r11;
  const double dx = (c.k0 * cx + c.k1 * cy) + c.k2 * cz;
  const double dy = (c.k3 * cx + c.k4 * cy) + c.k5 * cz;
  const double dz = (c.k6 * cx + c.k7 * cy) + c.k8 * cz;
  u = dx / dz;
  v = dy / dz;
  return cz > 0.0 && dz > 0.0 && __builtin_fabs(u) <= 1.7976931348623157e308 && __builtin_fabs(v) <= 1.7976931348623157e308;
}

// A projected triangle, its edge vectors taken once (each a single rounded subtraction: the same bits as in the definition's
// expressions), and its clipped pixel range.
struct Screen {
  double u0, v0, u1, v1, u2, v2, cz0, cz1, cz2;
  double a0, b0, a1, b1, a2, b2;  // (u2-u1, v2-v1), (u0-u2, v0-v2), (u1-u0, v1-v0)
  int x0, x1, y0, y1;
};
// false: skipped for this view, or no pixel centre in the clipped range
__device__ __forceinline__ bool setup(const Camera &c, double px0, double py0, double pz0, double px1, double py1, double pz1, double px2,
                                      double py2, double pz2, int W, int H, Screen &s) {
  bool ok = project_vertex(c, px0, py0, pz0, s.u0, s.v0, s.cz0);
  ok = project_vertex(c, px1, py1, pz1, s.u1, s.v1, s.cz1) && ok;
  ok = project_vertex(c, px2, py2, pz2, s.u2, s.v2, s.cz2) && ok;
  if (!ok) return false;
  const double fx0 = __builtin_fmax(0.0, __builtin_ceil(__builtin_fmin(__builtin_fmin(s.u0, s.u1), s.u2)));
  const double fx1 = __builtin_fmin((double)(W - 1), __builtin_floor(__builtin_fmax(__builtin_fmax(s.u0, s.u1), s.u2)));
  const double fy0 = __builtin_fmax(0.0, __builtin_ceil(__builtin_fmin(__builtin_fmin(s.v0, s.v1), s.v2)));
  const double fy1 = __builtin_fmin((double)(H - 1), __builtin_floor(__builtin_fmax(__builtin_fmax(s.v0, s.v1), s.v2)));
  if (!(fx0 <= fx1 && fy0 <= fy1)) return false;  // (both ends are then inside [0, W - 1] x [0, H - 1])
  s.x0 = (int)fx0;
  s.x1 = (int)fx1;
  s.y0 = (int)fy0;
  s.y1 = (int)fy1;
  s.a0 = s.u2 - s.u1; s.b0 = s.v2 - s.v1;
  s.a1 = s.u0 - s.u2; s.b1 = s.v0 - s.v2;
  s.a2 = s.u1 - s.u0; s.b2 = s.v1 - s.v0;
  return true;
}

// pixel (x, y), inside the image: coverage, depth, minimum
__device__ __forceinline__ void shade(const Screen &s, int x, int y, double *__restrict__ plane, int tiles_x) {
  const double fx = (double)x, fy = (double)y;
  const double e0 = s.a0 * (fy - s.v1) - s.b0 * (fx - s.u1);
  const double e1 = s.a1 * (fy - s.v2) - s.b1 * (fx - s.u2);
  const double e2 = s.a2 * (fy - s.v0) - s.b2 * (fx - s.u0);
  const bool covered = (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) || (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0);
  const double sum = (e0 + e1) + e2;
  if (!covered || sum == 0.0) return;
  const double q = (e0 / s.cz0 + e1 / s.cz1) + e2 / s.cz2;
  const double d = sum / q;
  if (!(d > 0.0 && d <= 1.7976931348623157e308)) return;  // NaN, <= 0, infinite
  const unsigned long long bits = (unsigned long long)__double_as_longlong(d);
  unsigned long long *p = reinterpret_cast<unsigned long long *>(plane) + texel_index(x, y, tiles_x);
  if (bits < *p) __hip_atomic_fetch_min(p, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void render_check_ids_kernel(const int64_t *__restrict__ triangles, int64_t n_ids, int64_t n_points,
                                                               uint32_t *__restrict__ flag) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= n_ids) return;
  const int64_t v = triangles[id];
  if (v < 0 || v >= n_points) atomicMax(flag, 1u);
}

__global__ __launch_bounds__(256) void render_init_kernel(unsigned long long *__restrict__ planes, int64_t n_texels) {
  for (int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; id < n_texels; id += (int64_t)gridDim.x * blockDim.x) planes[id] = kInfBits;
}

// SMALL pass: one lane per triangle, the views [m0, m0 + n) of the call
__global__ __launch_bounds__(256) void render_small_kernel(const double *__restrict__ points, const int64_t *__restrict__ triangles, int64_t n_triangles,
                                                           const RenderView *__restrict__ views, int m0, int n, int W, int H,
                                                           double *__restrict__ planes, int64_t plane_texels, RenderPair *__restrict__ queue,
                                                           uint32_t capacity, uint32_t *__restrict__ counter) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_triangles) return;
  const int64_t i0 = triangles[3 * t], i1 = triangles[3 * t + 1], i2 = triangles[3 * t + 2];
  const double px0 = points[3 * i0], py0 = points[3 * i0 + 1], pz0 = points[3 * i0 + 2];
  const double px1 = points[3 * i1], py1 = points[3 * i1 + 1], pz1 = points[3 * i1 + 2];
  const double px2 = points[3 * i2], py2 = points[3 * i2 + 1], pz2 = points[3 * i2 + 2];
  const int tiles_x = (W + kTexTileW - 1) / kTexTileW;
  for (int m = m0; m < m0 + n; ++m) {
    const Camera cam = load_camera(views + m);
    Screen s;
    if (!setup(cam, px0, py0, pz0, px1, py1, pz1, px2, py2, pz2, W, H, s)) continue;
    const int64_t pixels = (int64_t)(s.x1 - s.x0 + 1) * (s.y1 - s.y0 + 1);
    if (pixels <= kRenderLaneCap) {
      double *plane = planes + (int64_t)m * plane_texels;
      for (int y = s.y0; y <= s.y1; ++y)
        for (int x = s.x0; x <= s.x1; ++x) shade(s, x, y, plane, tiles_x);
    } else {
      const uint32_t slot = atomicAdd(counter, 1u);  // counted even when dropped: the size the queue should have had
      if (slot < capacity) queue[slot] = RenderPair{t, m, 0};
    }
  }
}

// LARGE pass: one wave per queued pair, 8 x 8 pixel blocks (two tiles of the plane, one above the other) round robin
__global__ __launch_bounds__(256) void render_large_kernel(const double *__restrict__ points, const int64_t *__restrict__ triangles,
                                                           const RenderView *__restrict__ views, int W, int H, double *__restrict__ planes,
                                                           int64_t plane_texels, const RenderPair *__restrict__ queue, uint32_t capacity,
                                                           const uint32_t *__restrict__ counter) {
  const uint32_t wanted = cload(counter);
  const uint32_t n_pairs = wanted < capacity ? wanted : capacity;
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)), n_waves = (uint32_t)(gridDim.x * (blockDim.x >> 6));
  const int tiles_x = (W + kTexTileW - 1) / kTexTileW;
  for (uint32_t pair = wave; pair < n_pairs; pair += n_waves) {
    const int64_t t = queue[pair].triangle;
    const int m = queue[pair].view;
    const int64_t i0 = triangles[3 * t], i1 = triangles[3 * t + 1], i2 = triangles[3 * t + 2];
    const Camera cam = load_camera(views + m);
    Screen s;
    // (the small pass queued the pair because this very setup succeeded there)
    if (!setup(cam, points[3 * i0], points[3 * i0 + 1], points[3 * i0 + 2], points[3 * i1], points[3 * i1 + 1], points[3 * i1 + 2],
               points[3 * i2], points[3 * i2 + 1], points[3 * i2 + 2], W, H, s))
      continue;
    double *plane = planes + (int64_t)m * plane_texels;
    const int bx0 = s.x0 >> 3, bx1 = s.x1 >> 3, by0 = s.y0 >> 3, by1 = s.y1 >> 3;
    for (int by = by0; by <= by1; ++by)
      for (int bx = bx0; bx <= bx1; ++bx) {
        const int x = (bx << 3) + (lane & 7), y = (by << 3) + (lane >> 3);
        if (x >= s.x0 && x <= s.x1 && y >= s.y0 && y <= s.y1) shade(s, x, y, plane, tiles_x);
      }
  }
}

__global__ __launch_bounds__(256) void unpack_depth_kernel(const double *__restrict__ plane, double *__restrict__ dst, int W, int H) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (int64_t)W * H) return;
  const int y = (int)(id / W), x = (int)(id % W);
  const double d = plane[texel_index(x, y, (W + kTexTileW - 1) / kTexTileW)];
  dst[(int64_t)(H - 1 - y) * W + x] = (unsigned long long)__double_as_longlong(d) == kInfBits ? -1.0 : d;
}

}  // namespace

hipError_t launch_render_check_ids(const RenderMesh &mesh, uint32_t *flag, hipStream_t stream) {
  const int64_t n_ids = 3 * mesh.n_triangles;
  if (n_ids == 0) return hipSuccess;
  hipLaunchKernelGGL(render_check_ids_kernel, dim3((unsigned)((n_ids + 255) / 256)), dim3(256), 0, stream, mesh.triangles, n_ids, mesh.n_points, flag);
  return hipGetLastError();
}

hipError_t launch_render_init(double *planes, int64_t n_texels, hipStream_t stream) {
  if (n_texels == 0) return hipSuccess;
  const unsigned blocks = (unsigned)std::min<int64_t>((n_texels + 255) / 256, 16384);
  hipLaunchKernelGGL(render_init_kernel, dim3(blocks), dim3(256), 0, stream, reinterpret_cast<unsigned long long *>(planes), n_texels);
  return hipGetLastError();
}

hipError_t launch_render_group(const RenderMesh &mesh, const RenderView *views, int m0, int n, int W, int H, double *planes, RenderPair *queue,
                               uint32_t capacity, uint32_t *counter, hipEvent_t between, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(counter, 0, sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  if (mesh.n_triangles == 0 || n == 0) return between ? hipEventRecord(between, stream) : hipSuccess;
  const int64_t plane_texels = color_plane_texels(W, H);
  hipLaunchKernelGGL(render_small_kernel, dim3((unsigned)((mesh.n_triangles + 255) / 256)), dim3(256), 0, stream, mesh.points, mesh.triangles,
                     mesh.n_triangles, views, m0, n, W, H, planes, plane_texels, queue, capacity, counter);
  e = hipGetLastError();
  if (e == hipSuccess && between) e = hipEventRecord(between, stream);
  if (e != hipSuccess) return e;
  // a fixed grid of waves that take the queue round robin: the number of pairs never has to come to the host between the passes
  const unsigned blocks = (unsigned)std::min<uint64_t>(((uint64_t)capacity + 3) / 4, 2048);
  hipLaunchKernelGGL(render_large_kernel, dim3(blocks), dim3(256), 0, stream, mesh.points, mesh.triangles, views, W, H, planes, plane_texels, queue,
                     capacity, counter);
  return hipGetLastError();
}

hipError_t launch_unpack_depth(const double *plane, double *dst, int W, int H, hipStream_t stream) {
  const int64_t total = (int64_t)W * H;
  hipLaunchKernelGGL(unpack_depth_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, plane, dst, W, H);
  return hipGetLastError();
}

}  // namespace dmi
