// depth_smooth.hip -- depth maps smoothed by an edge-preserving (bilateral) filter before they are fused (dmi_smooth_depths): every
// valid depth moves to the weighted mean of the valid depths round it that lie within a tolerance of it, the weight a spatial
// Gaussian times Tukey's biweight of the depth difference.  One kernel per iteration; fp64 VALU bound.
//
// Semantics (include/dmi.h states them in full; tests/depth_smooth_np.py restates them on the CPU and the result is
// identical): every output pixel is a function of the INPUT plane of its iteration alone, summed in one fixed order (dy outer,
// dx inner), so it is the same to the bit whatever order the hardware runs in.
//
// The kernel.  A workgroup of 256 lanes owns a tile of 64 x 32 pixels (depth_speckle_rules.h).  It stages the tile with a halo of
// r pixels on all four sides in LDS; a pixel that is not valid (step 1 of the definition, the best-cost threshold included) and a
// halo pixel outside the image are staged as a quiet NaN, so that the tap test u < T rejects them without a validity test of its
// own.  A lane owns a column; a wave owns eight rows and takes them as two vertical runs of four centres.  For a run the wave
// walks the 4 + 2r tap rows from the top: a tap row read from LDS once (lanes on consecutive doubles: conflict-free) serves every
// centre of the run whose window holds it, and each centre still meets its taps in the definition's order.
// The spatial weights s[|dy|] * s[|dx|] come from a table in the kernel's arguments, built once per launch on the host.
// Radii 1, 2 and 3 are instantiated with the tap loops unrolled (the table's entries are then scalar loads at fixed offsets);
// every other radius up to 8 runs the same body with the loops rolled.
//
// A rejected tap adds +0.0 to both sums instead of being skipped.  That leaves the bits alone: den is a sum of weights >= +0, and
// num starts at +0 and x + y is -0 only if both are, so neither sum is ever -0 and adding +0 is the identity.
//
// Stores: plain vector stores of the output planes, one pixel per lane.  No atomics.  Hang safety: no workgroup waits for
// another, one barrier that every lane reaches, every loop bounded by the tile and the radius.
#include "depth_smooth.h"

#include "depth_speckle_rules.h"

namespace dmi {
namespace {

namespace tiles = speckle_rules;
constexpr int kBlock = tiles::kWorkgroup;
constexpr int kTileW = tiles::kTileWidth;
constexpr int kTileH = tiles::kTileHeight;
constexpr int kRun = 4;  // centres a lane carries at a time
static_assert(kBlock == 256 && kTileW == 64 && kTileH == 2 * 4 * kRun, "four waves, a lane per column, two runs of rows per wave");

struct TileGrid {  // how a piece's tiles are counted (depth_speckle_rules.h: tile_index)
  int64_t across, down, tiles;
};

__device__ __forceinline__ bool valid_depth(double d) { return d > 0.0 && d < __builtin_huge_val(); }  // false for NaN

// one tap q at the centre c with T = tau * tau and the spatial weight P (the definition's loop body)
__device__ __forceinline__ void tap(double q, double c, double T, double P, double &num, double &den, int32_t &taken) {
  const double delta = q - c;
  const double u = delta * delta;
  const bool take = u < T;  // false for a NaN tap, a NaN centre
  const double g = T - u;
  const double w = P * (g * g);
  num = num + (take ? w * delta : 0.0);
  den = den + (take ? w : 0.0);
  taken += take ? 1 : 0;
}

// R >= 1: the radius, known to the compiler; R == -1: args.radius, anything in [0, kDepthSmoothMaxRadius]
template <int R>
__global__ __launch_bounds__(kBlock, 4) void depth_smooth_kernel(const double *__restrict__ src, const double *__restrict__ cost,
                                                              double threshold, double *__restrict__ dst, int32_t *__restrict__ count,
                                                              int32_t W, int32_t H, TileGrid grid, SmoothArgs args) {
  constexpr int kHalo = R >= 0 ? R : kDepthSmoothMaxRadius;
  constexpr int kPitch = kTileW + 2 * kHalo;
  __shared__ double s_depth[(kTileH + 2 * kHalo) * kPitch];
  const int r = R >= 0 ? R : args.radius;

  const int64_t tile = blockIdx.x;
  if (tile >= grid.tiles) return;  // (never: the launch has one workgroup per tile)
  const int64_t tx = tile % grid.across, ty = (tile / grid.across) % grid.down, view = tile / (grid.across * grid.down);
  const size_t base = (size_t)view * ((size_t)W * H);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t x0 = tx * kTileW, y0 = ty * kTileH;

  const int rows = kTileH + 2 * r, cols = kTileW + 2 * r;
  for (int i = threadIdx.x; i < rows * kPitch; i += kBlock) {
    const int row = i / kPitch, col = i - row * kPitch;
    if (col >= cols) continue;  // (only with the loops rolled, where the pitch is the largest radius's)
    const int64_t x = x0 - r + col, y = y0 - r + row;
    double d = __builtin_nan("");
    if (x >= 0 && y >= 0 && x < W && y < H) {
      const size_t at = base + (size_t)y * W + (size_t)x;
      const double v = src[at];
      if (valid_depth(v) && !(cost && cost[at] > threshold)) d = v;
    }
    s_depth[i] = d;
  }
  __syncthreads();

  const int64_t x = x0 + lane;
#pragma unroll 1
  for (int run = 0; run < 2; ++run) {
    const int row0 = (wave * 2 + run) * kRun;  // the run's first row in the tile
    if (y0 + row0 >= H) break;                 // (the whole wave)
    double c[kRun], T[kRun], num[kRun], den[kRun];
    int32_t taken[kRun];
#pragma unroll
    for (int j = 0; j < kRun; ++j) {
      c[j] = s_depth[(r + row0 + j) * kPitch + r + lane];
      const double tau = args.abs_tolerance + args.rel_tolerance * c[j];
      T[j] = tau * tau;
      num[j] = 0.0;
      den[j] = 0.0;
      taken[j] = 0;
    }
    // Tap row t of the run is row row0 + t of the staged tile (image row y0 + row0 + t - r): dy = t - j - r for centre j.  The rows
    // stay a loop -- unrolled, the (4 + 2R)(2R + 1) LDS reads of a run all rise to its top and spill at R = 3 --, so whether a
    // centre's window holds the row is a uniform branch and the row of the weight table a scalar load.
#pragma unroll 1
    for (int t = 0; t < kRun + 2 * r; ++t) {
      const double *const line = s_depth + (row0 + t) * kPitch + lane;
      double q[R >= 0 ? 2 * R + 1 : 1];  // the tap row, read once for every centre of the run (a known radius only)
      if constexpr (R >= 0) {
#pragma unroll
        for (int dx = 0; dx <= 2 * R; ++dx) q[dx] = line[dx];
      }
#pragma unroll
      for (int j = 0; j < kRun; ++j) {
        const int dy = t - j - r;
        if (dy < -r || dy > r) continue;
        const double *const weights = args.product + (dy < 0 ? -dy : dy) * kSmoothTableSide;
        if constexpr (R >= 0) {
#pragma unroll
          for (int dx = 0; dx <= 2 * R; ++dx) tap(q[dx], c[j], T[j], weights[dx < R ? R - dx : dx - R], num[j], den[j], taken[j]);
        } else {
#pragma unroll 1
          for (int dx = 0; dx <= 2 * r; ++dx) tap(line[dx], c[j], T[j], weights[dx < r ? r - dx : dx - r], num[j], den[j], taken[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kRun; ++j) {
      const int64_t y = y0 + row0 + j;
      if (x >= W || y >= H) continue;
      const size_t at = base + (size_t)y * W + (size_t)x;
      const bool valid = c[j] == c[j];  // staged as NaN otherwise
      double out = c[j] + num[j] / den[j];
      if (!(den[j] > 0.0 && den[j] < __builtin_huge_val() && out > 0.0 && out < __builtin_huge_val())) out = c[j];
      dst[at] = valid ? out : -1.0;
      if (count) count[at] = valid ? taken[j] : 0;
    }
  }
}

TileGrid tile_grid(int32_t W, int32_t H, int64_t count) {
  TileGrid g;
  g.across = tiles::tiles_across(W);
  g.down = tiles::tiles_down(H, kTileH);
  g.tiles = g.across * g.down * count;
  return g;
}

}  // namespace

SmoothArgs smooth_args(const double *s, int32_t radius, double abs_tolerance, double rel_tolerance) {
  SmoothArgs args{};
  for (int a = 0; a <= radius; ++a)
    for (int b = 0; b <= radius; ++b) args.product[a * kSmoothTableSide + b] = s[a] * s[b];
  args.abs_tolerance = abs_tolerance;
  args.rel_tolerance = rel_tolerance;
  args.radius = radius;
  return args;
}

hipError_t launch_depth_smooth(const double *src, const double *cost, double threshold, double *dst, int32_t *count, int64_t views,
                               int32_t W, int32_t H, const SmoothArgs &args, hipStream_t stream) {
  const TileGrid grid = tile_grid(W, H, views);
  if (args.radius < 0 || args.radius > kDepthSmoothMaxRadius || grid.tiles > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 blocks((unsigned)grid.tiles), lanes(kBlock);
  switch (args.radius) {
    case 1: hipLaunchKernelGGL(depth_smooth_kernel<1>, blocks, lanes, 0, stream, src, cost, threshold, dst, count, W, H, grid, args); break;
    case 2: hipLaunchKernelGGL(depth_smooth_kernel<2>, blocks, lanes, 0, stream, src, cost, threshold, dst, count, W, H, grid, args); break;
    case 3: hipLaunchKernelGGL(depth_smooth_kernel<3>, blocks, lanes, 0, stream, src, cost, threshold, dst, count, W, H, grid, args); break;
    default: hipLaunchKernelGGL(depth_smooth_kernel<-1>, blocks, lanes, 0, stream, src, cost, threshold, dst, count, W, H, grid, args);
  }
  return hipGetLastError();
}

}  // namespace dmi
