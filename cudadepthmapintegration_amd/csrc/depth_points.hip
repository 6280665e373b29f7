// depth_points.hip -- the fused point cloud of the resident view set (dmi_views_build_points): the points the views agree on, each
// once, with a normal taken from its own depth map.
//
// Semantics (include/dmi.h states them in full; tests/depth_points_np.py restates them on the CPU and the result is identical): f64
// throughout, every operation rounded (-ffp-contract=off), 8g's validity, back-projection, projection order and pixel rule.
//
// Passes, each a launch of its own in stream order (no workgroup ever waits for another: DESIGN.md 8n):
//   flags     one lane per source pixel in the consistency kernel's tile shape (a workgroup per 16 x 16 tile of one view, a wave per
//             8 x 8 quarter).  A candidate's world point is projected into the views t < s only, each camera arriving through scalar
//             loads; the target's depth and count are read at the pixel it lands on; a lane stops at its first owner and a wave
//             whose lanes have all stopped leaves the loop.  A wave without a candidate leaves at once.
//   counts    the valid, candidate and emitted pixels of every block of 256 consecutive pixels of one view (depth_points_rules.h)
//   scan      one workgroup: the exclusive sum of the blocks' emitted pixels in 64 bits, the total, and the report's sums
//   scatter   a workgroup per block again: an emitted pixel's rank is its block's offset plus its place inside the block; position
//             and normal are recomputed for emitted pixels only and stored with the view, the pixel and the count
//   normals   the blocks' points with a normal summed for the report
// The report costs no atomic per wave: a first version added three ballots per wave of the flag pass to three global counters, and
// at 256 views of 1280 x 720 those 10^7 adds to the same addresses took two thirds of the pass.
#include "depth_points.h"
#include "fusion_device.h"

namespace dmi {
namespace {

using namespace points_rules;

template <typename T>
__device__ __forceinline__ T cload(const T *p) {  // wave-uniform address -> scalar load
  return *reinterpret_cast<const T __attribute__((address_space(4))) *>(reinterpret_cast<uintptr_t>(p));
}

// what steps 2 and 5 read of the pixel's own view
struct SourceCamera {
  double rt[12], k00, k01, k02, k11, k12;
  __device__ __forceinline__ explicit SourceCamera(const ConsistencyCamera *__restrict__ c) {
#pragma unroll
    for (int q = 0; q < 12; ++q) rt[q] = cload(&c->rt[q]);
    k00 = cload(&c->k[0]), k01 = cload(&c->k[1]), k02 = cload(&c->k[2]), k11 = cload(&c->k[4]), k12 = cload(&c->k[5]);
  }
  // step 2's camera-space point of pixel (px, py) with depth d
  __device__ __forceinline__ void camera_point(int px, int py, double d, double c[3]) const {
    const double yn = ((double)py - k12) / k11;
    const double xn = (((double)px - k02) - k01 * yn) / k00;
    c[0] = xn * d, c[1] = yn * d, c[2] = d;
  }
  __device__ __forceinline__ void world_point(const double c[3], double w[3]) const {
    const double q0 = c[0] - rt[3], q1 = c[1] - rt[7], q2 = c[2] - rt[11];
#pragma unroll
    for (int j = 0; j < 3; ++j) w[j] = (rt[j] * q0 + rt[4 + j] * q1) + rt[8 + j] * q2;
  }
};

struct TargetCamera {
  double rt[12], k[7];
  __device__ __forceinline__ explicit TargetCamera(const ConsistencyCamera *__restrict__ c) {
#pragma unroll
    for (int q = 0; q < 12; ++q) rt[q] = cload(&c->rt[q]);
#pragma unroll
    for (int q = 0; q < 7; ++q) k[q] = cload(&c->k[q]);
  }
};

// Step 3 of 8g up to the pixel, as depth_consistency.hip's project() (that file is left alone: its kernel's registers are its
// tests' business): true when w lies in front of `cam` and projects into its image at (px, py); c2 is its camera z.
__device__ __forceinline__ bool project(const TargetCamera &cam, const double w[3], int W, int H, double &c2, int &px, int &py) {
  const double c0 = row4(cam.rt, w[0], w[1], w[2]), c1 = row4(cam.rt + 4, w[0], w[1], w[2]);
  c2 = row4(cam.rt + 8, w[0], w[1], w[2]);
  if (!(c2 > 0.0)) return false;
  const double h0 = ((cam.k[0] * c0 + cam.k[1] * c1) + cam.k[2] * c2) + cam.k[3];
  const double h1 = (cam.k[4] * c1 + cam.k[5] * c2) + cam.k[6];
  int in = pixel_fast(h0, h1, c2, W, H, px, py);
  if (in < 0) in = pixel_exact(h0, h1, c2, W, H, px, py) ? 1 : 0;
  return in != 0;
}

__device__ __forceinline__ bool agrees(double c2, double d, double abs_tol, double rel_tol) {
  const double bound = abs_tol + rel_tol * c2;
  return d > 0.0 && fabs(c2 - d) <= bound;
}

__device__ __forceinline__ bool takes_part(int px, int py, int step) { return px % step == 0 && py % step == 0; }

__global__ __launch_bounds__(kBlock) void points_flags_kernel(const double *__restrict__ planes, const int32_t *__restrict__ counts,
                                                              const ConsistencyCamera *__restrict__ cameras, int s0, int tiles_x,
                                                              PointsParams p, uint8_t *__restrict__ flags) {
  const int W = p.W, H = p.H;
  const int s = s0 + (int)blockIdx.y;
  const int tile_y = (int)blockIdx.x / tiles_x, tile_x = (int)blockIdx.x - tile_y * tiles_x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int px = tile_x * kConsistencyTile + (wave & 1) * 8 + (lane & 7);
  const int py = tile_y * kConsistencyTile + (wave >> 1) * 8 + (lane >> 3);
  const int64_t plane = (int64_t)W * H;
  const bool inside = px < W && py < H;
  const int64_t self = (int64_t)s * plane + (inside ? (int64_t)py * W + px : 0);
  const double d = inside ? planes[self] : -1.0;
  const bool valid = d > 0.0;  // the planes hold -1 for everything else
  if (__builtin_amdgcn_ballot_w64(valid) == 0) return;  // (the flags were zeroed)
  const bool candidate = valid && takes_part(px, py, p.pixel_step) && counts[self] >= p.min_views;
  if (__builtin_amdgcn_ballot_w64(candidate) == 0) {
    if (valid) flags[self] = kPointValid;
    return;
  }

  bool owned = false;
  if (p.dedupe && s > 0) {
    const SourceCamera src(cameras + s);
    double c[3], w[3];
    src.camera_point(px, py, d, c);
    src.world_point(c, w);
    bool pending = candidate;
    for (int view = 0; view < s; ++view) {
      if (__builtin_amdgcn_ballot_w64(pending) == 0) break;
      const int t = __builtin_amdgcn_readfirstlane(view);  // every lane is still in the loop: the camera's loads stay scalar
      const TargetCamera cam(cameras + t);
      if (pending) {
        double c2 = 0.0;
        int tx = 0, ty = 0;
        if (project(cam, w, W, H, c2, tx, ty)) {
          const int64_t at = (int64_t)t * plane + (int64_t)ty * W + tx;  // inside the target's plane: project() has tested it
          if (agrees(c2, planes[at], p.abs_tolerance, p.rel_tolerance) && takes_part(tx, ty, p.pixel_step) &&
              counts[at] >= p.min_views) {
            owned = true;
            pending = false;
          }
        }
      }
    }
  }
  if (valid) {
    const uint8_t taken = candidate ? kPointCandidate : (uint8_t)0, kept = candidate && !owned ? kPointEmitted : (uint8_t)0;
    flags[self] = (uint8_t)(kPointValid | taken | kept);
  }
}

// the emitted lanes of the workgroup's block: the lane's own flag, its rank among them, and their number
struct BlockRank {
  bool emitted;
  int rank, total;
};
__device__ __forceinline__ BlockRank rank_in_block(bool emitted, int *wave_total /* LDS, kBlock / 64 */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long mask = __builtin_amdgcn_ballot_w64(emitted);
  if (lane == 0) wave_total[wave] = __builtin_popcountll(mask);
  __syncthreads();
  BlockRank r{emitted, __builtin_popcountll(mask & ((1ull << lane) - 1)), 0};
#pragma unroll
  for (int v = 0; v < kBlock / 64; ++v) {
    if (v < wave) r.rank += wave_total[v];
    r.total += wave_total[v];
  }
  return r;
}

__global__ __launch_bounds__(kBlock) void points_block_counts_kernel(const uint8_t *__restrict__ flags, int64_t plane, int64_t per_view,
                                                                     uint32_t *__restrict__ block_counts) {
  __shared__ uint32_t wave_packed[kBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t block = blockIdx.x;
  const int64_t view = block_view(block, per_view), j = block_first_pixel(block, per_view) + threadIdx.x;
  const uint8_t f = j < plane ? flags[view * plane + j] : (uint8_t)0;
  const uint32_t valid = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64((f & kPointValid) != 0));
  const uint32_t candidates = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64((f & kPointCandidate) != 0));
  const uint32_t emitted = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64((f & kPointEmitted) != 0));
  if (lane == 0) wave_packed[wave] = pack_counts(valid, candidates, emitted);  // (a wave's counts end at 64, four waves' at 256:
  __syncthreads();                                                             //  the fields add without a carry)
  if (threadIdx.x == 0) block_counts[block] = wave_packed[0] + wave_packed[1] + wave_packed[2] + wave_packed[3];
}

__global__ __launch_bounds__(kBlock) void points_scan_kernel(const uint32_t *__restrict__ block_counts, int64_t blocks,
                                                             uint64_t *__restrict__ block_offsets, uint64_t *__restrict__ total,
                                                             unsigned long long *__restrict__ counters) {
  __shared__ uint64_t wave_sum[kBlock / 64];
  __shared__ unsigned long long report[2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < 2) report[threadIdx.x] = 0;  // (ordered before the adds below by the loop's barriers, or by the one behind it)
  uint64_t carry = 0;  // the sum of every chunk before this one: the same in every lane
  unsigned long long valid = 0, candidates = 0;  // this lane's share of the report
  const int64_t chunks = scan_chunks(blocks);
  for (int64_t chunk = 0; chunk < chunks; ++chunk) {
    const int64_t first = chunk * kScanChunk + (int64_t)threadIdx.x * kScanItems;
    uint32_t v[kScanItems];
    uint64_t sum = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
      const uint32_t packed = first + k < blocks ? block_counts[first + k] : 0u;
      valid += packed_valid(packed);
      candidates += packed_candidates(packed);
      v[k] = packed_emitted(packed);
      sum += v[k];
    }
    uint64_t inclusive = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint64_t below = __shfl_up((unsigned long long)inclusive, off, 64);
      if (lane >= off) inclusive += below;
    }
    if (lane == 63) wave_sum[wave] = inclusive;
    __syncthreads();
    uint64_t run = carry + (inclusive - sum);
#pragma unroll
    for (int u = 0; u < kBlock / 64; ++u) {
      if (u < wave) run += wave_sum[u];
      carry += wave_sum[u];
    }
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
      if (first + k < blocks) block_offsets[first + k] = run;
      run += v[k];
    }
    __syncthreads();  // wave_sum is written again by the next chunk
  }
  __syncthreads();
  atomicAdd(&report[0], valid);  // LDS, once per lane of the one workgroup
  atomicAdd(&report[1], candidates);
  __syncthreads();
  if (threadIdx.x == 0) {
    *total = carry;
    counters[kPtValid] = report[0];
    counters[kPtCandidates] = report[1];
    counters[kPtOwned] = report[1] - carry;
  }
}

__global__ __launch_bounds__(kBlock) void points_scatter_kernel(const double *__restrict__ planes, const int32_t *__restrict__ counts,
                                                                const ConsistencyCamera *__restrict__ cameras,
                                                                const uint8_t *__restrict__ flags, int64_t per_view, PointsParams p,
                                                                const uint64_t *__restrict__ block_offsets, Layout layout,
                                                                unsigned char *__restrict__ out, uint32_t *__restrict__ block_normals) {
  __shared__ int wave_total[kBlock / 64];
  __shared__ int wave_normals[kBlock / 64];
  const int W = p.W, H = p.H;
  const int64_t plane = (int64_t)W * H;
  const int64_t block = blockIdx.x;
  const int view = __builtin_amdgcn_readfirstlane((int)block_view(block, per_view));
  const int64_t j = block_first_pixel(block, per_view) + threadIdx.x;
  const bool emitted = j < plane && (flags[(int64_t)view * plane + j] & kPointEmitted) != 0;
  const BlockRank r = rank_in_block(emitted, wave_total);
  if (r.total == 0) {  // the whole workgroup
    if (threadIdx.x == 0) block_normals[block] = 0;
    return;
  }

  bool has_normal = false;
  if (emitted) {
    const uint64_t point = block_offsets[block] + (uint64_t)r.rank;
    const int py = (int)(j / W), px = (int)(j - (int64_t)py * W);
    const double *__restrict__ image = planes + (int64_t)view * plane;
    const SourceCamera src(cameras + view);
    const double d = image[j];
    double c[3], w[3];
    src.camera_point(px, py, d, c);
    src.world_point(c, w);

    // step 5: the neighbours (-1 outside the image: never usable), their usable bits, the tangents
    const double bound = p.normal_abs_tolerance + p.normal_rel_tolerance * d;
    const double d_right = px + 1 < W ? image[j + 1] : -1.0, d_left = px > 0 ? image[j - 1] : -1.0;
    const double d_down = py + 1 < H ? image[j + W] : -1.0, d_up = py > 0 ? image[j - W] : -1.0;
    auto usable = [&](double dn) { return dn > 0.0 && fabs(dn - d) <= bound; };
    const unsigned bits = (usable(d_right) ? kUsableRight : 0u) | (usable(d_left) ? kUsableLeft : 0u) |
                          (usable(d_down) ? kUsableDown : 0u) | (usable(d_up) ? kUsableUp : 0u);
    const Tangents tangents = tangents_of(bits);
    double c_right[3], c_left[3], c_down[3], c_up[3];
    src.camera_point(px + 1, py, d_right, c_right);
    src.camera_point(px - 1, py, d_left, c_left);
    src.camera_point(px, py + 1, d_down, c_down);
    src.camera_point(px, py - 1, d_up, c_up);
    double tx[3], ty[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      tx[q] = (tangent_high(tangents.x) ? c_right[q] : c[q]) - (tangent_low(tangents.x) ? c_left[q] : c[q]);
      ty[q] = (tangent_high(tangents.y) ? c_down[q] : c[q]) - (tangent_low(tangents.y) ? c_up[q] : c[q]);
    }
    double m[3] = {tx[1] * ty[2] - tx[2] * ty[1], tx[2] * ty[0] - tx[0] * ty[2], tx[0] * ty[1] - tx[1] * ty[0]};
    const double facing = (m[0] * c[0] + m[1] * c[1]) + m[2] * c[2];
    if (facing > 0.0) m[0] = -m[0], m[1] = -m[1], m[2] = -m[2];
    double g[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) g[q] = (src.rt[q] * m[0] + src.rt[4 + q] * m[1]) + src.rt[8 + q] * m[2];
    const double length = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
    has_normal = tangents_exist(tangents) && length > 0.0 && length < __builtin_inf();

    double *const xyz = reinterpret_cast<double *>(out + entry_offset(layout.xyz, point, 24));
    float *const normal = reinterpret_cast<float *>(out + entry_offset(layout.normal, point, 12));
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      xyz[q] = w[q];
      normal[q] = has_normal ? (float)(g[q] / length) : 0.0f;
    }
    *reinterpret_cast<int32_t *>(out + entry_offset(layout.view, point, 4)) = view;
    *reinterpret_cast<int32_t *>(out + entry_offset(layout.pixel, point, 4)) = (int32_t)j;
    *reinterpret_cast<int32_t *>(out + entry_offset(layout.count, point, 4)) = counts[(int64_t)view * plane + j];
  }
  // (the ballot is taken where the wave has converged again)
  const unsigned long long normals = __builtin_amdgcn_ballot_w64(has_normal);
  if ((threadIdx.x & 63) == 0) wave_normals[threadIdx.x >> 6] = __builtin_popcountll(normals);
  __syncthreads();
  if (threadIdx.x == 0) block_normals[block] = (uint32_t)(wave_normals[0] + wave_normals[1] + wave_normals[2] + wave_normals[3]);
}

constexpr int kSumGroups = 256;  // workgroups of the report's last sum: one atomic each

__global__ __launch_bounds__(kBlock) void points_sum_normals_kernel(const uint32_t *__restrict__ block_normals, int64_t blocks,
                                                                    unsigned long long *__restrict__ counters) {
  __shared__ unsigned long long group_sum;
  if (threadIdx.x == 0) group_sum = 0;
  __syncthreads();
  unsigned long long sum = 0;
  for (int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x; b < blocks; b += (int64_t)gridDim.x * kBlock) sum += block_normals[b];
  if (sum) atomicAdd(&group_sum, sum);  // LDS
  __syncthreads();
  if (threadIdx.x == 0 && group_sum) atomicAdd(counters + kPtWithNormal, group_sum);
}

}  // namespace

hipError_t launch_points_flags(const double *planes, const int32_t *counts, const ConsistencyCamera *cameras, int32_t n,
                               const PointsParams &params, uint8_t *flags, hipStream_t stream) {
  const int tiles_x = (params.W + kConsistencyTile - 1) / kConsistencyTile, tiles_y = (params.H + kConsistencyTile - 1) / kConsistencyTile;
  constexpr int kMaxGridY = 32768;  // source views per launch: the grid's second dimension ends at 65535
  for (int s0 = 0; s0 < n; s0 += kMaxGridY) {
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)(n - s0 < kMaxGridY ? n - s0 : kMaxGridY));
    hipLaunchKernelGGL(points_flags_kernel, grid, dim3(kBlock), 0, stream, planes, counts, cameras, s0, tiles_x, params, flags);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_points_block_counts(const uint8_t *flags, int32_t n, int32_t W, int32_t H, uint32_t *block_counts, hipStream_t stream) {
  if (!blocks_fit_one_launch(n, W, H)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(points_block_counts_kernel, dim3((unsigned)total_blocks(n, W, H)), dim3(kBlock), 0, stream, flags, (int64_t)W * H,
                     blocks_per_view(W, H), block_counts);
  return hipGetLastError();
}

hipError_t launch_points_scan(const uint32_t *block_counts, int64_t blocks, uint64_t *block_offsets, uint64_t *total,
                              unsigned long long *counters, hipStream_t stream) {
  hipLaunchKernelGGL(points_scan_kernel, dim3(1), dim3(kBlock), 0, stream, block_counts, blocks, block_offsets, total, counters);
  return hipGetLastError();
}

hipError_t launch_points_sum_normals(const uint32_t *block_normals, int64_t blocks, unsigned long long *counters, hipStream_t stream) {
  const int64_t needed = (blocks + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(points_sum_normals_kernel, dim3((unsigned)(needed < 1 ? 1 : needed < kSumGroups ? needed : kSumGroups)), dim3(kBlock),
                     0, stream, block_normals, blocks, counters);
  return hipGetLastError();
}

hipError_t launch_points_scatter(const double *planes, const int32_t *counts, const ConsistencyCamera *cameras, const uint8_t *flags,
                                 int32_t n, const PointsParams &params, const uint64_t *block_offsets, const Layout &layout,
                                 unsigned char *out, uint32_t *block_normals, hipStream_t stream) {
  if (!blocks_fit_one_launch(n, params.W, params.H)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(points_scatter_kernel, dim3((unsigned)total_blocks(n, params.W, params.H)), dim3(kBlock), 0, stream, planes, counts,
                     cameras, flags, blocks_per_view(params.W, params.H), params, block_offsets, layout, out, block_normals);
  return hipGetLastError();
}

}  // namespace dmi
