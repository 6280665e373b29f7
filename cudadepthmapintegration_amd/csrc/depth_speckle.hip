// depth_speckle.hip -- connected-component labelling of depth maps (dmi_filter_depth_speckles): the segments of every view under
// the definition's LINKED relation, their sizes, and the depths of the segments that are large enough.  Integer work and one f64
// compare per link; HBM-bound.
//
// Semantics (include/dmi.h states them in full; tests/depth_speckle_np.py restates them on the CPU and the result is
// identical): the result depends only on the partition into segments, so it is the same to the bit whatever order the hardware
// runs in.
//
// Passes, one kernel each (depth_speckle.h: SpecklePiece names the planes):
//   local    a workgroup of 256 lanes owns a tile of 64 x 32 pixels (depth_speckle_rules.h).  It stages the thresholded depths with
//            a one-pixel halo to the right and below in LDS, forms every pixel's right- and down-link once -- the only place the f64
//            compare runs --, labels each row's runs from one ballot, unites runs through the down-links in a union-find on the
//            tile's labels in LDS, counts every tile-local root's pixels, and writes label[] (the view-local index of the pixel's
//            tile-local root), size[] (the count at a root, 0 elsewhere) and the link bits across its right and bottom border.
//   border   one lane per pixel of a tile's last row or column: where the link bit is set, unite() of union_find_device.h on the
//            view's label plane, unless the lane before it makes the same link.  A tile-local root is the smallest index of its
//            local segment, so parent[v] <= v holds from the start.
//   sizes    a LATER kernel (no link is made while it runs): every tile-local root r -- size[r] != 0 -- finds its final root g,
//            stores it as its label and, if g != r, adds its count to size[g]: one integer atomic per tile-local root.
//   output   one lane per two pixels: g = label[label[p]] (a pixel's label is its tile-local root or, after a path halving of the
//            border pass, another tile-local root of its segment; the sizes pass left the final root in every one of them), the
//            segment's size size[g], and out = D where the size reaches min_pixels, -1 elsewhere; 16-byte loads and stores.
//
// Visibility: union_find_device.h states the argument for the label plane in the border pass (agent-scope atomics; a link is a
// successful compare-and-swap on a root).  The local pass's union-find lives in LDS, which a workgroup sees coherently: relaxed
// workgroup-scope atomics, with a barrier between the hooks and the reads of the roots.  The sizes pass reads size[] of non-final
// roots, which nobody adds to, and adds to size[] of final roots, which it reads only to see that they are not zero.
//
// Hang safety: no workgroup waits for another; every loop of a union-find ends because an index strictly decreased; all other
// loops are bounded by the tile.  No spin-waits, no flags between workgroups.
#include "depth_speckle.h"

#include "union_find_device.h"

namespace dmi {
namespace {

namespace rules = speckle_rules;
constexpr int kBlock = rules::kWorkgroup;
constexpr int kTileW = rules::kTileWidth;

__device__ __forceinline__ bool valid_depth(double d) { return d > 0.0 && d < __builtin_huge_val(); }  // false for NaN

// step 2 of the definition: the product, then the sum, then the difference, each rounded on its own (-ffp-contract=off)
__device__ __forceinline__ bool linked(double a, double b, double abs_tolerance, double rel_tolerance) {
  if (!valid_depth(a) || !valid_depth(b)) return false;
  const double bound = abs_tolerance + rel_tolerance * fmin(a, b);
  return fabs(a - b) <= bound;
}

// the tile's union-find in LDS: as union_find_device.h's, at workgroup scope
__device__ __forceinline__ uint32_t lds_parent(const uint32_t *label, uint32_t v) {
  return __hip_atomic_load(label + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ uint32_t lds_root(const uint32_t *label, uint32_t v) {  // each step moves to a strictly smaller index
  uint32_t p = lds_parent(label, v);
  while (p != v) {
    v = p;
    p = lds_parent(label, v);
  }
  return v;
}
__device__ __forceinline__ void lds_unite(uint32_t *label, uint32_t a, uint32_t b) {
  for (;;) {
    a = lds_root(label, a);
    b = lds_root(label, b);
    if (a == b) return;
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    uint32_t seen = hi;
    if (__hip_atomic_compare_exchange_strong(label + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
      return;
    a = seen;  // hi was linked meanwhile: seen < hi is a member of its set
    b = lo;
  }
}

struct TileGrid {  // how a piece's tiles are counted (depth_speckle_rules.h: tile_index)
  int64_t across, down, tiles;
};

// TH: the tile's rows (a multiple of 4, at most 64).  RUNS: a row's runs are the union-find's nodes; otherwise every pixel is.
template <int TH, bool RUNS>
__global__ __launch_bounds__(kBlock) void speckle_local_kernel(SpecklePiece piece, double threshold, int32_t W, int32_t H,
                                                               double abs_tolerance, double rel_tolerance, TileGrid grid) {
  constexpr int kPitch = kTileW + 1;
  constexpr int kNodes = TH * kTileW;
  static_assert(TH % 4 == 0 && TH <= 64, "four waves share the rows; a tile's right border is one u64");
  static_assert((TH + 1) * kPitch * sizeof(double) >= kNodes * sizeof(uint32_t), "the counts reuse the staged depths' LDS");
  __shared__ double s_depth[(TH + 1) * kPitch];  // the thresholded depths with their halo; the roots' counts once the links are formed
  __shared__ uint32_t s_label[kNodes];
  __shared__ uint64_t s_links[TH + 1], s_down[TH];
  uint32_t *const s_count = reinterpret_cast<uint32_t *>(s_depth);

  const int64_t tile = blockIdx.x;
  if (tile >= grid.tiles) return;  // (never: the launch has one workgroup per tile)
  const int64_t tx = tile % grid.across, ty = (tile / grid.across) % grid.down, view = tile / (grid.across * grid.down);
  const size_t plane = (size_t)W * H, base = (size_t)view * plane;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t x0 = tx * kTileW, y0 = ty * TH;

  auto staged = [&](int64_t x, int64_t y) -> double {  // step 1 of the definition; outside the image: not valid
    if (x >= W || y >= H) return -1.0;
    const size_t at = base + (size_t)y * W + (size_t)x;
    const double d = piece.depth[at];
    if (piece.cost && piece.cost[at] > threshold) return -1.0;
    return d;
  };
  for (int row = wave; row <= TH; row += 4) s_depth[row * kPitch + lane] = staged(x0 + lane, y0 + row);
  if (threadIdx.x <= TH) s_depth[threadIdx.x * kPitch + kTileW] = staged(x0 + kTileW, y0 + threadIdx.x);
  if (threadIdx.x == 0) s_links[TH] = 0;
  __syncthreads();

  // the links, once; each row's runs from one ballot
  for (int row = wave; row < TH; row += 4) {
    const double d = s_depth[row * kPitch + lane];
    const bool right = linked(d, s_depth[row * kPitch + lane + 1], abs_tolerance, rel_tolerance);
    const bool down = linked(d, s_depth[(row + 1) * kPitch + lane], abs_tolerance, rel_tolerance);
    const uint64_t links = __ballot(right), downs = __ballot(down);
    const uint32_t self = (uint32_t)(row * kTileW + lane);
    const uint32_t node = RUNS ? (uint32_t)(row * kTileW + rules::run_start(links, lane)) : self;
    s_label[self] = valid_depth(d) ? node : rules::kNoLabel;
    if (lane == 0) {
      s_links[row] = links;
      s_down[row] = downs;
    }
  }
  __syncthreads();  // the depths are not read again: their LDS becomes the counts
  for (int i = threadIdx.x; i < kNodes; i += kBlock) s_count[i] = 0;

  // the hooks
  for (int row = wave; row < TH; row += 4) {
    const uint32_t self = (uint32_t)(row * kTileW + lane);
    const uint64_t links = s_links[row], downs = row + 1 < TH ? s_down[row] : 0;  // the last row's down-links are the border pass's
    if (RUNS) {
      if ((rules::hooking_lanes(links, s_links[row + 1], downs) >> lane) & 1)
        lds_unite(s_label, lds_parent(s_label, self), lds_parent(s_label, self + kTileW));
    } else {
      if (lane + 1 < kTileW && ((links >> lane) & 1)) lds_unite(s_label, self, self + 1);
      if ((downs >> lane) & 1) lds_unite(s_label, self, self + kTileW);
    }
  }
  __syncthreads();

  // every pixel's tile-local root, and the roots' pixel counts
  uint32_t root[TH / 4];
#pragma unroll
  for (int i = 0; i < TH / 4; ++i) {
    const int row = wave + 4 * i;
    const uint32_t self = (uint32_t)(row * kTileW + lane);
    const uint32_t first = lds_parent(s_label, self);
    root[i] = first == rules::kNoLabel ? rules::kNoLabel : lds_root(s_label, first);
    if (root[i] == rules::kNoLabel) continue;
    if (RUNS) {
      const uint64_t links = s_links[row];
      if (rules::run_start(links, lane) == lane) atomicAdd(&s_count[root[i]], (uint32_t)(rules::run_end(links, lane) - lane + 1));
    } else {
      atomicAdd(&s_count[root[i]], 1u);
    }
  }
  __syncthreads();

#pragma unroll
  for (int i = 0; i < TH / 4; ++i) {
    const int row = wave + 4 * i;
    const int64_t x = x0 + lane, y = y0 + row;
    if (x >= W || y >= H) continue;
    const size_t at = base + (size_t)y * W + (size_t)x;
    const uint32_t r = root[i];
    const bool valid = r != rules::kNoLabel;
    // a tile-local root's view-local index; it is the smallest of its local segment, since both orders run row by row
    piece.label[at] = valid ? (uint32_t)((y0 + (r >> 6)) * W + x0 + (r & 63)) : rules::kNoLabel;
    piece.size[at] = valid && r == (uint32_t)(row * kTileW + lane) ? s_count[r] : 0u;
  }
  if (wave == 0) {
    const uint64_t rights = __ballot(lane < TH && (s_links[lane < TH ? lane : 0] >> 63) != 0);
    if (lane == 0) {
      piece.border_down[tile] = s_down[TH - 1];
      piece.border_right[tile] = rights;
    }
  }
}

// A tile's 128 border lanes are two waves: its last row's columns, then its last column's rows.  A lane whose neighbour one
// column to the left (one row up) joins the same two tile-local segments leaves the link to that neighbour: along the border of
// two surfaces a wave makes one link, not 64 (the border pass took 2.8 of 6.0 ms before).  The labels are read with
// plain loads while other lanes link: whatever such a load sees is a member of the pixel's own set, so equal labels mean equal sets.
template <int TH>
__global__ __launch_bounds__(kBlock) void speckle_border_kernel(SpecklePiece piece, int32_t W, int32_t H, TileGrid grid) {
  static_assert(rules::kBorderLanes == 128 && kBlock % rules::kBorderLanes == 0, "a border's lanes are whole waves");
  const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t tile = gid / rules::kBorderLanes;
  const int k = (int)(gid % rules::kBorderLanes);
  uint32_t a = 0, b = 0, label_a = rules::kNoLabel, label_b = rules::kNoLabel;
  uint32_t *parent = nullptr;
  bool active = false;
  if (tile < grid.tiles) {
    const uint64_t bits = k < kTileW ? piece.border_down[tile] : piece.border_right[tile];
    const int64_t tx = tile % grid.across, ty = (tile / grid.across) % grid.down, view = tile / (grid.across * grid.down);
    // (border_pair never refuses a set bit: no access outside the view's plane)
    if (((bits >> (k & 63)) & 1) && rules::border_pair(tx, ty, k, W, H, TH, &a, &b)) {
      parent = piece.label + (size_t)view * ((size_t)W * H);
      label_a = parent[a];
      label_b = parent[b];
      active = label_a != rules::kNoLabel && label_b != rules::kNoLabel;  // (always for a set bit: both pixels are valid)
    }
  }
  const uint32_t before_a = __shfl_up(label_a, 1), before_b = __shfl_up(label_b, 1);
  const bool before_active = __shfl_up((int)active, 1) != 0;
  if (!active) return;
  if ((threadIdx.x & 63) != 0 && before_active && before_a == label_a && before_b == label_b) return;
  uint32_t retries = 0;
  union_find::unite(parent, label_a, label_b, &retries);
}

__global__ __launch_bounds__(kBlock) void speckle_sizes_kernel(SpecklePiece piece, uint64_t plane, uint64_t total) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= total) return;
  const uint32_t count = piece.size[i];
  if (count == 0) return;  // not a tile-local root
  const uint64_t base = i / plane * plane;
  const uint32_t r = (uint32_t)(i - base);
  const uint32_t g = union_find::final_root(piece.label + base, r);
  if (g == r) return;
  __hip_atomic_store(piece.label + base + r, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // an ancestor: others may still pass through r
  atomicAdd(piece.size + base + g, count);
}

struct SpeckleResult {
  double depth;
  int32_t size;
};

__device__ __forceinline__ SpeckleResult speckle_result(const SpecklePiece &piece, uint64_t plane, uint64_t i, double d, uint32_t label,
                                                        int64_t min_pixels) {
  if (label == rules::kNoLabel) return {-1.0, 0};
  const uint64_t base = i / plane * plane;
  const uint32_t g = piece.label[base + label];
  const uint32_t size = piece.size[base + g];
  return {(int64_t)size >= min_pixels ? d : -1.0, (int32_t)size};
}

__global__ __launch_bounds__(kBlock) void speckle_output_kernel(SpecklePiece piece, uint64_t plane, uint64_t total, int64_t min_pixels) {
  const uint64_t i = 2 * ((uint64_t)blockIdx.x * kBlock + threadIdx.x);
  if (i >= total) return;
  if (i + 1 < total) {  // (the planes start at allocations: an even pixel index is 16-byte aligned in depth[])
    const double2 d = *reinterpret_cast<const double2 *>(piece.depth + i);
    const uint2 label = *reinterpret_cast<const uint2 *>(piece.label + i);
    const SpeckleResult r0 = speckle_result(piece, plane, i, d.x, label.x, min_pixels);
    const SpeckleResult r1 = speckle_result(piece, plane, i + 1, d.y, label.y, min_pixels);
    *reinterpret_cast<double2 *>(piece.depth + i) = make_double2(r0.depth, r1.depth);
    if (piece.out_size) *reinterpret_cast<int2 *>(piece.out_size + i) = make_int2(r0.size, r1.size);
  } else {
    const SpeckleResult r = speckle_result(piece, plane, i, piece.depth[i], piece.label[i], min_pixels);
    piece.depth[i] = r.depth;
    if (piece.out_size) piece.out_size[i] = r.size;
  }
}

TileGrid tile_grid(int32_t W, int32_t H, int64_t count, int tile_height) {
  TileGrid g;
  g.across = rules::tiles_across(W);
  g.down = rules::tiles_down(H, tile_height);
  g.tiles = g.across * g.down * count;
  return g;
}

inline unsigned blocks(uint64_t items) { return (unsigned)((items + kBlock - 1) / kBlock); }

template <int TH, bool RUNS>
hipError_t local_launch(const SpecklePiece &piece, double threshold, int32_t W, int32_t H, double abs_tolerance, double rel_tolerance,
                        hipStream_t stream) {
  const TileGrid grid = tile_grid(W, H, piece.count, TH);
  if (grid.tiles > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((speckle_local_kernel<TH, RUNS>), dim3((unsigned)grid.tiles), dim3(kBlock), 0, stream, piece, threshold, W, H,
                     abs_tolerance, rel_tolerance, grid);
  return hipGetLastError();
}

template <int TH>
hipError_t border_launch(const SpecklePiece &piece, int32_t W, int32_t H, hipStream_t stream) {
  const TileGrid grid = tile_grid(W, H, piece.count, TH);
  const uint64_t lanes = (uint64_t)grid.tiles * rules::kBorderLanes;
  if ((lanes + kBlock - 1) / kBlock > 0x7fffffffULL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((speckle_border_kernel<TH>), dim3(blocks(lanes)), dim3(kBlock), 0, stream, piece, W, H, grid);
  return hipGetLastError();
}

}  // namespace

int64_t speckle_tiles(int32_t W, int32_t H, int64_t count, const SpeckleTuning &tuning) {
  return tile_grid(W, H, count, tuning.tile_height).tiles;
}

hipError_t launch_speckle_local(const SpecklePiece &piece, double threshold, int32_t W, int32_t H, double abs_tolerance,
                                double rel_tolerance, const SpeckleTuning &tuning, hipStream_t stream) {
#ifdef DMI_TUNING
  if (!tuning.runs) {
    if (tuning.tile_height != rules::kTileHeight) return hipErrorInvalidValue;
    return local_launch<rules::kTileHeight, false>(piece, threshold, W, H, abs_tolerance, rel_tolerance, stream);
  }
  if (tuning.tile_height == 16) return local_launch<16, true>(piece, threshold, W, H, abs_tolerance, rel_tolerance, stream);
  if (tuning.tile_height == 64) return local_launch<64, true>(piece, threshold, W, H, abs_tolerance, rel_tolerance, stream);
#endif
  if (tuning.tile_height != rules::kTileHeight || !tuning.runs) return hipErrorInvalidValue;
  return local_launch<rules::kTileHeight, true>(piece, threshold, W, H, abs_tolerance, rel_tolerance, stream);
}

hipError_t launch_speckle_border(const SpecklePiece &piece, int32_t W, int32_t H, const SpeckleTuning &tuning, hipStream_t stream) {
#ifdef DMI_TUNING
  if (tuning.tile_height == 16) return border_launch<16>(piece, W, H, stream);
  if (tuning.tile_height == 64) return border_launch<64>(piece, W, H, stream);
#endif
  if (tuning.tile_height != rules::kTileHeight) return hipErrorInvalidValue;
  return border_launch<rules::kTileHeight>(piece, W, H, stream);
}

hipError_t launch_speckle_sizes(const SpecklePiece &piece, int32_t W, int32_t H, hipStream_t stream) {
  const uint64_t plane = (uint64_t)W * H, total = plane * (uint64_t)piece.count;
  if ((total + kBlock - 1) / kBlock > 0x7fffffffULL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(speckle_sizes_kernel, dim3(blocks(total)), dim3(kBlock), 0, stream, piece, plane, total);
  return hipGetLastError();
}

hipError_t launch_speckle_output(const SpecklePiece &piece, int32_t W, int32_t H, int64_t min_pixels, hipStream_t stream) {
  const uint64_t plane = (uint64_t)W * H, total = plane * (uint64_t)piece.count;
  hipLaunchKernelGGL(speckle_output_kernel, dim3(blocks((total + 1) / 2)), dim3(kBlock), 0, stream, piece, plane, total, min_pixels);
  return hipGetLastError();
}

}  // namespace dmi
