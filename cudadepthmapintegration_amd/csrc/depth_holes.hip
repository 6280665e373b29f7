// depth_holes.hip -- small holes of depth maps filled from their rims (dmi_fill_depth_holes): the connected components of the pixels
// that are NOT valid, per component its size, whether it touches the image's border and the smallest and largest depth on its rim,
// and for the pixels of the components that qualify a depth interpolated between the four nearest valid pixels of their row and
// column.  Integer work, one f64 compare per hole pixel and three divisions per filled pixel; HBM-bound.
//
// Semantics (include/dmi.h states them in full; tests/depth_holes_np.py restates them on the CPU and the result is
// identical): the result depends only on the partition into holes, on exact minima and maxima, and on INPUT depths at valid
// pixels, so it is the same to the bit whatever order the hardware runs in.
//
// Passes, one kernel each (depth_holes.h: HolesPiece names the planes):
//   local    a workgroup of 256 lanes owns a tile of 64 x 32 pixels (depth_speckle_rules.h).  It stages the thresholded depths with
//            a one-pixel halo on all four sides in LDS, forms every row's ballot of hole pixels, labels each row's runs of holes from
//            it, unites runs through the rows in a union-find on the tile's labels in LDS, and reduces four values per tile-local
//            root in LDS: the pixel count, the border flag (one u32 together: depth_holes_rules.h), and the minimum and the maximum of
//            the depths on the rim.  The rim is taken from the hole's side: every hole pixel looks at its four neighbours in the
//            staged tile, the halo included; depths are positive and finite, so their bit patterns order as u64 and the two bounds
//            are integer atomics.  It writes label[] (the view-local index of the pixel's tile-local root, kNoLabel at a valid
//            pixel), the three record planes at the roots (record[] = 0 elsewhere) and the link bits across its right and bottom border.
//   border   depth_speckle.hip's border pass as it is, on this piece's label plane and border bits (launch_speckle_border).
//   merge    a LATER kernel (no link is made while it runs): every tile-local root r -- record[r] != 0 -- finds its final root g,
//            stores it as its label and, if g != r, adds its count to record[g], ORs its flag in and takes its rim bounds into
//            rim_lo[g] and rim_hi[g]: at most four atomics per tile-local root, never one per pixel.
//   output   a workgroup per tile again, a wave per row: g = label[label[p]] as in the speckle filter, the hole's record at g, the
//            FILLABLE predicate, and for a pixel of a fillable hole the nearest valid pixel on each of its four sides -- in the row
//            from the wave's ballot of valid pixels where that holds one, otherwise and in the column by a walk over label[] of at
//            most min(max_pixels, W) or min(max_pixels, H) steps -- and the interpolation.  Only hole pixels are stored to; the
//            depths that are read are those of valid pixels, which nobody writes.
//
// Visibility.  The label plane: union_find_device.h's argument, unchanged.  The local pass's union-find and records live in LDS,
// which a workgroup sees coherently: relaxed workgroup-scope atomics, a barrier between the hooks and the reads of the roots and
// another between the reductions and the reads of the records.  The records in global memory: the local pass writes record[],
// rim_lo[] and rim_hi[] of every tile-local root with plain stores, and the kernel boundary makes them visible to the merge pass
// on every XCD.  The merge pass reads the records of NON-final roots only, which nobody modifies, and modifies the records of
// final roots only, by device-scope atomics (add, or, 64-bit unsigned min and max: performed at the memory side of the XCDs' L2s,
// so no update is lost whichever XCD issues it); the one plain read it makes of a final root's record is `record[g] != 0`, which
// holds before and after every update since a count is at least 1.  The output pass is a later kernel again and reads finished
// records.  Every update commutes (sum, or, min, max), so the records do not depend on the order of arrival.
//
// Hang safety: no workgroup waits for another; every loop of a union-find ends because an index strictly decreased; the output
// pass's walks count down a limit; all other loops are bounded by the tile.  No spin-waits, no flags between workgroups.
#include "depth_holes.h"

#include "depth_speckle.h"
#include "union_find_device.h"

namespace dmi {
namespace {

namespace tiles = speckle_rules;
namespace rules = holes_rules;
constexpr int kBlock = tiles::kWorkgroup;
constexpr int kTileW = tiles::kTileWidth;
constexpr int kTileH = tiles::kTileHeight;
static_assert(kBlock == 256 && kTileW == 64 && kTileH % 4 == 0, "four waves share a tile's rows, a lane per column");

__device__ __forceinline__ bool valid_depth(double d) { return d > 0.0 && d < __builtin_huge_val(); }  // false for NaN

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

__global__ __launch_bounds__(kBlock) void holes_local_kernel(HolesPiece piece, double threshold, int32_t W, int32_t H, TileGrid grid) {
  constexpr int TH = kTileH;
  constexpr int kPitch = kTileW + 2;  // a column of halo on either side
  constexpr int kNodes = TH * kTileW;
  static_assert((TH + 2) * kPitch * sizeof(double) >= kNodes * sizeof(uint64_t), "the rim minima reuse the staged depths' LDS");
  __shared__ double s_depth[(TH + 2) * kPitch];  // the thresholded depths with their halo; the roots' rim minima once the rows are read
  __shared__ uint64_t s_hi[kNodes];
  __shared__ uint32_t s_label[kNodes], s_record[kNodes];
  __shared__ uint64_t s_links[TH + 1], s_down[TH];
  uint64_t *const s_lo = reinterpret_cast<uint64_t *>(s_depth);

  const int64_t tile = blockIdx.x;
  if (tile >= grid.tiles) return;  // (never: the launch has one workgroup per tile)
  const int64_t tx = tile % grid.across, ty = (tile / grid.across) % grid.down, view = tile / (grid.across * grid.down);
  const size_t plane = (size_t)W * H, base = (size_t)view * plane;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t x0 = tx * kTileW, y0 = ty * TH;

  auto staged = [&](int64_t x, int64_t y) -> double {  // step 1 of the definition; outside the image: not valid (and no hole either)
    if (x < 0 || y < 0 || x >= W || y >= H) return -1.0;
    const size_t at = base + (size_t)y * W + (size_t)x;
    const double d = piece.depth[at];
    if (piece.cost && piece.cost[at] > threshold) return -1.0;
    return d;
  };
  auto cell = [&](int row, int col) -> double & { return s_depth[(row + 1) * kPitch + col + 1]; };  // row in [-1, TH], col in [-1, 64]
  for (int row = wave - 1; row <= TH; row += 4) cell(row, lane) = staged(x0 + lane, y0 + row);
  if (threadIdx.x < TH + 2) cell((int)threadIdx.x - 1, -1) = staged(x0 - 1, y0 + (int)threadIdx.x - 1);
  if (threadIdx.x >= 64 && threadIdx.x < 64 + TH + 2) cell((int)threadIdx.x - 65, kTileW) = staged(x0 + kTileW, y0 + (int)threadIdx.x - 65);
  if (threadIdx.x == 0) s_links[TH] = 0;
  __syncthreads();

  // every row's holes from one ballot, its runs, and every hole pixel's own share of the rim
  uint64_t rim_lo[TH / 4], rim_hi[TH / 4];
#pragma unroll
  for (int i = 0; i < TH / 4; ++i) {
    const int row = wave + 4 * i;
    const int64_t x = x0 + lane, y = y0 + row;
    const double d = cell(row, lane);
    const double left = cell(row, lane - 1), right = cell(row, lane + 1), up = cell(row - 1, lane), below = cell(row + 1, lane);
    const bool hole = x < W && y < H && !valid_depth(d);
    const bool hole_right = x + 1 < W && y < H && !valid_depth(right);
    const bool hole_below = x < W && y + 1 < H && !valid_depth(below);
    const uint64_t holes = __ballot(hole);
    const uint64_t links = rules::hole_links(holes, __ballot(lane == kTileW - 1 && hole_right) != 0);
    const uint64_t downs = __ballot(hole && hole_below);
    uint64_t lo = rules::kNoRimLo, hi = rules::kNoRimHi;
    auto take = [&](double rim) {
      if (!hole || !valid_depth(rim)) return;
      const uint64_t bits = (uint64_t)__double_as_longlong(rim);
      lo = bits < lo ? bits : lo;
      hi = bits > hi ? bits : hi;
    };
    take(left);
    take(right);
    take(up);
    take(below);
    rim_lo[i] = lo;
    rim_hi[i] = hi;
    const uint32_t self = (uint32_t)(row * kTileW + lane);
    s_label[self] = hole ? (uint32_t)(row * kTileW + tiles::run_start(links, lane)) : tiles::kNoLabel;
    if (lane == 0) {
      s_links[row] = links;
      s_down[row] = downs;
    }
  }
  __syncthreads();  // the depths are not read again: their LDS becomes the rim minima
  for (int i = threadIdx.x; i < kNodes; i += kBlock) {
    s_record[i] = 0;
    s_lo[i] = rules::kNoRimLo;
    s_hi[i] = rules::kNoRimHi;
  }

  // the hooks
  for (int row = wave; row < TH; row += 4) {
    const uint32_t self = (uint32_t)(row * kTileW + lane);
    const uint64_t links = s_links[row], downs = row + 1 < TH ? s_down[row] : 0;  // the last row's down-links are the border pass's
    if ((tiles::hooking_lanes(links, s_links[row + 1], downs) >> lane) & 1)
      lds_unite(s_label, lds_parent(s_label, self), lds_parent(s_label, self + kTileW));
  }
  __syncthreads();

  // every hole pixel's tile-local root, and the roots' four values
  uint32_t root[TH / 4];
#pragma unroll
  for (int i = 0; i < TH / 4; ++i) {
    const int row = wave + 4 * i;
    const int64_t x = x0 + lane, y = y0 + row;
    const uint32_t self = (uint32_t)(row * kTileW + lane);
    const uint32_t first = lds_parent(s_label, self);
    root[i] = first == tiles::kNoLabel ? tiles::kNoLabel : lds_root(s_label, first);
    if (root[i] == tiles::kNoLabel) continue;
    const uint64_t links = s_links[row];
    if (tiles::run_start(links, lane) == lane) atomicAdd(&s_record[root[i]], (uint32_t)(tiles::run_end(links, lane) - lane + 1));
    if (x == 0 || y == 0 || x == W - 1 || y == H - 1) atomicOr(&s_record[root[i]], rules::kBorderFlag);
    if (rim_lo[i] != rules::kNoRimLo) {
      __hip_atomic_fetch_min(&s_lo[root[i]], rim_lo[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_max(&s_hi[root[i]], rim_hi[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
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
    const bool hole = r != tiles::kNoLabel;
    // a tile-local root's view-local index; it is the smallest of its local hole, since both orders run row by row
    piece.label[at] = hole ? (uint32_t)((y0 + (r >> 6)) * W + x0 + (r & 63)) : tiles::kNoLabel;
    if (hole && r == (uint32_t)(row * kTileW + lane)) {
      piece.record[at] = s_record[r];
      piece.rim_lo[at] = s_lo[r];
      piece.rim_hi[at] = s_hi[r];
    } else {
      piece.record[at] = 0u;
    }
  }
  if (wave == 0) {
    const uint64_t rights = __ballot(lane < TH && (s_links[lane < TH ? lane : 0] >> 63) != 0);
    if (lane == 0) {
      piece.border_down[tile] = s_down[TH - 1];
      piece.border_right[tile] = rights;
    }
  }
}

__global__ __launch_bounds__(kBlock) void holes_merge_kernel(HolesPiece piece, uint64_t plane, uint64_t total) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= total) return;
  const uint32_t word = piece.record[i];
  if (word == 0) return;  // not a tile-local root
  const uint64_t base = i / plane * plane;
  const uint32_t r = (uint32_t)(i - base);
  const uint32_t g = union_find::final_root(piece.label + base, r);
  if (g == r) return;
  __hip_atomic_store(piece.label + base + r, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // an ancestor: others may still pass through r
  atomicAdd(piece.record + base + g, rules::record_count(word));
  if (rules::record_touches_border(word)) atomicOr(piece.record + base + g, rules::kBorderFlag);
  const uint64_t lo = piece.rim_lo[i], hi = piece.rim_hi[i];
  if (lo != rules::kNoRimLo) {
    __hip_atomic_fetch_min(piece.rim_lo + base + g, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(piece.rim_hi + base + g, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The nearest valid pixel from `from` on in steps of `step` along a line of `extent` pixels `stride` apart, or -1 if none shows
// within `limit` pixels or inside the line (neither happens for a pixel of a fillable hole).
__device__ __forceinline__ int64_t nearest_valid(const uint32_t *line, int64_t stride, int64_t from, int64_t step, int64_t extent,
                                                 int64_t limit) {
  int64_t p = from;
  for (int64_t left = limit; left > 0; --left, p += step) {
    if (p < 0 || p >= extent) return -1;
    if (line[p * stride] == tiles::kNoLabel) return p;
  }
  return -1;
}

__global__ __launch_bounds__(kBlock) void holes_output_kernel(HolesPiece piece, int32_t W, int32_t H, double abs_tolerance,
                                                              double rel_tolerance, int64_t max_pixels, TileGrid grid) {
  const int64_t tile = blockIdx.x;
  if (tile >= grid.tiles) return;  // (never: the launch has one workgroup per tile)
  const int64_t tx = tile % grid.across, ty = (tile / grid.across) % grid.down, view = tile / (grid.across * grid.down);
  const size_t plane = (size_t)W * H, base = (size_t)view * plane;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t x = tx * kTileW + lane;
  const int64_t limit_x = rules::walk_limit(max_pixels, W), limit_y = rules::walk_limit(max_pixels, H);
  const uint32_t *const labels = piece.label + base;
  const double *const depths = piece.depth + base;
  for (int row = wave; row < kTileH; row += 4) {
    const int64_t y = ty * kTileH + row;
    if (y >= H) break;  // (the whole wave)
    const bool inside = x < W;
    const size_t at = (size_t)y * W + (size_t)(inside ? x : 0);
    const uint32_t label = inside ? labels[at] : tiles::kNoLabel;
    const bool hole = inside && label != tiles::kNoLabel;
    const uint64_t valid = __ballot(inside && !hole);  // the row's valid pixels inside this tile
    if (!hole) {
      if (inside && piece.out_size) piece.out_size[base + at] = 0;
      continue;  // (a valid pixel keeps its depth: D is the input there)
    }
    const uint32_t g = labels[label];
    const uint32_t word = piece.record[base + g];
    const int64_t size = (int64_t)rules::record_count(word);
    if (piece.out_size) piece.out_size[base + at] = (int32_t)size;
    double value = -1.0;
    bool fillable = size <= max_pixels && !rules::record_touches_border(word);  // (the rim is read for these holes only)
    if (fillable) {  // step 4: depth_holes_rules.h
      const uint64_t lo_bits = piece.rim_lo[base + g], hi_bits = piece.rim_hi[base + g];
      fillable = rules::fillable(word, lo_bits != rules::kNoRimLo, __longlong_as_double((long long)lo_bits),
                                 __longlong_as_double((long long)hi_bits), max_pixels, abs_tolerance, rel_tolerance);
    }
    if (fillable) {
      const int below = rules::nearest_valid_below(valid, lane), above = rules::nearest_valid_above(valid, lane);
      const uint32_t *const row_labels = labels + (size_t)y * W;
      const int64_t xl = below >= 0 ? tx * kTileW + below : nearest_valid(row_labels, 1, tx * kTileW - 1, -1, W, limit_x);
      const int64_t xr = above < kTileW ? tx * kTileW + above : nearest_valid(row_labels, 1, (tx + 1) * kTileW, 1, W, limit_x);
      const int64_t yu = nearest_valid(labels + x, W, y - 1, -1, H, limit_y);
      const int64_t yd = nearest_valid(labels + x, W, y + 1, 1, H, limit_y);
      if (xl >= 0 && xr >= 0 && yu >= 0 && yd >= 0) {  // (always)
        const double dl = depths[(size_t)y * W + (size_t)xl], dr = depths[(size_t)y * W + (size_t)xr];
        const double du = depths[(size_t)yu * W + (size_t)x], dd = depths[(size_t)yd * W + (size_t)x];
        const double span_x = (double)(xr - xl), span_y = (double)(yd - yu);
        const double h = (dl * (double)(xr - x) + dr * (double)(x - xl)) / span_x;
        const double v = (du * (double)(yd - y) + dd * (double)(y - yu)) / span_y;
        value = (h * span_y + v * span_x) / (span_y + span_x);
      }
    }
    piece.depth[base + at] = value;
  }
}

TileGrid tile_grid(int32_t W, int32_t H, int64_t count) {
  TileGrid g;
  g.across = tiles::tiles_across(W);
  g.down = tiles::tiles_down(H, kTileH);
  g.tiles = g.across * g.down * count;
  return g;
}

inline unsigned blocks(uint64_t items) { return (unsigned)((items + kBlock - 1) / kBlock); }

}  // namespace

int64_t holes_tiles(int32_t W, int32_t H, int64_t count) { return tile_grid(W, H, count).tiles; }

hipError_t launch_holes_local(const HolesPiece &piece, double threshold, int32_t W, int32_t H, hipStream_t stream) {
  const TileGrid grid = tile_grid(W, H, piece.count);
  if (grid.tiles > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(holes_local_kernel, dim3((unsigned)grid.tiles), dim3(kBlock), 0, stream, piece, threshold, W, H, grid);
  return hipGetLastError();
}

// the speckle filter's border pass reads a piece's label plane, its border bits and its view count, and nothing else
hipError_t launch_holes_border(const HolesPiece &piece, int32_t W, int32_t H, hipStream_t stream) {
  SpecklePiece as_segments;
  as_segments.depth = nullptr;
  as_segments.cost = nullptr;
  as_segments.label = piece.label;
  as_segments.size = nullptr;
  as_segments.border_down = piece.border_down;
  as_segments.border_right = piece.border_right;
  as_segments.out_size = nullptr;
  as_segments.count = piece.count;
  return launch_speckle_border(as_segments, W, H, SpeckleTuning(), stream);
}

hipError_t launch_holes_merge(const HolesPiece &piece, int32_t W, int32_t H, hipStream_t stream) {
  const uint64_t plane = (uint64_t)W * H, total = plane * (uint64_t)piece.count;
  if ((total + kBlock - 1) / kBlock > 0x7fffffffULL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(holes_merge_kernel, dim3(blocks(total)), dim3(kBlock), 0, stream, piece, plane, total);
  return hipGetLastError();
}

hipError_t launch_holes_output(const HolesPiece &piece, int32_t W, int32_t H, double abs_tolerance, double rel_tolerance,
                               int64_t max_pixels, hipStream_t stream) {
  const TileGrid grid = tile_grid(W, H, piece.count);
  if (grid.tiles > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(holes_output_kernel, dim3((unsigned)grid.tiles), dim3(kBlock), 0, stream, piece, W, H, abs_tolerance, rel_tolerance,
                     max_pixels, grid);
  return hipGetLastError();
}

}  // namespace dmi
