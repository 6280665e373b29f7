// depth_speckle_rules.h -- the rules of dmi_filter_depth_speckles that are plain integer arithmetic (include/dmi.h states the
// definition, DESIGN.md 8j the kernels): the tile a workgroup owns, how many tiles cover a view, where a tile's border links are
// kept and which two pixels a border link joins, and the wave-wide run arithmetic on one row's 64 right-link bits.  No HIP types:
// depth_speckle.hip and the host program tests/cpp/depth_speckle_rules_host.cpp compile the same text.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define DMI_SPECKLE_HD __host__ __device__
#else
#define DMI_SPECKLE_HD
#endif

namespace dmi {
namespace speckle_rules {

constexpr int kTileWidth = 64;   // pixels: one lane of a wave per column, so a row's right-links are one ballot
constexpr int kTileHeight = 32;  // rows (64 x 16 and 64 x 64 are the tuning build's alternatives)
constexpr int kWorkgroup = 256;  // lanes: four waves, wave w owns the tile's rows w, w + 4, ...
constexpr int kBorderLanes = 128;  // lanes the border pass spends on a tile: its last row's 64 columns, then up to 64 rows

constexpr uint32_t kNoLabel = 0xffffffffu;  // the label of a pixel that is not valid; no pixel has this index (W * H <= 2^30)

DMI_SPECKLE_HD inline int64_t tiles_across(int32_t W) { return ((int64_t)W + kTileWidth - 1) / kTileWidth; }
DMI_SPECKLE_HD inline int64_t tiles_down(int32_t H, int tile_height = kTileHeight) { return ((int64_t)H + tile_height - 1) / tile_height; }
DMI_SPECKLE_HD inline int64_t tiles_per_view(int32_t W, int32_t H, int tile_height = kTileHeight) {
  return tiles_across(W) * tiles_down(H, tile_height);
}

// Bit c of a row's link mask says that column c of the tile is LINKED to column c + 1 (bit 63: across the tile's right border).
// The run of lane `lane` starts one above the highest clear bit below the lane, at 0 if there is none: one mask, one complement,
// one count of leading zeros.
DMI_SPECKLE_HD inline int count_leading_zeros64(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __clzll((long long)v);
#else
  return v ? __builtin_clzll(v) : 64;
#endif
}
DMI_SPECKLE_HD inline int count_trailing_zeros64(uint64_t v) {  // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return __ffsll((unsigned long long)v) - 1;
#else
  return __builtin_ctzll(v);
#endif
}
DMI_SPECKLE_HD inline int run_start(uint64_t links, int lane) {
  const uint64_t below = (uint64_t(1) << lane) - 1;  // lane in [0, 63]
  const uint64_t breaks = ~links & below;
  return 64 - count_leading_zeros64(breaks);
}
// the last column of the run that holds `lane`, inside the tile: the lowest clear bit at or above the lane, bit 63 taken as clear
DMI_SPECKLE_HD inline int run_end(uint64_t links, int lane) {
  const uint64_t breaks = (~links | (uint64_t(1) << 63)) >> lane;
  return lane + count_trailing_zeros64(breaks);
}

// A lane whose down-link is set hooks its run to the run below unless the lane to its left is in the same run on both rows and
// hooks already: then the two runs are united by that lane.  links = this row's right-links, links_below = the next row's,
// down = this row's down-links.  Bit c of the result: lane c hooks.
DMI_SPECKLE_HD inline uint64_t hooking_lanes(uint64_t links, uint64_t links_below, uint64_t down) {
  return down & ~((down & links & links_below) << 1);
}

// Where the local pass leaves a tile's border links for the border pass: one u64 per tile for the down-links of its last row
// (bit c: column c), one u64 per tile for the right-links of its last column (bit r: row r; tile heights up to 64).  The tile
// index counts the tiles of a piece's views row by row: ((view * tiles_down) + ty) * tiles_across + tx.
DMI_SPECKLE_HD inline int64_t tile_index(int64_t view, int64_t ty, int64_t tx, int32_t W, int32_t H, int tile_height = kTileHeight) {
  return (view * tiles_down(H, tile_height) + ty) * tiles_across(W) + tx;
}

// The two pixels (view-local indices y * W + x) that border lane k of tile (tx, ty) joins, or false if the lane stands for no
// pair inside the image.  k < 64: column k of the tile's last row and the pixel below it; 64 <= k < 64 + tile_height: row k - 64
// of the tile's last column and the pixel to its right.
DMI_SPECKLE_HD inline bool border_pair(int64_t tx, int64_t ty, int k, int32_t W, int32_t H, int tile_height, uint32_t *a, uint32_t *b) {
  int64_t x, y;
  if (k < 0 || k >= kTileWidth + tile_height) return false;
  if (k < kTileWidth) {
    x = tx * kTileWidth + k;
    y = ty * tile_height + tile_height - 1;
    if (x >= W || y + 1 >= H) return false;
    *a = (uint32_t)(y * W + x);
    *b = (uint32_t)((y + 1) * W + x);
  } else {
    x = tx * kTileWidth + kTileWidth - 1;
    y = ty * tile_height + (k - kTileWidth);
    if (x + 1 >= W || y >= H) return false;
    *a = (uint32_t)(y * W + x);
    *b = (uint32_t)(y * W + x + 1);
  }
  return true;
}

}  // namespace speckle_rules
}  // namespace dmi
