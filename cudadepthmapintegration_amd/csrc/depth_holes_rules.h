// depth_holes_rules.h -- the rules of dmi_fill_depth_holes that are plain integer arithmetic and that depth_speckle_rules.h does
// not have already (include/dmi.h states the definition, DESIGN.md 8k the kernels): a row's right-links between HOLE pixels from
// its ballot, how a root's pixel count and border flag share one u32, the nearest valid column on either side of a lane inside a
// row's 64 validity bits, and the bound of the output pass's walks.  No HIP types: depth_holes.hip and the host program
// tests/cpp/depth_holes_rules_host.cpp compile the same text.
#pragma once
#include <cstdint>

#include "depth_speckle_rules.h"

namespace dmi {
namespace holes_rules {

// A root's record word: its pixels in the low 31 bits (a view has at most 2^30), bit 31 set iff one of them lies on the image's
// border.  Counts are ADDED to a word, the flag is ORed in: the sum of a view's counts never reaches bit 31.
constexpr uint32_t kBorderFlag = 0x80000000u;
constexpr uint32_t kCountMask = 0x7fffffffu;
DMI_SPECKLE_HD inline uint32_t record_count(uint32_t word) { return word & kCountMask; }
DMI_SPECKLE_HD inline bool record_touches_border(uint32_t word) { return (word & kBorderFlag) != 0; }

// The rim bounds of a root that has no rim pixel yet: the identities of the unsigned minimum and maximum.  (A depth's bit
// pattern is never 0 -- a valid depth is > 0 -- and never all ones, which is a NaN.)
constexpr uint64_t kNoRimLo = ~uint64_t(0);
constexpr uint64_t kNoRimHi = 0;

// Bit c of `holes`: column c of the tile's row is a hole pixel.  The row's links in the sense of depth_speckle_rules.h -- bit c:
// column c and column c + 1 belong to the same run -- with bit 63 taken from the pixel right of the tile.
DMI_SPECKLE_HD inline uint64_t hole_links(uint64_t holes, bool right_of_tile_is_hole) {
  const uint64_t next = (holes >> 1) | (right_of_tile_is_hole ? uint64_t(1) << 63 : 0);
  return holes & next;
}

// Bit c of `valid`: column c of the tile's row is a valid pixel.  The nearest valid column below `lane`, -1 if the row's 64 bits
// hold none; the nearest above it, 64 if they hold none.  lane in [0, 63].
DMI_SPECKLE_HD inline int nearest_valid_below(uint64_t valid, int lane) {
  const uint64_t below = valid & ((uint64_t(1) << lane) - 1);
  return 63 - speckle_rules::count_leading_zeros64(below);
}
DMI_SPECKLE_HD inline int nearest_valid_above(uint64_t valid, int lane) {
  const uint64_t above = lane == 63 ? 0 : valid >> (lane + 1);
  return above ? lane + 1 + speckle_rules::count_trailing_zeros64(above) : 64;
}

// Step 4 of the definition at a hole's final root: `word` is its record, lo and hi the smallest and largest depth on its rim
// (has_rim: it has one).  The product, then the sum, then the difference, each rounded on its own (-ffp-contract=off).  The output
// pass asks this per hole pixel, the resident view set's report (view_set_kernels.hip) once per hole.
DMI_SPECKLE_HD inline bool fillable(uint32_t word, bool has_rim, double lo, double hi, int64_t max_pixels, double abs_tolerance,
                                    double rel_tolerance) {
  if ((int64_t)record_count(word) > max_pixels || record_touches_border(word) || !has_rim) return false;
  const double bound = abs_tolerance + rel_tolerance * lo;
  return hi - lo <= bound;
}

// A pixel of a fillable hole reaches its nearest valid pixel in a row or column within SIZE <= max_pixels steps, and within the
// image: the walk makes at most this many.
DMI_SPECKLE_HD inline int64_t walk_limit(int64_t max_pixels, int32_t extent) { return max_pixels < extent ? max_pixels : extent; }

}  // namespace holes_rules
}  // namespace dmi
