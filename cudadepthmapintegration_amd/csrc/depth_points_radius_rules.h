// depth_points_radius_rules.h -- the rules of dmi_count_point_neighbors / dmi_views_filter_points_radius that are plain arithmetic
// (include/dmi.h states the definition, DESIGN.md 8p the kernels and the proof): which radii are accepted, the cell size of the
// search grid and its bins, where a work unit of the count kernel starts, the key ranges of the nine rows a unit searches, and the
// bytes of the filtered cloud.  No HIP types: the kernels of depth_points_radius.hip and the host program
// tests/cpp/depth_points_radius_rules_host.cpp compile the same text.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>

#include "depth_points_thin_rules.h"

namespace dmi {
namespace radius_rules {

constexpr int kBlock = thin_rules::kBlock;
constexpr uint64_t kMaxBins = thin_rules::kMaxBins;
constexpr uint64_t kMaxPoints = thin_rules::kMaxPoints;

// ---- the radius ----
// accepted: finite, > 0, and its square a normal positive number (neither 0, subnormal nor infinite)
inline bool radius_accepted(double radius) {
  const double r2 = radius * radius;
  return radius > 0.0 && r2 >= std::numeric_limits<double>::min() && r2 <= std::numeric_limits<double>::max();
}

// ---- the search grid ----
// A cell is wider than the radius by the factor 1 + 2^-10: two points with d2 <= r2 then lie in the same or in adjacent bins on
// every axis however the quotients round.  The product rounds once; its error is far below the slack.
constexpr double kCellSlack = 1.0 + 1.0 / 1024.0;

// the bins of an axis of extent e = hi - lo (rounded) at cell size h: floor(e / h) + 1, as the thinning has them.  An extent that
// is not finite (hi - lo overflows) gives the axis ONE bin: every point is in bin 0 there, which is a superset as good as any.
DMI_THIN_HD inline uint64_t bins_of_extent(double extent, double h) {
  const double q = floor(extent / h);
  return q >= 0.0 && q < 2097152.0 ? (uint64_t)q + 1 : 1;
}
DMI_THIN_HD inline bool extent_is_finite(double extent) { return extent - extent == 0.0; }

// h = max(radius * (1 + 2^-10), the smallest h for which every axis of finite extent has at most 2^21 bins): a stray far away
// makes the cells larger, which costs time and nothing else
inline double cell_size_of(double radius, const double extent[3]) {
  double h = radius * kCellSlack;
  for (int d = 0; d < 3; ++d) {
    const double e = extent[d];
    if (!extent_is_finite(e) || std::floor(e / h) < 2097152.0) continue;
    double least = e / 2097152.0;
    if (least > h) h = least;
    while (!(std::floor(e / h) < 2097152.0)) h = std::nextafter(h, std::numeric_limits<double>::infinity());
  }
  return h;
}

// the bin of a coordinate on an axis of n bins: 0 on an axis of one bin, whatever the quotient would be
DMI_THIN_HD inline uint64_t bin_of(double x, double lo, double h, uint64_t n) {
  if (n == 1) return 0;
  const double q = floor((x - lo) / h);  // 0 <= q <= n - 1: lo <= x <= hi and both roundings are monotone
  return (uint64_t)q;
}

// ---- the count kernel's work units ----
// A unit is a run of consecutive sorted positions within one (b_1, b_2) row, of at most `group` points (1 <= group <= 64): a wave
// takes a unit, a lane each point.  Position i starts a unit iff it is the first, a multiple of `group`, or in another row than
// position i - 1.  row = key / n_0.
constexpr uint32_t kMaxGroupPoints = 64;
constexpr uint32_t kDefaultGroupPoints = 64;
DMI_THIN_HD inline bool unit_head(uint64_t i, uint64_t key, uint64_t key_before, uint64_t n0, uint32_t group) {
  return i == 0 || i % group == 0 || key / n0 != key_before / n0;
}

// The keys [*lo, *hi] of the row (b_1 + d1, b_2 + d2) that a unit spanning bins b0_min .. b0_max of row (b_1, b_2) searches:
// b_0 from b0_min - 1 to b0_max + 1, clamped to the grid -- an unclamped range would run into the neighbouring row and test a
// candidate twice.  false: the row lies outside the grid.
DMI_THIN_HD inline bool row_key_range(uint64_t b0_min, uint64_t b0_max, uint64_t b1, uint64_t b2, int d1, int d2, uint64_t n0, uint64_t n1,
                                      uint64_t n2, uint64_t *lo, uint64_t *hi) {
  if ((d1 < 0 && b1 == 0) || (d1 > 0 && b1 + 1 >= n1) || (d2 < 0 && b2 == 0) || (d2 > 0 && b2 + 1 >= n2)) return false;
  const uint64_t row = (uint64_t)((int64_t)b2 + d2) * n1 + (uint64_t)((int64_t)b1 + d1);
  *lo = row * n0 + (b0_min > 0 ? b0_min - 1 : 0);
  *hi = row * n0 + (b0_max + 1 < n0 ? b0_max + 1 : n0 - 1);
  return true;
}

// ---- the filtered cloud: the arrays of the input cloud's layout for Q points (48 Q bytes of a built cloud, 52 Q of a thinned
// one) and neighbors u32[Q] behind them ----
DMI_THIN_HD inline bool filtered_bytes(uint64_t points, uint64_t bytes_per_point, uint64_t *neighbors_offset, uint64_t *bytes) {
  if (points > ~uint64_t(0) / (bytes_per_point + 4)) return false;
  *neighbors_offset = bytes_per_point * points;
  *bytes = (bytes_per_point + 4) * points;
  return true;
}

// ---- what a call holds on the device beside the cloud it reads and the result it builds: two key arrays of P + 1 u64 (the unit
// heads and ranks, then the kept flags and output numbers, live in them), two id arrays, the units' first positions, the
// coordinates in sorted order as three planes, the counts in input order, and 16 counters: 56 bytes a point ----
DMI_THIN_HD inline uint64_t scratch_bytes(uint64_t points) {
  return 2 * 8 * (points + 1) + 2 * 4 * points + 4 * (points + 1) + 24 * points + 4 * points + 16 * 8;
}

}  // namespace radius_rules
}  // namespace dmi
