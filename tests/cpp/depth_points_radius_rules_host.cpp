// depth_points_radius_rules_host.cpp -- csrc/depth_points_radius_rules.h on the CPU, built with AddressSanitizer + UBSan by
// tests/test_depth_points_radius_rules_host.py: the accepted radii, the cell-size rule at the 2^21 edge and with zero or infinite
// extent on an axis, the work units' heads, the clamped row ranges against a plain walk over small grids, the completeness of the
// 27-cell search on adversarial pairs, and the filtered cloud's bytes.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "depth_points_radius_rules.h"

using namespace dmi::radius_rules;

static int failed = 0, checked = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    ++checked;                                                   \
    if (!(cond)) {                                               \
      ++failed;                                                  \
      std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); \
    }                                                            \
  } while (0)

static void radii() {
  CHECK(radius_accepted(1.0) && radius_accepted(1e-3) && radius_accepted(1e150) && radius_accepted(1.5e-154));
  CHECK(!radius_accepted(0.0) && !radius_accepted(-1.0) && !radius_accepted(NAN) && !radius_accepted(INFINITY) && !radius_accepted(-INFINITY));
  CHECK(!radius_accepted(1e-160) && !radius_accepted(1e-200) && !radius_accepted(1e155) && !radius_accepted(1e308));
  CHECK(!radius_accepted(5e-324));
}

static void cell_sizes() {
  // inside the limit: the radius with its slack, whatever the extents are (zero on an axis included)
  const double flat[3] = {3.0, 0.0, 1.5};
  CHECK(cell_size_of(0.1, flat) == 0.1 * kCellSlack && cell_size_of(0.1, flat) > 0.1);
  CHECK(bins_of_extent(0.0, cell_size_of(0.1, flat)) == 1 && bins_of_extent(3.0, cell_size_of(0.1, flat)) == 30);
  const double none[3] = {0.0, 0.0, 0.0};
  CHECK(cell_size_of(1e-3, none) == 1e-3 * kCellSlack);
  // at the edge: the smallest h that keeps every axis within 2^21 bins, and not one ulp less
  for (double extent : {1.0, 3.0, 0.7, 1234.5678, 1e7, 4.5e8}) {
    const double e[3] = {extent * 0.25, extent, 0.0};
    const double h = cell_size_of(1e-9, e);
    CHECK(h > 1e-9 * kCellSlack);
    CHECK(bins_of_extent(extent, h) == kMaxBins && bins_of_extent(extent * 0.25, h) <= kMaxBins && bins_of_extent(0.0, h) == 1);
    CHECK(!(std::floor(extent / std::nextafter(h, 0.0)) < 2097152.0));
    // a radius just large enough needs no enlargement
    const double enough = extent / 2097151.0;
    CHECK(cell_size_of(enough, e) == enough * kCellSlack);
  }
  // one stray at 1e7 with a radius of 1e-3: larger cells, not a refusal
  const double stray[3] = {1e7, 2.0, 2.0};
  const double h = cell_size_of(1e-3, stray);
  CHECK(h > 4.0 && h < 5.0 && bins_of_extent(1e7, h) == kMaxBins && bins_of_extent(2.0, h) == 1);
  // an extent that overflowed: one bin on that axis, the others by the rule
  const double over[3] = {INFINITY, 10.0, 0.0};
  CHECK(cell_size_of(1.0, over) == kCellSlack && bins_of_extent(INFINITY, kCellSlack) == 1 && bins_of_extent(10.0, kCellSlack) == 10);
  CHECK(bin_of(1.7e308, -1.7e308, 1.0, 1) == 0 && bin_of(5.0, 5.0, 1.0, 1) == 0 && bin_of(7.5, 5.0, 1.0, 4) == 2);
}

static void units() {
  const uint64_t n0 = 5;
  // keys of sorted positions: rows 0, 0, 0, 1, 1, 3
  const uint64_t keys[6] = {0, 0, 4, 5, 9, 15};
  for (uint32_t group : {1u, 2u, 4u, 64u}) {
    for (uint64_t i = 0; i < 6; ++i) {
      const bool want = i == 0 || i % group == 0 || keys[i] / n0 != keys[i - 1] / n0;
      CHECK(unit_head(i, keys[i], i ? keys[i - 1] : 0, n0, group) == want);
    }
  }
  CHECK(unit_head(0, 0, 0, n0, 64) && !unit_head(1, 0, 0, n0, 64) && unit_head(3, 5, 4, n0, 64) && unit_head(64, 1, 1, n0, 64));
  CHECK(kDefaultGroupPoints >= 1 && kDefaultGroupPoints <= kMaxGroupPoints && kMaxGroupPoints == 64);
}

// every unit a single cell, then wider spans: the nine ranges of a span hold every cell within +-1 of any of its cells exactly
// once, no cell twice, and no cell beyond +-1 of the span in b_0 or of the row in b_1, b_2
static void row_ranges() {
  const uint64_t shapes[][3] = {{1, 1, 1}, {2, 1, 1}, {1, 2, 3}, {2, 2, 2}, {3, 1, 4}, {4, 3, 2}, {5, 4, 3}, {1, 1, 5}};
  for (const auto &n : shapes) {
    const uint64_t n0 = n[0], n1 = n[1], n2 = n[2];
    for (uint64_t b2 = 0; b2 < n2; ++b2)
      for (uint64_t b1 = 0; b1 < n1; ++b1)
        for (uint64_t lo = 0; lo < n0; ++lo)
          for (uint64_t hi = lo; hi < n0; ++hi) {
            std::map<uint64_t, int> seen;
            for (int t = 0; t < 9; ++t) {
              uint64_t from = 0, to = 0;
              if (!row_key_range(lo, hi, b1, b2, t % 3 - 1, t / 3 - 1, n0, n1, n2, &from, &to)) continue;
              CHECK(from <= to && to < n0 * n1 * n2);
              for (uint64_t key = from; key <= to; ++key) ++seen[key];
            }
            // the plain walk
            uint64_t expected = 0;
            for (int64_t c2 = (int64_t)b2 - 1; c2 <= (int64_t)b2 + 1; ++c2)
              for (int64_t c1 = (int64_t)b1 - 1; c1 <= (int64_t)b1 + 1; ++c1)
                for (int64_t c0 = (int64_t)lo - 1; c0 <= (int64_t)hi + 1; ++c0) {
                  if (c0 < 0 || c1 < 0 || c2 < 0 || c0 >= (int64_t)n0 || c1 >= (int64_t)n1 || c2 >= (int64_t)n2) continue;
                  ++expected;
                  const auto it = seen.find(dmi::thin_rules::key_of((uint64_t)c0, (uint64_t)c1, (uint64_t)c2, n0, n1));
                  CHECK(it != seen.end() && it->second == 1);
                }
            CHECK(seen.size() == expected);
          }
  }
}

// |delta| equal to the radius and one ulp either side, at small and geo-referenced offsets, with points on cell faces and on the
// upper bound: wherever d2 <= r2 the bins differ by at most 1
static void completeness() {
  int near_pairs = 0, face_pairs = 0;
  for (double offset : {0.0, 5e6, 4.5e8}) {
    for (double radius : {1e-3, 0.05, 0.1, 0.3, 1.0, 7.0}) {
      for (double extent : {0.0, 1.0, 37.0, 1000.0, 3e6}) {
        const double lo = offset, hi = offset + extent + 3 * radius;
        const double e[3] = {hi - lo, 0.0, 0.0};
        const double h = cell_size_of(radius, e);
        const uint64_t n = bins_of_extent(e[0], h);
        CHECK(n >= 1 && n <= kMaxBins);
        std::vector<double> starts = {lo, hi - radius, std::nextafter(hi - radius, lo), lo + extent * 0.5};
        for (uint64_t m : {uint64_t(1), uint64_t(2), n / 2, n > 2 ? n - 2 : 1}) {  // on and next to the faces m h
          const double face = lo + (double)m * h;
          for (double x : {face, std::nextafter(face, lo), std::nextafter(face, hi), face - radius, std::nextafter(face - radius, lo)})
            if (x >= lo && x + radius <= hi) starts.push_back(x), ++face_pairs;
        }
        for (double x : starts) {
          if (!(x >= lo)) continue;
          for (double step : {radius, std::nextafter(radius, 0.0), std::nextafter(radius, INFINITY)}) {
            for (double y : {x + step, std::nextafter(x + step, lo), std::nextafter(x + step, hi + 1.0)}) {
              if (!(y <= hi)) continue;
              const double d = y - x, d2 = (d * d + 0.0 * 0.0) + 0.0 * 0.0;
              const uint64_t bx = bin_of(x, lo, h, n), by = bin_of(y, lo, h, n);
              CHECK(bx < n && by < n);
              if (d2 <= radius * radius) {
                ++near_pairs;
                CHECK(by - bx <= 1);
              }
            }
          }
        }
      }
    }
  }
  CHECK(near_pairs > 500 && face_pairs > 100);
}

static void bytes() {
  uint64_t at = 0, all = 0;
  CHECK(filtered_bytes(0, 48, &at, &all) && at == 0 && all == 0);
  CHECK(filtered_bytes(1267, 48, &at, &all) && at == 48 * 1267 && all == 52 * 1267);
  CHECK(filtered_bytes(uint64_t(1) << 33, 52, &at, &all) && at == (uint64_t(52) << 33) && all == (uint64_t(56) << 33));
  CHECK(filtered_bytes(~uint64_t(0) / 52, 48, &at, &all) && !filtered_bytes(~uint64_t(0) / 52 + 1, 48, &at, &all));
  dmi::thin_rules::Layout layout;
  CHECK(dmi::thin_rules::layout_of(1000, &layout) && filtered_bytes(1000, 48, &at, &all) && at == layout.members);  // (a built cloud has no members)
  CHECK(filtered_bytes(1000, 52, &at, &all) && at == layout.bytes);
  CHECK(scratch_bytes(1) == 32 + 8 + 8 + 24 + 4 + 128 && scratch_bytes(1000) / 1000 == 56);
}

int main() {
  radii();
  cell_sizes();
  units();
  row_ranges();
  completeness();
  bytes();
  std::printf("%d checked, %d failed\n", checked, failed);
  return failed ? 1 : 0;
}
