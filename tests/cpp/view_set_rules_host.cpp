// view_set_rules_host.cpp -- csrc/view_set_rules.h on the CPU, stand-alone: built with AddressSanitizer and UBSan by
// tests/test_view_set_host.py and run.  The piece partition with its tails, a view larger than the piece, the even pieces of an
// odd image, the byte estimates with their overflow guard, the peel before a 16-byte boundary and the report arithmetic.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "view_set_rules.h"

static int checks = 0, failed = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    ++checks;                                                    \
    if (!(cond)) {                                               \
      ++failed;                                                  \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);      \
    }                                                            \
  } while (0)

namespace rules = dmi::view_set_rules;

namespace {

// the pieces cover [0, n) once, in order, none empty, none above `per`
void check_partition(int64_t n, int64_t per) {
  const int64_t count = rules::piece_count(n, per);
  int64_t next = 0;
  std::vector<int> seen((size_t)n, 0);
  for (int64_t q = 0; q < count; ++q) {
    const rules::Piece p = rules::piece_at(n, per, q);
    CHECK(p.first == next && p.count >= 1 && p.count <= per);
    CHECK(q + 1 == count || p.count == per);
    for (int64_t m = p.first; m < p.first + p.count; ++m) seen[(size_t)m] += 1;
    next = p.first + p.count;
  }
  CHECK(next == n);
  for (const int s : seen) CHECK(s == 1);
}

}  // namespace

int main() {
  // the partition: 5 views in pieces of 2 are 2, 2, 1; every tail from n = 1 to 40
  const uint64_t plane_bytes = uint64_t(150) * 70 * 8;
  CHECK(rules::piece_views(2 * plane_bytes, 150, 70, 5) == 2);
  CHECK(rules::piece_count(5, 2) == 3);
  CHECK(rules::piece_at(5, 2, 2).first == 4 && rules::piece_at(5, 2, 2).count == 1);
  CHECK(rules::piece_views(plane_bytes, 150, 70, 5) == 1);
  CHECK(rules::piece_views(2 * plane_bytes - 1, 150, 70, 5) == 1);
  CHECK(rules::piece_views(1000 * plane_bytes, 150, 70, 5) == 5);
  for (int64_t n = 1; n <= 40; ++n)
    for (int64_t per = 1; per <= n; ++per) check_partition(n, per);
  // a view larger than the piece goes whole; the default is the context-free calls' 256 MiB
  CHECK(rules::piece_views(1, 150, 70, 5) == 1);
  CHECK(rules::piece_views(rules::kDefaultPieceBytes, 32768, 32768, 3) == 1);
  CHECK(rules::piece_views(rules::kDefaultPieceBytes, 1280, 720, 256) == (int64_t)((uint64_t(256) << 20) / (uint64_t(1280) * 720 * 8)));
  CHECK(rules::piece_views(rules::kDefaultPieceBytes, 640, 480, 64) == 64);
  // an odd image: pieces of an even number of views, two at least, so that each starts at an even pixel
  CHECK(rules::piece_views(1, 3, 3, 5) == 2);
  CHECK(rules::piece_views(3 * 72, 3, 3, 7) == 2);
  CHECK(rules::piece_views(5 * 72, 3, 3, 7) == 4);
  CHECK(rules::piece_views(5 * 72, 3, 3, 1) == 1);
  for (int64_t per = 1; per <= 9; ++per) {
    const int64_t views = rules::piece_views((uint64_t)per * 72, 3, 3, 9);
    for (int64_t q = 0; q < rules::piece_count(9, views); ++q) CHECK(rules::piece_at(9, views, q).first * 9 % 2 == 0);
  }

  // the bytes: 16 per pixel and view resident, 12 more at the peak of a consistency pass
  uint64_t bytes = 7;
  CHECK(rules::resident_bytes(256, 1280, 720, &bytes) && bytes == uint64_t(256) * 1280 * 720 * 16);
  CHECK(rules::peak_bytes(256, 1280, 720, rules::kDefaultPieceBytes, &bytes) && bytes == uint64_t(256) * 1280 * 720 * 28);
  CHECK(rules::peak_bytes(1, 1280, 720, rules::kDefaultPieceBytes, &bytes) && bytes == uint64_t(1280) * 720 * (16 + 28));
  bytes = 7;
  CHECK(!rules::resident_bytes(~uint64_t(0) / 16, 32768, 32768, &bytes) && bytes == 7);
  CHECK(!rules::resident_bytes((uint64_t(1) << 34) / 16 + 1, 32768, 32768, &bytes) && bytes == 7);
  CHECK(rules::resident_bytes((uint64_t(1) << 34) / 16 - 1, 32768, 32768, &bytes));
  CHECK(!rules::peak_bytes(~uint64_t(0), 1, 1, 1, &bytes));
  uint64_t v = 3;
  CHECK(!rules::checked_mul(~uint64_t(0), 2, &v) && v == 3 && rules::checked_mul(0, ~uint64_t(0), &v) && v == 0);
  CHECK(!rules::checked_add(~uint64_t(0), 1, &v) && rules::checked_add(~uint64_t(0) - 1, 1, &v) && v == ~uint64_t(0));
  CHECK(rules::scratch_bytes_per_pixel(rules::kHoles, true, false) == 28 && rules::scratch_bytes_per_pixel(rules::kSpeckles, false, false) == 8);
  CHECK(rules::scratch_bytes_per_pixel(rules::kSmooth, true, true) == 12 && rules::scratch_bytes_per_pixel(rules::kIngest, false, false) == 16);

  // the peel: doubles stand 0 or 1 before a boundary, ints 0 to 3
  CHECK(rules::elements_before_16(0x1000, 8) == 0 && rules::elements_before_16(0x1008, 8) == 1);
  for (uint64_t a = 0; a < 64; a += 4) CHECK((a + 4 * rules::elements_before_16(a, 4)) % 16 == 0 && rules::elements_before_16(a, 4) < 4);

  // the report: groups for the two labelling steps only, the tap sum for the smoothing only
  const rules::Counters c = {100, 90, 10, 555, 7, 3};
  const rules::Report speckles = rules::make_report(rules::kSpeckles, c), smooth = rules::make_report(rules::kSmooth, c);
  const rules::Report consistency = rules::make_report(rules::kConsistency, c), holes = rules::make_report(rules::kHoles, c);
  CHECK(speckles.valid_before == 100 && speckles.valid_after == 90 && speckles.changed == 10);
  CHECK(speckles.groups == 7 && speckles.groups_kept == 3 && speckles.aux_sum == 0);
  CHECK(holes.groups == 7 && holes.groups_kept == 3 && holes.aux_sum == 0);
  CHECK(smooth.groups == 0 && smooth.groups_kept == 0 && smooth.aux_sum == 555 && smooth.changed == 10);
  CHECK(consistency.groups == 0 && consistency.groups_kept == 0 && consistency.aux_sum == 0 && consistency.valid_after == 90);

  std::printf("%d checks, %d failed\n", checks, failed);
  return failed ? 1 : 0;
}
