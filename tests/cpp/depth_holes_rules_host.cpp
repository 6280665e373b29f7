// depth_holes_rules_host.cpp -- csrc/depth_holes_rules.h on the CPU, built with AddressSanitizer + UBSan by
// tests/test_depth_holes_rules_host.py: a row's links between hole pixels against a naive loop and, through
// depth_speckle_rules.h's run arithmetic, the runs of holes they stand for; the nearest valid column on either side of every lane
// against naive scans, for all-ones, all-zeros, single-bit and random masks; the record word; the walk limit.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "depth_holes_rules.h"

using namespace dmi::holes_rules;
namespace tiles = dmi::speckle_rules;

static int failed = 0, checked = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    ++checked;                                                   \
    if (!(cond)) {                                               \
      ++failed;                                                  \
      std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); \
    }                                                            \
  } while (0)

static uint64_t next_random(uint64_t *state) {  // splitmix64
  uint64_t z = (*state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

static std::vector<uint64_t> masks() {
  std::vector<uint64_t> m = {0ull, ~0ull, ~0ull >> 1, ~0ull << 1, 0x5555555555555555ull, 0xaaaaaaaaaaaaaaaaull};
  for (int b = 0; b < 64; ++b) {
    m.push_back(uint64_t(1) << b);
    m.push_back(~(uint64_t(1) << b));
  }
  uint64_t state = 4711;
  for (int i = 0; i < 2000; ++i) {
    const uint64_t r = next_random(&state);
    m.push_back(r);
    m.push_back(r | next_random(&state));  // denser
    m.push_back(r & next_random(&state));  // sparser
  }
  return m;
}

static bool bit(uint64_t v, int b) { return ((v >> b) & 1) != 0; }

static void check_links(uint64_t holes, bool right) {
  const uint64_t links = hole_links(holes, right);
  for (int c = 0; c < 64; ++c) {
    const bool next = c < 63 ? bit(holes, c + 1) : right;
    CHECK(bit(links, c) == (bit(holes, c) && next));
  }
  // the runs the speckle rules make of these links are the maximal runs of hole pixels
  for (int lane = 0; lane < 64; ++lane) {
    if (!bit(holes, lane)) continue;
    int s = lane, e = lane;
    while (s > 0 && bit(holes, s - 1)) --s;
    while (e < 63 && bit(holes, e + 1)) ++e;
    CHECK(tiles::run_start(links, lane) == s);
    CHECK(tiles::run_end(links, lane) == e);
  }
}

static void check_nearest(uint64_t valid) {
  for (int lane = 0; lane < 64; ++lane) {
    int below = lane - 1, above = lane + 1;
    while (below >= 0 && !bit(valid, below)) --below;
    while (above < 64 && !bit(valid, above)) ++above;
    CHECK(nearest_valid_below(valid, lane) == below);
    CHECK(nearest_valid_above(valid, lane) == above);
  }
}

int main() {
  for (const uint64_t m : masks()) {
    check_links(m, false);
    check_links(m, true);
    check_nearest(m);
  }

  CHECK(record_count(0) == 0 && !record_touches_border(0));
  CHECK(record_count(kBorderFlag | 5u) == 5 && record_touches_border(kBorderFlag | 5u));
  CHECK(record_count(1u << 30) == (1u << 30) && !record_touches_border(1u << 30));  // the largest view, one hole
  CHECK(((uint64_t)32768 * 32768) <= kCountMask);
  // a sum of counts and ORed flags, in any order, is the count of the whole and the OR of the flags
  uint32_t word = 0;
  for (const uint32_t part : {7u, kBorderFlag | 9u, 100u, kBorderFlag | 1u}) {
    word += record_count(part);
    if (record_touches_border(part)) word |= kBorderFlag;
  }
  CHECK(record_count(word) == 117 && record_touches_border(word));
  CHECK(kNoRimLo > kNoRimHi && kNoRimHi == 0);

  CHECK(walk_limit(0, 640) == 0 && walk_limit(16, 640) == 16 && walk_limit(640, 640) == 640 && walk_limit(641, 640) == 640);
  CHECK(walk_limit(INT64_MAX, 32768) == 32768 && walk_limit(1, 1) == 1);

  std::printf("%d checked, %d failed\n", checked, failed);
  return failed ? 1 : 0;
}
