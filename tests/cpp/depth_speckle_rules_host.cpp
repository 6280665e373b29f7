// depth_speckle_rules_host.cpp -- csrc/depth_speckle_rules.h on the CPU, built with AddressSanitizer + UBSan by
// tests/test_depth_speckle_rules_host.py: the run arithmetic on a row's 64 link bits against naive loops, for all-ones, all-zeros,
// single-bit and random masks at every lane; which lanes hook, against the union of runs they must produce; the tile counts and
// the border pairs for widths and heights at and around the tile sizes and at the largest image.
#include <cstdint>
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "depth_speckle_rules.h"

using namespace dmi::speckle_rules;

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

static int naive_run_start(uint64_t links, int lane) {
  int s = lane;
  while (s > 0 && ((links >> (s - 1)) & 1)) --s;
  return s;
}
static int naive_run_end(uint64_t links, int lane) {
  int e = lane;
  while (e < 63 && ((links >> e) & 1)) ++e;
  return e;
}

static void check_mask(uint64_t links) {
  for (int lane = 0; lane < 64; ++lane) {
    CHECK(run_start(links, lane) == naive_run_start(links, lane));
    CHECK(run_end(links, lane) == naive_run_end(links, lane));
  }
}

static std::vector<uint64_t> masks() {
  std::vector<uint64_t> m = {0ull, ~0ull, ~0ull >> 1, ~0ull << 1, 0x5555555555555555ull, 0xaaaaaaaaaaaaaaaaull};
  for (int b = 0; b < 64; ++b) {
    m.push_back(uint64_t(1) << b);
    m.push_back(~(uint64_t(1) << b));
  }
  uint64_t state = 12345;
  for (int i = 0; i < 2000; ++i) {
    const uint64_t r = next_random(&state);
    m.push_back(r);
    m.push_back(r | next_random(&state));  // denser: long runs
    m.push_back(r & next_random(&state));  // sparser
  }
  return m;
}

static void runs() {
  CHECK(count_leading_zeros64(0) == 64 && count_leading_zeros64(1) == 63 && count_leading_zeros64(~0ull) == 0);
  CHECK(count_trailing_zeros64(1) == 0 && count_trailing_zeros64(uint64_t(1) << 63) == 63);
  for (const uint64_t m : masks()) check_mask(m);
}

// The hooks of one pair of rows must unite exactly the pairs (run above, run below) that some set down-link joins, and no lane
// hooks a pair that the lane to its left already hooks.
static void hooks() {
  uint64_t state = 777;
  std::vector<uint64_t> m = masks();
  for (size_t i = 0; i + 2 < m.size(); i += 3) {
    const uint64_t links = m[i], below = m[i + 1], down = m[i + 2] | (i % 2 ? next_random(&state) : 0);
    const uint64_t hook = hooking_lanes(links, below, down);
    CHECK((hook & ~down) == 0);  // only lanes whose down-link is set hook
    std::set<std::pair<int, int>> wanted, hooked;
    int redundant = 0;
    for (int lane = 0; lane < 64; ++lane) {
      const std::pair<int, int> pair(naive_run_start(links, lane), naive_run_start(below, lane));
      if ((down >> lane) & 1) wanted.insert(pair);
      if ((hook >> lane) & 1) {
        if (lane > 0 && ((hook >> (lane - 1)) & 1) && pair == std::make_pair(naive_run_start(links, lane - 1), naive_run_start(below, lane - 1)))
          ++redundant;
        hooked.insert(pair);
      }
    }
    CHECK(wanted == hooked);
    CHECK(redundant == 0);
  }
}

static void tiles() {
  const int32_t sizes[] = {1, 63, 64, 65, 32768};
  const int heights[] = {16, 32, 64};
  for (const int32_t W : sizes) {
    CHECK(tiles_across(W) == (W + 63) / 64);
    CHECK(tiles_across(W) * kTileWidth >= W && (tiles_across(W) - 1) * kTileWidth < W);
    for (const int32_t H : sizes)
      for (const int th : heights) {
        CHECK(tiles_down(H, th) * th >= H && (tiles_down(H, th) - 1) * th < H);
        CHECK(tiles_per_view(W, H, th) == tiles_across(W) * tiles_down(H, th));
        const int64_t across = tiles_across(W), down = tiles_down(H, th);
        // tile indices count the tiles of consecutive views without a gap
        CHECK(tile_index(0, 0, 0, W, H, th) == 0);
        CHECK(tile_index(0, down - 1, across - 1, W, H, th) == across * down - 1);
        CHECK(tile_index(3, 0, 0, W, H, th) == 3 * across * down);
        CHECK(tile_index(2, down - 1, across - 1, W, H, th) + 1 == tile_index(3, 0, 0, W, H, th));
        // the border pairs of the corner tiles and one in the middle: inside the image, neighbours, and across the tile's border
        const int64_t txs[] = {0, across / 2, across - 1}, tys[] = {0, down / 2, down - 1};
        for (const int64_t tx : txs)
          for (const int64_t ty : tys)
            for (int k = -1; k <= kBorderLanes; ++k) {
              uint32_t a = 0xdeadbeef, b = 0xdeadbeef;
              const bool ok = border_pair(tx, ty, k, W, H, th, &a, &b);
              bool want = false;
              int64_t x = 0, y = 0, x2 = 0, y2 = 0;
              if (k >= 0 && k < 64) {
                x = x2 = tx * 64 + k, y = ty * th + th - 1, y2 = y + 1;
                want = x < W && y2 < H;
              } else if (k >= 64 && k < 64 + th) {
                x = tx * 64 + 63, x2 = x + 1, y = y2 = ty * th + (k - 64);
                want = x2 < W && y < H;
              }
              CHECK(ok == want);
              if (ok) {
                CHECK((int64_t)a == y * W + x && (int64_t)b == y2 * W + x2);
                CHECK((int64_t)b < (int64_t)W * H && a < b);
              } else {
                CHECK(a == 0xdeadbeef && b == 0xdeadbeef);  // a refused lane writes nothing
              }
            }
      }
  }
  CHECK(kTileHeight % 4 == 0 && kTileWidth == 64 && kWorkgroup == 256 && kBorderLanes >= kTileWidth + 64);
  CHECK((uint64_t)32768 * 32768 <= (uint64_t)1 << 30 && kNoLabel >= ((uint64_t)1 << 30));  // no pixel index is kNoLabel
}

int main() {
  runs();
  hooks();
  tiles();
  std::printf("%d checked, %d failed\n", checked, failed);
  return failed ? 1 : 0;
}
