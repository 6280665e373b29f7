// win_pair_index of csrc/fusion_launch_rules.h -- where a (brick, view) pair's entry lies in the window-pair table -- checked
// exhaustively on small tables (tests/test_winpair_index_host.py builds this with AddressSanitizer and UBSan and runs it): a
// bijection onto [0, bricks * pitch), a brick's 32 views of a block side by side, block b of brick k at (b * bricks + k) * 32.
// Every failed line is printed, the exit status is their number.
#include "fusion_launch_rules.h"

#include <cstdio>
#include <vector>

using namespace dmi;

static int failures = 0;
#define EXPECT(cond)                                                                                  \
  do {                                                                                                \
    if (!(cond)) {                                                                                    \
      if (failures < 50) std::printf("line %d (bricks %lld, pitch %d): %s\n", __LINE__, (long long)bricks, pitch, #cond); \
      ++failures;                                                                                     \
    }                                                                                                 \
  } while (0)

static void check_table(int64_t bricks, int pitch) {
  const int64_t entries = bricks * pitch;
  std::vector<unsigned char> hit((size_t)entries, 0);
  for (int64_t k = 0; k < bricks; ++k) {
    for (int v = 0; v < pitch; ++v) {
      const int64_t e = win_pair_index(k, v, bricks);
      EXPECT(e >= 0 && e < entries);
      if (e < 0 || e >= entries) continue;
      EXPECT(hit[(size_t)e] == 0);  // injective; with as many pairs as entries, onto
      hit[(size_t)e] = 1;
      if ((v & 31) == 0)
        EXPECT(e == ((int64_t)(v / 32) * bricks + k) * 32);  // block b of brick k
      else
        EXPECT(e == win_pair_index(k, v - 1, bricks) + 1);  // a block's views are consecutive
    }
  }
  int64_t n_hit = 0;
  for (unsigned char h : hit) n_hit += h;
  EXPECT(n_hit == entries);
}

int main() {
  static_assert(kWinPairBlockViews == 32, "the fusion kernel reads 32 views of a brick as one piece");
  const int64_t brick_counts[] = {1, 63, 64, 135, 4097};
  const int pitches[] = {64, 128};
  for (int64_t bricks : brick_counts)
    for (int pitch : pitches) {
      check_table(bricks, pitch);
      // every pitch the class table takes is a whole number of blocks
      EXPECT(class_table_pitch(pitch) % kWinPairBlockViews == 0 && class_table_pitch(pitch - 1) % kWinPairBlockViews == 0);
    }
  {
    // a table beyond 2^31 entries: the index does not wrap (the last brick's last view is the table's last entry)
    const int64_t bricks = (int64_t)1 << 21;
    const int pitch = 2048;
    EXPECT(win_pair_index(bricks - 1, pitch - 1, bricks) == bricks * pitch - 1);
    EXPECT(win_pair_index(0, pitch - 32, bricks) == (int64_t)(pitch / 32 - 1) * bricks * 32);
  }
  std::printf("%d failed\n", failures);
  return failures;
}
