// win_pair_fill / win_pair_piece_stride of csrc/fusion_launch_rules.h -- the buffers of the loads that bring a brick's window
// pairs into LDS (fuse_tile_kernel: four loads per group of 256 views, each lane 16 bytes) -- checked on the CPU
// (tests/test_winpair_fill_host.py builds this with AddressSanitizer and UBSan and runs it).  What the hardware does with a
// descriptor is modelled here: a lane whose 16 bytes end beyond `range` gets zeros, every other lane reads those bytes.  So
//   * no lane ever reads a byte outside the table, whatever the group (also groups beyond the table's pitch);
//   * the lane that lands at (view & 255) * 16 of the area has read exactly the entry win_pair_index names, for every view below
//     the pitch; for views beyond it, nothing.
// Every failed line is printed, the exit status is their number.
#include "fusion_launch_rules.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace dmi;

static int failures = 0;
#define EXPECT(cond)                                                                                                          \
  do {                                                                                                                        \
    if (!(cond)) {                                                                                                            \
      if (failures < 50) std::printf("line %d (bricks %lld, pitch %d): %s\n", __LINE__, (long long)bricks, pitch, #cond); \
      ++failures;                                                                                                             \
    }                                                                                                                         \
  } while (0)

// the table holds its own entry numbers; the area is filled as the kernel fills it
static void check_table(int64_t bricks, int pitch, int groups) {
  const int64_t entries = bricks * pitch;
  std::vector<uint64_t> table((size_t)entries * 2);  // 16 bytes per entry
  for (int64_t e = 0; e < entries; ++e) table[(size_t)e * 2] = table[(size_t)e * 2 + 1] = (uint64_t)e + 1;
  const uint64_t table_bytes = (uint64_t)entries * 16;
  for (int64_t k = 0; k < bricks; ++k) {
    for (int g = 0; g < groups; ++g) {
      std::vector<uint64_t> area(256 * 2, ~0ull);
      for (int q = 0; q < 4; ++q) {
        const WinPairFill f = win_pair_fill((uint64_t)k, (uint32_t)(8 * g + 2 * q), (uint64_t)bricks, (uint32_t)pitch);
        EXPECT(f.first + f.range <= table_bytes || f.range == 0);
        for (int lane = 0; lane < 64; ++lane) {
          const uint64_t voff = (uint64_t)(lane & 31) * 16 + ((lane & 32) ? win_pair_piece_stride((uint64_t)bricks) : 0);
          EXPECT(voff <= 0xffffffffull);
          uint64_t got[2] = {0, 0};
          if (voff + 16 <= f.range) {  // the range check of a raw buffer
            EXPECT(f.first + voff + 16 <= table_bytes);
            if (f.first + voff + 16 <= table_bytes) std::memcpy(got, reinterpret_cast<const char *>(table.data()) + f.first + voff, 16);
          }
          area[(size_t)(64 * q + lane) * 2] = got[0];
          area[(size_t)(64 * q + lane) * 2 + 1] = got[1];
        }
      }
      for (int v = 256 * g; v < 256 * g + 256; ++v) {
        const uint64_t want = v < pitch ? (uint64_t)win_pair_index(k, v, bricks) + 1 : 0;
        EXPECT(area[(size_t)(v & 255) * 2] == want && area[(size_t)(v & 255) * 2 + 1] == want);
      }
    }
  }
}

int main() {
  {
    const int64_t brick_counts[] = {1, 63, 135};
    const int pitches[] = {64, 128, 256, 512};
    for (int64_t bricks : brick_counts)
      for (int pitch : pitches) check_table(bricks, pitch, pitch / 256 + 2);  // ... and two groups beyond the table
  }
  {
    // the largest table the host gives windows to: the stride and a piece fit a 32-bit offset, the range saturates, and the last
    // brick's last load ends with the table
    const int64_t bricks = ((int64_t)1 << 22) - 1;
    const int pitch = 2048;
    EXPECT(win_pair_pieces_addressable(bricks) && !win_pair_pieces_addressable(bricks + 1));
    EXPECT(win_pair_piece_stride((uint64_t)bricks) + 512 <= 0xffffffffull);
    const WinPairFill a = win_pair_fill(0, 0, (uint64_t)bricks, (uint32_t)pitch);
    EXPECT(a.first == 0 && a.range == 0xffffffffu);  // (the table has 2^37 bytes)
    const WinPairFill z = win_pair_fill((uint64_t)bricks - 1, (uint32_t)(pitch / 32 - 2), (uint64_t)bricks, (uint32_t)pitch);
    EXPECT(z.first + z.range == (uint64_t)bricks * pitch * 16 && z.range == win_pair_piece_stride((uint64_t)bricks) + 512);
    const WinPairFill beyond = win_pair_fill(0, (uint32_t)(pitch / 32), (uint64_t)bricks, (uint32_t)pitch);
    EXPECT(beyond.range == 0);
  }
  std::printf("%d failed\n", failures);
  return failures;
}
