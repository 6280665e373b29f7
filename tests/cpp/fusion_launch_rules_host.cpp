// The launch decisions of csrc/fusion_launch_rules.h at their boundaries (tests/test_fusion_launch_host.py builds this with
// AddressSanitizer and UBSan and runs it).  The expected values restate the expressions fuse_run carried before the rules had a
// header of their own; every failed line is printed, the exit status is their number.
#include "fusion_launch_rules.h"

#include <cstdio>

using namespace dmi;

static int failures = 0;
#define EXPECT(cond)                                            \
  do {                                                          \
    if (!(cond)) {                                              \
      std::printf("line %d: %s\n", __LINE__, #cond);            \
      ++failures;                                               \
    }                                                           \
  } while (0)

static HoleTraits scattered_traits(unsigned long long mingled) { return hole_traits(mingled, 6 * mingled, 16000, 128000); }
static int shape_bits(int variant) { return (variant & VAR_TILE_SHAPE_MASK) >> VAR_TILE_SHAPE_SHIFT; }

int main() {
  // ---- hole traits: 16000 strips, hole pixels = 6 x mingled strips (still "scattered")
  EXPECT(scattered_traits(100).scattered && !scattered_traits(100).holes);
  EXPECT(scattered_traits(101).holes);
  EXPECT(!scattered_traits(200).tall_by_holes && scattered_traits(200).holes);
  EXPECT(scattered_traits(201).tall_by_holes && !scattered_traits(201).many_borders);
  EXPECT(!scattered_traits(640).many_borders);
  EXPECT(scattered_traits(641).many_borders && scattered_traits(641).tall_by_holes && scattered_traits(641).holes);
  {
    const HoleTraits regions = hole_traits(641, 6 * 641 + 1, 16000, 128000);  // one hole pixel more: not scattered
    EXPECT(!regions.scattered && !regions.holes && regions.many_borders && regions.tall_by_holes);
    const HoleTraits fewer = hole_traits(201, 6 * 201 + 1, 16000, 128000);
    EXPECT(!fewer.scattered && !fewer.holes && !fewer.tall_by_holes && !fewer.many_borders);
  }
  EXPECT(hole_traits(0, 32000, 16000, 128000).mostly_empty);   // hole pixels x 4 == pixels
  EXPECT(!hole_traits(0, 31999, 16000, 128000).mostly_empty);
  EXPECT(!hole_traits(0, 0, 0, 0).mostly_empty);               // never without pixels
  EXPECT(!hole_traits(0, 0, 16000, 128000).mostly_empty && !hole_traits(0, 0, 16000, 128000).holes);
  {
    const HoleTraits h = hole_traits(101, 606, 16000, 2000);   // a quarter of the pixels and more are holes, but `holes` is on
    EXPECT(h.holes && !h.mostly_empty);
  }

  // ---- the default tile shape
  const HoleTraits none, tall = scattered_traits(201), empty = hole_traits(0, 32000, 16000, 128000);
  EXPECT(shape_bits(with_default_tile_shape(0, true, none, 512, 512, 512)) == 7);
  EXPECT(shape_bits(with_default_tile_shape(0, true, none, 528, 528, 528)) == 0);
  EXPECT(shape_bits(with_default_tile_shape(0, true, none, 528, 512, 512)) == 0);
  EXPECT(tall.tall_by_holes && !tall.mostly_empty);
  EXPECT(shape_bits(with_default_tile_shape(0, true, tall, 240, 240, 240)) == 7);
  EXPECT(shape_bits(with_default_tile_shape(0, true, tall, 256, 256, 256)) == 0);
  EXPECT(empty.mostly_empty && !empty.tall_by_holes);
  EXPECT(shape_bits(with_default_tile_shape(0, true, empty, 368, 368, 368)) == 7);
  EXPECT(shape_bits(with_default_tile_shape(0, true, empty, 384, 384, 384)) == 0);
  EXPECT(shape_bits(with_default_tile_shape(0, true, empty, 256, 256, 256)) == 7);   // (the holes' threshold is not the empty maps')
  for (int carried = 1; carried <= 7; ++carried) {
    const int v = carried << VAR_TILE_SHAPE_SHIFT;
    EXPECT(with_default_tile_shape(v, true, none, 64, 64, 64) == v);
  }
  EXPECT(with_default_tile_shape(VAR_FIXED_TILE_SHAPE, true, none, 64, 64, 64) == VAR_FIXED_TILE_SHAPE);
  EXPECT(with_default_tile_shape(0, false, none, 64, 64, 64) == 0);
  EXPECT(with_default_tile_shape(VAR_NO_WINDOWS, true, none, 64, 64, 64) == (VAR_NO_WINDOWS | (7 << VAR_TILE_SHAPE_SHIFT)));

  // ---- brick classes or not
  EXPECT(fuse_without_classes(0, 1024, 47));
  EXPECT(!fuse_without_classes(0, 1024, 48));
  EXPECT(!fuse_without_classes(0, 1088, 47));
  EXPECT(fuse_without_classes(VAR_NO_BRICK_CLASSES, 1 << 20, 256));
  EXPECT(!fuse_without_classes(VAR_BRICK_CLASSES_ALWAYS, 1024, 47));
  EXPECT(!fuse_without_classes(VAR_BRICK_CLASSES_ALWAYS, 1, 1));

  // ---- the class tables' pitch
  EXPECT(class_table_pitch(1) == 64 && class_table_pitch(64) == 64 && class_table_pitch(65) == 128 && class_table_pitch(128) == 128 &&
         class_table_pitch(129) == 256);

  // ---- windows: true with everything satisfied, false with any single conjunct flipped
  WindowsQuestion all{};
  all.tier1 = true, all.general_k = false, all.count_hits = false, all.variant = 0, all.holes = true, all.many_borders = false;
  all.any_tier1 = true, all.zero_free = true, all.depth_f64 = false;
  EXPECT(use_windows(all));
  { WindowsQuestion q = all; q.tier1 = false; EXPECT(!use_windows(q)); }
  { WindowsQuestion q = all; q.general_k = true; EXPECT(!use_windows(q)); }
  { WindowsQuestion q = all; q.count_hits = true; EXPECT(!use_windows(q)); }
  { WindowsQuestion q = all; q.variant = VAR_NO_WINDOWS; EXPECT(!use_windows(q)); }
  { WindowsQuestion q = all; q.variant = VAR_NO_INTERIOR; EXPECT(!use_windows(q)); }
  { WindowsQuestion q = all; q.holes = false; EXPECT(!use_windows(q)); }
  { WindowsQuestion q = all; q.holes = false; q.many_borders = true; EXPECT(use_windows(q)); }
  { WindowsQuestion q = all; q.holes = false; q.variant = VAR_WINDOWS_ALWAYS; EXPECT(use_windows(q)); }
  { WindowsQuestion q = all; q.variant = VAR_WINDOWS_ALWAYS | VAR_NO_WINDOWS; EXPECT(!use_windows(q)); }
  { WindowsQuestion q = all; q.any_tier1 = false; EXPECT(!use_windows(q)); }
  { WindowsQuestion q = all; q.zero_free = false; EXPECT(!use_windows(q)); }
  { WindowsQuestion q = all; q.depth_f64 = true; EXPECT(!use_windows(q)); }

  // ---- the views' record tables: capacity, bytes read, bytes allocated (tests/test_gpu_sequence_fuzz.py restates these numbers)
  {
    const uint64_t ns[10] = {1, 31, 32, 33, 63, 64, 65, 129, 130, 131};
    const uint64_t caps[10] = {64, 64, 64, 66, 126, 128, 130, 258, 260, 262};
    const uint64_t sizes[kRecordTables] = {208, 368, 64, 320, 8};
    for (int q = 0; q < 10; ++q) {
      const uint64_t n = ns[q];
      EXPECT(record_capacity(n) == caps[q]);
      for (int t = 0; t < kRecordTables; ++t) {
        const uint64_t ahead = t == REC_WIN ? 1 : 0;   // the window column's prefetch: offset 0x40 of the last view's record
        EXPECT(record_bytes_read((RecordTable)t, n) == (n + ahead) * sizes[t]);
        EXPECT(record_bytes_allocated((RecordTable)t, n) == caps[q] * sizes[t]);
        EXPECT(record_bytes_allocated((RecordTable)t, n) >= record_bytes_read((RecordTable)t, n));
      }
      // the prefetch's four bytes, at 64 (n - 1) + 0x40 .. + 4, lie inside what the launch is said to read
      EXPECT(64 * (n - 1) + 0x40 + 4 <= record_bytes_read(REC_WIN, n));
    }
    EXPECT(record_capacity(0) == 64);
    // a context that fuses at a views and then at b >= a (dmi_buffer.h: a table that holds what is needed is kept, any other is
    // allocated anew, all four as a unit): what it holds covers what the second launch reads, for every table
    int uncovered = 0, kept_at_capacity = 0;
    for (uint64_t a = 1; a <= 140; ++a)
      for (uint64_t b = a; b <= 140; ++b) {
        uint64_t held[kRecordTables];
        for (int t = 0; t < kRecordTables; ++t) held[t] = record_bytes_allocated((RecordTable)t, a);   // the first fuse: nothing held before
        bool enough = true;
        for (int t = REC_MAP; t <= REC_FOOT; ++t) enough = enough && held[t] >= record_bytes_read((RecordTable)t, b);
        if (!enough)
          for (int t = REC_MAP; t <= REC_FOOT; ++t) held[t] = record_bytes_allocated((RecordTable)t, b);
        if (held[REC_HITS] < record_bytes_read(REC_HITS, b)) held[REC_HITS] = record_bytes_allocated(REC_HITS, b);   // grown by itself
        for (int t = 0; t < kRecordTables; ++t)
          if (held[t] < record_bytes_read((RecordTable)t, b)) ++uncovered;
        // b == the capacity held: the window table must have been grown (the old rule kept it, 4 bytes short)
        if (b == record_capacity(a) && held[REC_WIN] == record_bytes_allocated(REC_WIN, a)) ++kept_at_capacity;
      }
    EXPECT(uncovered == 0);
    EXPECT(kept_at_capacity == 0);
    // (the pair the defect was reported with: 32 views, then 64)
    EXPECT(record_bytes_allocated(REC_WIN, 32) == 4096 && record_bytes_read(REC_WIN, 64) == 4160);
  }

  // ---- no sum can be -0.0: the ZF instantiations and the behind mask
  EXPECT(zero_free(false, false, false, 0));
  EXPECT(zero_free(false, true, false, 0));
  EXPECT(!zero_free(true, false, false, 0));
  EXPECT(zero_free(true, true, false, 0));
  EXPECT(!zero_free(false, true, true, 0));
  EXPECT(!zero_free(false, true, false, VAR_KEEP_BEHIND_ADDS));

  // ---- the cost order
  EXPECT(cost_order(1, VAR_COST_ORDER, 4096));
  EXPECT(!cost_order(1, VAR_COST_ORDER | VAR_NO_COST_ORDER, 4096));
  EXPECT(!cost_order(4, VAR_COST_ORDER, 4096) && !cost_order(2, VAR_COST_ORDER, 4096));
  EXPECT(kCostOrderMaxSlots == 0);
  EXPECT(!cost_order(1, 0, 32) && !cost_order(1, 0, 1));

  std::printf("%d failed\n", failures);
  return failures;
}
