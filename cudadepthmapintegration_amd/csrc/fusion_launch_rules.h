// fusion_launch_rules.h -- what a fusion launch looks like, decided from what the depth maps, the grid and the caller's variant
// bits look like: plain arithmetic on integers and flags, no HIP type, so that every threshold can be checked at its boundary
// without a GPU (tests/test_fusion_launch_host.py).  fuse_run (dmi_capi_fuse.hip) calls these and carries none of the
// expressions itself.  Every number here was measured; the comment beside it says where.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dmi {

// launches of at most this many wave bricks (the chip's SIMDs) run without brick classes (fuse_without_classes)
constexpr int64_t kNoClassesMaxBricks = 1024;
constexpr int kNoClassesMaxViews = 48;  // ... and only launches of fewer views than this

// tuning-variant bits (dmi_options::kernel_variant)
enum VariantBits : int {
  VAR_EXACT_DIVISION = 1,   // general kernel: no checked-reciprocal fast path
  VAR_GENERAL_K = 2,        // general kernel: ignore K structure
  VAR_BLOCK_SHAPE_MASK = 12,  // general kernel: bits 2..3 pick the 256-thread block shape
  VAR_FORCE_GENERAL = 16,   // never use the tiled kernel
  VAR_TILE_SHAPE_MASK = 0xE0,  // tiled kernel: bits 5..7 pick column height / workgroup shape
  VAR_TILE_SHAPE_SHIFT = 5,
  VAR_NO_BRICK_CLASSES = 256,  // tiled kernel: every (brick, map) pair takes the per-voxel path
  VAR_SPATIAL_ORDER = 512,     // tiled kernel: workgroups in spatial order, not heaviest bricks first
  VAR_FIXED_TILE_SHAPE = 4096,  // tiled kernel: tile-shape bits 0 mean shape 0 whatever the grid size (no automatic choice)
  VAR_KEEP_BEHIND_ADDS = 1024,  // tiled kernel: perform the +0.0 adds of BRICK_BEHIND pairs even when they cannot matter
  VAR_NO_INTERIOR = 2048,       // tiled kernel: full in-front / in-image tests for every mixed pair (never the INTERIOR variant)
  VAR_XCD_RUNS = 8192,          // tiled kernel: ordered bricks dealt to the XCDs in runs (round 1) instead of one eighth of a level each
  VAR_ZMAJOR_SLOTS = 16384,     // tiled kernel: super-bricks enumerated x fastest, then y, then z (until r03h) instead of in Z-order
  VAR_PERSISTENT_ALWAYS = 32768,  // tiled kernel, one-wave workgroups: persistent whatever the number of views (default: from 96 views on)
  VAR_PERSISTENT_NEVER = 65536,   // tiled kernel, one-wave workgroups: one workgroup per brick whatever the number of views
  VAR_BRICK_CLASSES_ALWAYS = 131072,  // tiled kernel: classify and order the bricks of tiny grids too (default: not below 1025 bricks)
  VAR_NO_WINDOWS = 262144,           // tiled kernel: the FREE column always gathers from the validity maps (no bit windows)
  VAR_WINDOWS_ALWAYS = 524288,       // tiled kernel: bit windows whatever the depth maps look like (default: maps with scattered holes)
  VAR_COST_ORDER = 1048576,          // tiled kernel, one-wave workgroups: bricks ordered by their number of mixed views whatever the grid's size
  VAR_NO_COST_ORDER = 2097152        // ... never (four levels, an eighth of each per XCD, as on large grids)
};

// slabs of up to this many bricks are fused in cost order (cost_order).  0: by kernel_variant only -- measured at 128^3 .. 512^3
// (profiles/r16f_form_sweep.txt) the fusion kernel gains 0-4 % from it and the two ordering launches, whose level counters are
// atomics on 64 addresses, take 0.3 ms instead of 0.01 at 256^3
constexpr int kCostOrderMaxSlots = 0;

// What the holes of the resident depth maps look like.  `scattered` is an intermediate of the three rules it enters, kept for
// the reader of a test's table.
struct HoleTraits {
  bool scattered = false;
  bool holes = false;          // FuseConfig::holes
  bool tall_by_holes = false;  // 16-voxel columns from 256^3 on
  bool many_borders = false;   // windows, and 16-voxel columns
  bool mostly_empty = false;   // 16-voxel columns from 384^3 on
};

// mingled: 8-pixel strips (a column of a tile row) with both a hole and a depth; without: pixels without a depth; strips, pixels:
// all there are -- each summed over the resident views.
inline HoleTraits hole_traits(unsigned long long mingled, unsigned long long without, unsigned long long strips, unsigned long long pixels) {
  HoleTraits h;
  // Holes SCATTERED over the depth maps (a best-cost threshold's work): from a hole density of a tenth of a per cent on,
  // nearly every brick's footprint (600 - 1300 pixels) holds one, and the free-space pairs -- most of a fusion's pairs -- are
  // per-voxel work (the FREE column): that decides the launch.  Measured at cfg 3 (profiles/r19m_hole_sweep.jsonl,
  // r19n_hole_variants.jsonl; ms per fusion for 8-voxel columns / + windows / 16-voxel columns + windows):
  //   f = 0.03 %  7.3 / 7.4 / 8.1     0.1 %  10.2 / 9.8 / 10.7     0.5 %  15.0 / 13.4 / 13.2     1 %  15.5 / 13.8 / 13.3
  // (round 4's one bit -- an eighth of the 8-pixel strips holding both a hole and a depth, f >= 1.7 % -- left 0.5 % and 1 % at
  // 15 ms, slower than 2 %'s 13.3).  The density is read from the share p of 8-pixel strips that hold both a hole and a depth
  // (p ~ 8 f); holes in REGIONS (silhouettes against an empty background, patches a filter removed) have mingled strips only
  // along their borders, many hole pixels per mingled strip, and keep the launch of maps without holes (1024^3 x 64 views of
  // the sparse scene: 4.3 against 8.1 ms the other way).
  h.scattered = without <= 6 * mingled;     // a scattered hole has its strip to itself; a disc of radius r has ~0.8 r pixels per border strip
  h.holes = h.scattered && mingled * 160 > strips;    // p > 1/160 (f > 0.08 %): windows, persistent workgroups from 48 views on
  // (1/40 until the kernel of late round 5: at f = 0.2 % and 0.3 % the 16-voxel columns then took 10.9 and 11.5 ms where the
  // 8-voxel ones took 11.2 and 12.2, at 0.1 % a tie -- profiles/r21t_hole_variants.jsonl)
  h.tall_by_holes = h.scattered && mingled * 80 > strips;         // p > 1/80 (f > 0.16 %): 16-voxel columns from 256^3 on
  // holes in regions, but so many that a twenty-fifth of all strips lie on a border: windows for the free-space pairs along those
  // borders, and 16-voxel columns.  Discs of 8-40 pixels radius (`--scene blobs`; share of mingled strips 1.7 / 2.7 / 4.8 / 8.5 %
  // at 5 / 10 / 20 / 40 % of the image): default / windows + 16-voxel columns 6.1 / 6.2, 7.0 / 7.0, 8.5 / 8.1, 11.1 / 9.2 ms
  // (profiles/r21v_hole_variants_blobs.jsonl; the first rule, a tenth of the strips, never fired on that scene).
  h.many_borders = mingled * 25 > strips;
  h.tall_by_holes = h.tall_by_holes || h.many_borders;
  // ... and maps that are mostly EMPTY in large regions (a silhouette against nothing: a quarter of the pixels or more without a
  // depth, the holes not mingled with depths): most (brick, view) pairs are skipped and a brick's fixed costs dominate
  if (!h.holes) h.mostly_empty = without * 4 >= pixels && pixels > 0;
  return h;
}

// The variant with the tile-shape bits of a launch whose caller did not pick a shape (any other launch: the variant as it is).
// Tile shape when the caller did not pick one: grids up to 512^3 do better with 8-voxel columns at five waves per
// SIMD (more, smaller work items and a finer brick classification: 0.65 vs 0.74 ms at 256^3 x 64 views, 11.2 vs 11.5
// ms at 512^3 x 256), 1024^3 with 16-voxel columns (15.5 vs 17.7 ms at 1024^3 x 64: the classification of twice as
// many bricks costs more than it saves); profiles/r01zc_*, r01zd_*, r01zi_*
inline int with_default_tile_shape(int variant, bool tiled, const HoleTraits &h, int32_t nx, int32_t ny, int32_t nz) {
  if (tiled && !(variant & (VAR_TILE_SHAPE_MASK | VAR_FIXED_TILE_SHAPE))) {
    const int64_t bricks16 = (int64_t)((nx + 15) / 16) * ((ny + 15) / 16) * ((nz + 15) / 16);
    // With holes in the depth maps (cfg.holes) most pairs are the FREE column's, whose voxels are cheap next to the set-up
    // of a (brick, view) pair: 16-voxel columns halve the set-ups per voxel and win from 256^3 on (cfg 2 -2.7 %, 384^3 -3.7 %,
    // cfg 3 -2.2 %, cfg 3 with VGA maps -5.6 %, cfg 4's share -5.7 %; 128^3 ties; dense cfg 3 +6.7 %: profiles/r08z_*)
    // Mostly empty maps: 16-voxel columns from 384^3 on (sparse scene, round 4's last build: 512^3 x 256 views 2.36 -> 2.12 ms,
    // 512^3 x 64 0.65 -> 0.57, 384^3 x 128 0.62 -> 0.59; 256^3 x 64 the other way, 0.13 -> 0.15: profiles/r18i_*, r18j_*)
    if (bricks16 <= 32768 && !(h.tall_by_holes && bricks16 >= 4096) && !(h.mostly_empty && bricks16 >= 13824))
      variant |= 7 << VAR_TILE_SHAPE_SHIFT;
  }
  return variant;
}

// wave_bricks: the 8 x 8 x column bricks of the WHOLE grid; views: those of this launch.
// A launch of no more bricks than the chip has SIMDs (64^3 voxels in 8-voxel columns) fuses without classes: every brick
// has a SIMD to itself, and the seven launches that classify and order the bricks take longer than the per-voxel work
// they would save (64^3: 79 -> 49 us at 4 views, 278 -> 192 us at 64; from 96^3 on the classes win;
// profiles/r07o_small_fusions_classes_on_off.txt).  Round 4, the preparation down to four launches: 64^3 x 4 views
// 48 -> 40 us, x 16 73 -> 63 without classes -- and x 64 views 164 us WITH them against 201 (dense; speckle 218 / 204):
// the rule now ends at 48 views (profiles/r16i_small_fusions_classes_on_off.txt).
// (decided from the WHOLE grid's bricks: a slab launch of a larger grid -- dmi_fuse_slab, the overlapped exchanges of
// dmi_multi_fuse -- keeps its classes, as the whole-grid launches the rule was calibrated on)
inline bool fuse_without_classes(int variant, int64_t wave_bricks, int32_t views) {
  if (variant & VAR_NO_BRICK_CLASSES) return true;
  return !(variant & VAR_BRICK_CLASSES_ALWAYS) && wave_bricks <= kNoClassesMaxBricks && views < kNoClassesMaxViews;
}

// row pitch of the class tables: a power of two >= 64 views, so that views arriving in chunks (add, fuse, add,
// fuse ...) change the layout -- and force a reallocation, which waits for the device -- only at doublings
inline int32_t class_table_pitch(int32_t resident_views) {
  int32_t pitch = 64;
  while (pitch < resident_views) pitch *= 2;
  return pitch;
}

// Entry of a (brick, view) pair in the window-pair table (TileArgs::win_origin), in entries of one WinPair.
// brick: the class table's brick number over the WHOLE grid, (bz * wbricks_y + by) * wbricks_x + bx (a slab launch keeps
// it); view: the resident view; n_class_bricks: wbricks_x * wbricks_y * bricks_z.
// [block of 32 views][brick][32 views]: the fusion kernel reads a brick's 32 views of a block as one piece of 512 bytes, as it
// did from a [brick][view] table, and window_origin_kernel -- a workgroup of 64 consecutive bricks and one block -- writes
// 64 x 512 consecutive bytes, where the brick-major table had a line of it every 4 KB.  class_table_pitch is a
// multiple of 32, so the blocks tile the table: the index is a bijection onto [0, n_class_bricks * pitch).
// -DDMI_WINPAIR_BRICK_MAJOR builds both kernels for the [brick][view] table again (tools/exp_list_winpair_layout.txt);
// they do not call this function then.
#if defined(__HIP__)  // (compiled as HIP: the kernels call it)
#define DMI_RULES_HD __host__ __device__
#else
#define DMI_RULES_HD
#endif
constexpr int kWinPairBlockViews = 32;
DMI_RULES_HD inline int64_t win_pair_index(int64_t brick, int32_t view, int64_t n_class_bricks) {
  return (((int64_t)(view >> 5) * n_class_bricks + brick) << 5) + (view & 31);
}

// The fusion kernel fetches a brick's pieces of two consecutive blocks with one buffer load (fusion_tile.hip: the pair area in
// LDS): the distance between them, n_class_bricks * 32 entries of 16 bytes, plus a piece must be below 2^32 - 1, the largest
// range a buffer has (at 2^23 - 1 bricks the second piece's last entry would lie beyond it and read as zeros).  A grid of 2^22
// bricks or more (2 G voxels with 8-voxel columns) is fused without windows.
inline bool win_pair_pieces_addressable(int64_t n_class_bricks) { return n_class_bricks < (int64_t(1) << 22); }
// One of those loads: the buffer it reads from starts at byte `first` of the table -- the brick's piece of `block` -- and ranges over
// `range` bytes, to the table's end (n_class_bricks * class_pitch entries) or 2^32 - 1 bytes, whichever comes first.  A lane reads 16
// bytes at (lane & 31) * 16, plus win_pair_piece_stride for lanes 32-63 (the piece of block + 1).  A block beyond the pitch has range
// 0: the hardware's range check answers every lane with zeros, and no byte outside the table is ever asked for.
struct WinPairFill {
  uint64_t first;
  uint32_t range;
};
DMI_RULES_HD inline uint64_t win_pair_piece_stride(uint64_t n_class_bricks) { return n_class_bricks << 9; }
DMI_RULES_HD inline WinPairFill win_pair_fill(uint64_t brick, uint32_t block, uint64_t n_class_bricks, uint32_t class_pitch) {
  const uint64_t table_bytes = (n_class_bricks * class_pitch) << 4;
  WinPairFill f;
  f.first = (n_class_bricks * block + brick) << 9;
  const uint64_t rest = table_bytes > f.first ? table_bytes - f.first : 0;
  f.range = rest > 0xffffffffull ? 0xffffffffu : (uint32_t)rest;
  return f;
}

// ---- the views' record tables (sync_maps, dmi_capi_fuse.hip): how many records a growth allocates, and how many bytes of each
// table a launch over the resident views [0, n) may read.  sync_maps asks for record_bytes_read and allocates
// record_bytes_allocated, so a table is grown exactly when a launch could read past its end.
// What reads a table beyond the launch's last view (every consumer in fusion_tile.hip, fusion_classify.hip, fusion_kernels.hip and
// fusion_device.h read once, for an index of first_map + n_maps or more):
//   MapRec      none.  The general kernel's loop and tile_exact stop at m_end; classify_bricks clamps its view to n_maps - 1 and
//               the coarse pass returns for mm >= n_maps; fill_launch_tables takes e / kpad < n_maps.
//   TileMapRec  none.  Read beside MapRec under the same index everywhere; the tiled kernel's view loop masks the class words to
//               [first_map, m_end) before it touches a record.
//   WinRec      ONE record: the window column of fusion_tile.hip fetches a dword at offset 0x40 of the record it works on -- the
//               first dword of the NEXT view's record, a prefetch whose value is never used -- so the launch's last view reaches
//               record n.  window_origin_kernel tests m < m_end first: none there.
//   FootRec     none.  Only window_origin_kernel reads it, under that same test.
//   hit counters (u64 per view): none.  atomicAdd at the view's own index inside the loops above.
// The sizes are those of view_records.h; dmi_capi_fuse.hip asserts that they are.
enum RecordTable : int { REC_MAP = 0, REC_TILE_MAP = 1, REC_WIN = 2, REC_FOOT = 3, REC_HITS = 4, kRecordTables = 5 };
constexpr uint64_t kRecordBytes[kRecordTables] = {208, 368, 64, 320, 8};
constexpr uint64_t kRecordsReadAhead[kRecordTables] = {0, 0, 1, 0, 0};
// views often arrive in chunks (add, fuse, add, fuse ...): a growth allocates twice the records there are views, 64 at least
inline uint64_t record_capacity(uint64_t n_views) { return n_views * 2 > 64 ? n_views * 2 : 64; }
inline uint64_t record_bytes_read(RecordTable t, uint64_t n_views) { return (n_views + kRecordsReadAhead[t]) * kRecordBytes[t]; }
inline uint64_t record_bytes_allocated(RecordTable t, uint64_t n_views) { return record_capacity(n_views) * kRecordBytes[t]; }

// No sum of the launch can be -0.0 (the launches the kernel's ZF instantiations serve, fusion_tile.hip), and the +0.0 adds of the
// pairs far behind every surface can be dropped (TileArgs::behind_mask):
// +0.0 adds are no-ops unless a sum can be -0.0 (only an uploaded grid can bring one) or hits are counted
inline bool zero_free(bool init_from_grid, bool grid_free_of_negative_zero, bool count_hits, int variant) {
  return (!init_from_grid || grid_free_of_negative_zero) && !count_hits && !(variant & VAR_KEEP_BEHIND_ADDS);
}

// The window origins of the FREE column (TileArgs::win_origin), one word per class byte
// (for depth maps with holes scattered all over them -- cfg.holes: what makes the FREE column the busiest one -- ; the
// launch then runs the kernel's WIN instantiation, which pays for the window code in every column, fusion_tile.hip)
struct WindowsQuestion {
  bool tier1;        // DMI_TIER1 != 0: the build selects pixels in two tiers
  bool general_k;    // FuseConfig::general_k
  bool count_hits;
  int variant;
  bool holes, many_borders;  // HoleTraits
  bool any_tier1;    // (a launch none of whose views has a window record has no window pair: the plain instantiation serves it)
  // (and only where no sum can be -0.0 -- the launches the kernel's ZF instantiations serve, fusion_tile.hip -- and the depth
  // tables are f32: elsewhere the FREE column keeps its gathers)
  bool zero_free;
  bool depth_f64;
};
inline bool use_windows(const WindowsQuestion &q) {
  return q.tier1 && !q.general_k && !q.count_hits && !(q.variant & (VAR_NO_WINDOWS | VAR_NO_INTERIOR)) &&
         (q.holes || q.many_borders || (q.variant & VAR_WINDOWS_ALWAYS)) && q.any_tier1 && q.zero_free && !q.depth_f64;
}

// waves_per_workgroup: TileShape::wx * wy; n_slots: the launch's workgroup slots.
// Small grids (one-wave workgroups): the bricks ordered by their NUMBER of mixed views and dealt to the XCDs in short runs.
// With a few bricks per wave the launch ends when its longest bricks do -- a brick's views are serial, ~3 us each however
// empty the chip -- and four levels let a 30-view brick start halfway through (256^3 x 64 views: the last 0.1 of 0.35 ms
// with under a third of the waves at work, profiles/r16b_wg_cfg2_*).  Large grids keep the four levels, an eighth of each
// per XCD: their tail is short against the launch, and the XCDs' compact regions save L2 traffic.
inline bool cost_order(int waves_per_workgroup, int variant, size_t n_slots) {
  return waves_per_workgroup == 1 && !(variant & VAR_NO_COST_ORDER) && ((variant & VAR_COST_ORDER) || n_slots <= (size_t)kCostOrderMaxSlots);
}

}  // namespace dmi
