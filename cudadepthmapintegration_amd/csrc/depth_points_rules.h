// depth_points_rules.h -- the rules of dmi_views_build_points that are plain integer arithmetic (include/dmi.h states the
// definition, DESIGN.md 8n the kernels): which difference a tangent is taken as from the usable bits of a pixel's four neighbours,
// the blocks the ordered compaction cuts the views into, the packed counts of a block and the chunks the scan walks, and the byte
// offsets of the five point arrays inside the one allocation that holds them.  No HIP types: the kernels of depth_points.hip and the host program
// tests/cpp/depth_points_rules_host.cpp compile the same text.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define DMI_POINTS_HD __host__ __device__
#else
#define DMI_POINTS_HD
#endif

namespace dmi {
namespace points_rules {

// ---- step 5: the tangent along one image axis ----
enum Tangent : int {
  kTangentNone = 0,      // neither neighbour is usable: no normal
  kTangentCentral = 1,   // c(plus) - c(minus)
  kTangentForward = 2,   // c(plus) - c(centre)
  kTangentBackward = 3,  // c(centre) - c(minus)
};
DMI_POINTS_HD inline Tangent tangent_choice(bool plus_usable, bool minus_usable) {
  if (plus_usable) return minus_usable ? kTangentCentral : kTangentForward;
  return minus_usable ? kTangentBackward : kTangentNone;
}

// the usable bits of the four neighbours of (px, py)
enum UsableBit : unsigned {
  kUsableRight = 1u,  // (px + 1, py)
  kUsableLeft = 2u,   // (px - 1, py)
  kUsableDown = 4u,   // (px, py + 1)
  kUsableUp = 8u,     // (px, py - 1)
};
struct Tangents {
  Tangent x, y;
};
DMI_POINTS_HD inline Tangents tangents_of(unsigned usable) {
  return {tangent_choice((usable & kUsableRight) != 0, (usable & kUsableLeft) != 0),
          tangent_choice((usable & kUsableDown) != 0, (usable & kUsableUp) != 0)};
}
DMI_POINTS_HD inline bool tangents_exist(const Tangents &t) { return t.x != kTangentNone && t.y != kTangentNone; }
DMI_POINTS_HD inline bool one_sided(const Tangents &t) {
  return tangents_exist(t) && (t.x != kTangentCentral || t.y != kTangentCentral);
}
// which neighbour's camera-space point stands on either side of the difference: +1 the plus neighbour, 0 the centre, -1 the minus
DMI_POINTS_HD inline int tangent_high(Tangent t) { return t == kTangentCentral || t == kTangentForward ? 1 : 0; }
DMI_POINTS_HD inline int tangent_low(Tangent t) { return t == kTangentCentral || t == kTangentBackward ? -1 : 0; }

// ---- step 6: the ordered compaction ----
// A block is kBlock consecutive pixels (py * W + px) of ONE view, the last block of a view shorter: ascending block order, and
// ascending lane order inside a block, is ascending (view, py, px).  Whole views per block row keep a block's camera wave-uniform.
constexpr int kBlock = 256;
constexpr int kScanItems = 8;                     // block counts a lane of the scan sums per chunk ...
constexpr int kScanChunk = kBlock * kScanItems;   // ... so one workgroup walks this many blocks per iteration

DMI_POINTS_HD inline int64_t blocks_per_view(int32_t W, int32_t H) { return ((int64_t)W * H + kBlock - 1) / kBlock; }
DMI_POINTS_HD inline int64_t total_blocks(int32_t n, int32_t W, int32_t H) { return (int64_t)n * blocks_per_view(W, H); }
DMI_POINTS_HD inline int64_t block_view(int64_t block, int64_t per_view) { return block / per_view; }
DMI_POINTS_HD inline int64_t block_first_pixel(int64_t block, int64_t per_view) { return (block % per_view) * kBlock; }
// the pixels of the block: kBlock, or what is left of the view
DMI_POINTS_HD inline int32_t block_pixels(int64_t block, int64_t per_view, int64_t plane) {
  const int64_t left = plane - block_first_pixel(block, per_view);
  return (int32_t)(left < kBlock ? left : kBlock);
}
// what the block-count pass leaves per block, in one u32: its valid pixels, its candidates and its emitted pixels, none above
// kBlock.  The scan sums the first two over all blocks for the report and scans the third.
constexpr int kCountBits = 10;
constexpr uint32_t kCountMask = (1u << kCountBits) - 1;
static_assert(kBlock <= (int)kCountMask, "a block's counts must fit their fields");
DMI_POINTS_HD inline uint32_t pack_counts(uint32_t valid, uint32_t candidates, uint32_t emitted) {
  return emitted | (candidates << kCountBits) | (valid << (2 * kCountBits));
}
DMI_POINTS_HD inline uint32_t packed_emitted(uint32_t packed) { return packed & kCountMask; }
DMI_POINTS_HD inline uint32_t packed_candidates(uint32_t packed) { return (packed >> kCountBits) & kCountMask; }
DMI_POINTS_HD inline uint32_t packed_valid(uint32_t packed) { return (packed >> (2 * kCountBits)) & kCountMask; }
DMI_POINTS_HD inline int64_t scan_chunks(int64_t blocks) { return (blocks + kScanChunk - 1) / kScanChunk; }
// a grid's first dimension ends at 2^31 - 1 blocks
DMI_POINTS_HD inline bool blocks_fit_one_launch(int32_t n, int32_t W, int32_t H) { return total_blocks(n, W, H) <= 0x7fffffffLL; }

// ---- step 7: the five arrays of P points in one allocation of 48 P bytes ----
constexpr uint64_t kBytesPerPoint = 48;  // xyz f64[3], normal f32[3], view, pixel and count int32
struct Layout {
  uint64_t xyz, normal, view, pixel, count, bytes;  // byte offsets of the arrays; xyz stays 8-byte aligned, the rest 4-byte
};
// false: 48 P does not fit 64 bits
DMI_POINTS_HD inline bool layout_of(uint64_t points, Layout *out) {
  if (points > ~uint64_t(0) / kBytesPerPoint) return false;
  out->xyz = 0;
  out->normal = 24 * points;
  out->view = 36 * points;
  out->pixel = 40 * points;
  out->count = 44 * points;
  out->bytes = kBytesPerPoint * points;
  return true;
}
// the byte offset of point p's entry in an array of `stride` bytes per point that starts at `base`
DMI_POINTS_HD inline uint64_t entry_offset(uint64_t base, uint64_t p, uint64_t stride) { return base + p * stride; }

}  // namespace points_rules
}  // namespace dmi
