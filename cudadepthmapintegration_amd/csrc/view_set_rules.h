// view_set_rules.h -- the rules of the resident view set (dmi_views_*; include/dmi.h states the definition, DESIGN.md 8m the
// kernels) that are plain integer arithmetic: how the views are cut into pieces of whole views for a pass's scratch, what the set
// holds on the device, how many elements stand before a 16-byte boundary, and how a step's counters become its report.  No HIP
// types: dmi_capi_viewset.hip, view_set_kernels.hip and the host program tests/cpp/view_set_rules_host.cpp compile the same text.
#pragma once
#include <cstdint>

namespace dmi {
namespace view_set_rules {

constexpr uint64_t kDefaultPieceBytes = uint64_t(256) << 20;  // what the context-free calls stage at a time
constexpr int32_t kMaxSide = 32768;

// The views of one piece: as many f64 planes as fit piece_bytes, at least one (a view larger than the piece goes whole), at most
// n.  The rule of the context-free calls, with their constant for piece_bytes.  One addition: where W * H is odd the number is even
// (two at least), so that every piece starts at an even pixel of the set's planes, a 16-byte boundary, as a context-free call's
// staged piece does (the speckle filter's output pass loads pixel pairs).  n >= 1, W and H in [1, kMaxSide].
inline int64_t piece_views(uint64_t piece_bytes, int32_t W, int32_t H, int64_t n) {
  const uint64_t plane = (uint64_t)W * (uint64_t)H;  // <= 2^30
  uint64_t fit = piece_bytes / (plane * 8);
  if (fit < 1) fit = 1;
  if (plane % 2 == 1) fit = fit < 2 ? 2 : fit - fit % 2;
  return fit < (uint64_t)n ? (int64_t)fit : n;
}

struct Piece {
  int64_t first, count;
};
inline int64_t piece_count(int64_t n, int64_t per_piece) { return (n + per_piece - 1) / per_piece; }
inline Piece piece_at(int64_t n, int64_t per_piece, int64_t index) {  // index in [0, piece_count)
  const int64_t first = index * per_piece;
  const int64_t left = n - first;
  return {first, left < per_piece ? left : per_piece};
}

// a * b into *out; false (and *out untouched) when the product does not fit 64 bits
inline bool checked_mul(uint64_t a, uint64_t b, uint64_t *out) {
  if (a != 0 && b > ~uint64_t(0) / a) return false;
  *out = a * b;
  return true;
}
inline bool checked_add(uint64_t a, uint64_t b, uint64_t *out) {
  if (b > ~uint64_t(0) - a) return false;
  *out = a + b;
  return true;
}

// Bytes per pixel of a piece that a step's scratch takes beside the two resident planes (aux: the size or count plane, which the
// smoothing always writes for its report).
enum Step { kIngest = 0, kSpeckles = 1, kHoles = 2, kSmooth = 3, kConsistency = 4, kBounds = 5 };
inline uint64_t scratch_bytes_per_pixel(Step step, bool aux, bool second_plane) {
  switch (step) {
    case kIngest: return 16;                           // the staged depths and costs
    case kSpeckles: return 8 + (aux ? 4 : 0);          // label, size
    case kHoles: return 24 + (aux ? 4 : 0);            // label, record, rim_lo, rim_hi
    case kSmooth: return 4 + (second_plane ? 8 : 0);   // the tap counts; the plane the iterations alternate with
    case kConsistency: return aux ? 4 : 0;             // the counts in vtk order, when asked for
    default: return 0;
  }
}

// What the set holds for n views of W x H: the two planes (16 bytes per pixel and view), and at the peak of a consistency or
// bounds pass the flipped planes and counts (12 more).  false: the figure does not fit 64 bits (n is not bounded by the ABI).
inline bool resident_bytes(uint64_t n, int32_t W, int32_t H, uint64_t *out) {
  uint64_t pixels;
  if (!checked_mul(n, (uint64_t)W * (uint64_t)H, &pixels)) return false;
  return checked_mul(pixels, 16, out);
}
inline bool peak_bytes(uint64_t n, int32_t W, int32_t H, uint64_t piece_bytes, uint64_t *out) {
  uint64_t pixels, resident, whole, scratch;
  if (!checked_mul(n, (uint64_t)W * (uint64_t)H, &pixels)) return false;
  if (!checked_mul(pixels, 16, &resident) || !checked_mul(pixels, 12, &whole)) return false;
  const uint64_t per = (uint64_t)piece_views(piece_bytes, W, H, n > (uint64_t)INT64_MAX ? INT64_MAX : (int64_t)n);
  if (!checked_mul(per * (uint64_t)W * (uint64_t)H, 28, &scratch)) return false;  // the hole fill's, the largest
  uint64_t sum;
  if (!checked_add(resident, whole > scratch ? whole : scratch, &sum)) return false;
  *out = sum;
  return true;
}

// Elements of `element_bytes` (a power of two <= 16) that stand between byte address `address` (a multiple of element_bytes) and the
// next 16-byte boundary: what a pass peels off before its 16-byte loads.
inline uint64_t elements_before_16(uint64_t address, uint64_t element_bytes) { return ((16 - (address & 15)) & 15) / element_bytes; }

// What the report kernels count, and the report made of it (include/dmi.h: dmi_views_step_report).
struct Counters {
  uint64_t valid_before, valid_after, differing, aux_sum, roots, roots_kept;
};
struct Report {
  uint64_t valid_before, valid_after, changed, groups, groups_kept, aux_sum;
};
inline Report make_report(Step step, const Counters &c) {
  Report r = {c.valid_before, c.valid_after, c.differing, 0, 0, 0};
  if (step == kSpeckles || step == kHoles) {
    r.groups = c.roots;
    r.groups_kept = c.roots_kept;
  }
  if (step == kSmooth) r.aux_sum = c.aux_sum;
  return r;
}

}  // namespace view_set_rules
}  // namespace dmi
