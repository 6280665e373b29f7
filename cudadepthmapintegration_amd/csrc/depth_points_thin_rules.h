// depth_points_thin_rules.h -- the rules of dmi_thin_point_cloud / dmi_views_thin_points that are plain integer arithmetic
// (include/dmi.h states the definition, DESIGN.md 8o the kernels): the limit on an axis' bins and the bits a key needs, the key
// itself, the byte offsets of the six output arrays inside the one allocation that holds them, which cells go to the wave pass and
// how many of them there can be, and the bytes a call holds.  No HIP types: the kernels of depth_points_thin.hip and the host
// program tests/cpp/depth_points_thin_rules_host.cpp compile the same text.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define DMI_THIN_HD __host__ __device__
#else
#define DMI_THIN_HD
#endif

namespace dmi {
namespace thin_rules {

constexpr int kBlock = 256;

// ---- step 1: bins and keys ----
constexpr uint64_t kMaxBins = uint64_t(1) << 21;  // per axis: three of them keep the key within 63 bits
constexpr uint64_t kMaxPoints = (uint64_t(1) << 32) - 1;  // ids, sorted positions and cell sizes are u32

// the bins of one axis from q = floor((hi - lo) / h): q + 1, or 0 when that is more than 2^21 (an infinite or NaN quotient included)
DMI_THIN_HD inline uint64_t bins_of_top(double q) { return q >= 0.0 && q < 2097152.0 ? (uint64_t)q + 1 : 0; }
DMI_THIN_HD inline uint64_t key_of(uint64_t b0, uint64_t b1, uint64_t b2, uint64_t n0, uint64_t n1) { return (b2 * n1 + b1) * n0 + b0; }
// the smallest B >= 1 with count < 2^B
DMI_THIN_HD inline int bits_for(uint64_t count) {
  int b = 1;
  while (b < 64 && (count >> b) != 0) ++b;
  return b;
}
// the bits of the largest key, n_0 n_1 n_2 - 1 (every n_d in [1, 2^21]: the product is at most 2^63)
DMI_THIN_HD inline int key_bits(uint64_t n0, uint64_t n1, uint64_t n2) {
  const uint64_t last = n0 * n1 * n2 - 1;
  return last == 0 ? 1 : bits_for(last);
}

// ---- step 4: the six arrays of Q output points in one allocation of 52 Q bytes ----
// The first five stand where depth_points_rules.h's Layout puts them for Q points (dmi_views_download_points serves a thinned cloud
// with the offsets it has always used); members follows them.
constexpr uint64_t kBytesPerPoint = 52;
struct Layout {
  uint64_t xyz, normal, view, pixel, count, members, bytes;
};
DMI_THIN_HD inline bool layout_of(uint64_t points, Layout *out) {  // false: 52 Q does not fit 64 bits
  if (points > ~uint64_t(0) / kBytesPerPoint) return false;
  out->xyz = 0;
  out->normal = 24 * points;
  out->view = 36 * points;
  out->pixel = 40 * points;
  out->count = 44 * points;
  out->members = 48 * points;
  out->bytes = kBytesPerPoint * points;
  return true;
}

// ---- the representatives: which pass sums a cell ----
// A cell of more than `threshold` members is summed by a wave of its own (the queue), any other by one lane.  No value of the
// threshold changes a bit of the result.  The default comes from a sweep.
constexpr uint32_t kDefaultWaveCellPoints = 32;
DMI_THIN_HD inline bool wave_cell(uint32_t members, uint32_t threshold) { return members > threshold; }
// the most cells of P points that can have more than `threshold` members each: the queue's capacity (at least one entry)
DMI_THIN_HD inline uint64_t wave_queue_capacity(uint64_t points, uint32_t threshold) {
  const uint64_t most = points / ((uint64_t)threshold + 1);
  return most < 1 ? 1 : most;
}
// a wave takes a cell's members 64 at a time
DMI_THIN_HD inline uint32_t wave_chunks(uint32_t members) { return members / 64 + (members % 64 ? 1 : 0); }

// ---- what a call holds on the device beside the cloud it reads and the result it builds ----
// two key arrays of P + 1 u64 (the head flags and ranks, then the kept flags and output numbers, live in them once the sort is
// done), two id arrays, the cells' first sorted positions, the members' xyz, normal and count in sorted order (40 bytes a point),
// the queue, and 16 counters
DMI_THIN_HD inline uint64_t scratch_bytes(uint64_t points, uint32_t threshold) {
  return 2 * 8 * (points + 1) + 2 * 4 * points + 4 * (points + 1) + 40 * points + 4 * wave_queue_capacity(points, threshold) + 16 * 8;
}

}  // namespace thin_rules
}  // namespace dmi
