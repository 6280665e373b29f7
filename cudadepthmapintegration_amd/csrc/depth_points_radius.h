// depth_points_radius.h -- the launches of depth_points_radius.hip: the neighbours of every point of a cloud within a radius, and
// the cloud without the points that have too few (dmi_count_point_neighbors, dmi_views_filter_points_radius; include/dmi.h states
// the definition, DESIGN.md 8p the kernels).  Private: never installed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "depth_points_radius_rules.h"
#include "depth_points_thin.h"

namespace dmi {

// The counters of a call, u64 each, in one device array of kThinCounters: the bounds pass is the thinning's and leaves
// [kThinLo .. kThinNonFinite] where it always has; the others start at zero
enum RadiusCounter {
  kRadiusUnits = 7,      // the count kernel's work units
  kRadiusIsolated = 8,   // points without a neighbour
  kRadiusMost = 9,       // the largest count
  kRadiusSum = 10,       // the sum of the counts
  kRadiusTests = 11      // the d2 a lane evaluated for a query it holds
};

struct RadiusGrid {
  double lo[3], h;
  uint64_t n[3];
};

// what a call holds beside the cloud and the result (radius_rules::scratch_bytes, and rocPRIM's own storage: thin_temp_bytes)
struct RadiusScratch {
  unsigned long long *counters;  // kThinCounters
  uint64_t *keys[2];             // n + 1 each
  uint32_t *ids[2];              // n each
  uint32_t *start;               // n + 1: a unit's first sorted position, the end of the last behind it
  double *sorted_xyz;            // three planes of n: the coordinates in sorted order
  uint32_t *neighbors;           // n, in input order
  void *temp;
  size_t temp_bytes;
};

// where the flags pass leaves what the compaction reads: pointers into the key arrays
struct RadiusKept {
  const uint32_t *kept;       // n + 1: 1 where input point i is kept; [n] = 0
  const uint32_t *out_index;  // n + 1: the output number of input point i; [n] = the number of kept points
};

// the arrays of a cloud on the device, each n entries apart from the last two, which a cloud may lack (nullptr); the compaction
// carries every one that is there bit for bit
struct RadiusCloud {
  const double *xyz;     // [n][3]
  const float *normal;   // [n][3]
  const int32_t *view, *pixel, *count;
  const uint32_t *members;  // a thinned cloud's, or nullptr
  uint64_t n;
};

// what the front passes leave for the kernel that searches: pointers into the scratch
struct RadiusSorted {
  const uint64_t *keys;  // n, ascending
  const uint32_t *ids;   // n: the input index of every sorted position
  uint32_t *free_words;  // 2 (n + 1) u32 in the key array the sort did not end in: the head flags and ranks, read for the last time
};

// The front passes both searching kernels share (the count below, the plane fit of depth_points_planes.hip): keys, sort, units
// (heads, ranks, starts) and the permutation into sorted planes.  events[0..5) stand in front of keys, sort, ranks, permute and
// behind the permutation.  Leaves scratch.start, scratch.sorted_xyz, counters[kRadiusUnits] and *sorted.
hipError_t launch_radius_front(const double *xyz, uint64_t n, const RadiusGrid &grid, uint32_t group_points, const RadiusScratch &scratch,
                               hipEvent_t events[5], RadiusSorted *sorted, hipStream_t stream);
// keys, sort, units, permutation, count and flags in stream order: events[0..7) stand in front of keys, sort, ranks, permute,
// count, flags and behind the flags' scan.  Leaves neighbors (input order), counters[kRadiusUnits ..] and *kept.
hipError_t launch_radius_counts(const double *xyz, uint64_t n, const RadiusGrid &grid, double r2, uint32_t min_neighbors,
                                uint32_t group_points, const RadiusScratch &scratch, hipEvent_t events[7], RadiusKept *kept,
                                hipStream_t stream);
// the kept points of `cloud`, in input order, into `out`: thin_rules::Layout's offsets for kept.out_index[n] points (members only
// where the cloud has them) and their counts at neighbors_offset
hipError_t launch_radius_compaction(const RadiusCloud &cloud, const RadiusKept &kept, const uint32_t *neighbors,
                                    const thin_rules::Layout &layout, uint64_t neighbors_offset, unsigned char *out, hipStream_t stream);

}  // namespace dmi
