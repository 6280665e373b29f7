// depth_points.h -- the launches of depth_points.hip: the fused point cloud of the resident view set (dmi_views_build_points;
// include/dmi.h states the definition, DESIGN.md 8n the kernels).  Private: never installed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "depth_consistency.h"
#include "depth_points_rules.h"

namespace dmi {

// The counters of a build, u64 each, in one device array the caller zeroes before the first pass
enum PointsCounter {
  kPtValid = 0,       // valid pixels
  kPtCandidates = 1,  // step 2
  kPtOwned = 2,       // step 3
  kPtWithNormal = 3,  // emitted points that have a normal
  kPtCounters = 4
};

// bits of a pixel's flag byte
constexpr uint8_t kPointCandidate = 1, kPointEmitted = 2, kPointValid = 4;

struct PointsParams {
  int32_t W, H;
  int32_t min_views, pixel_step, dedupe;
  double abs_tolerance, rel_tolerance, normal_abs_tolerance, normal_rel_tolerance;
};

// Steps 2 and 3.  planes, counts and flags are [n][H][W] in image row order (planes as launch_consistency_upload leaves them,
// counts as launch_consistency_count does); the caller has zeroed flags.  A valid pixel's flags = kPointValid, with kPointCandidate
// where it is one, and kPointEmitted where the candidate is not owned.  No counter is touched: the passes behind count the flags.
hipError_t launch_points_flags(const double *planes, const int32_t *counts, const ConsistencyCamera *cameras, int32_t n,
                               const PointsParams &params, uint8_t *flags, hipStream_t stream);
// block_counts[b] = the valid, candidate and emitted pixels of block b, packed (depth_points_rules.h), for every block of the n views
hipError_t launch_points_block_counts(const uint8_t *flags, int32_t n, int32_t W, int32_t H, uint32_t *block_counts, hipStream_t stream);
// block_offsets[b] = the emitted pixels of the blocks [0, b); *total = those of all; counters[kPtValid / kPtCandidates / kPtOwned]
// = the sums over all blocks (owned: candidates that are not emitted).  One workgroup, no waiting between workgroups.
hipError_t launch_points_scan(const uint32_t *block_counts, int64_t blocks, uint64_t *block_offsets, uint64_t *total,
                              unsigned long long *counters, hipStream_t stream);
// Steps 4, 5 and 7 for the emitted pixels, stored at their rank (step 6) in the arrays `layout` places inside `out`.
// block_normals[b] = the points of block b that have a normal (block_counts' memory may be given: the scan has read it).
hipError_t launch_points_scatter(const double *planes, const int32_t *counts, const ConsistencyCamera *cameras, const uint8_t *flags,
                                 int32_t n, const PointsParams &params, const uint64_t *block_offsets, const points_rules::Layout &layout,
                                 unsigned char *out, uint32_t *block_normals, hipStream_t stream);
// counters[kPtWithNormal] += the sum of block_normals[0 .. blocks): a few hundred workgroups, one atomic each
hipError_t launch_points_sum_normals(const uint32_t *block_normals, int64_t blocks, unsigned long long *counters, hipStream_t stream);

}  // namespace dmi
