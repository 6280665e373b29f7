// view_set_kernels.h -- the launches of view_set_kernels.hip: what the resident view set (dmi_views_*; include/dmi.h states the
// definition, DESIGN.md 8m the kernels) runs beside the filters' own passes -- the ingest of staged depths and the counters of a
// step's report.  Private: never installed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "depth_holes.h"
#include "depth_speckle.h"

namespace dmi {

// The counters of one step, u64 each, in one device array the set zeroes before the step's first piece
enum ViewSetCounter {
  kVsValidBefore = 0,
  kVsValidAfter = 1,
  kVsDiffering = 2,
  kVsAuxSum = 3,
  kVsRoots = 4,
  kVsRootsKept = 5,
  kVsIngested = 6,  // valid pixels an ingest has stored
  kVsCounters = 8
};

// the workgroups of a bandwidth-bound pass over `items` lane-iterations on a device of `compute_units`: never more than the work,
// never more than eight per compute unit (the lanes stride over the rest)
unsigned view_set_blocks(uint64_t items, int compute_units);

// out[i] = depth[i] where it is valid (> 0 and < +inf) and cost (nullable) is not > threshold, -1 elsewhere, for i in [0, total);
// counters[kVsIngested] += the valid ones.  depth, cost and out must stand at the same offset from a 16-byte boundary
// (hipErrorInvalidValue otherwise): the set stages accordingly.
hipError_t launch_view_set_ingest(const double *depth, const double *cost, double threshold, double *out, uint64_t total,
                                  unsigned long long *counters, int compute_units, hipStream_t stream);

// One read of a step's planes: counters[kVsValidBefore / kVsValidAfter] += the values > 0 of before / after, [kVsDiffering] += the
// places where the two differ, [kVsAuxSum] += aux (nullable) over the places where after > 0.  before, after and aux must start on
// 16-byte boundaries (hipErrorInvalidValue otherwise): a step's piece does (view_set_rules.h: piece_views).
hipError_t launch_view_set_report(const double *before, const double *after, const int32_t *aux, uint64_t total,
                                  unsigned long long *counters, int compute_units, hipStream_t stream);

// After a piece's size / merge pass: counters[kVsRoots] += the pixels that are their segment's (hole's) final root,
// [kVsRootsKept] += those whose segment has at least min_pixels pixels (whose hole is fillable: depth_holes_rules.h).
hipError_t launch_view_set_segment_roots(const SpecklePiece &piece, int32_t W, int32_t H, int64_t min_pixels, unsigned long long *counters,
                                         int compute_units, hipStream_t stream);
hipError_t launch_view_set_hole_roots(const HolesPiece &piece, int32_t W, int32_t H, double abs_tolerance, double rel_tolerance,
                                      int64_t max_pixels, unsigned long long *counters, int compute_units, hipStream_t stream);

}  // namespace dmi
