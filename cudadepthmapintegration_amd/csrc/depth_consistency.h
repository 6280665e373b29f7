// depth_consistency.h -- the launches of depth_consistency.hip: depth maps filtered by cross-view geometric consistency before they
// are fused (dmi_filter_depth_consistency; include/dmi.h states the definition, DESIGN.md 8g the kernel).  Private: never installed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dmi {

// What the pass reads of a view's K4 and RT4.  The entry point has checked the K: K4[1][0] == 0, third row (0, 0, 1, 0), non-zero
// K4[0][0] and K4[1][1], so h_2 = c'_2 and the K4[1][0] product drops out of h_1 without changing a selected pixel.
// The 3 x 3 block of RT4 is taken as orthonormal: the back-projection uses its transpose.
struct ConsistencyCamera {
  double rt[12];  // rows 0..2 of RT4
  double k[8];    // K4[0][0], K4[0][1], K4[0][2], K4[0][3], K4[1][1], K4[1][2], K4[1][3], unused
};

constexpr int kConsistencyTile = 16;        // a workgroup's square of source pixels: four waves of 8 x 8
constexpr int kConsistencyViewGroup = 0;    // target views per launch of the count kernel; 0: all of them in one launch
constexpr int kConsistencyGatherAhead = 0;  // 1: a target's depth is requested one view before it is compared

struct ConsistencyTuning {  // what a launch runs with; the defaults above unless a tuning build's environment says otherwise
  int view_group = kConsistencyViewGroup;
  int gather_ahead = kConsistencyGatherAhead;
};

// `count` staged images of W x H in vtk point order (depth, and cost or null) -> planes[first_view ...]: thresholded, rows flipped
// to image order (row 0 = the top image row), every value that is not valid (> 0 and < +inf) stored as -1
hipError_t launch_consistency_upload(const double *depth, const double *cost, double threshold, int W, int H, int64_t count,
                                     double *planes, int64_t first_view, hipStream_t stream);
// counts[s][py][px] += the views of [t0, t1) other than s that agree with source pixel (px, py) of view s, for every s in [0, n).
// counts are in image row order, as the planes; the caller has zeroed them before the first launch.  *undecided (nullable,
// device): += the pairs whose pixel the checked reciprocal left to the exact division.
hipError_t launch_consistency_count(const double *planes, const ConsistencyCamera *cameras, int n, int W, int H, int t0, int t1,
                                    double abs_tolerance, double rel_tolerance, int gather_ahead, int32_t *counts,
                                    unsigned long long *undecided, hipStream_t stream);
// the outputs of views [first_view, first_view + count) in vtk point order: out_depth = the plane's value where it is valid and
// its count >= min_views, -1 elsewhere; out_count (nullable) = the counts
hipError_t launch_consistency_finish(const double *planes, const int32_t *counts, int W, int H, int64_t first_view, int64_t count,
                                     int32_t min_views, double *out_depth, int32_t *out_count, hipStream_t stream);

}  // namespace dmi
