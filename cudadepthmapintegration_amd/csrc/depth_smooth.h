// depth_smooth.h -- the launch of depth_smooth.hip: depth maps smoothed by an edge-preserving filter before they are fused
// (dmi_smooth_depths; include/dmi.h states the definition, DESIGN.md 8l the kernel).  Private: never installed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "depth_smooth_rules.h"

namespace dmi {

// What one launch needs beside the planes.  product[a * kSmoothTableSide + b] = s[a] * s[b] for a, b in [0, radius]: the spatial
// weight of the tap |dy| = a, |dx| = b, rounded once on the host (the definition's (s[|dy|] * s[|dx|])); the rest is not read.
constexpr int kSmoothTableSide = kDepthSmoothMaxRadius + 1;
struct SmoothArgs {
  double product[kSmoothTableSide * kSmoothTableSide];
  double abs_tolerance, rel_tolerance;
  int32_t radius;
};

// the table of one launch from the weights s[0..radius] of depth_smoothing_weights
SmoothArgs smooth_args(const double *s, int32_t radius, double abs_tolerance, double rel_tolerance);

// One iteration over `views` planes of W x H in vtk point order: dst = the smoothed src.  src and dst must not overlap.  cost
// (nullable): src's best costs, src counts as -1 wherever cost > threshold.  count (nullable): the taps taken per pixel.
hipError_t launch_depth_smooth(const double *src, const double *cost, double threshold, double *dst, int32_t *count, int64_t views,
                               int32_t W, int32_t H, const SmoothArgs &args, hipStream_t stream);

}  // namespace dmi
