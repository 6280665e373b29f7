// scene_bounds.h -- the launches of scene_bounds.hip: the bounds of the scene the depth maps see, as exact order statistics of the
// back-projected pixels per grid axis (dmi_estimate_scene_bounds; include/dmi.h states the definition, DESIGN.md 8h the kernels).
// Private: never installed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "depth_consistency.h"  // ConsistencyCamera and the upload pass: the planes are 8g's
#include "scene_bounds_rules.h"

namespace dmi {

// What the passes keep on the device between launches: no host round trip until the last select has written `result`.
struct BoundsState {
  uint64_t prefix[bounds_rules::kTargets];  // the digits fixed so far, as the top bits of the target's key shifted down
  uint64_t rank[bounds_rules::kTargets];    // the target's rank among the keys that carry its prefix
  uint64_t n;                               // the counted points (pass 0)
  double result[bounds_rules::kTargets];    // lo_0, hi_0, lo_1, hi_1, lo_2, hi_2 after the last pass; NaN when n == 0
  uint32_t shared[3];                       // 1 while the axis's lo and hi still carry the same prefix: one histogram serves both
  uint32_t done;                            // 1: n == 0, the remaining passes leave at once
};

struct BoundsAxes {
  double a[9];  // row-major: s_a = (a[3a]*w_0 + a[3a+1]*w_1) + a[3a+2]*w_2
};

constexpr int kBoundsBlock = 256;
constexpr int kBoundsItems = 4;                               // pixels per lane and chunk
constexpr int kBoundsChunk = kBoundsBlock * kBoundsItems;     // taking-part pixels of one view that a workgroup visits at a time
constexpr int64_t kBoundsMaxChunksPerGroup = int64_t(1) << 21;  // keeps a workgroup's 32-bit LDS counters below 2^31
constexpr int kBoundsAggregateRounds = 1;  // wave-aggregated LDS adds per histogram before the lanes left add on their own; 0: off
                                           // (measured: 0, 1, 2, 4, 64 rounds)

struct BoundsTuning {  // what a tuning build's environment may ask for; the default build runs the constants above, compiled in
  int aggregate_rounds = kBoundsAggregateRounds;
  int share_histograms = 1;
};

// hist: kTargets x kBins u64 counters, zero before pass 0 (the select leaves them zero again).  One pass: every taking-part valid
// pixel of planes[n][H][W] (image row order, -1 = not valid: launch_consistency_upload) is back-projected, turned into its three
// keys, and the digit `pass` of every key that carries a target's prefix is counted.  blocks: the workgroups to launch.
hipError_t launch_bounds_count(const double *planes, const ConsistencyCamera *cameras, int n, int W, int H, int pixel_step,
                               const BoundsAxes &axes, int pass, const BoundsState *state, unsigned long long *hist, unsigned blocks,
                               const BoundsTuning &tuning, hipStream_t stream);
// one workgroup: per target the bin that holds its rank, the next digit of its prefix, the rank left; pass 0 first takes n and the
// trimmed ranks, the last pass writes `result`
hipError_t launch_bounds_select(BoundsState *state, unsigned long long *hist, int pass, double trim_fraction, hipStream_t stream);
// the workgroups a count pass should run with on a device of `compute_units`
unsigned bounds_count_blocks(int n, int W, int H, int pixel_step, int compute_units);
#ifdef DMI_TUNING
// the yardstick of tools/gpu_scene_bounds_time.py: a plain read of the same planes, summed into *sink
hipError_t launch_bounds_plain_read(const double *planes, int64_t total, double *sink, unsigned blocks, hipStream_t stream);
#endif

}  // namespace dmi
