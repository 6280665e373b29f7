// depth_speckle.h -- the launches of depth_speckle.hip: small segments of a depth map removed before the maps are fused
// (dmi_filter_depth_speckles; include/dmi.h states the definition, DESIGN.md 8j the kernels).  Private: never installed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "depth_speckle_rules.h"
#include "dmi_buffer.h"

namespace dmi {

struct SpeckleTuning {  // what a launch runs with; anything but the defaults exists in a tuning build only
  int tile_height = speckle_rules::kTileHeight;  // 16, 32 or 64
  bool runs = true;                              // false: every pixel is a node of the tile's union-find and hooks for itself
};

// The device planes of one staged piece of `count` views of W x H, all in vtk point order as the views came (the relation does
// not care which way the rows run).
struct SpecklePiece {
  double *depth;          // [count][H][W] in: the staged depths; out: the filtered depths (the output pass works in place)
  const double *cost;     // [count][H][W] staged best costs, or null
  uint32_t *label;        // [count][H][W] view-local index of the pixel's tile-local root (kNoLabel: not valid); the roots' entries
                          //               are the parent array of the border pass and hold the final root after the size pass
  uint32_t *size;         // [count][H][W] pixels of the local segment at a tile-local root, 0 elsewhere; the whole segment's at its final root
  uint64_t *border_down;  // [tiles] the down-links of every tile's last row
  uint64_t *border_right; // [tiles] the right-links of every tile's last column
  int32_t *out_size;      // [count][H][W] or null
  int64_t count;
};
// a piece of `count` views over its buffers, for the context-free call's staged piece and the resident view set's alike
inline SpecklePiece speckle_piece(double *depth, const double *cost, const DeviceBuffer &label, const DeviceBuffer &size,
                                  const DeviceBuffer &border_down, const DeviceBuffer &border_right, int32_t *out_size, int64_t count) {
  return {depth, cost, label.as<uint32_t>(), size.as<uint32_t>(), border_down.as<uint64_t>(), border_right.as<uint64_t>(), out_size, count};
}

// tiles of a piece under `tuning` (the border arrays hold this many entries each)
int64_t speckle_tiles(int32_t W, int32_t H, int64_t count, const SpeckleTuning &tuning);

// the four passes, in this order, on one stream
hipError_t launch_speckle_local(const SpecklePiece &piece, double threshold, int32_t W, int32_t H, double abs_tolerance,
                                double rel_tolerance, const SpeckleTuning &tuning, hipStream_t stream);
hipError_t launch_speckle_border(const SpecklePiece &piece, int32_t W, int32_t H, const SpeckleTuning &tuning, hipStream_t stream);
hipError_t launch_speckle_sizes(const SpecklePiece &piece, int32_t W, int32_t H, hipStream_t stream);
hipError_t launch_speckle_output(const SpecklePiece &piece, int32_t W, int32_t H, int64_t min_pixels, hipStream_t stream);

}  // namespace dmi
