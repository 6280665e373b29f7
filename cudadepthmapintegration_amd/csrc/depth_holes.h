// depth_holes.h -- the launches of depth_holes.hip: small holes of a depth map filled from their rims before the maps are fused
// (dmi_fill_depth_holes; include/dmi.h states the definition, DESIGN.md 8k the kernels).  Private: never installed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "depth_holes_rules.h"
#include "dmi_buffer.h"

namespace dmi {

// The device planes of one staged piece of `count` views of W x H, all in vtk point order as the views came.  The labelled
// pixels are the ones that are NOT valid; a "root" is a hole pixel that stands for its hole (tile-local after the local pass,
// final after the merge pass).
struct HolesPiece {
  double *depth;          // [count][H][W] in: the staged depths; out: the filled depths (the output pass writes hole pixels only)
  const double *cost;     // [count][H][W] staged best costs, or null
  uint32_t *label;        // [count][H][W] view-local index of the pixel's tile-local root (kNoLabel: a valid pixel); the roots' entries
                          //               are the parent array of the border pass and hold the final root after the merge pass
  uint32_t *record;       // [count][H][W] at a root: its pixels | kBorderFlag (depth_holes_rules.h); 0 elsewhere
  uint64_t *rim_lo;       // [count][H][W] at a root: the bits of the smallest depth on its rim (kNoRimLo: none); elsewhere not written
  uint64_t *rim_hi;       // [count][H][W] at a root: the bits of the largest (kNoRimHi: none); elsewhere not written
  uint64_t *border_down;  // [tiles] the down-links of every tile's last row
  uint64_t *border_right; // [tiles] the right-links of every tile's last column
  int32_t *out_size;      // [count][H][W] or null
  int64_t count;
};
// a piece of `count` views over its buffers, for the context-free call's staged piece and the resident view set's alike
inline HolesPiece holes_piece(double *depth, const double *cost, const DeviceBuffer &label, const DeviceBuffer &record,
                              const DeviceBuffer &rim_lo, const DeviceBuffer &rim_hi, const DeviceBuffer &border_down,
                              const DeviceBuffer &border_right, int32_t *out_size, int64_t count) {
  return {depth, cost, label.as<uint32_t>(), record.as<uint32_t>(), rim_lo.as<uint64_t>(), rim_hi.as<uint64_t>(), border_down.as<uint64_t>(),
          border_right.as<uint64_t>(), out_size, count};
}

// tiles of a piece (the border arrays hold this many entries each): depth_speckle_rules.h's 64 x 32
int64_t holes_tiles(int32_t W, int32_t H, int64_t count);

// the four passes, in this order, on one stream
hipError_t launch_holes_local(const HolesPiece &piece, double threshold, int32_t W, int32_t H, hipStream_t stream);
hipError_t launch_holes_border(const HolesPiece &piece, int32_t W, int32_t H, hipStream_t stream);
hipError_t launch_holes_merge(const HolesPiece &piece, int32_t W, int32_t H, hipStream_t stream);
hipError_t launch_holes_output(const HolesPiece &piece, int32_t W, int32_t H, double abs_tolerance, double rel_tolerance,
                               int64_t max_pixels, hipStream_t stream);

}  // namespace dmi
