// depth_points_thin.h -- the launches of depth_points_thin.hip: a point cloud thinned and merged on a voxel grid
// (dmi_thin_point_cloud, dmi_views_thin_points; include/dmi.h states the definition, DESIGN.md 8o the kernels).  Private: never
// installed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "depth_points_thin_rules.h"

namespace dmi {

// The counters of a call, u64 each, in one device array; launch_thin_bounds sets them all
enum ThinCounter {
  kThinLo = 0,          // [0..3): the minima as order-preserving integers (thin_decode_bound)
  kThinHi = 3,          // [3..6): the maxima
  kThinNonFinite = 6,   // 1 when a coordinate is not finite
  kThinCells = 7,       // occupied cells
  kThinLargest = 8,     // the members of the largest cell
  kThinMultiView = 9,   // kept cells whose first and last member differ in view
  kThinQueued = 10,     // kept cells that go to the wave pass
  kThinWithNormal = 11, // output points whose normal is not the zero vector
  kThinCounters = 16
};

// the input on the device: five arrays of n entries
struct ThinCloud {
  const double *xyz;    // [n][3]
  const float *normal;  // [n][3]
  const int32_t *view, *pixel, *count;
  uint64_t n;
};

struct ThinGrid {
  double lo[3], h;
  uint64_t n[3];
};

// what a call holds beside the cloud and the result (thin_rules::scratch_bytes, and rocPRIM's own storage)
struct ThinScratch {
  unsigned long long *counters;  // kThinCounters
  uint64_t *keys[2];             // n + 1 each
  uint32_t *ids[2];              // n each
  uint32_t *start;               // n + 1: a cell's first sorted position, the end of the last behind it
  double *sorted_xyz;            // three planes of n: the members' coordinates in sorted order
  float *sorted_normal;          // three planes of n
  int32_t *sorted_count;         // n
  uint32_t *queue;               // thin_rules::wave_queue_capacity entries
  uint64_t queue_capacity;
  void *temp;
  size_t temp_bytes;
};

// where the ranks pass leaves what the representatives read: pointers into the key arrays
struct ThinRanks {
  const uint32_t *sorted_ids;  // n
  const uint32_t *kept;        // n + 1: 1 where cell c is kept
  const uint32_t *out_index;   // n + 1: the output number of cell c; [n] = the number of kept cells
};

hipError_t thin_temp_bytes(uint64_t n, size_t *bytes);
// rocPRIM's stable radix sort of (key, value) pairs over the low `bits` of the keys between two buffers each; with temp == nullptr
// it only returns the storage it needs in *temp_bytes.  *sorted_keys, *sorted_values: where the result stands.  The search grid of
// depth_points_radius.hip sorts with it too.
hipError_t thin_sort_pairs(void *temp, size_t *temp_bytes, uint64_t *ka, uint64_t *kb, uint32_t *va, uint32_t *vb, uint64_t n, int bits,
                           uint64_t **sorted_keys, uint32_t **sorted_values, hipStream_t stream);
double thin_decode_bound(unsigned long long ordered);
// the bounds pass: counters[kThinLo .. kThinNonFinite], every other counter zero
hipError_t launch_thin_bounds(const ThinCloud &cloud, unsigned long long *counters, hipStream_t stream);
// keys, sort and ranks, in stream order, an event in front of each and one behind the last (events[0..4)).  Leaves
// counters[kThinCells, kThinLargest, kThinMultiView, kThinQueued], the queue and *ranks.
hipError_t launch_thin_cells(const ThinCloud &cloud, const ThinGrid &grid, uint32_t min_points, uint32_t wave_cell_points,
                             const ThinScratch &scratch, hipEvent_t events[4], ThinRanks *ranks, hipStream_t stream);
// the representatives: the permutation into sorted order, the lane pass over `cells` cells and the wave pass over `queued` of
// them; `out` holds `layout`'s arrays for out_index[n] points.  Adds to counters[kThinWithNormal].
hipError_t launch_thin_representatives(const ThinCloud &cloud, const ThinScratch &scratch, const ThinRanks &ranks, uint64_t cells,
                                       uint64_t queued, uint32_t wave_cell_points, const thin_rules::Layout &layout, unsigned char *out,
                                       hipStream_t stream);

}  // namespace dmi
