// dmi_mesh_stage.h -- what the stages on the context's iso-surface mesh share (dmi_capi_mesh.hip: the component filter, the
// smoother, the decimation, the hole fill, the support trim): the mesh's state with the one operation that makes a stage's result
// the mesh and drops what the change invalidates, the table of what each stage drops, a stage's events and the times read from
// them, the sizes a stage refuses, and the carving of a scratch buffer into u32 arrays.  Needs nothing but dmi_buffer.h, the
// status codes and the HIP runtime's names, so all of it also runs on the CPU (tests/test_mesh_stage_host.py).  Private: never
// installed.
#pragma once
#include "../../include/dmi.h"
#include "dmi_buffer.h"

#include <array>
#include <string>
#include <utility>

namespace dmi {

// The events of a stage and the times of its last call: the kernels' milliseconds and, where the stage has passes, each pass's.
// Every function returns the runtime's status (the caller wraps it in DMI_HIP).
template <int Events, int Passes = 0>
struct StageTimes {
  hipEvent_t events[Events] = {};
  double last_kernel_ms = 0.0;
  std::array<double, Passes> last_pass_ms{};

  // Created at the first call that needs them, all or none: a failure destroys those it had created, and the next call starts over
  hipError_t create(unsigned flags = 0) {
    if (events[0]) return hipSuccess;
    for (hipEvent_t &e : events) {
      const hipError_t status = flags ? hipEventCreateWithFlags(&e, flags) : hipEventCreate(&e);
      if (status == hipSuccess) continue;
      e = nullptr;
      release();
      return status;
    }
    return hipSuccess;
  }
  void zero() {
    last_kernel_ms = 0.0;
    last_pass_ms.fill(0.0);
  }
  hipError_t elapsed(int a, int b, double *ms) const {
    float f = 0.f;
    const hipError_t status = hipEventElapsedTime(&f, events[a], events[b]);
    *ms = (double)f;
    return status;
  }
  // The kernels' time over [first, last] and the passes between consecutive events from `first` on, n_passes of them; the rest 0
  hipError_t read(int first, int last, int n_passes = Passes) {
    hipError_t status = elapsed(first, last, &last_kernel_ms);
    for (int p = 0; p < Passes && status == hipSuccess; ++p) {
      last_pass_ms[p] = 0.0;
      if (p < n_passes) status = elapsed(first + p, first + p + 1, &last_pass_ms[p]);
    }
    return status;
  }
  void release() { destroy_events(events); }
};

// What a change of the mesh invalidates.  One row per way a stage ends; the stage bodies name theirs.
struct MeshDrops {
  bool regions, colors, support;
};
namespace drops {
// (smoothing with 0 iterations, a fill that fills nothing, a support call on an empty mesh or one that removes nothing drop
// nothing: those branches call neither drop nor a commit)
// the component filter (the regions become its own: it sets `filtered` and the components it kept) and the smoother with
// iterations > 0 (the positions move, the vertices and their regions stay), both on an empty mesh too
constexpr MeshDrops kComponents{false, true, true}, kSmoothing{false, true, true};
// the decimation (on an empty mesh too) and a fill that fills something
constexpr MeshDrops kDecimation{true, true, true}, kFill{true, true, true};
// a support trim that removes something: its counts are compacted with the mesh
constexpr MeshDrops kSupportTrim{true, true, false};
}  // namespace drops

// The mesh of the last extraction, as the support trim, the filter, the smoother, the decimation and the fill have left it.  The
// stages write into the alternates (the smoother steps through alt_vertices and a buffer of its own, normals into alt_normals);
// commit_alternates / commit_positions then swap whichever holds the result with the mesh's own buffer, after the last call
// that can fail.
struct MeshState {
  DeviceBuffer vertices, triangles, normals;  // [n][3] f64, [n][3] int64, [n][3] f32
  DeviceBuffer alt_vertices, alt_triangles, alt_normals;
  DeviceBuffer region_id, region_size;  // int64 per vertex / per kept component, of the last filter
  uint64_t n_vertices = 0, n_triangles = 0;
  uint64_t regions = 0;      // kept components of that filter
  bool valid = false;
  bool has_normals = false;  // the last successful extraction wrote them
  bool filtered = false;     // a filter has run since the last extraction or decimation: the region arrays are the mesh's
  // dmi_color_process_isosurface's results, [n][3] u8, [n][3] u8, [n] int32; written into the alternates and swapped in last
  DeviceBuffer color_mean, color_median, color_count;
  DeviceBuffer alt_color_mean, alt_color_median, alt_color_count;
  bool colored = false;      // the colour arrays describe this mesh (dropped by whatever changes it)
  bool support_counted = false;  // dmi_context::Support::counts describes this mesh (likewise)

  void drop(MeshDrops what) {
    if (what.regions) filtered = false, regions = 0;  // (regions is read only behind `filtered`)
    if (what.colors) colored = false;
    if (what.support) support_counted = false;
  }
  // new positions (and normals, where the mesh has them) for the same vertices and triangles; the buffer replaced is `result` now
  void commit_positions(DeviceBuffer &result, MeshDrops what) {
    std::swap(vertices, result);
    if (has_normals) std::swap(normals, alt_normals);
    drop(what);
  }
  // the mesh in the alternates becomes the context's; the buffers it came from are the next stage's output
  void commit_alternates(uint64_t nv, uint64_t nt, MeshDrops what) {
    std::swap(triangles, alt_triangles);
    n_vertices = nv;
    n_triangles = nt;
    commit_positions(alt_vertices, what);
  }
  void release() {
    free_buffers({&vertices, &triangles, &normals, &alt_vertices, &alt_triangles, &alt_normals, &region_id, &region_size,
                  &color_mean, &color_median, &color_count, &alt_color_mean, &alt_color_median, &alt_color_count});
  }
};

// ---- sizes refused, never wrapped: the text behind "<entry>: ", empty when the size is accepted ----
constexpr uint64_t kTwoTo32 = uint64_t(1) << 32;
// vertex and triangle ids are int64 (vtkIdType) and the buffers' byte sizes (24 a vertex or triangle) must fit a size_t
inline std::string extraction_refusal(uint64_t nv, uint64_t nt) {
  const uint64_t limit = (uint64_t)INT64_MAX / 24;
  return nv > limit || nt > limit ? "mesh too large for int64 ids" : "";
}
// the stages' ids are u32 on the device; `what` says whose ("32-bit vertex ids")
inline std::string ids_refusal(uint64_t nv, uint64_t nt, const char *what) {
  return nv >= kTwoTo32 || nt >= kTwoTo32 ? std::string("mesh too large for ") + what : "";
}
// ... and so are indices into `factor` entries per triangle (nt < 2^32: ids_refusal comes first)
inline std::string product_refusal(uint64_t factor, uint64_t nt, const char *what) {
  return factor * nt >= kTwoTo32 ? std::string("mesh too large for ") + what : "";
}
// an edge key of the fill is two ids and the direction bit in 64 bits
inline std::string direction_bit_refusal(uint64_t nv) {
  return nv >= (uint64_t(1) << 31) ? "mesh too large for the edge keys' direction bit (vertices >= 2^31)" : "";
}
inline std::string filled_refusal(uint64_t nv, uint64_t nt) {
  const bool fits = nv < kTwoTo32 && nt < kTwoTo32 && 6 * nt < kTwoTo32;
  return fits ? "" : "the filled mesh would be too large for 32-bit ids (vertices or 6 x triangles >= 2^32)";
}

// `count` u32 arrays of `pitch` entries each, one behind the other in a scratch buffer: the size asked for and the arrays carved
// come from the same count
struct U32Lanes {
  uint32_t *base;
  uint64_t pitch;
  uint32_t *lane(int i) const { return base + (uint64_t)i * pitch; }
  uint64_t bytes(int count) const { return (uint64_t)count * pitch * sizeof(uint32_t); }
};
// components: parent, size, vmap, rmap; smoother (behind the fixed bits): row starts, valences, offsets; decimation: sorted ids
// (2), head, rank, cluster, start, mark, map, and keep, map per triangle; fill: out-degree, in-degree, successor, flag, rank, and
// per loop slot id, next, 2 pointers, 2 labels, count, 2 additions, 2 offsets; support: mark, vmap
constexpr int kComponentsLanes = 4, kSmoothingLanes = 3, kDecimationLanes = 8, kDecimationTriangleLanes = 2, kHolesLanes = 5,
              kHolesLoopLanes = 11, kSupportLanes = 2;

}  // namespace dmi
