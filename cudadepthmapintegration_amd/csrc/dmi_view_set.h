// dmi_view_set.h -- the resident view set behind dmi_views_* of include/dmi.h (dmi_capi_viewset.hip): the depth planes
// of n views that stay on one device from the first filter to the fusion, the scratch of one piece of a pass, and the per-piece
// bodies that the context-free entry points (dmi_capi_speckle.hip, dmi_capi_holes.hip, dmi_capi_smooth.hip,
// dmi_capi_consistency.hip, dmi_capi_bounds.hip) share with it: one implementation per filter.  What those calls and the set's
// entries share around the bodies -- checks, staging, cameras, spans -- is dmi_depth_call.h's.  Private: never installed.
#pragma once
#include "../../include/dmi.h"
#include "depth_consistency.h"
#include "depth_holes.h"
#include "depth_points.h"
#include "depth_points_planes.h"
#include "depth_points_radius.h"
#include "depth_points_thin.h"
#include "depth_smooth.h"
#include "depth_speckle.h"
#include "dmi_depth_call.h"
#include "scene_bounds.h"
#include "view_set_rules.h"

#include <string>
#include <vector>

struct dmi_view_set {
  int32_t device = 0, W = 0, H = 0;
  int32_t n = 0;
  int compute_units = 0;
  // D is plane[current], [n][H][W] f64 in vtk point order, normalised: a valid depth or -1.  A step writes plane[current ^ 1] and
  // the two change places when it has succeeded; an add grows both.
  dmi::DeviceBuffer plane[2];
  int current = 0;
  std::vector<double> K4, RT4;  // [n][16] each, as they came
  // the scratch of one piece, kept while large enough: the staging of an add; the labelling planes of the speckle filter and the
  // hole fill (label and record serve both); the plane the smoothing's iterations alternate with; the size or count plane
  dmi::DeviceBuffer stage_depth, stage_cost, label, record, rim_lo, rim_hi, border_down, border_right, second, aux;
  // held during a consistency or bounds pass only: the planes in image row order, the counts, the cameras, the select's state
  dmi::DeviceBuffer flipped, counts, cameras, state, hist;
  // held during dmi_views_build_points only, beside flipped, counts and cameras: a flag byte per pixel, and per block of the
  // compaction its count and its offset (depth_points_rules.h)
  dmi::DeviceBuffer flags, block_counts, block_offsets;
  // the point cloud of the last dmi_views_build_points, 48 bytes per point (points_rules::Layout); dropped by whatever changes D
  dmi::DeviceBuffer points;
  uint64_t n_points = 0;
  bool points_current = false;
  // dmi_views_thin_points has replaced the build's cloud by its thinned one: 52 bytes per point (thin_rules::Layout, whose first
  // five arrays stand where points_rules::Layout has them); dropped with the points
  bool points_thinned = false;
  double thin_pass_ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // the last thinning's bounds, keys, sort, ranks with their scans, representatives
  uint32_t thin_wave_cell_points = dmi::thin_rules::kDefaultWaveCellPoints;  // dmi_views_set_thin_wave_cell_points
  // dmi_views_filter_points_radius has replaced the cloud by its kept points: the arrays it had (48 or 52 bytes per point) and a u32
  // `neighbors` array behind them; a thinning or whatever drops the points drops it
  bool points_filtered = false;
  double radius_pass_ms[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // the last filter's bounds, keys, sort, ranks, permute, count, compaction
  uint32_t radius_group_points = dmi::radius_rules::kDefaultGroupPoints;  // dmi_views_set_radius_group_points
  // dmi_views_fit_point_planes was the cloud's last step: plane_rms f32[n_points] in a buffer of its own, dropped by whatever
  // replaces or drops the cloud (a build, a thinning, the radius filter, a change of D)
  dmi::DeviceBuffer plane_rms;
  bool points_fitted = false;
  double plane_fit_pass_ms[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // the last fit's bounds, keys, sort, ranks, permute, fit
  double points_pass_ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // the last build's flip, count, flags, block counts + scan, scatter
  dmi::DeviceBuffer counters;  // dmi::kVsCounters u64 (view_set_kernels.h); a build's dmi::kPtCounters stand in the same array
  hipStream_t stream = nullptr;
  hipEvent_t events[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // around a piece's passes
  hipEvent_t report_events[2] = {nullptr, nullptr};                      // around a piece's report kernels
  hipEvent_t handed_over = nullptr;  // what a fusion context's upload stream waits for (dmi_add_views_from_set)
  uint64_t piece_bytes = dmi::view_set_rules::kDefaultPieceBytes;
  uint64_t device_bytes = 0;  // the sum of the capacities held
  uint64_t steps = 0, h2d_plane_bytes = 0, d2h_plane_bytes = 0;
  double last_report_kernel_ms = 0.0;
  std::string err;
};

namespace dmi {

int views_fail(dmi_view_set *s, int code, const std::string &msg);  // records msg (s == nullptr: for dmi_views_last_error(nullptr))

// ---- one implementation per filter: defined beside the context-free entry point that runs it between its copies ----

// dmi_capi_points_thin.hip: the thinning of a cloud that is on the device (n in [1, 2^32), cell_size and min_points checked by the
// caller): bounds, keys, sort, ranks and representatives with their three synchronisations; everything but the result is freed
// before it returns, `held` following every allocation.  DMI_OK, or a code with *message saying why (`entry` names the caller): then
// nothing is left allocated and the cloud is as it was.
struct ThinOutcome {
  DeviceBuffer result;  // thin_rules::Layout for n_out points; empty when there are none.  The caller's to free.
  uint64_t n_out = 0;
  dmi_points_thin_report report{};
  double pass_ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
};
int run_thin_points(const std::string &entry, const ThinCloud &cloud, double cell_size, int32_t min_points, uint32_t wave_cell_points,
                    hipStream_t stream, uint64_t &held, ThinOutcome *outcome, std::string *message);
// dmi_capi_points_radius.hip: the neighbour counts of a cloud that is on the device (n in [1, 2^32), radius and min_neighbors
// checked with radius_refusal by the caller) and, with bytes_per_point != 0 (the bytes of the cloud's own arrays: 48, or 52 with
// members), its kept points in a buffer of their own; with 0 the counts themselves, in input order, are the outcome.  Everything
// else is freed before it returns, `held` following every allocation.  DMI_OK, or a code with *message saying why: then nothing is
// left allocated and the cloud is as it was.
struct RadiusOutcome {
  DeviceBuffer result;     // the cloud's layout for n_kept points, neighbors u32[n_kept] behind it; empty when there are none
  DeviceBuffer neighbors;  // u32[n] (bytes_per_point == 0 only).  Both are the caller's to free.
  uint64_t n_kept = 0;
  dmi_points_radius_report report{};
  double pass_ms[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
};
const char *radius_refusal(double radius, int32_t min_neighbors);  // what is wrong with the first of them that is, or null
int run_radius_points(const std::string &entry, const RadiusCloud &cloud, double radius, int32_t min_neighbors, uint32_t group_points,
                      uint64_t bytes_per_point, hipStream_t stream, uint64_t &held, RadiusOutcome *outcome, std::string *message);
// dmi_capi_points_planes.hip: the plane fit of a cloud that is on the device (n in [1, 2^32), the parameters checked with
// plane_fit_refusal by the caller).  out_xyz and out_normal, each asked for by its flag and null without it, hold copies of the
// input (zeros for absent normals) when the call begins and are never the arrays being read: the kernel writes the fitted points
// into them.  plane_rms f32[n] and neighbors u32[n] come back in buffers of their own, the caller's to free; everything else is
// freed before it returns, `held` following every allocation.  DMI_OK, or a code with *message saying why: then nothing is left
// allocated.
struct PlaneFitOutcome {
  DeviceBuffer plane_rms, neighbors;
  dmi_points_planes_report report{};
  double pass_ms[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
};
const char *plane_fit_refusal(double radius, int32_t min_neighbors, int32_t flags);  // what is wrong with the first that is, or null
int run_plane_fit_points(const std::string &entry, const double *xyz, const float *normal, uint64_t n, double radius, int32_t min_neighbors,
                         int32_t flags, uint32_t group_points, double *out_xyz, float *out_normal, hipStream_t stream, uint64_t &held,
                         PlaneFitOutcome *outcome, std::string *message);
// dmi_capi_speckle.hip: the four passes on a piece, an event before the first and one behind each
hipError_t run_speckle_piece(const SpecklePiece &piece, double threshold, int32_t W, int32_t H, double abs_tolerance, double rel_tolerance,
                             int64_t min_pixels, const SpeckleTuning &tuning, hipStream_t stream, hipEvent_t events[5]);
SpeckleTuning speckle_tuning_from_environment();  // the defaults, unless a tuning build's environment says otherwise
// dmi_capi_holes.hip: the same for the hole fill
hipError_t run_holes_piece(const HolesPiece &piece, double threshold, int32_t W, int32_t H, double abs_tolerance, double rel_tolerance,
                           int64_t max_pixels, hipStream_t stream, hipEvent_t events[5]);
// dmi_capi_smooth.hip: the iterations on a piece, src -> ping -> pong -> ping ...; *result: what the last one wrote
hipError_t run_smooth_piece(const double *src, const double *cost, double threshold, double *ping, double *pong, int32_t *count,
                            int64_t views, int32_t W, int32_t H, const SmoothArgs &args, int32_t iterations, hipStream_t stream,
                            hipEvent_t events[2], const double **result);
// dmi_capi_consistency.hip: the K4 check both camera-reading calls make, their cameras (consistency_cameras, declared where it is
// uploaded: dmi_depth_call.h), and the count launches on flipped planes
int32_t first_view_with_other_k(const double *K4, int32_t n);  // -1: every K4 is of the form SetMatrixK produces
std::string other_k_message(int32_t view);
ConsistencyTuning consistency_tuning_from_environment();
hipError_t run_consistency_count(const double *planes, const ConsistencyCamera *cameras, int32_t n, int32_t W, int32_t H,
                                 double abs_tolerance, double rel_tolerance, const ConsistencyTuning &tuning, int32_t *counts,
                                 unsigned long long *undecided, hipStream_t stream, hipEvent_t events[2]);
// dmi_capi_bounds.hip: the axes (false: one is not finite), and the count and select passes with the state's download
bool bounds_axes(const double *axes9, BoundsAxes *out);
BoundsTuning bounds_tuning_from_environment();
hipError_t run_bounds_select(const double *planes, const ConsistencyCamera *cameras, int32_t n, int32_t W, int32_t H, int32_t pixel_step,
                             const BoundsAxes &axes, double trim_fraction, BoundsState *state, unsigned long long *hist, int compute_units,
                             const BoundsTuning &tuning, hipStream_t stream, hipEvent_t events[2], BoundsState *result);

}  // namespace dmi
