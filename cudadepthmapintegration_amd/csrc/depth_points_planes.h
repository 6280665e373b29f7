// depth_points_planes.h -- the launch of depth_points_planes.hip: a plane fitted to the points within a radius of every point of a
// cloud, the point moved onto it and its normal replaced by the plane's (dmi_fit_point_planes, dmi_views_fit_point_planes;
// include/dmi.h states the definition, DESIGN.md 8q the kernel).  Private: never installed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "depth_points_planes_rules.h"
#include "depth_points_radius.h"

namespace dmi {

// The counters the fit kernel adds to those of the radius search (RadiusCounter; one device array of kThinCounters).  Of the
// search's it leaves kRadiusMost, kRadiusSum and kRadiusTests itself: no flags pass follows it.
enum PlanesCounter {
  kPlanesFitted = 12,   // points with a fit
  kPlanesCrowded = 13,  // points with more than 2^22 members
  kPlanesShift = 14     // the bits of the largest |t| (a non-negative double orders as its bits do)
};

struct PlaneFitArgs {
  double r2, s, inv_s;
  uint32_t min_neighbors, flags;
  const float *normal;  // [n][3] in input order: the old normals, or nullptr (zeros)
  double *out_xyz;      // [n][3]: written for fitted points with kMove; nullptr without it.  Never the cloud the search reads.
  float *out_normal;    // [n][3]: written for fitted points with kNormals; nullptr without it.  Never `normal`.
  float *plane_rms;     // [n]: written for every point
};

// The front passes of the radius search (launch_radius_front: events[0..5)) and the fit kernel behind them, events[5] behind it.
// Leaves scratch.neighbors (input order), args.plane_rms, the outputs asked for and the counters.
hipError_t launch_plane_fit(const double *xyz, uint64_t n, const RadiusGrid &grid, const PlaneFitArgs &args, uint32_t group_points,
                            const RadiusScratch &scratch, hipEvent_t events[6], hipStream_t stream);

}  // namespace dmi
