// depth_points_planes.hip -- a plane fitted to the points within a radius of every point of a cloud, the point moved onto it along
// the plane's normal and its normal replaced by the plane's (dmi_fit_point_planes, dmi_views_fit_point_planes): what PCL's
// MovingLeastSquares (order 0, unweighted) and NormalEstimation, or Open3D's estimate_normals, do to a cloud, on the device where
// the resident view set's cloud already is.
//
// Semantics (include/dmi.h states them in full; tests/depth_points_planes_np.py restates them on the CPU over all pairs, without a
// grid, and the result is identical): the members of a point's ball are the radius count's (depth_points_radius.hip), the point
// included; their offsets from the point are rounded to a lattice of 2^-15 of the radius' power of two, so the ten moments of a
// ball are sums of integers, which no order of evaluation changes; the fit from the moments (depth_points_planes_rules.h) is f64
// written down operation for operation (-ffp-contract=off).  The only atomics are integer sums and maxima, one per workgroup and
// counter.
//
// Passes: bounds, keys, sort, ranks and permute are the radius count's (launch_radius_front); then
//   fit      a wave per unit, a lane per query, the count kernel's shape: eighteen binary searches, nine clamped runs, 64 candidates
//            at a time through the wave's own LDS slots, read as broadcasts, between wavefront-scope fences.  A test adds the
//            count and nine moments, in fp64 registers: three lattice offsets (a product and a rounding each), selected to zero
//            outside the ball, three sums and six fused multiply-adds of integers.  Behind the runs the lane fits its plane in
//            registers -- six Jacobi sweeps unrolled --, orients it by the point's old normal and stores to ids[q], in input order,
//            into arrays that are not the ones being read.
#include <algorithm>

#include "depth_points_planes.h"
#include "depth_points_search_device.h"

namespace dmi {
namespace {

using namespace radius_rules;
namespace pl = planes_rules;

__global__ __launch_bounds__(kBlock) void plane_fit_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ ids,
                                                           const uint32_t *__restrict__ start, const double *__restrict__ sorted_xyz,
                                                           uint64_t n, uint64_t n0, uint64_t n1, uint64_t n2, PlaneFitArgs a,
                                                           uint32_t *__restrict__ neighbors, unsigned long long *__restrict__ counters) {
  __shared__ unsigned long long part[kBlock / 64];
  __shared__ double staged[kBlock / 64][64][4];  // a wave's batch of candidates: x, y, z and a word of padding (one b128 and one b64 read)
  double(*const mine)[4] = staged[threadIdx.x >> 6];
  const uint64_t units = counters[kRadiusUnits], waves = (uint64_t)gridDim.x * (kBlock / 64);
  const uint32_t lane = threadIdx.x & 63;
  const double r2 = a.r2, s = a.s;
  unsigned long long tests = 0, fitted = 0, crowded = 0, most = 0, sum = 0, shift = 0;  // this lane's
  for (uint64_t u = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); u < units; u += waves) {  // (the same trips for the whole wave)
    const uint32_t lo = __builtin_amdgcn_readfirstlane(start[u]), k = __builtin_amdgcn_readfirstlane(start[u + 1]) - lo;  // 1 <= k <= 64
    const bool active = lane < k;
    const uint32_t q = lo + (active ? lane : 0u);  // (a query that is there: unused beyond k)
    const double q0 = sorted_xyz[q], q1 = sorted_xyz[n + q], q2 = sorted_xyz[2 * n + q];
    const uint64_t first = keys[lo], last = keys[lo + k - 1];  // the same row: key / n0
    const uint64_t row = first / n0, b0_min = first - row * n0, b0_max = last - row * n0, b2 = row / n1, b1 = row - b2 * n1;
    // lanes 2 t and 2 t + 1 find the run of row t of the nine; an absent row's run is empty
    uint32_t found = 0;
    if (lane < 18) {
      const int t = (int)(lane >> 1);
      uint64_t from = 0, to = 0;
      if (row_key_range(b0_min, b0_max, b1, b2, t % 3 - 1, t / 3 - 1, n0, n1, n2, &from, &to))
        found = lower_bound(keys, n, (lane & 1) ? to + 1 : from);
    }
    uint32_t count = 0;  // the members, the query among them: its offsets are +0
    pl::Moments mo = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const uint32_t sb = (uint32_t)__builtin_amdgcn_readlane((int)found, 2 * t), e = (uint32_t)__builtin_amdgcn_readlane((int)found, 2 * t + 1);
      for (uint64_t base = sb; base < e; base += 64) {
        const uint32_t left = (uint32_t)(e - base);
        const uint32_t here = (uint32_t)__builtin_amdgcn_readfirstlane((int)(left < 64 ? left : 64));  // (uniform: the loop's bound is a scalar)
        const uint64_t c = base + (lane < here ? lane : 0u);  // (a candidate that is there: unused beyond `here`)
        const double c0 = sorted_xyz[c], c1 = sorted_xyz[n + c], c2 = sorted_xyz[2 * n + c];
        // the wave's own 64 slots of LDS, as in the count kernel: a lane writes its candidate, then every lane reads every slot
        wave_fence();  // (the reads of the batch before are done)
        mine[lane][0] = c0, mine[lane][1] = c1, mine[lane][2] = c2;
        wave_fence();
#pragma unroll 4
        for (uint32_t j = 0; j < here; ++j) {
          const double d0 = mine[j][0] - q0, d1 = mine[j][1] - q1, d2 = mine[j][2] - q2;
          const double dd = (d0 * d0 + d1 * d1) + d2 * d2;
          const bool member = dd <= r2;
          // selected, not multiplied: a far candidate's product may be infinite
          const double u0 = member ? pl::lattice_offset(d0, s) : 0.0, u1 = member ? pl::lattice_offset(d1, s) : 0.0,
                       u2 = member ? pl::lattice_offset(d2, s) : 0.0;
          pl::add_member(&mo, u0, u1, u2);
          count += member ? 1u : 0u;
        }
        tests += active ? here : 0u;
      }
    }
    if (active) {
      const uint64_t id = ids[q];
      float rms = -1.f;
      if (pl::crowded(count)) {
        crowded += 1;
      } else if (pl::supported(count, a.min_neighbors)) {
        pl::Plane plane;
        pl::fit_plane(count, mo, &plane);
        double old[3] = {0.0, 0.0, 0.0};
        if (a.normal) {
#pragma unroll
          for (int d = 0; d < 3; ++d) old[d] = (double)a.normal[3 * id + d];
        }
        pl::orient(plane.n, old);
        rms = pl::plane_rms_of(plane.lambda, a.inv_s);
        if (a.flags & pl::kMove) {
          const double t = pl::shift_of(plane, a.inv_s);
          a.out_xyz[3 * id + 0] = pl::moved(q0, t, plane.n[0]);
          a.out_xyz[3 * id + 1] = pl::moved(q1, t, plane.n[1]);
          a.out_xyz[3 * id + 2] = pl::moved(q2, t, plane.n[2]);
          const unsigned long long bits = (unsigned long long)__double_as_longlong(fabs(t));
          shift = bits > shift ? bits : shift;
        }
        if (a.flags & pl::kNormals) {
#pragma unroll
          for (int d = 0; d < 3; ++d) a.out_normal[3 * id + d] = (float)plane.n[d];
        }
        fitted += 1;
      }
      a.plane_rms[id] = rms;
      neighbors[id] = count - 1;
      most = count - 1 > most ? count - 1 : most;
      sum += count - 1;
    }
  }
  const unsigned long long block_tests = block_sum(tests, part), block_fitted = block_sum(fitted, part),
                           block_crowded = block_sum(crowded, part), block_total = block_sum(sum, part),
                           block_most = block_max(most, part), block_shift = block_max(shift, part);
  if (threadIdx.x == 0) {
    if (block_tests) atomicAdd(&counters[kRadiusTests], block_tests);
    if (block_fitted) atomicAdd(&counters[kPlanesFitted], block_fitted);
    if (block_crowded) atomicAdd(&counters[kPlanesCrowded], block_crowded);
    if (block_total) atomicAdd(&counters[kRadiusSum], block_total);
    if (block_most) atomicMax(&counters[kRadiusMost], block_most);
    if (block_shift) atomicMax(&counters[kPlanesShift], block_shift);
  }
}

}  // namespace

hipError_t launch_plane_fit(const double *xyz, uint64_t n, const RadiusGrid &g, const PlaneFitArgs &args, uint32_t group_points,
                            const RadiusScratch &s, hipEvent_t events[6], hipStream_t stream) {
  RadiusSorted sorted{};
  hipError_t e = launch_radius_front(xyz, n, g, group_points, s, events, &sorted, stream);
  if (e != hipSuccess) return e;
  const unsigned fit_blocks = (unsigned)std::min<uint64_t>(std::max<uint64_t>((n + 31) / 32, 1), kCountBlocks);
  hipLaunchKernelGGL(plane_fit_kernel, dim3(fit_blocks), dim3(kBlock), 0, stream, sorted.keys, sorted.ids, s.start, s.sorted_xyz, n, g.n[0],
                     g.n[1], g.n[2], args, s.neighbors, s.counters);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return hipEventRecord(events[5], stream);
}

}  // namespace dmi
