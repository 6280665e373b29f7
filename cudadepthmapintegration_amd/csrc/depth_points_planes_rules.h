// depth_points_planes_rules.h -- the rules of dmi_fit_point_planes / dmi_views_fit_point_planes that are plain arithmetic
// (include/dmi.h states the definition, DESIGN.md 8q the kernel): the lattice of a radius, what a member adds to the moments, the
// plane fit from the moments operation for operation, the orientation of its normal and the results.  No HIP types: the kernel of
// depth_points_planes.hip and the host program tests/cpp/depth_points_planes_rules_host.cpp compile the same text, both with
// -ffp-contract=off: every operation below is rounded on its own.  The moments are sums of integers held in doubles; their
// fused multiply-adds are exact and written out as such.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>

#include "depth_points_radius_rules.h"

namespace dmi {
namespace planes_rules {

constexpr uint32_t kMove = 1, kNormals = 2;      // DMI_PLANE_FIT_MOVE, DMI_PLANE_FIT_NORMALS
constexpr uint32_t kMaxMembers = 1u << 22;       // a ball of more members is crowded: its sums could pass 2^52
constexpr int kSweeps = 6;

// ---- step 2: the lattice.  radius = f 2^e with f in [0.5, 1): s = 2^(15 - e), inv_s = 2^(e - 15); |d| <= radius (1 + 2^-51)
// gives |rint(d s)| <= 2^15 ----
struct Lattice {
  double s, inv_s;
};
inline bool normal_and_finite(double x) { return x >= std::numeric_limits<double>::min() && x <= std::numeric_limits<double>::max(); }
inline bool lattice_of(double radius, Lattice *out) {  // false: s or inv_s is not a normal finite number
  int e = 0;
  (void)std::frexp(radius, &e);
  out->s = std::ldexp(1.0, 15 - e);
  out->inv_s = std::ldexp(1.0, e - 15);
  return normal_and_finite(out->s) && normal_and_finite(out->inv_s);
}

// ---- step 3: the moments of a ball: m members, S_k = sum q_k, T = sum q_a q_b in the order 00 01 02 11 12 22, integers all ----
struct Moments {  // named, not arrays: they stay in registers
  double s0, s1, s2, t00, t01, t02, t11, t12, t22;
};
DMI_THIN_HD inline double lattice_offset(double d, double s) { return rint(d * s); }  // ties to even
// one member's offsets added: every sum stays an integer below 2^52 while m <= 2^22, so the adds and FMAs are exact
DMI_THIN_HD inline void add_member(Moments *a, double q0, double q1, double q2) {
  a->s0 += q0, a->s1 += q1, a->s2 += q2;
  a->t00 = fma(q0, q0, a->t00), a->t01 = fma(q0, q1, a->t01), a->t02 = fma(q0, q2, a->t02);
  a->t11 = fma(q1, q1, a->t11), a->t12 = fma(q1, q2, a->t12), a->t22 = fma(q2, q2, a->t22);
}

// which points are fitted
DMI_THIN_HD inline bool crowded(uint64_t m) { return m > kMaxMembers; }
DMI_THIN_HD inline bool supported(uint64_t m, uint32_t min_neighbors) { return m - 1 >= min_neighbors; }

// ---- step 4: the fit ----
struct Plane {
  double c[3];     // the centroid's offset from the point, in lattice units
  double n[3];     // the unit normal, not yet oriented
  double lambda;   // the smallest eigenvalue, in lattice units squared
};

// one Jacobi rotation of the pair (p, q), r the third index, on scalars (the matrices stay in registers): app, aqq, apq, arp, arq of
// the symmetric A, and the columns p and q of V
DMI_THIN_HD inline __attribute__((always_inline)) void rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p, double &v0q, double &v1p,
                               double &v1q, double &v2p, double &v2q) {
  const double a = apq;
  if (a == 0.0) return;
  const double theta = (aqq - app) / (2.0 * a);
  const double root = sqrt(theta * theta + 1.0);
  const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + root);  // (an infinite theta theta: +-0)
  const double c = 1.0 / sqrt(t * t + 1.0), sigma = t * c;
  const double ta = t * a;
  app = app - ta;
  aqq = aqq + ta;
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - sigma * rq;
  arq = sigma * rp + c * rq;
  const double p0 = v0p, q0 = v0q, p1 = v1p, q1 = v1q, p2 = v2p, q2 = v2q;
  v0p = c * p0 - sigma * q0, v0q = sigma * p0 + c * q0;
  v1p = c * p1 - sigma * q1, v1q = sigma * p1 + c * q1;
  v2p = c * p2 - sigma * q2, v2q = sigma * p2 + c * q2;
}

DMI_THIN_HD inline __attribute__((always_inline)) void fit_plane(uint64_t m, const Moments &a, Plane *out) {
  const double count = (double)m;
  const double c0 = a.s0 / count, c1 = a.s1 / count, c2 = a.s2 / count;
  out->c[0] = c0, out->c[1] = c1, out->c[2] = c2;
  double a00 = a.t00 / count - c0 * c0, a01 = a.t01 / count - c0 * c1, a02 = a.t02 / count - c0 * c2;
  double a11 = a.t11 / count - c1 * c1, a12 = a.t12 / count - c1 * c2, a22 = a.t22 / count - c2 * c2;
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;  // V[row][column]
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int sweep = 0; sweep < kSweeps; ++sweep) {
    rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0, 1), r = 2
    rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0, 2), r = 1
    rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1, 2), r = 0
  }
  // the column of the smallest eigenvalue, the lowest index at ties
  const bool one = a11 < a00;
  double lambda = one ? a11 : a00, n0 = one ? v01 : v00, n1 = one ? v11 : v10, n2 = one ? v21 : v20;
  const bool two = a22 < lambda;
  lambda = two ? a22 : lambda, n0 = two ? v02 : n0, n1 = two ? v12 : n1, n2 = two ? v22 : n2;
  const double length = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
  out->n[0] = n0 / length, out->n[1] = n1 / length, out->n[2] = n2 / length;
  out->lambda = lambda;
}

// ---- step 5: the side of the old normal o; without one (g == 0) the component of largest magnitude becomes positive ----
DMI_THIN_HD inline void orient(double n[3], const double o[3]) {
  const double g = (n[0] * o[0] + n[1] * o[1]) + n[2] * o[2];
  bool negate = g < 0.0;
  if (g == 0.0) {
    double most = n[0];
    if (fabs(n[1]) > fabs(most)) most = n[1];
    if (fabs(n[2]) > fabs(most)) most = n[2];
    negate = most < 0.0;
  }
  if (negate) n[0] = -n[0], n[1] = -n[1], n[2] = -n[2];
}

// ---- step 6: the results ----
DMI_THIN_HD inline float plane_rms_of(double lambda, double inv_s) { return (float)(sqrt(lambda > 0.0 ? lambda : 0.0) * inv_s); }
DMI_THIN_HD inline double shift_of(const Plane &p, double inv_s) { return ((p.c[0] * p.n[0] + p.c[1] * p.n[1]) + p.c[2] * p.n[2]) * inv_s; }
DMI_THIN_HD inline double moved(double x, double t, double n) { return x + t * n; }

// ---- what a call holds on the device beside the cloud it reads and the cloud it writes: the radius search's 56 bytes a point (its
// counts are this stage's neighbors) and plane_rms f32: 60 bytes a point ----
DMI_THIN_HD inline uint64_t scratch_bytes(uint64_t points) { return radius_rules::scratch_bytes(points) + 4 * points; }

}  // namespace planes_rules
}  // namespace dmi
