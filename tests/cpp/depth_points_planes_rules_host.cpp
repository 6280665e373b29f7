// depth_points_planes_rules_host.cpp -- csrc/depth_points_planes_rules.h on the CPU, built with AddressSanitizer + UBSan by
// tests/test_depth_points_planes_rules_host.py: the lattice at powers of two and one ulp either side, |q| <= 2^15 on adversarial
// offsets, the fit on zero, rank-one, diagonal and equal-eigenvalue matrices, the crowded rule at 2^22 and 2^22 + 1 members (from
// moments: no cloud of that size is built), and, behind the line "FITS", a fixed list of moments and old normals (13 numbers) with
// the fit's outputs for them (8 numbers) as hex floats, which the Python test compares bit for bit with the numpy restatement.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <limits>

#include "depth_points_planes_rules.h"

using namespace dmi::planes_rules;

static int failed = 0, checked = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    ++checked;                                                   \
    if (!(cond)) {                                               \
      ++failed;                                                  \
      std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); \
    }                                                            \
  } while (0)

static void lattices() {
  Lattice l;
  for (int e = -900; e <= 900; e += 17) {
    const double p = std::ldexp(1.0, e);  // radius = 0.5 * 2^(e + 1)
    CHECK(lattice_of(p, &l) && l.s == std::ldexp(1.0, 14 - e) && l.inv_s == std::ldexp(1.0, e - 14) && l.s * l.inv_s == 1.0);
    CHECK(lattice_of(std::nextafter(p, 2 * p), &l) && l.s == std::ldexp(1.0, 14 - e));
    CHECK(lattice_of(std::nextafter(p, 0.0), &l) && l.s == std::ldexp(1.0, 15 - e));  // one ulp below: the finer lattice
    // the radius itself lies in [2^14, 2^15) lattice units
    CHECK(p * std::ldexp(1.0, 14 - e) == 16384.0 && std::nextafter(p, 0.0) * std::ldexp(1.0, 15 - e) < 32768.0);
  }
  CHECK(lattice_of(0.1, &l) && l.s == 262144.0 && l.inv_s == 1.0 / 262144.0);  // 0.1 = 0.8 * 2^-3
  CHECK(lattice_of(0.05, &l) && l.s == 524288.0);
  // s or inv_s leaves the normal numbers: refused, though the radius count accepts the radius
  CHECK(dmi::radius_rules::radius_accepted(1e-153) && dmi::radius_rules::radius_accepted(1e153));
  CHECK(lattice_of(std::ldexp(1.0, -510), &l) && lattice_of(std::ldexp(1.0, 510), &l));
  CHECK(lattice_of(std::numeric_limits<double>::max(), &l) && l.s == std::ldexp(1.0, -1009));
  CHECK(!lattice_of(std::ldexp(1.0, -1009), &l) && lattice_of(std::ldexp(1.0, -1008), &l));
}

static void offsets_stay_within_2_to_15() {
  for (double radius : {1.0, 0.75, 0.1, 0.05, 3.0e-7, 12345.678, std::nextafter(1.0, 0.0), std::nextafter(0.5, 1.0), 0.5, 5.0 * 0x1p30}) {
    Lattice l;
    CHECK(lattice_of(radius, &l));
    const double most = radius * (1.0 + 0x1p-51);  // what a member's |d_k| can reach
    for (double d : {most, -most, radius, -radius, std::nextafter(most, 0.0), radius * 0.5, 0.0, -0.0}) {
      const double q = lattice_offset(d, l.s);
      CHECK(std::fabs(q) <= 32768.0 && q == std::rint(q));
    }
    CHECK(lattice_offset(0.5 * l.inv_s, l.s) == 0.0 && lattice_offset(1.5 * l.inv_s, l.s) == 2.0 && lattice_offset(-2.5 * l.inv_s, l.s) == -2.0);  // ties to even
  }
}

static Moments moments_of(const double (*q)[3], int n) {
  Moments a = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < n; ++i) add_member(&a, q[i][0], q[i][1], q[i][2]);
  return a;
}

static void fits() {
  Plane p;
  // zero: every member at the point.  No rotation happens; the first axis, positive.
  Moments zero = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  fit_plane(5, zero, &p);
  const double none[3] = {0.0, 0.0, 0.0};
  orient(p.n, none);
  CHECK(p.n[0] == 1.0 && p.n[1] == 0.0 && p.n[2] == 0.0 && p.lambda == 0.0 && shift_of(p, 1.0) == 0.0 && plane_rms_of(p.lambda, 1.0) == 0.f);
  // diagonal: points on the axes; z has the least spread
  const double axes[6][3] = {{8, 0, 0}, {-8, 0, 0}, {0, 4, 0}, {0, -4, 0}, {0, 0, 1}, {0, 0, -1}};
  fit_plane(6, moments_of(axes, 6), &p);
  CHECK(p.n[0] == 0.0 && p.n[1] == 0.0 && p.n[2] == 1.0 && p.lambda == 2.0 / 6.0 && p.c[0] == 0.0);
  const double down[3] = {0.0, 0.0, -1.0};
  orient(p.n, down);
  CHECK(p.n[2] == -1.0);
  // a plane z = 16 above the point: the shift is the centroid's height, the residual zero
  const double lifted[5][3] = {{0, 0, 0}, {32, 0, 16}, {-32, 0, 16}, {0, 32, 16}, {0, -32, 16}};
  Moments m = moments_of(lifted + 1, 4);
  fit_plane(4, m, &p);
  orient(p.n, none);
  CHECK(p.n[2] == 1.0 && p.lambda == 0.0 && shift_of(p, 0.5) == 8.0 && moved(1.0, 8.0, p.n[2]) == 9.0);
  // rank one: points on a line.  Two eigenvalues vanish; the normal is a unit vector orthogonal to the line.
  const double line[5][3] = {{-6, -8, 0}, {-3, -4, 0}, {0, 0, 0}, {3, 4, 0}, {6, 8, 0}};
  fit_plane(5, moments_of(line, 5), &p);
  CHECK(std::fabs(p.n[0] * 3 + p.n[1] * 4) < 1e-14 && std::fabs((p.n[0] * p.n[0] + p.n[1] * p.n[1] + p.n[2] * p.n[2]) - 1.0) < 1e-15);
  CHECK(std::fabs(p.lambda) < 1e-12);
  // equal eigenvalues: the corners of a cube.  C is diagonal already: the lowest index wins.
  double cube[8][3];
  for (int i = 0; i < 8; ++i)
    for (int k = 0; k < 3; ++k) cube[i][k] = (i >> k & 1) ? 5 : -5;
  fit_plane(8, moments_of(cube, 8), &p);
  CHECK(p.n[0] == 1.0 && p.n[1] == 0.0 && p.n[2] == 0.0 && p.lambda == 25.0);
  // orientation without an old normal: the largest component becomes positive, the lowest index at ties
  double n[3] = {-0.6, 0.0, 0.8};
  orient(n, none);
  CHECK(n[2] == 0.8);
  double tie[3] = {-0.7071067811865476, 0.7071067811865476, 0.0};
  orient(tie, none);
  CHECK(tie[0] > 0.0 && tie[1] < 0.0);
}

static void crowds() {
  CHECK(!crowded(kMaxMembers) && crowded((uint64_t)kMaxMembers + 1) && !crowded(1));
  CHECK(supported(3, 2) && !supported(2, 2) && !supported(1, 2));
  // 2^22 members at the corners (+-2^15)^3: every sum is an integer at most 2^52, exact; the fit is the cube's
  const double top = 32768.0, each = (double)(kMaxMembers / 8);
  Moments a = {0.0, 0.0, 0.0, 8 * each * top * top, 0.0, 0.0, 8 * each * top * top, 0.0, 8 * each * top * top};
  CHECK(a.t00 == 0x1p52 && a.t00 + 1.0 != a.t00 - 1.0);
  Plane p;
  fit_plane(kMaxMembers, a, &p);
  CHECK(p.lambda == top * top && p.n[0] == 1.0);
  // one member more at a corner could not be added exactly to every sum: the point is left out, not fitted
  Moments b = a;
  add_member(&b, top, top, top);
  CHECK(b.t00 == 0x1p52 + 0x1p30 && crowded((uint64_t)kMaxMembers + 1));
}

// m, S[3], T[6], old normal[3]: balls of a noisy cap, ties, zeros, large counts
static const double kCases[][13] = {
    {5, 3, -2, 7, 1021, 33, -412, 977, 120, 300, 0, 0, 1},
    {3, 0, 0, 0, 200, 100, 0, 50, 0, 0, 0, 0, 0},
    {7, 12040, -33011, 402, 90211733, -40112, 5530021, 188020113, -70114, 3302113, 0.5, -0.5, 0.70703125},
    {4, 0, 0, 0, 100, 0, 0, 100, 0, 100, 0, 0, 0},
    {9, 10, 20, 30, 4000, 3000, 2000, 5000, 1000, 6000, -1, 0, 0},
    {6, -196608, 196608, 0, 6442450944.0, -6442450944.0, 0, 6442450944.0, 0, 0, 0, 0, -1},
    {4194304, 1234567, -7654321, 424242, 1125899906842624.0, -55555555555.0, 77777777777.0, 2251799813685248.0, 1234567891.0, 562949953421312.0, 0.25, 0.25, 0.25},
    {12, 5, 5, 5, 1000, 1000, 1000, 1000, 1000, 1000, 0, 0, 0},
    {3, 3, 3, 3, 5, 3, 3, 3, 3, 3, 0, 1, 0},
    {10, -31, 17, 2, 64021, -20110, 140, 33017, -212, 96, 0, 0, -0.001},
};

int main() {
  lattices();
  offsets_stay_within_2_to_15();
  fits();
  crowds();
  std::printf("FITS\n");
  const double inv_s = 0x1p-18;
  for (const auto &c : kCases) {
    const Moments a = {c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9]};
    Plane p;
    fit_plane((uint64_t)c[0], a, &p);
    const double old[3] = {c[10], c[11], c[12]};
    orient(p.n, old);
    const double t = shift_of(p, inv_s);
    for (double x : c) std::printf("%a ", x);
    std::printf("%a %a %a %a %a %a %a %a\n", p.n[0], p.n[1], p.n[2], p.lambda, t, (double)plane_rms_of(p.lambda, inv_s), moved(1.25, t, p.n[0]),
                moved(-3.5, t, p.n[2]));
  }
  std::printf("%d checked, %d failed\n", checked, failed);
  return failed ? 1 : 0;
}
