// rounded_quotient.h -- std::round(num / den) as a pixel index, with and without the correctly rounded division: shared by the
// mesh coloration (coloration_kernels.hip) and the support count of the iso-surface (isosurface_support.hip), which select a
// vertex's pixel in a view the same way.  Device code, inline in every translation unit that uses it.
#pragma once

#include <hip/hip_runtime.h>

namespace dmi {

__device__ __forceinline__ bool to_pixel(double u, int &p) {  // round half away from zero; NaN/inf/|x| >= 2^31 outside
  const double r = round(u);
  if (!(r > -2147483648.0 && r < 2147483648.0)) return false;
  p = (int)r;
  return true;
}

// std::round(num / den) as an int (RD.cxx:177-181) without the correctly rounded division, when that provably changes
// nothing: r = 1/den from the hardware seed and two Newton steps, its residual 1 - den*r CHECKED to be below 2^-40, so
// ua = num*r is within |Q| * 2^-39 of the real quotient Q and within 2^-21 of the reference's q = fl(num/den) as long as
// |ua| < 2^16; if ua is further than 2^-20 from every half-integer, q lies on the same side of the same half-integers
// and rounds -- half away from zero or not, no tie is near -- to the integer nearest to ua.  Everything else (a pixel
// coordinate beyond 65 536, a near-tie, a zero / tiny / NaN denominator) takes the division.  Two quotients share r.
struct FastQuotient {
  double r;
  bool usable;
  __device__ __forceinline__ explicit FastQuotient(double den) {
    double x = __builtin_amdgcn_rcp(den);
    x = __builtin_fma(__builtin_fma(-den, x, 1.0), x, x);
    x = __builtin_fma(__builtin_fma(-den, x, 1.0), x, x);
    r = x;
    usable = __builtin_fabs(__builtin_fma(-den, x, 1.0)) < 0x1p-40;  // NaN: false
  }
  __device__ __forceinline__ bool round_to_pixel(double num, double den, int &p) const {
    const double ua = num * r;
    const double fl = __builtin_floor(ua), fr = ua - fl;  // fr in [0, 1), exact
    if (usable && __builtin_fabs(ua) < 65536.0 && __builtin_fabs(fr - 0.5) > 0x1p-20) {
      p = (int)fl + (fr > 0.5 ? 1 : 0);
      return true;
    }
    return to_pixel(num / den, p);
  }
  // The same for a numerator and a denominator that are only NEAR the reference's (each within the bounds behind
  // `margin` = (E_num + 65537 E_den)): |num/den - num_ref/den_ref| <= (E_num + |u| E_den) / |den| with |u| < 2^16, so
  // ua is within margin * |r| + 2^-21 of the reference's quotient; accepted iff further than that + 2^-21 from every
  // half-integer.  false = not decided (the caller takes the reference's own expression).
  __device__ __forceinline__ bool round_to_pixel_near(double num, double margin, int &p) const {
    const double ua = num * r;
    const double fl = __builtin_floor(ua), fr = ua - fl;
    const double reach = __builtin_fma(margin, __builtin_fabs(r), 0x1p-20);
    if (usable && __builtin_fabs(ua) < 65536.0 && __builtin_fabs(fr - 0.5) > reach) {  // a NaN margin or r: not taken
      p = (int)fl + (fr > 0.5 ? 1 : 0);
      return true;
    }
    return false;
  }
};

}  // namespace dmi
