// depth_smooth_rules.h -- the host arithmetic of the depth smoothing (include/dmi.h: dmi_depth_smoothing_weights): the
// radius and the spatial weights of one axis.  Needs nothing but <cmath>, so the command line's parser checks a radius with the
// library's own rule without linking the library.  No HIP types.  Private: never installed.
#pragma once
#include <cmath>
#include <cstdint>

namespace dmi {

constexpr int kDepthSmoothMaxRadius = 8;
constexpr int kDepthSmoothMaxIterations = 16;

// r = (int)ceil(truncate * sigma); s[0] = 1, s[i] = exp(-(double)(i*i) / (2*sigma*sigma)) into weights[0..r]: NOT normalised, the
// filter's quotient cancels any scale.  0, or 1 for a null pointer, a sigma that is not finite and >= 0, a truncate that is not
// finite and in (0, 4], and a radius above kDepthSmoothMaxRadius (nothing is written then).
inline int depth_smoothing_weights(double sigma, double truncate, int32_t *radius, double *weights) {
  if (!radius || !weights) return 1;
  if (!std::isfinite(sigma) || sigma < 0.0 || !std::isfinite(truncate) || !(truncate > 0.0) || truncate > 4.0) return 1;
  const double reach = std::ceil(truncate * sigma);
  if (reach > (double)kDepthSmoothMaxRadius) return 1;
  const int r = (int)reach;
  weights[0] = 1.0;  // exp(-0 / ...), also for sigma == 0 (r == 0), where the quotient would be 0 / 0
  for (int i = 1; i <= r; ++i) weights[i] = std::exp(-(double)(i * i) / (2 * sigma * sigma));
  *radius = r;
  return 0;
}

}  // namespace dmi
