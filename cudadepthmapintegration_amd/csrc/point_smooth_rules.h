// point_smooth_rules.h -- the host arithmetic of the point smoothing (include/dmi.h: dmi_point_smoothing_weights): the
// radius and the normalised weights of one axis.  Needs nothing but <cmath>, so the command line's parser checks a radius with the
// library's own rule without linking the library.  Private: never installed.
#pragma once
#include <cmath>
#include <cstdint>

namespace dmi {

constexpr int kPointSmoothMaxRadius = 16;

// r = (int)ceil(truncate * sigma); w_i = exp(-(double)(i*i) / (2*sigma*sigma)), S = w_0 + 2*(((w_1 + w_2) + ...) + w_r), k_i = w_i / S
// into weights[0..r].  0, or 1 for a null pointer, a sigma that is not finite and >= 0, a truncate that is not finite and in (0, 4],
// and a radius above kPointSmoothMaxRadius (nothing is written then).
inline int point_smoothing_weights(double sigma, double truncate, int32_t *radius, double *weights) {
  if (!radius || !weights) return 1;
  if (!std::isfinite(sigma) || sigma < 0.0 || !std::isfinite(truncate) || !(truncate > 0.0) || truncate > 4.0) return 1;
  const double reach = std::ceil(truncate * sigma);
  if (reach > (double)kPointSmoothMaxRadius) return 1;
  const int r = (int)reach;
  double w[kPointSmoothMaxRadius + 1];
  w[0] = 1.0;  // exp(-0 / ...), also for sigma == 0 (r == 0), where the quotient would be 0 / 0
  for (int i = 1; i <= r; ++i) w[i] = std::exp(-(double)(i * i) / (2 * sigma * sigma));
  double side = 0.0;  // ((w_1 + w_2) + ...) + w_r
  for (int i = 1; i <= r; ++i) side = i == 1 ? w[1] : side + w[i];
  const double S = w[0] + 2 * side;
  for (int i = 0; i <= r; ++i) weights[i] = w[i] / S;
  *radius = r;
  return 0;
}

}  // namespace dmi
