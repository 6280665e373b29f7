// depth_smooth_rules_host.cpp -- csrc/depth_smooth_rules.h on the CPU, stand-alone: built with AddressSanitizer and
// UBSan by tests/test_depth_smooth_rules_host.py and run.  The radius rule at its edges, the weights against exp in long double,
// and the refusals, which must write nothing.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "depth_smooth_rules.h"

static int checks = 0, failed = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    ++checks;                                                    \
    if (!(cond)) {                                               \
      ++failed;                                                  \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);      \
    }                                                            \
  } while (0)

namespace {

constexpr double kSentinel = -77.0;
constexpr int kRoom = dmi::kDepthSmoothMaxRadius + 1;

struct Result {
  int code;
  int32_t radius;
  double weights[kRoom + 1];  // one more than the rule may write: the last stays the sentinel
};

Result call(double sigma, double truncate) {
  Result r;
  r.radius = -5;
  for (double &w : r.weights) w = kSentinel;
  r.code = dmi::depth_smoothing_weights(sigma, truncate, &r.radius, r.weights);
  return r;
}

bool untouched(const Result &r) {
  if (r.radius != -5) return false;
  for (const double w : r.weights)
    if (w != kSentinel) return false;
  return true;
}

double ulp(double x) { return std::nextafter(x, std::numeric_limits<double>::infinity()) - x; }

void accepted(double sigma, double truncate, int radius) {
  const Result r = call(sigma, truncate);
  CHECK(r.code == 0);
  CHECK(r.radius == radius);
  CHECK(r.weights[0] == 1.0);
  for (int i = 1; i <= radius && i < kRoom; ++i) {
    const double argument = -(double)(i * i) / (2 * sigma * sigma);  // the rule's own, rounded in double: exp's error is what is tested
    const long double exact = std::exp((long double)argument);
    const double w = r.weights[i];
    CHECK(std::fabs((long double)w - exact) <= (long double)ulp((double)exact));
    CHECK(w > 0.0 && w < 1.0 && w < r.weights[i - 1]);
  }
  for (int i = radius + 1; i <= kRoom; ++i) CHECK(r.weights[i] == kSentinel);  // nothing beyond s[r]
}

void refused(double sigma, double truncate) {
  const Result r = call(sigma, truncate);
  CHECK(r.code == 1);
  CHECK(untouched(r));
}

}  // namespace

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  static_assert(dmi::kDepthSmoothMaxRadius == 8, "the header's limit");

  // the radius: truncate * sigma exactly integral is that integer, the least bit more is the next
  accepted(1.5, 2.0, 3);
  accepted(std::nextafter(1.5, 2.0), 2.0, 4);
  accepted(std::nextafter(1.5, 1.0), 2.0, 3);
  accepted(1.0, 1.0, 1);
  accepted(0.5, 2.0, 1);
  accepted(0.25, 2.0, 1);
  accepted(1.0, 3.0, 3);
  accepted(0.0, 2.0, 0);   // r == 0: s[0] = 1 and no quotient 0 / 0
  accepted(0.0, 4.0, 0);
  // r = 8 against 8 + epsilon
  accepted(4.0, 2.0, 8);
  accepted(2.0, 4.0, 8);
  accepted(8.0, 1.0, 8);
  refused(std::nextafter(4.0, 5.0), 2.0);
  refused(2.0, std::nextafter(4.0, 5.0));  // truncate above 4 as well
  refused(std::nextafter(8.0, 9.0), 1.0);
  refused(4.5, 2.0);
  refused(1e300, 4.0);

  // sigma and truncate outside the definition
  refused(-1.0, 2.0);
  refused(-0.5, 2.0);
  refused(nan, 2.0);
  refused(inf, 2.0);
  refused(-inf, 2.0);
  refused(1.0, 0.0);
  refused(1.0, -1.0);
  refused(1.0, 4.5);
  refused(1.0, nan);
  refused(1.0, inf);

  // null pointers: refused, and the other argument is not written
  {
    int32_t radius = -5;
    double weights[kRoom];
    for (double &w : weights) w = kSentinel;
    CHECK(dmi::depth_smoothing_weights(1.0, 2.0, nullptr, weights) == 1);
    CHECK(dmi::depth_smoothing_weights(1.0, 2.0, &radius, nullptr) == 1);
    CHECK(radius == -5);
    for (const double w : weights) CHECK(w == kSentinel);
  }

  // a tiny sigma: the exponent overflows to -inf and the weight is exactly 0, not a NaN
  {
    const Result r = call(1e-300, 1.0);
    CHECK(r.code == 0 && r.radius == 1 && r.weights[1] == 0.0);
  }

  std::printf("%d checks, %d failed\n", checks, failed);
  return failed ? 1 : 0;
}
