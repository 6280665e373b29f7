// scene_bounds_rules.h -- the rules of dmi_estimate_scene_bounds that are plain integer arithmetic (include/dmi.h states the
// definition, DESIGN.md 8h the kernels): the order-preserving key of an f64 and its inverse, the trimmed rank k from trim_fraction
// and N, and the step of a most-significant-digit radix select -- which bin of a digit's histogram holds rank r, and what rank is
// left inside it.  No HIP types: the select kernel of scene_bounds.hip and the host program tests/cpp/scene_bounds_rules_host.cpp
// compile the same text.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define DMI_BOUNDS_HD __host__ __device__
#else
#define DMI_BOUNDS_HD
#endif

namespace dmi {
namespace bounds_rules {

constexpr int kDigitBits = 8;                 // the key is consumed from its top in digits of this many bits ...
constexpr int kPasses = 64 / kDigitBits;      // ... in this many passes
constexpr int kBins = 1 << kDigitBits;
constexpr int kTargets = 6;                   // target 2a is lo of axis a, target 2a + 1 its hi

// ascending key order is numeric order of the doubles the bits stand for, -0.0 before +0.0 (negative NaNs first, positive NaNs
// last: the kernel never orders one)
DMI_BOUNDS_HD inline uint64_t key_of_bits(uint64_t bits) { return bits ^ ((bits >> 63) ? ~uint64_t(0) : (uint64_t(1) << 63)); }
DMI_BOUNDS_HD inline uint64_t bits_of_key(uint64_t key) { return key ^ ((key >> 63) ? (uint64_t(1) << 63) : ~uint64_t(0)); }

inline uint64_t key_of(double v) {
  uint64_t bits;
  std::memcpy(&bits, &v, 8);
  return key_of_bits(bits);
}
inline double value_of(uint64_t key) {
  const uint64_t bits = bits_of_key(key);
  double v;
  std::memcpy(&v, &bits, 8);
  return v;
}

// k = min((uint64_t)(trim_fraction * (double)N), (N - 1) / 2): lo is the element of rank k, hi the one of rank N - 1 - k.
// trim_fraction lies in [0, 0.5] and N below 2^53 (the entry point refuses everything else), so the conversion cannot overflow.
DMI_BOUNDS_HD inline uint64_t trim_rank(double trim_fraction, uint64_t n) {
  if (n == 0) return 0;
  const uint64_t k = (uint64_t)(trim_fraction * (double)n), half = (n - 1) / 2;
  return k < half ? k : half;
}

// The bin of hist[0 .. bins) that holds the element of 0-based rank `rank` when the bins are laid end to end, and in *remaining
// that element's rank inside the bin.  -1 (and *remaining untouched) when the histogram holds no more than `rank` elements.
DMI_BOUNDS_HD inline int bin_of_rank(const uint64_t *hist, int bins, uint64_t rank, uint64_t *remaining) {
  uint64_t before = 0;
  for (int b = 0; b < bins; ++b) {
    const uint64_t c = hist[b];
    if (rank - before < c) {  // before <= rank always holds here
      *remaining = rank - before;
      return b;
    }
    before += c;
  }
  return -1;
}

// the digit of `key` that pass p (0 = the top digit) looks at, and the key's bits above that digit
DMI_BOUNDS_HD inline int digit_of(uint64_t key, int pass) { return (int)((key >> (64 - kDigitBits * (pass + 1))) & (kBins - 1)); }
DMI_BOUNDS_HD inline uint64_t prefix_of(uint64_t key, int pass) { return pass == 0 ? 0 : key >> (64 - kDigitBits * pass); }

}  // namespace bounds_rules
}  // namespace dmi
