// scene_bounds_rules_host.cpp -- csrc/scene_bounds_rules.h on the CPU, built with AddressSanitizer + UBSan by
// tests/test_scene_bounds_host.py: the key and its inverse at the sign boundary, the trimmed rank at its edges, and the step of the
// radix select -- the bin that holds a rank and the rank left in it -- with the rank on a bin's first and last element and empty
// bins around it; then a whole select, digit by digit, against std::sort.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "scene_bounds_rules.h"

using namespace dmi::bounds_rules;

static int failed = 0, checked = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    ++checked;                                                   \
    if (!(cond)) {                                               \
      ++failed;                                                  \
      std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); \
    }                                                            \
  } while (0)

static void keys() {
  const double inf = std::numeric_limits<double>::infinity(), denormal = std::numeric_limits<double>::denorm_min();
  const double ordered[] = {-inf, -std::numeric_limits<double>::max(), -1.0, -denormal, -0.0, 0.0, denormal, 1.0,
                            std::numeric_limits<double>::max(), inf};
  for (size_t i = 0; i + 1 < sizeof(ordered) / sizeof(ordered[0]); ++i) CHECK(key_of(ordered[i]) < key_of(ordered[i + 1]));
  for (const double v : ordered) {
    const double back = value_of(key_of(v));
    CHECK(back == v && std::signbit(back) == std::signbit(v));
  }
  // the sign boundary: the largest key of a negative number and the smallest of a non-negative one are neighbours
  CHECK(key_of(-0.0) == 0x7fffffffffffffffull);
  CHECK(key_of(0.0) == 0x8000000000000000ull);
  CHECK(key_of(-0.0) + 1 == key_of(0.0));
  CHECK(std::signbit(value_of(0x7fffffffffffffffull)) && value_of(0x7fffffffffffffffull) == 0.0);
  CHECK(!std::signbit(value_of(0x8000000000000000ull)) && value_of(0x8000000000000000ull) == 0.0);
  CHECK(value_of(0x7ffffffffffffffeull) == -denormal && value_of(0x8000000000000001ull) == denormal);
  for (const uint64_t bits : {0ull, 1ull, 0x8000000000000000ull, 0x8000000000000001ull, 0x7ff0000000000000ull, 0xfff0000000000000ull,
                              0xffffffffffffffffull, 0x7fffffffffffffffull, 0x3ff0000000000000ull})
    CHECK(bits_of_key(key_of_bits(bits)) == bits);
  // digits and prefixes
  const uint64_t key = 0x0123456789abcdefull;
  CHECK(digit_of(key, 0) == 0x01 && digit_of(key, 3) == 0x67 && digit_of(key, kPasses - 1) == 0xef);
  CHECK(prefix_of(key, 0) == 0 && prefix_of(key, 1) == 0x01 && prefix_of(key, kPasses - 1) == 0x0123456789abcdull);
  CHECK(kPasses * kDigitBits == 64 && kBins == 1 << kDigitBits);
}

static void ranks() {
  CHECK(trim_rank(0.25, 8) == 2);        // trim * N an exact integer
  CHECK(trim_rank(0.125, 24) == 3);
  CHECK(trim_rank(0.1, 10) == 1);        // 0.1 * 10 rounds to exactly 1
  CHECK(trim_rank(0.1, 9) == 0);         // just below one
  CHECK(trim_rank(std::nextafter(0.25, 0.0), 4) == 0);
  CHECK(trim_rank(std::nextafter(0.25, 0.0), 8) == 1);
  CHECK(trim_rank(0.0, 1) == 0 && trim_rank(0.5, 1) == 0 && trim_rank(0.3, 1) == 0);   // N = 1: lo and hi are the one element
  CHECK(trim_rank(0.0, 2) == 0 && trim_rank(0.5, 2) == 0 && trim_rank(0.49, 2) == 0);  // N = 2: rank 0 and rank 1
  CHECK(trim_rank(0.5, 3) == 1 && trim_rank(0.5, 4) == 1 && trim_rank(0.5, 5) == 2);   // trim 0.5: the median(s)
  CHECK(trim_rank(0.5, 1001) == 500 && trim_rank(0.5, 1000) == 499);
  CHECK(trim_rank(0.0, 0) == 0 && trim_rank(0.5, 0) == 0);
  CHECK(trim_rank(0.5, (uint64_t(1) << 53) - 1) == ((uint64_t(1) << 53) - 2) / 2);
  CHECK(trim_rank(0.005, 19660800) == 98304);
  for (const uint64_t n : {1ull, 2ull, 3ull, 10ull, 1000003ull})
    for (const double trim : {0.0, 0.005, 0.25, 0.5}) CHECK(trim_rank(trim, n) <= n - 1 - trim_rank(trim, n));  // lo's rank <= hi's
}

static void bins() {
  std::vector<uint64_t> hist(kBins, 0);
  hist[3] = 5;
  hist[4] = 0;
  hist[7] = 1;
  hist[200] = 4;
  hist[kBins - 1] = 2;  // 12 elements: ranks 0..4 in bin 3, 5 in bin 7, 6..9 in bin 200, 10..11 in the last bin
  uint64_t left = 99;
  CHECK(bin_of_rank(hist.data(), kBins, 0, &left) == 3 && left == 0);     // a bin's first element, empty bins before it
  CHECK(bin_of_rank(hist.data(), kBins, 4, &left) == 3 && left == 4);     // its last
  CHECK(bin_of_rank(hist.data(), kBins, 5, &left) == 7 && left == 0);     // a bin of one, empty bins on both sides
  CHECK(bin_of_rank(hist.data(), kBins, 6, &left) == 200 && left == 0);
  CHECK(bin_of_rank(hist.data(), kBins, 9, &left) == 200 && left == 3);
  CHECK(bin_of_rank(hist.data(), kBins, 10, &left) == kBins - 1 && left == 0);
  CHECK(bin_of_rank(hist.data(), kBins, 11, &left) == kBins - 1 && left == 1);
  left = 99;
  CHECK(bin_of_rank(hist.data(), kBins, 12, &left) == -1 && left == 99);  // past the end: nothing written
  CHECK(bin_of_rank(hist.data(), kBins, ~uint64_t(0), &left) == -1 && left == 99);
  std::vector<uint64_t> none(kBins, 0);
  CHECK(bin_of_rank(none.data(), kBins, 0, &left) == -1);
  std::vector<uint64_t> one(kBins, 0);
  one[0] = uint64_t(1) << 40;  // counts beyond 32 bits
  one[1] = 1;
  CHECK(bin_of_rank(one.data(), kBins, (uint64_t(1) << 40) - 1, &left) == 0 && left == (uint64_t(1) << 40) - 1);
  CHECK(bin_of_rank(one.data(), kBins, uint64_t(1) << 40, &left) == 1 && left == 0);
  CHECK(bin_of_rank(one.data(), 1, uint64_t(1) << 40, &left) == -1);      // only the bins it was given
}

// the whole select as the device runs it, pass by pass, for every rank of a small sample with both signs, zeros and neighbours
static void select() {
  std::vector<double> values = {-3.5, 2.0, -0.0, 0.0, 2.0, std::nextafter(2.0, 3.0), 1e-310, -1e-310, 5e6, 5e6 + 1.0 / 1024, -5e6, 0.75,
                                0.75, 0.75, -1.0};
  std::vector<uint64_t> keys;
  for (const double v : values) keys.push_back(key_of(v));
  std::vector<uint64_t> sorted = keys;
  std::sort(sorted.begin(), sorted.end());
  for (uint64_t rank = 0; rank < keys.size(); ++rank) {
    uint64_t prefix = 0, left = rank;
    for (int pass = 0; pass < kPasses; ++pass) {
      std::vector<uint64_t> hist(kBins, 0);
      for (const uint64_t k : keys)
        if (prefix_of(k, pass) == prefix) ++hist[digit_of(k, pass)];
      const int bin = bin_of_rank(hist.data(), kBins, left, &left);
      CHECK(bin >= 0);
      if (bin < 0) return;
      prefix = (prefix << kDigitBits) | (uint64_t)bin;
    }
    CHECK(prefix == sorted[rank]);
  }
}

int main() {
  keys();
  ranks();
  bins();
  select();
  std::printf("%d checked, %d failed\n", checked, failed);
  return failed ? 1 : 0;
}
