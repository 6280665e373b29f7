// depth_points_thin_rules_host.cpp -- csrc/depth_points_thin_rules.h on the CPU, built with AddressSanitizer + UBSan by
// tests/test_depth_points_thin_rules_host.py: the bin limit at its edge, keys and their bits up to the largest grid, the byte
// offsets of the output arrays beyond 2^32 bytes and against the build's layout, the wave pass's threshold, the queue's capacity
// against the worst distribution of cell sizes, and a whole head / rank / start / kept numbering on the host against a plain walk.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "depth_points_rules.h"
#include "depth_points_thin_rules.h"

using namespace dmi::thin_rules;

static int failed = 0, checked = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    ++checked;                                                   \
    if (!(cond)) {                                               \
      ++failed;                                                  \
      std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); \
    }                                                            \
  } while (0)

static void bins() {
  CHECK(bins_of_top(0.0) == 1 && bins_of_top(1.0) == 2 && bins_of_top(2097151.0) == kMaxBins);
  CHECK(bins_of_top(2097152.0) == 0 && bins_of_top(1e300) == 0);
  CHECK(bins_of_top(INFINITY) == 0 && bins_of_top(NAN) == 0 && bins_of_top(-1.0) == 0);
  // the smallest accepted cell size of an extent, as the entry points find it, gives exactly 2^21 bins
  for (double extent : {1.0, 3.0, 0.7, 1234.5678, 5e-7}) {
    double least = extent / 2097152.0;
    while (!(std::floor(extent / least) < 2097152.0)) least = std::nextafter(least, INFINITY);
    CHECK(bins_of_top(std::floor(extent / least)) == kMaxBins);
    CHECK(bins_of_top(std::floor(extent / std::nextafter(least, 0.0))) == 0);
  }
}

static void keys() {
  CHECK(bits_for(0) == 1 && bits_for(1) == 1 && bits_for(2) == 2 && bits_for(3) == 2 && bits_for(4) == 3);
  CHECK(bits_for((uint64_t(1) << 32) - 1) == 32 && bits_for(uint64_t(1) << 32) == 33 && bits_for(~uint64_t(0)) == 64);
  CHECK(key_bits(1, 1, 1) == 1 && key_bits(2, 1, 1) == 1 && key_bits(3, 1, 1) == 2 && key_bits(2, 2, 2) == 3 && key_bits(3, 3, 3) == 5);
  CHECK(key_bits(kMaxBins, kMaxBins, kMaxBins) == 63);
  // the largest key of the largest grid stays below 2^63 and is the last of its order
  const uint64_t top = kMaxBins - 1;
  CHECK(key_of(top, top, top, kMaxBins, kMaxBins) == (uint64_t(1) << 63) - 1);
  // the key orders cells by (b_2, b_1, b_0), and distinct cells have distinct keys
  const uint64_t n0 = 5, n1 = 3, n2 = 4;
  uint64_t expected = 0;
  for (uint64_t b2 = 0; b2 < n2; ++b2)
    for (uint64_t b1 = 0; b1 < n1; ++b1)
      for (uint64_t b0 = 0; b0 < n0; ++b0) CHECK(key_of(b0, b1, b2, n0, n1) == expected++);
  CHECK(expected - 1 < (uint64_t(1) << key_bits(n0, n1, n2)));
}

static void layouts() {
  for (uint64_t q : {uint64_t(0), uint64_t(1), uint64_t(257), uint64_t(1) << 27, (uint64_t(1) << 32) - 1}) {
    Layout t;
    dmi::points_rules::Layout b;
    CHECK(layout_of(q, &t) && dmi::points_rules::layout_of(q, &b));
    // the first five arrays stand where the build's layout has them: dmi_views_download_points serves either cloud
    CHECK(t.xyz == b.xyz && t.normal == b.normal && t.view == b.view && t.pixel == b.pixel && t.count == b.count);
    CHECK(t.members == b.bytes && t.bytes == t.members + 4 * q && t.bytes == kBytesPerPoint * q);
    CHECK(t.xyz % 8 == 0 && t.normal % 4 == 0 && t.members % 4 == 0);
    // no two arrays overlap
    CHECK(t.xyz + 24 * q == t.normal && t.normal + 12 * q == t.view && t.view + 4 * q == t.pixel && t.pixel + 4 * q == t.count &&
          t.count + 4 * q == t.members);
  }
  Layout t;
  CHECK(!layout_of(~uint64_t(0) / kBytesPerPoint + 1, &t) && layout_of(~uint64_t(0) / kBytesPerPoint, &t));
}

static void wave_pass() {
  CHECK(!wave_cell(1, 1) && wave_cell(2, 1) && !wave_cell(32, 32) && wave_cell(33, 32) && !wave_cell(0, 1));
  CHECK(wave_chunks(1) == 1 && wave_chunks(64) == 1 && wave_chunks(65) == 2 && wave_chunks(128) == 2 && wave_chunks(129) == 3);
  CHECK(wave_chunks(0xffffffffu) == 67108864u);
  // the queue holds every cell above the threshold whatever the cell sizes are: the worst case is all of them threshold + 1
  for (uint32_t threshold : {1u, 4u, 32u, 1000u, 0xffffffffu})
    for (uint64_t points : {uint64_t(1), uint64_t(2), uint64_t(33), uint64_t(66), uint64_t(3000), (uint64_t(1) << 32) - 1}) {
      const uint64_t worst = points / ((uint64_t)threshold + 1);
      CHECK(wave_queue_capacity(points, threshold) >= worst && wave_queue_capacity(points, threshold) >= 1);
      CHECK(wave_queue_capacity(points, threshold) <= std::max<uint64_t>(points / 2, 1));
    }
  CHECK(scratch_bytes(1000, 32) == 16 * 1001 + 8 * 1000 + 4 * 1001 + 40 * 1000 + 4 * 30 + 128);
  CHECK(scratch_bytes((uint64_t(1) << 32) - 1, 1) < (uint64_t(1) << 39));  // 68 bytes a point and the queue: no overflow
}

// the ranks pass on the host, array for array as depth_points_thin.hip runs it, against a plain walk over the sorted keys
static void numbering(unsigned seed, size_t n, uint64_t distinct, uint32_t min_points, uint32_t threshold) {
  std::srand(seed);
  std::vector<uint64_t> keys(n);
  for (uint64_t &k : keys) k = (uint64_t)std::rand() % distinct;
  std::sort(keys.begin(), keys.end());
  std::vector<uint32_t> head(n), rank(n), start(n + 1, 0xdeadbeefu), kept(n + 1), out_index(n + 1);
  for (size_t i = 0; i < n; ++i) head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
  uint32_t sum = 0;
  for (size_t i = 0; i < n; ++i) rank[i] = (sum += head[i]);
  for (size_t i = 0; i < n; ++i) {
    const uint32_t c = rank[i] - 1;
    if (head[i]) start[c] = (uint32_t)i;
    if (i == n - 1) start[c + 1] = (uint32_t)n;
  }
  const uint32_t cells = rank[n - 1];
  uint64_t queued = 0, largest = 0;
  for (size_t c = 0; c <= n; ++c) {
    uint32_t k = 0;
    if (c < n && c < cells) k = start[c + 1] - start[c];
    kept[c] = k >= min_points && k > 0 ? 1u : 0u;
    if (kept[c] && wave_cell(k, threshold)) ++queued;
    largest = std::max<uint64_t>(largest, k);
  }
  sum = 0;
  for (size_t c = 0; c <= n; ++c) {
    out_index[c] = sum;
    sum += kept[c];
  }
  // the plain walk
  uint64_t want_cells = 0, want_kept = 0, want_largest = 0, members = 0;
  for (size_t i = 0; i < n;) {
    size_t j = i;
    while (j < n && keys[j] == keys[i]) ++j;
    CHECK(start[want_cells] == i && start[want_cells + 1] == j);
    CHECK(kept[want_cells] == (j - i >= min_points ? 1u : 0u) && out_index[want_cells] == want_kept);
    want_kept += j - i >= min_points;
    want_largest = std::max<uint64_t>(want_largest, j - i);
    members += j - i;
    ++want_cells;
    i = j;
  }
  CHECK(cells == want_cells && out_index[n] == want_kept && largest == want_largest && members == n);
  CHECK(queued <= wave_queue_capacity(n, threshold));
}

int main() {
  bins();
  keys();
  layouts();
  wave_pass();
  numbering(1, 1, 1, 1, 1);
  numbering(2, 2, 1, 1, 1);
  numbering(3, 255, 40, 1, 4);
  numbering(4, 256, 40, 3, 4);
  numbering(5, 257, 300, 2, 1);
  numbering(6, 3000, 27, 1, 32);
  numbering(7, 3000, 5000, 1, 1);
  numbering(8, 1000, 1, 5, 32);
  std::printf("%d checked, %d failed\n", checked, failed);
  return failed ? 1 : 0;
}
