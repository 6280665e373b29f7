// depth_points_rules_host.cpp -- csrc/depth_points_rules.h on the CPU, built with AddressSanitizer + UBSan by
// tests/test_depth_points_rules_host.py: the choice of tangent over all sixteen patterns of usable neighbours; the blocks the
// compaction cuts views into, at sizes around the block size; a whole count / scan / rank on the host against a plain walk; and
// the byte offsets of the point arrays beyond 2^32 bytes.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "depth_points_rules.h"

using namespace dmi::points_rules;

static int failed = 0, checked = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    ++checked;                                                   \
    if (!(cond)) {                                               \
      ++failed;                                                  \
      std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); \
    }                                                            \
  } while (0)

static void tangents() {
  CHECK(tangent_choice(true, true) == kTangentCentral && tangent_choice(true, false) == kTangentForward);
  CHECK(tangent_choice(false, true) == kTangentBackward && tangent_choice(false, false) == kTangentNone);
  int with_normal = 0, one_sided_count = 0;
  for (unsigned bits = 0; bits < 16; ++bits) {
    const bool right = bits & kUsableRight, left = bits & kUsableLeft, down = bits & kUsableDown, up = bits & kUsableUp;
    const Tangents t = tangents_of(bits);
    // the definition, spelt out: both -> plus minus minus; one -> that one against the centre; none -> no normal
    const Tangent want_x = right && left ? kTangentCentral : right ? kTangentForward : left ? kTangentBackward : kTangentNone;
    const Tangent want_y = down && up ? kTangentCentral : down ? kTangentForward : up ? kTangentBackward : kTangentNone;
    CHECK(t.x == want_x && t.y == want_y);
    CHECK(tangents_exist(t) == ((right || left) && (down || up)));
    CHECK(one_sided(t) == (tangents_exist(t) && !(right && left && down && up)));
    // the ends of the difference: the plus neighbour only if it is usable, the minus one only if it is
    CHECK((tangent_high(t.x) == 1) == right && (tangent_low(t.x) == -1) == left);
    CHECK((tangent_high(t.y) == 1) == down && (tangent_low(t.y) == -1) == up);
    with_normal += tangents_exist(t);
    one_sided_count += one_sided(t);
  }
  CHECK(with_normal == 9 && one_sided_count == 8);
}

static void blocks() {
  struct Case {
    int32_t n, W, H;
    int64_t per_view;
  };
  const Case cases[] = {{1, 1, 1, 1},   {3, 255, 1, 1}, {3, 256, 1, 1}, {3, 257, 1, 2},   {2, 16, 16, 1},
                        {2, 17, 16, 2}, {5, 150, 70, 42}, {256, 1280, 720, 3600}, {7, 32768, 32768, 4194304}};
  for (const Case &c : cases) {
    const int64_t plane = (int64_t)c.W * c.H, per = blocks_per_view(c.W, c.H), total = total_blocks(c.n, c.W, c.H);
    CHECK(per == c.per_view && total == per * c.n && blocks_fit_one_launch(c.n, c.W, c.H));
    // first, last and the blocks around a view's end: every pixel of every view is in exactly one block, in order
    for (const int64_t b : {(int64_t)0, per - 1, per, total - 1}) {
      if (b < 0 || b >= total) continue;
      const int64_t view = block_view(b, per), first = block_first_pixel(b, per);
      const int32_t pixels = block_pixels(b, per, plane);
      CHECK(view >= 0 && view < c.n && first >= 0 && first < plane && pixels >= 1 && pixels <= kBlock);
      CHECK(first + pixels <= plane && (first + pixels == plane) == ((b + 1) % per == 0));
      if ((b + 1) % per != 0) CHECK(pixels == kBlock && block_first_pixel(b + 1, per) == first + kBlock && block_view(b + 1, per) == view);
      else if (b + 1 < total) CHECK(block_first_pixel(b + 1, per) == 0 && block_view(b + 1, per) == view + 1);
    }
    CHECK(scan_chunks(total) * kScanChunk >= total && (scan_chunks(total) - 1) * kScanChunk < total);
  }
  // a block's three counts in one word: every field holds a whole block, four waves' words add without a carry
  for (const uint32_t v : {0u, 1u, 64u, 255u, 256u})
    for (const uint32_t c : {0u, 1u, 256u})
      for (const uint32_t e : {0u, 3u, 256u}) {
        const uint32_t packed = pack_counts(v, c, e);
        CHECK(packed_valid(packed) == v && packed_candidates(packed) == c && packed_emitted(packed) == e);
      }
  const uint32_t wave = pack_counts(64, 64, 64);
  CHECK(packed_valid(4 * wave) == 256 && packed_candidates(4 * wave) == 256 && packed_emitted(4 * wave) == 256);
  CHECK(packed_emitted(pack_counts(256, 256, 0)) == 0 && packed_valid(pack_counts(0, 256, 256)) == 0);
  CHECK(scan_chunks(0) == 0 && scan_chunks(1) == 1 && scan_chunks(kScanChunk) == 1 && scan_chunks(kScanChunk + 1) == 2);
  CHECK(!blocks_fit_one_launch(0x7fffffff, 257, 1) && blocks_fit_one_launch(0x7fffffff, 256, 1));
  CHECK(total_blocks(0x7fffffff, 32768, 32768) == (int64_t)0x7fffffff * 4194304);  // no overflow of 64 bits at the largest set
}

// the four launches on the host, with the rules' arithmetic: flags -> block counts -> exclusive scan chunk by chunk -> ranks
static void compaction(int32_t n, int32_t W, int32_t H, unsigned seed) {
  const int64_t plane = (int64_t)W * H, per = blocks_per_view(W, H), total = total_blocks(n, W, H);
  std::vector<unsigned char> flags((size_t)(n * plane));
  std::srand(seed);
  for (unsigned char &f : flags) f = std::rand() % 3 == 0;
  std::vector<uint32_t> counts((size_t)total);
  for (int64_t b = 0; b < total; ++b) {
    uint32_t c = 0;
    for (int32_t lane = 0; lane < block_pixels(b, per, plane); ++lane)
      c += flags[(size_t)(block_view(b, per) * plane + block_first_pixel(b, per) + lane)];
    counts[(size_t)b] = c;
  }
  std::vector<uint64_t> offsets((size_t)total + 1);
  uint64_t carry = 0;
  for (int64_t chunk = 0; chunk < scan_chunks(total); ++chunk)
    for (int64_t b = chunk * kScanChunk; b < (chunk + 1) * kScanChunk && b < total; ++b) {
      offsets[(size_t)b] = carry;
      carry += counts[(size_t)b];
    }
  offsets[(size_t)total] = carry;
  // a plain walk in (view, pixel) order gives every emitted pixel the same rank
  uint64_t rank = 0;
  bool same = true;
  for (int64_t view = 0; view < n; ++view)
    for (int64_t j = 0; j < plane; ++j) {
      if (!flags[(size_t)(view * plane + j)]) continue;
      const int64_t b = view * per + j / kBlock;
      uint64_t inside = 0;
      for (int64_t k = block_first_pixel(b, per); k < j; ++k) inside += flags[(size_t)(view * plane + k)];
      same = same && block_view(b, per) == view && offsets[(size_t)b] + inside == rank;
      ++rank;
    }
  CHECK(same && rank == carry);
}

static void layouts() {
  Layout l;
  CHECK(layout_of(0, &l) && l.bytes == 0 && l.normal == 0 && l.count == 0);
  for (const uint64_t points : {uint64_t(1), uint64_t(3), uint64_t(255), uint64_t(44965), (uint64_t(1) << 32) / 48 + 1, uint64_t(240000000),
                                uint64_t(1) << 40}) {
    CHECK(layout_of(points, &l));
    CHECK(l.xyz == 0 && l.normal == 24 * points && l.view == l.normal + 12 * points && l.pixel == l.view + 4 * points);
    CHECK(l.count == l.pixel + 4 * points && l.bytes == l.count + 4 * points && l.bytes == kBytesPerPoint * points);
    CHECK(l.normal % 4 == 0 && l.view % 4 == 0 && l.pixel % 4 == 0 && l.count % 4 == 0);
    // the last point's entries end where the next array begins: nothing overlaps and nothing is left over
    const uint64_t last = points - 1;
    CHECK(entry_offset(l.xyz, last, 24) + 24 == l.normal && entry_offset(l.normal, last, 12) + 12 == l.view);
    CHECK(entry_offset(l.view, last, 4) + 4 == l.pixel && entry_offset(l.pixel, last, 4) + 4 == l.count);
    CHECK(entry_offset(l.count, last, 4) + 4 == l.bytes);
    CHECK(entry_offset(l.xyz, last, 24) % 8 == 0);
  }
  // 256 views of 1280 x 720, every pixel a point: the offsets pass 2^32 bytes long before the end
  CHECK(layout_of(uint64_t(256) * 1280 * 720, &l) && l.normal == 5662310400ull && l.bytes == 11324620800ull);
  CHECK(entry_offset(l.count, uint64_t(256) * 1280 * 720 - 1, 4) == 11324620796ull);
  CHECK(layout_of(~uint64_t(0) / 48, &l) && !layout_of(~uint64_t(0) / 48 + 1, &l) && !layout_of(~uint64_t(0), &l));
}

int main() {
  tangents();
  blocks();
  compaction(1, 1, 1, 1);
  compaction(3, 255, 1, 2);
  compaction(3, 256, 1, 3);
  compaction(3, 257, 1, 4);
  compaction(5, 150, 70, 5);
  compaction(2, 640, 480, 6);  // 2400 blocks: more than one chunk of the scan
  layouts();
  std::printf("%d checked, %d failed\n", checked, failed);
  return failed ? 1 : 0;
}
