// The growth rules of csrc/dmi_buffer.h against host stand-ins for hipMalloc, hipFree and hipStreamSynchronize
// (tests/cpp/support_host/hip/hip_runtime.h) whose allocator fails on the N-th call, for every N: a unit of four buffers -- the
// views' record arrays -- and a single buffer, each from empty and from an earlier, smaller capacity.  After a failure no buffer
// keeps an old capacity, the byte count is the sum of the capacities, and the same call with a working allocator succeeds; a
// buffer freed twice or never is AddressSanitizer's to report (tests/test_fusion_launch_host.py builds this with it and UBSan).
#include "dmi_buffer.h"

#include <cstdio>
#include <vector>

using dmi::BufferGrowth;
using dmi::DeviceBuffer;

static int failures = 0;
#define EXPECT(cond)                                                       \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("line %d (%s): %s\n", __LINE__, scenario, #cond);        \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

struct Unit {
  std::vector<DeviceBuffer> buffers;
  uint64_t held = 0;
  explicit Unit(size_t n) : buffers(n) {}
  uint64_t sum() const {
    uint64_t s = 0;
    for (const DeviceBuffer &b : buffers) s += b.capacity;
    return s;
  }
  // record sizes of 208, 320, 64 and 208 bytes, as the four arrays of a context (any four distinct sizes would do)
  hipError_t grow(uint64_t records, uint64_t allocate_records, bool *fresh) {
    static const uint64_t size[4] = {208, 320, 64, 208};
    if (buffers.size() == 1) return dmi::grow_idle_buffers({{&buffers[0], records * size[0], allocate_records * size[0]}}, nullptr, held, fresh);
    return dmi::grow_idle_buffers({{&buffers[0], records * size[0], allocate_records * size[0]},
                                   {&buffers[1], records * size[1], allocate_records * size[1]},
                                   {&buffers[2], records * size[2], allocate_records * size[2]},
                                   {&buffers[3], records * size[3], allocate_records * size[3]}}, nullptr, held, fresh);
  }
  bool all_empty() const {
    for (const DeviceBuffer &b : buffers)
      if (b.ptr || b.capacity) return false;
    return true;
  }
  bool all_hold(uint64_t records, uint64_t allocate_records) const {
    static const uint64_t size[4] = {208, 320, 64, 208};
    for (size_t i = 0; i < buffers.size(); ++i)
      if (!buffers[i].ptr || buffers[i].capacity != allocate_records * size[i] || !dmi::holds(buffers[i], records * size[i])) return false;
    return true;
  }
  void release() {
    for (DeviceBuffer &b : buffers) dmi::free_buffers({&b}, held);
  }
};

// `n` buffers, grown from `old_records` (0: from empty) to 70 records allocated as 140, the allocator failing at call `fail_at` of
// the growth (0: never)
static void growth(const char *scenario, size_t n, uint64_t old_records, long fail_at) {
  hip_host = hip_host_state{};
  Unit u(n);
  bool fresh = false;
  if (old_records) {
    EXPECT(u.grow(old_records, 2 * old_records, &fresh) == hipSuccess && fresh);
    EXPECT(u.all_hold(old_records, 2 * old_records) && u.held == u.sum());
    EXPECT(hip_host.synchronizes == 0);   // nothing was in use
    // kept while large enough: not one call of the runtime
    const hip_host_state before = hip_host;
    EXPECT(u.grow(2 * old_records, 4 * old_records, &fresh) == hipSuccess && !fresh);
    EXPECT(hip_host.mallocs == before.mallocs && hip_host.frees == before.frees && hip_host.synchronizes == before.synchronizes);
    EXPECT(u.all_hold(old_records, 2 * old_records));
  }
  const hip_host_state before = hip_host;
  hip_host.fail_malloc_at = fail_at ? before.mallocs + fail_at : 0;
  const hipError_t e = u.grow(70, 140, &fresh);
  hip_host.fail_malloc_at = 0;
  EXPECT(fresh);
  EXPECT(hip_host.synchronizes - before.synchronizes == (old_records ? 1 : 0));   // before a buffer in use is freed, and only then
  EXPECT(u.held == u.sum());
  if (fail_at) {
    EXPECT(e == hipErrorOutOfMemory);
    // every buffer at the new capacity or empty, never at the old one -- and, as a unit, all the same
    for (const DeviceBuffer &b : u.buffers) EXPECT((!b.ptr && b.capacity == 0) || (b.ptr && b.capacity >= 70 * 64));
    EXPECT(u.all_empty());
    EXPECT(u.held == 0);
    EXPECT(u.grow(70, 140, &fresh) == hipSuccess && fresh);   // the same call, a working allocator
  } else {
    EXPECT(e == hipSuccess);
  }
  EXPECT(u.all_hold(70, 140) && u.held == u.sum() && u.held > 0);
  u.release();
  EXPECT(u.all_empty() && u.held == 0);
  EXPECT(hip_host.frees == hip_host.mallocs - (fail_at ? 1 : 0));   // every allocation that succeeded, once
}

// dmi::grow_buffer with the byte count: the plain rule of buffers nothing queued reads
static void plain_growth(long fail_at) {
  const char *scenario = "plain";
  hip_host = hip_host_state{};
  DeviceBuffer b;
  uint64_t held = 0;
  EXPECT(dmi::grow_buffer(b, 100, held) == hipSuccess && b.capacity == 100 && held == 100);
  EXPECT(dmi::grow_buffer(b, 60, held) == hipSuccess && b.capacity == 100 && hip_host.mallocs == 1);   // kept
  hip_host.fail_malloc_at = fail_at ? hip_host.mallocs + fail_at : 0;
  const hipError_t e = dmi::grow_buffer(b, 300, held);
  hip_host.fail_malloc_at = 0;
  EXPECT(hip_host.synchronizes == 0);
  if (fail_at) {
    EXPECT(e == hipErrorOutOfMemory && !b.ptr && b.capacity == 0 && held == 0);
    EXPECT(dmi::grow_buffer(b, 300, held) == hipSuccess);
  }
  EXPECT(b.ptr && b.capacity == 300 && held == 300);
  dmi::free_buffers({&b}, held);
  EXPECT(!b.ptr && held == 0);
}

int main() {
  for (uint64_t old_records : {uint64_t(0), uint64_t(32)}) {
    for (long fail_at = 0; fail_at <= 4; ++fail_at) growth(old_records ? "four buffers, grown" : "four buffers, from empty", 4, old_records, fail_at);
    for (long fail_at = 0; fail_at <= 1; ++fail_at) growth(old_records ? "one buffer, grown" : "one buffer, from empty", 1, old_records, fail_at);
  }
  for (long fail_at = 0; fail_at <= 1; ++fail_at) plain_growth(fail_at);
  std::printf("%d failed\n", failures);
  return failures;
}
