// The scaffold of the context-free depth-map calls, csrc/dmi_depth_call.h, against the host stand-ins of tests/cpp/support_host/:
// what a call holds is released exactly once whatever way it ends -- the allocator failing at the N-th hipMalloc, for every N over
// the buffers a call grows; a failing device count and an ordinal out of range create nothing --, the staging rule, the checks the
// calls share, and the staged upload's pieces.  A stream, event or buffer freed twice or never is AddressSanitizer's to report
// (tests/test_depth_call_host.py builds this with it and UBSan).
#include "dmi_depth_call.h"

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

static int failures = 0;
static const char *scenario = "";
#define EXPECT(cond)                                                       \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("line %d (%s): %s\n", __LINE__, scenario, #cond);        \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

// ---- the two names of the library the staged upload calls: the cameras as the library builds them, the flip as a record ----
struct Flip {
  int64_t first, count;
  bool with_cost;
  double first_depth;
};
static std::vector<Flip> flips;
namespace dmi {
std::vector<ConsistencyCamera> consistency_cameras(const double *K4, const double *, size_t views) {
  std::vector<ConsistencyCamera> cameras(views);
  for (size_t m = 0; m < views; ++m) cameras[m].k[0] = K4[16 * m];
  return cameras;
}
hipError_t launch_consistency_upload(const double *depth, const double *cost, double, int, int, int64_t count, double *, int64_t first_view,
                                     hipStream_t) {
  flips.push_back({first_view, count, cost != nullptr, depth[0]});
  return hipSuccess;
}
}  // namespace dmi

static bool nothing_left(bool an_allocation_failed = false) {   // every allocation that succeeded freed, once
  return hip_host.frees == hip_host.mallocs - (an_allocation_failed ? 1 : 0) && hip_host.streams_destroyed == hip_host.streams_created &&
         hip_host.events_destroyed == hip_host.events_created;
}

// A call as the entry points make it: named buffers registered with the holdings, opened, grown one after the other; the
// allocator fails at the fail_at-th hipMalloc (0: never)
static void holdings(int n_buffers, int n_events, bool compute_units, long fail_at) {
  scenario = "holdings";
  hip_host = hip_host_state{};
  hip_host.fail_malloc_at = fail_at;
  {
    struct {
      dmi::DeviceBuffer depth, cost, label, record, rim_lo, rim_hi, border_down, border_right, out_size;
    } b;
    dmi::DeviceBuffer *const all[9] = {&b.depth, &b.cost, &b.label, &b.record, &b.rim_lo, &b.rim_hi, &b.border_down, &b.border_right, &b.out_size};
    dmi::CallHoldings h({&b.depth, &b.cost, &b.label, &b.record, &b.rim_lo, &b.rim_hi, &b.border_down, &b.border_right, &b.out_size});
    const dmi::CallFailure f = h.open("dmi_x: ", 0, n_events, compute_units);
    EXPECT(f.code == DMI_OK && f.text.empty());
    // the order every entry point has: count, select, attribute where asked for, stream, events
    EXPECT(hip_host.device_counts == 1 && hip_host.set_devices == 1 && hip_host.attributes == (compute_units ? 1 : 0));
    EXPECT(hip_host.streams_created == 1 && hip_host.events_created == n_events && h.stream != nullptr);
    EXPECT(h.compute_units == (compute_units ? 256 : 0));
    for (int e = 0; e < 5; ++e) EXPECT((h.events[e] != nullptr) == (e < n_events));
    hipError_t e = hipSuccess;
    int grown = 0;
    for (; e == hipSuccess && grown < n_buffers; ++grown) e = dmi::grow_buffer(*all[grown], 64 * (uint64_t)(grown + 1));
    EXPECT((e == hipSuccess) == (fail_at == 0 || fail_at > n_buffers));
    if (e != hipSuccess) EXPECT(e == hipErrorOutOfMemory && grown == fail_at && !all[grown - 1]->ptr && all[grown - 1]->capacity == 0);
    EXPECT(hip_host.synchronizes == 0);
  }  // the call ends here, however it went
  EXPECT(hip_host.synchronizes == 1);  // the stream, once, before anything is freed
  const bool failed = fail_at && fail_at <= n_buffers;
  EXPECT(hip_host.streams_created == 1 && hip_host.events_created == n_events && nothing_left(failed));
  EXPECT(hip_host.mallocs == (failed ? fail_at : n_buffers));
}

static void refused_openings() {
  for (int devices : {-1, 0}) {
    scenario = "no device";
    hip_host = hip_host_state{};
    hip_host.devices = devices;
    dmi::DeviceBuffer depth;
    {
      dmi::CallHoldings h({&depth});
      const dmi::CallFailure f = h.open("dmi_x: ", 0, 5, true);
      EXPECT(f.code == DMI_ERR_DEVICE && f.text == "dmi_x: no HIP device available");
      EXPECT(!h.stream && !h.events[0]);
    }
    EXPECT(hip_host.set_devices == 0 && hip_host.attributes == 0 && hip_host.streams_created == 0 && hip_host.events_created == 0);
    EXPECT(hip_host.mallocs == 0 && hip_host.frees == 0 && hip_host.synchronizes == 0 && hip_host.streams_destroyed == 0);
  }
  for (int device : {-1, 2, 3}) {
    scenario = "ordinal out of range";
    hip_host = hip_host_state{};
    hip_host.devices = 2;
    dmi::DeviceBuffer depth;
    {
      dmi::CallHoldings h({&depth});
      const dmi::CallFailure f = h.open("dmi_x: ", device, 2);
      EXPECT(f.code == DMI_ERR_INVALID_ARGUMENT && f.text == "dmi_x: device ordinal out of range");
    }
    EXPECT(hip_host.set_devices == 0 && hip_host.streams_created == 0 && hip_host.events_created == 0 && hip_host.synchronizes == 0);
  }
  scenario = "the last ordinal";
  hip_host = hip_host_state{};
  hip_host.devices = 2;
  {
    dmi::CallHoldings h({});
    EXPECT(h.open("dmi_x: ", 1, 0).code == DMI_OK && hip_host.events_created == 0 && hip_host.streams_created == 1);
  }
  EXPECT(nothing_left());
}

static void staging_rule() {
  scenario = "staging rule";
  const size_t MiB = size_t(1) << 20;
  EXPECT(dmi::kStageBytes == 256 * MiB);
  EXPECT(dmi::staged_views(300 * MiB, 7) == 1);                  // a plane larger than the stage goes whole
  EXPECT(dmi::staged_views(257 * MiB, 1) == 1);
  EXPECT(dmi::staged_views(64 * MiB, 3) == 3);                   // fewer views than fit
  EXPECT(dmi::staged_views(64 * MiB, 4) == 4 && dmi::staged_views(64 * MiB, 9) == 4);   // an exact division
  EXPECT(dmi::staged_views(100 * MiB, 5) == 2);                  // a remainder of the stage
  EXPECT(dmi::staged_views(8, 5, 24) == 3);                      // 5 views, 3 per piece: pieces of 3 and 2 (below)
  EXPECT(dmi::staged_views(640 * 480 * 8, 64) == 64 && dmi::staged_views(640 * 480 * 8, 200) == 109);
  // the expression the entry points carried, on a sweep of small values
  for (size_t stage = 1; stage <= 40; ++stage)
    for (size_t plane = 1; plane <= 45; ++plane)
      for (size_t views = 1; views <= 12; ++views) {
        const size_t was = std::min(views, std::max<size_t>(1, stage / plane));
        EXPECT(dmi::staged_views(plane, views, stage) == was);
        EXPECT(was >= 1 && was <= views && (was == 1 || was * plane <= stage));
      }
}

static void predicates() {
  scenario = "predicates";
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  EXPECT(dmi::finite_and_not_negative(0.0) && dmi::finite_and_not_negative(-0.0) && dmi::finite_and_not_negative(DBL_MAX));
  EXPECT(dmi::finite_and_not_negative(DBL_MIN) && dmi::finite_and_not_negative(4.9e-324));
  EXPECT(!dmi::finite_and_not_negative(nan) && !dmi::finite_and_not_negative(inf) && !dmi::finite_and_not_negative(-inf));
  EXPECT(!dmi::finite_and_not_negative(-4.9e-324) && !dmi::finite_and_not_negative(-1.0));
  auto is = [](const char *got, const char *want) { return want ? got && !std::strcmp(got, want) : !got; };
  const char *const bad_n = "n >= 1 required", *const bad_w = "W must lie in [1, 32768]", *const bad_h = "H must lie in [1, 32768]";
  for (int32_t side : {1, 2, 32768}) EXPECT(is(dmi::size_refusal(1, side, side), nullptr) && is(dmi::side_refusal(side, 1), nullptr));
  for (int32_t side : {0, -1, 32769, INT32_MAX, INT32_MIN}) {
    EXPECT(is(dmi::size_refusal(1, side, 1), bad_w) && is(dmi::size_refusal(1, 1, side), bad_h));
    EXPECT(is(dmi::size_refusal(1, side, side), bad_w));   // the first that fails
    EXPECT(is(dmi::side_refusal(side, side), bad_w) && is(dmi::side_refusal(32768, side), bad_h));
  }
  for (int32_t n : {0, -1, INT32_MIN}) EXPECT(is(dmi::size_refusal(n, 1, 1), bad_n) && is(dmi::size_refusal(n, 0, 0), bad_n));
  EXPECT(is(dmi::size_refusal(INT32_MAX, 32768, 32768), nullptr));
  const char *const bad_abs = "abs_tolerance must be finite and >= 0", *const bad_rel = "rel_tolerance must be finite and >= 0";
  for (double ok : {0.0, -0.0, 1e-3, DBL_MAX}) EXPECT(is(dmi::tolerance_refusal(ok, ok), nullptr));
  for (double bad : {nan, inf, -inf, -1.0}) {
    EXPECT(is(dmi::tolerance_refusal(bad, 0.0), bad_abs) && is(dmi::tolerance_refusal(0.0, bad), bad_rel));
    EXPECT(is(dmi::tolerance_refusal(bad, bad), bad_abs));   // the first that fails
  }
}

static void spans() {
  scenario = "spans";
  hip_host = hip_host_state{};
  hipEvent_t events[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  double per_pass[4] = {10.0, 20.0, 30.0, 40.0}, sum = 5.0;
  EXPECT(dmi::add_spans(events, 4, per_pass) == hipSuccess && hip_host.elapsed_times == 4);
  EXPECT(per_pass[0] == 11.0 && per_pass[1] == 21.0 && per_pass[2] == 31.0 && per_pass[3] == 41.0);
  EXPECT(dmi::add_spans(events, 4, &sum, 0) == hipSuccess && sum == 9.0);
  EXPECT(dmi::add_spans(events, 0, &sum) == hipSuccess && sum == 9.0 && hip_host.elapsed_times == 8);
}

// 5 views of 3 pixels through a stage of 3 views: pieces of 3 and 2, each flipped from the stage, waited for and timed
static void staged_upload(bool with_cost) {
  scenario = "staged upload";
  hip_host = hip_host_state{};
  flips.clear();
  const int W = 3, H = 1;
  const size_t views = 5, chunk = dmi::staged_views(W * H * 8, views, 3 * W * H * 8);
  EXPECT(chunk == 3);
  std::vector<double> depth(views * W * H), cost(views * W * H, 0.5), K4(views * 16, 0.0), RT(views * 16, 0.0);
  for (size_t i = 0; i < depth.size(); ++i) depth[i] = (double)(i + 1);
  for (size_t m = 0; m < views; ++m) K4[16 * m] = 100.0 + (double)m;
  double ms = 0.0;
  {
    struct {
      dmi::DeviceBuffer planes, cameras, stage_depth, stage_cost;
    } b;
    dmi::CallHoldings h({&b.planes, &b.cameras, &b.stage_depth, &b.stage_cost});
    EXPECT(h.open("dmi_x: ", 0, 2).code == DMI_OK);
    EXPECT(dmi::grow_buffer(b.planes, views * W * H * 8) == hipSuccess && dmi::grow_buffer(b.cameras, views * sizeof(dmi::ConsistencyCamera)) == hipSuccess);
    EXPECT(dmi::grow_buffer(b.stage_depth, chunk * W * H * 8) == hipSuccess);   // exactly a piece: ASan sees a copy beyond it
    if (with_cost) EXPECT(dmi::grow_buffer(b.stage_cost, chunk * W * H * 8) == hipSuccess);
    EXPECT(dmi::upload_cameras(b.cameras, K4.data(), RT.data(), views, h.stream) == hipSuccess);
    EXPECT(hip_host.copies == 1 && hip_host.synchronizes == 1 && b.cameras.as<dmi::ConsistencyCamera>()[4].k[0] == 104.0);
    EXPECT(dmi::upload_flipped(depth.data(), with_cost ? cost.data() : nullptr, 0.25, W, H, views, chunk, b.stage_depth, b.stage_cost,
                               b.planes.as<double>(), h.stream, h.events, &ms) == hipSuccess);
  }
  EXPECT(flips.size() == 2);
  if (flips.size() == 2) {
    EXPECT(flips[0].first == 0 && flips[0].count == 3 && flips[0].first_depth == 1.0 && flips[0].with_cost == with_cost);
    EXPECT(flips[1].first == 3 && flips[1].count == 2 && flips[1].first_depth == 10.0 && flips[1].with_cost == with_cost);
  }
  EXPECT(hip_host.copies == 1 + (with_cost ? 4 : 2) && hip_host.elapsed_times == 2 && ms == 2.0);
  EXPECT(hip_host.synchronizes == 1 + 2 + 1);   // the cameras, every piece, the call's end
  EXPECT(nothing_left());
}

int main() {
  // the nine buffers of the hole fill with five events, the four of the smoothing with two, the six of the bounds with the compute
  // units read, the two of the thinning with no event: the allocator failing at every one of them, and never
  for (long fail_at = 0; fail_at <= 9; ++fail_at) holdings(9, 5, false, fail_at);
  for (long fail_at = 0; fail_at <= 4; ++fail_at) holdings(4, 2, false, fail_at);
  for (long fail_at = 0; fail_at <= 6; ++fail_at) holdings(6, 2, true, fail_at);
  for (long fail_at = 0; fail_at <= 2; ++fail_at) holdings(2, 0, false, fail_at);
  refused_openings();
  staging_rule();
  predicates();
  spans();
  staged_upload(false);
  staged_upload(true);
  std::printf("%d failed\n", failures);
  return failures;
}
