// What the mesh stages share, csrc/dmi_mesh_stage.h, against the host stand-ins of tests/cpp/support_host/: a stage's events are
// created all or none -- the creation failing at the N-th event, for every N -- and destroyed exactly once; the times read from
// them; every size refusal on both sides of its bound, with the texts the stages carried before they shared them; the commit of a
// stage's result for every row of the drop table, with and without normals; the carving of a scratch buffer against the
// expressions it replaced.  An event destroyed twice or never is AddressSanitizer's to report (tests/test_mesh_stage_host.py
// builds this with it and UBSan).  The size limits cannot be reached on a device in a test: this is where they are pinned.
#include "dmi_mesh_stage.h"

#include <cstdio>
#include <string>

static int failures = 0;
static const char *scenario = "";
#define EXPECT(cond)                                                       \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("line %d (%s): %s\n", __LINE__, scenario, #cond);        \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

template <int Events, int Passes>
static void event_creation() {
  scenario = "event creation";
  for (long fail_at = 0; fail_at <= Events; ++fail_at) {
    hip_host = hip_host_state{};
    hip_host.fail_event_create_at = fail_at;
    dmi::StageTimes<Events, Passes> t;
    const hipError_t first = t.create();
    EXPECT((first == hipSuccess) == (fail_at == 0));
    if (fail_at) {  // none is left, and those that had been created are gone
      EXPECT(first == hipErrorOutOfMemory && hip_host.events_created == fail_at - 1 && hip_host.events_destroyed == fail_at - 1);
      for (hipEvent_t e : t.events) EXPECT(e == nullptr);
      EXPECT(t.create() == hipSuccess);  // the next call starts over
      EXPECT(hip_host.event_creations == fail_at + Events);
    }
    EXPECT(hip_host.events_created - hip_host.events_destroyed == Events);
    for (hipEvent_t e : t.events) EXPECT(e != nullptr);
    const long calls = hip_host.event_creations;
    EXPECT(t.create() == hipSuccess && hip_host.event_creations == calls);  // lazy: they are there
    EXPECT(hip_host.events_without_timing == 0);
    t.release();
    EXPECT(hip_host.events_destroyed == hip_host.events_created);
    for (hipEvent_t e : t.events) EXPECT(e == nullptr);
    t.release();  // nothing left to destroy
    EXPECT(hip_host.events_destroyed == hip_host.events_created);
  }
}

static void event_flags() {
  scenario = "event flags";
  hip_host = hip_host_state{};
  dmi::StageTimes<1> wait;  // the coloration's: what another stream waits for
  EXPECT(wait.create(hipEventDisableTiming) == hipSuccess && hip_host.events_created == 1 && hip_host.events_without_timing == 1);
  wait.release();
  hip_host.fail_event_create_at = hip_host.event_creations + 1;
  EXPECT(wait.create(hipEventDisableTiming) == hipErrorOutOfMemory && wait.events[0] == nullptr);
  EXPECT(hip_host.events_destroyed == hip_host.events_created);
}

static void reading_times() {
  scenario = "reading times";
  hip_host = hip_host_state{};
  dmi::StageTimes<4, 3> t;
  EXPECT(t.create() == hipSuccess);
  const float ticks[4] = {0.25f, 1.75f, 4.25f, 10.25f};
  for (int e = 0; e < 4; ++e) {
    hip_host.clock = ticks[e];
    EXPECT(hipEventRecord(t.events[e], nullptr) == hipSuccess);
  }
  t.last_kernel_ms = -1.0;
  t.last_pass_ms = {-1.0, -1.0, -1.0};
  EXPECT(t.read(0, 3) == hipSuccess && hip_host.elapsed_times == 4);
  EXPECT(t.last_kernel_ms == 10.0 && t.last_pass_ms[0] == 1.5 && t.last_pass_ms[1] == 2.5 && t.last_pass_ms[2] == 6.0);
  for (int n_passes = 0; n_passes <= 3; ++n_passes) {  // the support stage without a trim: one pass, the others exactly 0
    t.last_pass_ms = {-1.0, -1.0, -1.0};
    EXPECT(t.read(0, n_passes ? n_passes : 1, n_passes) == hipSuccess);
    EXPECT(t.last_kernel_ms == (double)(ticks[n_passes ? n_passes : 1] - ticks[0]));
    for (int p = 0; p < 3; ++p) EXPECT(t.last_pass_ms[p] == (p < n_passes ? (double)(ticks[p + 1] - ticks[p]) : 0.0));
  }
  double span = -1.0;
  EXPECT(t.elapsed(1, 3, &span) == hipSuccess && span == 8.5);  // the decimation's: not consecutive
  EXPECT(t.read(1, 3, 2) == hipSuccess && t.last_kernel_ms == 8.5 && t.last_pass_ms[0] == 2.5 && t.last_pass_ms[1] == 6.0 && t.last_pass_ms[2] == 0.0);
  t.zero();
  EXPECT(t.last_kernel_ms == 0.0 && !std::signbit(t.last_kernel_ms));
  for (double p : t.last_pass_ms) EXPECT(p == 0.0 && !std::signbit(p));
  t.release();
  dmi::StageTimes<2> plain;  // no passes: the kernels' time alone
  EXPECT(plain.create() == hipSuccess);
  EXPECT(hipEventRecord(plain.events[0], nullptr) == hipSuccess && hipEventRecord(plain.events[1], nullptr) == hipSuccess);
  EXPECT(plain.read(0, 1) == hipSuccess && plain.last_kernel_ms == 1.0 && plain.last_pass_ms.empty());
  plain.zero();
  EXPECT(plain.last_kernel_ms == 0.0);
  plain.release();
  EXPECT(hip_host.events_destroyed == hip_host.events_created);
}

static void size_refusals() {
  scenario = "size refusals";
  const uint64_t two32 = uint64_t(1) << 32, two31 = uint64_t(1) << 31;
  // the texts of the stages before they shared them, behind "<entry>: "
  const struct {
    const char *what, *text;
  } ids[] = {{"32-bit component labels", "mesh too large for 32-bit component labels"}, {"32-bit vertex ids", "mesh too large for 32-bit vertex ids"}};
  for (const auto &c : ids) {
    EXPECT(dmi::ids_refusal(0, 0, c.what).empty() && dmi::ids_refusal(two32 - 1, two32 - 1, c.what).empty());
    EXPECT(dmi::ids_refusal(two32, 0, c.what) == c.text && dmi::ids_refusal(0, two32, c.what) == c.text);
    EXPECT(dmi::ids_refusal(two32, two32 - 1, c.what) == c.text && dmi::ids_refusal(two32 - 1, two32, c.what) == c.text);
    EXPECT(dmi::ids_refusal(UINT64_MAX, UINT64_MAX, c.what) == c.text);
  }
  const uint64_t sixth = 715827883, third = 1431655766;  // the least T with 6 T >= 2^32, with 3 T >= 2^32
  EXPECT(6 * (sixth - 1) < two32 && 6 * sixth >= two32 && 3 * (third - 1) < two32 && 3 * third >= two32);
  const struct {
    uint64_t factor, least;
    const char *what, *text;
  } products[] = {
      {6, sixth, "32-bit adjacency offsets (6 x triangles >= 2^32)", "mesh too large for 32-bit adjacency offsets (6 x triangles >= 2^32)"},
      {6, sixth, "32-bit edge positions (6 x triangles >= 2^32)", "mesh too large for 32-bit edge positions (6 x triangles >= 2^32)"},
      {3, third, "32-bit corner indices (3 T >= 2^32)", "mesh too large for 32-bit corner indices (3 T >= 2^32)"}};
  for (const auto &c : products) {
    EXPECT(dmi::product_refusal(c.factor, 0, c.what).empty() && dmi::product_refusal(c.factor, c.least - 1, c.what).empty());
    EXPECT(dmi::product_refusal(c.factor, c.least, c.what) == c.text && dmi::product_refusal(c.factor, two32 - 1, c.what) == c.text);
  }
  EXPECT(dmi::direction_bit_refusal(0).empty() && dmi::direction_bit_refusal(two31 - 1).empty());
  EXPECT(dmi::direction_bit_refusal(two31) == "mesh too large for the edge keys' direction bit (vertices >= 2^31)");
  EXPECT(dmi::direction_bit_refusal(two32 - 1) == dmi::direction_bit_refusal(two31));
  const std::string filled = "the filled mesh would be too large for 32-bit ids (vertices or 6 x triangles >= 2^32)";
  EXPECT(dmi::filled_refusal(two32 - 1, sixth - 1).empty() && dmi::filled_refusal(1, 1).empty());
  EXPECT(dmi::filled_refusal(two32, 1) == filled && dmi::filled_refusal(1, sixth) == filled && dmi::filled_refusal(1, two32) == filled);
  const uint64_t most = (uint64_t)INT64_MAX / (3 * sizeof(double));  // what the extraction's byte sizes allow
  EXPECT(dmi::extraction_refusal(most, most).empty() && dmi::extraction_refusal(0, 0).empty());
  EXPECT(dmi::extraction_refusal(most + 1, 0) == "mesh too large for int64 ids" && dmi::extraction_refusal(0, most + 1) == "mesh too large for int64 ids");
}

// the six buffers as numbers, so that where each ends up can be read off
static dmi::DeviceBuffer tagged(uintptr_t tag) {
  dmi::DeviceBuffer b;
  b.ptr = reinterpret_cast<void *>(tag);
  b.capacity = 100 * tag;
  return b;
}
static bool is(const dmi::DeviceBuffer &b, uintptr_t tag) { return b.ptr == reinterpret_cast<void *>(tag) && b.capacity == 100 * tag; }
static dmi::MeshState hand_made(bool normals) {
  dmi::MeshState m;
  m.vertices = tagged(1), m.triangles = tagged(2), m.normals = tagged(3);
  m.alt_vertices = tagged(4), m.alt_triangles = tagged(5), m.alt_normals = tagged(6);
  m.n_vertices = 10, m.n_triangles = 20, m.regions = 7;
  m.valid = true, m.has_normals = normals, m.filtered = true, m.colored = true, m.support_counted = true;
  return m;
}
static bool flags_after(const dmi::MeshState &m, dmi::MeshDrops what) {
  return m.valid && m.filtered == !what.regions && m.regions == (what.regions ? 0u : 7u) && m.colored == !what.colors &&
         m.support_counted == !what.support;
}

static void commits() {
  scenario = "commit";
  // every row, as the stages' tails stood: {regions, colours, support counts} dropped
  const struct {
    dmi::MeshDrops row;
    bool regions, colors, support;
  } table[] = {{dmi::MeshDrops{false, false, false}, false, false, false},   {dmi::drops::kComponents, false, true, true},
               {dmi::drops::kSmoothing, false, true, true},   {dmi::drops::kDecimation, true, true, true},
               {dmi::drops::kFill, true, true, true},         {dmi::drops::kSupportTrim, true, true, false}};
  for (const auto &c : table) {
    EXPECT(c.row.regions == c.regions && c.row.colors == c.colors && c.row.support == c.support);
    for (bool normals : {false, true}) {
      dmi::MeshState m = hand_made(normals);
      m.commit_alternates(3, 4, c.row);
      EXPECT(is(m.vertices, 4) && is(m.alt_vertices, 1) && is(m.triangles, 5) && is(m.alt_triangles, 2));
      EXPECT(is(m.normals, normals ? 6 : 3) && is(m.alt_normals, normals ? 3 : 6));
      EXPECT(m.n_vertices == 3 && m.n_triangles == 4 && m.has_normals == normals && flags_after(m, c.row));
      // the smoother's: the positions from one of two buffers, the triangles and the counts as they were
      m = hand_made(normals);
      dmi::DeviceBuffer own = tagged(9);
      m.commit_positions(own, c.row);
      EXPECT(is(m.vertices, 9) && is(own, 1) && is(m.alt_vertices, 4) && is(m.triangles, 2) && is(m.alt_triangles, 5));
      EXPECT(is(m.normals, normals ? 6 : 3) && is(m.alt_normals, normals ? 3 : 6));
      EXPECT(m.n_vertices == 10 && m.n_triangles == 20 && flags_after(m, c.row));
      // the branches that swap nothing
      m = hand_made(normals);
      m.drop(c.row);
      EXPECT(is(m.vertices, 1) && is(m.triangles, 2) && is(m.normals, 3) && is(m.alt_vertices, 4) && is(m.alt_triangles, 5) && is(m.alt_normals, 6));
      EXPECT(m.n_vertices == 10 && m.n_triangles == 20 && flags_after(m, c.row));
    }
  }
  dmi::MeshState fresh = hand_made(false);  // a drop of regions that are not there stays a drop
  fresh.filtered = false;
  fresh.drop(dmi::drops::kDecimation);
  EXPECT(!fresh.filtered && fresh.regions == 0);
}

static void carving() {
  scenario = "carving";
  EXPECT(dmi::kComponentsLanes == 4 && dmi::kSmoothingLanes == 3 && dmi::kDecimationLanes == 8 && dmi::kDecimationTriangleLanes == 2);
  EXPECT(dmi::kHolesLanes == 5 && dmi::kHolesLoopLanes == 11 && dmi::kSupportLanes == 2);
  static uint32_t storage[11 * 66];
  for (uint64_t nv : {0, 1, 63, 64, 65}) {
    const dmi::U32Lanes lanes{storage, nv + 1};
    for (int i = 0; i < 11; ++i) EXPECT(lanes.lane(i) == storage + (uint64_t)i * (nv + 1));
    const uint64_t nt = nv, fixed_words = (nv + 63) / 64;
    const uint32_t n_slots = (uint32_t)nv;
    // the sizes the stages asked of ensure_buffers
    EXPECT(lanes.bytes(dmi::kComponentsLanes) == (nv + 1) * 16);
    EXPECT(fixed_words * 8 + lanes.bytes(dmi::kSmoothingLanes) == fixed_words * 8 + 3 * (nv + 1) * 4);
    EXPECT(lanes.bytes(dmi::kDecimationLanes) == 8 * (nv + 1) * 4 && lanes.bytes(dmi::kDecimationTriangleLanes) == 2 * (nt + 1) * 4);
    EXPECT(lanes.bytes(dmi::kHolesLanes) == 5 * (nv + 1) * 4 && lanes.bytes(dmi::kHolesLoopLanes) == 11 * ((uint64_t)n_slots + 1) * 4);
    EXPECT(lanes.bytes(dmi::kSupportLanes) == 2 * (nv + 1) * 4);
    // ... and the last entry of the last lane is the last of those bytes
    EXPECT((const char *)(lanes.lane(10) + nv + 1) == (const char *)storage + lanes.bytes(11));
  }
  const dmi::U32Lanes large{nullptr, (uint64_t(1) << 32)};  // 2^32 - 1 vertices: no 32-bit product anywhere
  EXPECT(large.bytes(8) == (uint64_t(1) << 37));
}

int main() {
  event_creation<8, 4>();  // the decimation's
  event_creation<5, 4>();  // the component filter's
  event_creation<4, 3>();  // the smoother's, the fill's, the support trim's
  event_creation<4, 0>();  // the extraction's
  event_creation<2, 0>();  // the point data's
  event_creation<1, 0>();
  event_flags();
  reading_times();
  size_refusals();
  commits();
  carving();
  std::printf("%d failed\n", failures);
  return failures;
}
