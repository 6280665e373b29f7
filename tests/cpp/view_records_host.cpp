// make_view_records of csrc/view_records.h -- the per-view records of the fusion kernels: TileMapRec, WinRec, FootRec, the view's
// KMode and the tiled kernel's per-view test -- replayed against recorded bytes (tests/test_view_records_host.py builds this with
// AddressSanitizer and UBSan and runs it).  tests/golden/view_records.bin holds, per case, the inputs (ViewFrame, rt, k) beside
// the records as they came out for them when the fixture was recorded; the program recomputes and compares tile, win and foot as
// bytes, k_mode, finite and tile_ok as values.  A case with a NaN among its inputs is compared by its decisions only (a
// propagated NaN's payload depends on the operand order the compiler picked).  The case set as a whole must reach every kind of
// record, or the program fails; view_path and grid_axis_aligned are checked against tables written out below.
// Every mismatch is printed with its case and byte offset, the exit status is their number.
#include "view_records.h"
#include "../../include/dmi.h"

#include <cstdio>
#include <vector>

using namespace dmi;

static int failures = 0;
static void fail_line(const char *where, const char *what) {
  if (failures < 100) std::printf("%s: %s\n", where, what);
  ++failures;
}
#define EXPECT(where, cond)                     \
  do {                                          \
    if (!(cond)) fail_line(where, #cond);       \
  } while (0)

// one case of the fixture, as recorded
struct FixtureCase {
  char name[32];
  dmi_grid_desc grid;
  int32_t z_first, W, H, pad0;
  double rt[12], k[12];
  unsigned char tile[368], win[64], foot[320];
  int32_t k_mode, finite, tile_ok, pad1;
};
static_assert(sizeof(FixtureCase) == 1200, "fixture case layout");
static_assert(sizeof(TileMapRec) == 368 && sizeof(WinRec) == 64 && sizeof(FootRec) == 320, "record sizes of the fixture");

static void compare_bytes(const char *name, const char *record, const void *got, const unsigned char *want, size_t n) {
  const unsigned char *g = static_cast<const unsigned char *>(got);
  for (size_t i = 0; i < n; ++i)
    if (g[i] != want[i]) {
      if (failures < 100) std::printf("%s: %s byte %zu is %02x, recorded %02x\n", name, record, i, g[i], want[i]);
      ++failures;
    }
}

// what the case set reaches
struct Coverage {
  bool t1_ok[3] = {false, false, false};
  bool e_abs_finite = false, e_abs_inf = false;
  bool tile_ok[2] = {false, false};
  bool k_mode[3] = {false, false, false};
  bool aligned = false, rotated = false;
};

static int check_fixture(const char *path) {
  std::FILE *f = std::fopen(path, "rb");
  if (!f) {
    std::printf("cannot open %s\n", path);
    return 1;
  }
  char magic[8];
  int32_t head[2] = {0, 0};
  bool ok = std::fread(magic, 1, 8, f) == 8 && std::memcmp(magic, "DMIVREC1", 8) == 0 && std::fread(head, 4, 2, f) == 2 &&
            head[0] > 0 && head[0] < 1000 && head[1] == (int32_t)sizeof(FixtureCase);
  std::vector<FixtureCase> cases(ok ? (size_t)head[0] : 0);
  ok = ok && std::fread(cases.data(), sizeof(FixtureCase), cases.size(), f) == cases.size() && std::fgetc(f) == EOF;
  std::fclose(f);
  if (!ok) {
    std::printf("%s is not a view-record fixture of this layout\n", path);
    return 1;
  }
  Coverage cov;
  for (const FixtureCase &c : cases) {
    char name[33];
    std::memcpy(name, c.name, 32);
    name[32] = 0;
    ViewFrame frame;
    frame.grid = c.grid;
    frame.z_first = c.z_first;
    frame.W = c.W;
    frame.H = c.H;
    const ViewRecords v = make_view_records(frame, c.rt, c.k);
    TileMapRec want_tile;
    WinRec want_win;
    std::memcpy(&want_tile, c.tile, sizeof(want_tile));
    std::memcpy(&want_win, c.win, sizeof(want_win));
    bool has_nan = false;
    for (int q = 0; q < 12; ++q) has_nan = has_nan || std::isnan(c.rt[q]) || std::isnan(c.k[q]);
    EXPECT(name, v.k_mode == c.k_mode);
    EXPECT(name, (v.finite ? 1 : 0) == c.finite);
    EXPECT(name, (v.tile_ok ? 1 : 0) == c.tile_ok);
    if (has_nan) {
      const float inf = std::numeric_limits<float>::infinity();
      EXPECT(name, v.tile.t1_ok == want_tile.t1_ok);
      EXPECT(name, v.tile.t1_e1 == inf && want_tile.t1_e1 == inf);
      EXPECT(name, v.win.e_abs == inf && want_win.e_abs == inf);
    } else {
      compare_bytes(name, "tile", &v.tile, c.tile, sizeof(v.tile));
      compare_bytes(name, "win", &v.win, c.win, sizeof(v.win));
      compare_bytes(name, "foot", &v.foot, c.foot, sizeof(v.foot));
    }
    // the pointers are the caller's
    EXPECT(name, v.tile.depth == nullptr && v.tile.valid == nullptr && v.tile.vbits == nullptr && v.win.vbits == nullptr);
    // (from the recorded bytes: what the fixture holds, whatever the code under test gives)
    if (want_tile.t1_ok >= 0 && want_tile.t1_ok <= 2) cov.t1_ok[want_tile.t1_ok] = true;
    (std::isfinite(want_win.e_abs) ? cov.e_abs_finite : cov.e_abs_inf) = true;
    cov.tile_ok[c.tile_ok ? 1 : 0] = true;
    if (c.k_mode >= 0 && c.k_mode <= 2) cov.k_mode[c.k_mode] = true;
    (grid_axis_aligned(c.grid) ? cov.aligned : cov.rotated) = true;
  }
  EXPECT("case set", cov.t1_ok[0] && cov.t1_ok[1] && cov.t1_ok[2]);
  EXPECT("case set", cov.e_abs_finite && cov.e_abs_inf);
  EXPECT("case set", cov.tile_ok[0] && cov.tile_ok[1]);
  EXPECT("case set", cov.k_mode[K_GENERAL] && cov.k_mode[K_PINHOLE_SKEW] && cov.k_mode[K_PINHOLE]);
  EXPECT("case set", cov.aligned && cov.rotated);
  std::printf("%zu cases\n", cases.size());
  return 0;
}

// view_path over the product of its inputs.  [tiled_possible][tile_ok][k_mode]: the path for t1_ok = 0, 1, 2, and whether a
// view with a finite e_abs counts as one with windows (one with an infinite e_abs never does).
struct PathRow {
  int path[3];
  bool windows[3];
};
static const PathRow kPaths[2][2][3] = {
    {{{{0, 0, 0}, {false, false, false}}, {{0, 0, 0}, {false, false, false}}, {{0, 0, 0}, {false, false, false}}},
     {{{0, 0, 0}, {false, false, false}}, {{0, 0, 0}, {false, false, false}}, {{0, 0, 0}, {false, false, false}}}},
    {{{{0, 0, 0}, {false, false, false}}, {{0, 0, 0}, {false, false, false}}, {{0, 0, 0}, {false, false, false}}},
     {{{1, 1, 1}, {false, false, false}},                                  // K_GENERAL: the GENK instantiation
      {{2, 3, 4}, {false, true, true}},                                    // K_PINHOLE_SKEW
      {{2, 3, 4}, {false, true, true}}}}};                                 // K_PINHOLE

static void check_view_path() {
  for (int possible = 0; possible < 2; ++possible)
    for (int tile_ok = 0; tile_ok < 2; ++tile_ok)
      for (int k_mode = 0; k_mode < 3; ++k_mode)
        for (int t1_ok = 0; t1_ok < 3; ++t1_ok)
          for (int e_finite = 0; e_finite < 2; ++e_finite) {
            TileMapRec t;
            WinRec w;
            std::memset(&t, 0, sizeof(t));
            std::memset(&w, 0, sizeof(w));
            t.t1_ok = t1_ok;
            w.e_abs = e_finite ? 0x1p-14f : std::numeric_limits<float>::infinity();
            bool windows = true;
            const int path = view_path(possible != 0, tile_ok != 0, k_mode, t, w, &windows);
            const PathRow &row = kPaths[possible][tile_ok][k_mode];
            char where[96];
            std::snprintf(where, sizeof(where), "view_path(possible %d, tile_ok %d, k_mode %d, t1_ok %d, e_abs %s)", possible, tile_ok, k_mode,
                          t1_ok, e_finite ? "finite" : "inf");
            EXPECT(where, path == row.path[t1_ok]);
            EXPECT(where, windows == (e_finite ? row.windows[t1_ok] : false));
          }
}

static void check_axis_aligned() {
  dmi_grid_desc g;
  std::memset(&g, 0, sizeof(g));
  for (int i = 0; i < 4; ++i) g.grid_matrix[5 * i] = 1.0;
  EXPECT("grid_axis_aligned(identity)", grid_axis_aligned(g));
  g.grid_matrix[0] = -2.0; g.grid_matrix[5] = 0.5; g.grid_matrix[10] = 3.0;                 // any diagonal ...
  g.grid_matrix[3] = 5e6; g.grid_matrix[7] = -4e6; g.grid_matrix[11] = 300.0;               // ... and any translation
  EXPECT("grid_axis_aligned(scaled, translated)", grid_axis_aligned(g));
  const int off_diagonal[6] = {1, 2, 4, 6, 8, 9};
  for (int e : off_diagonal) {
    dmi_grid_desc r = g;
    r.grid_matrix[e] = 0x1p-60;
    char where[64];
    std::snprintf(where, sizeof(where), "grid_axis_aligned(entry %d set)", e);
    EXPECT(where, !grid_axis_aligned(r));
  }
}

int main(int argc, char **argv) {
  if (argc != 2) {
    std::printf("usage: view_records_host tests/golden/view_records.bin\n");
    return 1;
  }
  static_assert(kMaxColumn == 32, "the recorded bounds were derived for columns of up to 32 voxels");
  if (check_fixture(argv[1]) != 0) ++failures;
  check_view_path();
  check_axis_aligned();
  std::printf("%d failed\n", failures);
  return failures < 255 ? failures : 255;
}
