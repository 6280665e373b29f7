// view_records.h -- the per-view records of the fusion kernels and the host arithmetic that forms them: MapRec, TileMapRec, WinRec
// and FootRec, the constants of the validity maps and of the window column, and make_view_records, which turns a view's K and
// [R|T] into the error bounds and margins that DESIGN.md 4, 4b, 4d and 4e are proofs about.  Plain C++17 on doubles and floats,
// no HIP type and no dmi_context: all the arithmetic ever reads of a context is a ViewFrame, so that every number can be pinned
// without a GPU (tests/test_view_records_host.py, tests/cpp/view_records_host.cpp).  fusion_kernels.h includes this header for
// the kernels; dmi_capi_views.hip (add_views_impl) calls make_view_records and sets the records' device pointers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "../../include/dmi.h"  // dmi_grid_desc

#if defined(__HIP__)  // (compiled as HIP: the kernels call the validity maps' size functions)
#define DMI_RECORDS_HD __host__ __device__
#else
#define DMI_RECORDS_HD
#endif

namespace dmi {

struct DepthTile;  // fusion_kernels.h: one tile of a depth table's min/max pyramid

// One depth map as the general kernel (and the exact fallback of the tiled kernel) reads it.  The loop
// index over maps is wave-uniform, so a record arrives through scalar loads into SGPRs: no VGPRs, no LDS.
struct alignas(16) MapRec {
  double rt[12];      // rows 0..2 of [R|T]   (reference: matrixTR, cu:159,172)
  double k[12];       // rows 0..2 of the 4x4 K (reference: matrixK, cu:159,176)
  const void *depth;  // W*H depth table, float or double, image row order (row 0 = TOP row: the
                      // reference's bottom-up vtk order, cu:141-149, is flipped once at upload)
  const DepthTile *pyramid;  // this view's min/max pyramid (PyramidDesc::total_tiles entries)
};
static_assert(sizeof(MapRec) == 208, "MapRec layout");

// What the tiled kernel needs per map (scalar loads, 128 B).  Only cz -- the camera-space depth that
// enters the ray potential (cu:207) -- is evaluated in the reference's exact arithmetic; the
// homogeneous pixel coordinates hx, hy only select a pixel, so the fast path evaluates them as an
// affine function of the (axis-aligned) world coordinates and proves its choice (DESIGN.md
// "Tiled kernel: proof obligations"); anything unproven goes through the exact expression.
struct alignas(16) TileMapRec {
  double rz0, rz1, rz3;    // RT row 2: r20, r21, r23 (r22 * wz(k) comes from the cz table)
  double px, py, pz, p0;   // hx ~ px*wx + py*wy + pz*wz + p0   (row 0 of K*[R|T])
  double qx, qy, qz, q0;   // hy ~ qx*wx + qy*wy + qz*wz + q0   (row 1 of K*[R|T])
  double dhx, dhy;         // increments of hx, hy per voxel step along k
  double err;              // bound on |hx_ref - hx_fast| and |hy_ref - hy_fast| (absolute)
  const void *depth;       // same table as MapRec::depth
  double cz_err;           // rotated grids: bound on |computed c.z - real c.z| (0 for axis-aligned grids, where the
                           // computed c.z is monotone in every index and needs no margin)
  double errk;             // what the fusion kernel multiplies by 1/h.z in its acceptance test: err, 2^16 * errz and 2^-22
                           // times a bound on h.z over the grid, so that the test compares with the constant 1/2
  // general K (third row not 0 0 1 0, cu:176): h.z ~ sx*wx + sy*wy + sz*wz + s0 (row 2 of K*[R|T]) and its step per
  // voxel along k; errz bounds |h.z_ref - h.z_affine|.  For a pinhole K these restate RT row 2 and errz is 0.
  double sx, sy, sz, s0, dhz, errz;
  // Pinhole view on an axis-aligned grid: the same two rows in pixel coordinates measured from the image centre
  // (cxc, cyc) = (W / 2, H / 2): hx'' = hx - cxc*c.z, i.e. row 0 of K*[R|T] minus cxc times row 2 of [R|T] (and hy''
  // likewise).  round(h.x/h.z) = cxc + round(hx''/h.z) in exact arithmetic, |u''| <= W/2 halves what a relative error
  // costs in pixels, and the fusion kernel's two-tier pixel selection (fusion_tile.hip "tier 1") works in them; cerr,
  // cerrk: err and errk for these rows.  The classification kernels keep reading px .. q0.
  double cpx, cpy, cpz, cp0, cqx, cqy, cqz, cq0;
  double cdhx, cdhy, cerrk;
  // tier 1 of the pixel selection: the centred numerators, c.z and the acceptance threshold as fp32 affine functions of
  // the voxel's position in its column: steps per voxel of hx'', hy'', c.z and of the threshold
  // c1*c.z - e1 (c1 = 1/2 - 2^-20, e1 the absolute margin of the view; +inf when the view does not qualify)
  float t1_dhx, t1_dhy, t1_dcz, t1_dthr;
  float t1_e1, t1_c1;  // e1 = t1_e1 + t1_erel * (max(|hx''|, |hy''|) at the column's first voxel + t1_hspan)
  float t1_erel, t1_hspan;
  int32_t t1_cidx;  // W * cyc + cxc: pixel index of the image centre
  int32_t t1_ok;  // 0: tier 1 never accepts (t1_e1 = +inf); 1: e1 is the view's constant; 2: e1 per lane (t1_b)
  // Validity map of the view (round 3): one byte per pixel, 1 = the pixel holds a depth (anything but the -1 sentinel), in
  // tiles of 8 image rows over the image and its margin (kValidMargin): with X = x + margin, Y = y + margin and Wp = W + 2 margin,
  // byte (x, y) at ((Y >> 3) * Wp + X) * 8 + (Y & 7), valid_map_bytes(W, H) in all.  The FREE column of
  // the fusion kernel asks only "does my pixel hold a depth?"; an 8 x 8-lane patch of such questions touches a quarter of the
  // cache lines in this layout and a quarter of the bytes, and costs the texture addresser half of what the same gather from
  // the row-major f32 table costs (profiles/r06q_microbench_gather.txt).
  const uint8_t *valid;
  // ... and what turns a centred pixel into a byte of that map (fusion_tile.hip, FREE column), the same for every view of a
  // context but read with the record, in the same scalar loads: (cyc + margin - 3.5) / 8, 8 Wp - 8, 8 (cxc + margin) + cyc + margin, valid_map_bytes
  float vm_c0, vm_w8;
  int32_t vm_base, vm_bytes;
  // Validity BITS of the view (round 4): one bit per pixel of the padded image (the same margin), in tiles of 32 x 32 pixels =
  // 32 dwords = one 128-byte line: bit (X & 31) of dword ((Y >> 5) * tiles_x + (X >> 5)) * 32 + (Y & 31), valid_bits_bytes(W, H)
  // in all.  The FREE column's window form (fusion_tile.hip) fetches, per (brick, view), the 32 x 64 pixel window that holds
  // every voxel's pixel -- one row per lane, two dword loads from one or two lines each -- and asks it with ds_bpermute_b32.
  const uint32_t *vbits;
  int32_t vb_bytes;    // valid_bits_bytes(W, H): the buffer range of one view's bits
  int32_t vb_rowskip;  // (tiles_x - 1) * 128: what a step to the next tile row adds beyond the 128 bytes of the tile itself
  int32_t vb_mx, vb_my;  // 0x4B400000 + margin + W / 2 (H / 2): the bits of the float 1.5 * 2^23 + (centre of the padded image)
  // t1_ok == 2 (round 4): the view has no positive lower bound of c.z over the grid -- its camera stands inside or next to the
  // volume -- so the bound |P| <= pmax that the margin e1 needs is formed per lane and (brick, view) from the column's own c.z:
  // e1 = t1_e1 + t1_b * (HB / min c.z of the column + 1) + t1_erel * HB (fusion_tile.hip)
  float t1_b;
  int32_t vb_pad;
};
// The maps carry a margin of kValidMargin pixels of "no depth" on every side: a pixel that far outside the image reads as a
// hole, so the FREE column, which has no range test, also serves pairs whose footprint sticks out of the image by less (4b.9).
constexpr int kValidMargin = 32;  // a multiple of 8 (whole tile rows)
// A pixel with a depth holds this byte, one without 0: ((1 << byte) - 1) << 20 (one v_bfm_b32) is then the high word of the
// double 1.0 or +0.0 that the FREE column multiplies its constant with (fusion_tile.hip, phase B)
constexpr unsigned kValidByte = 10;
DMI_RECORDS_HD inline int64_t valid_map_bytes(int W, int H) {
  return (int64_t)((H + 2 * kValidMargin + 7) / 8) * (W + 2 * kValidMargin) * 8;
}
// the same image in bits (TileMapRec::vbits): tiles of 32 x 32 pixels, one column of tiles more than the padded image needs (a
// window's second dword may lie in it)
DMI_RECORDS_HD inline int valid_bits_tiles_x(int W) { return (W + 2 * kValidMargin + 31) / 32 + 1; }
DMI_RECORDS_HD inline int valid_bits_tiles_y(int H) { return (H + 2 * kValidMargin + 31) / 32; }
DMI_RECORDS_HD inline int64_t valid_bits_bytes(int W, int H) { return (int64_t)valid_bits_tiles_x(W) * valid_bits_tiles_y(H) * 128; }
// the window of the FREE column: kWindowCols x kWindowRows pixels (a dword per lane); TileArgs::win_origin holds the window's
// first pixel for the pair.  A launch with windows gives one to nearly every pair of class MIXED_FREE_OR_NODEPTH (99 % at cfg 3),
// so the class byte marks the EXCEPTIONS: CLASS_NO_WINDOW (fusion_kernels.h), written by window_origin_kernel for the few pairs
// whose footprint does not fit (until round 5 the bit said "has a window": sixteen million scattered read-modify-writes per fusion)
constexpr int kWindowCols = 32, kWindowRows = 64;
static_assert(sizeof(TileMapRec) == 368, "TileMapRec layout");

// What the window form of the FREE column needs of a view (round 5): ONE 64-byte line, all fp32, fetched with one scalar load per
// (brick, view) -- the 368-byte TileMapRec took five or six dependent batches of them, which with four waves per SIMD was what
// the column waited for.  The centred numerators hx'', hy'' (TileMapRec::cpx ...) and c.z are affine in the voxel's indices; the
// column works in coordinates relative to the WINDOW's centre Xc = first pixel + (kWinAnchorX, kWinAnchorY), hw = h'' - Xc * c.z,
// whose value at the brick's first voxel window_origin_kernel has formed in fp64 (WinPair): |hw| <= (half a window + 1/2) * c.z, so
// every fp32 rounding on the way costs 2^-24 of some thirty c.z instead of 2^-24 of up to W/2 c.z.  d*: steps of (hx'', hy'') per
// voxel along i, j, k; c*: (step of c.z, c1 times it) -- the second half steps the acceptance threshold c1 * c.z - e_abs.
struct alignas(64) WinRec {
  const uint32_t *vbits;  // TileMapRec::vbits
  float di[2], dj[2], dk[2];
  float ci[2], cj[2], ck[2];
  float e_abs;            // the absolute part of the margin (rounded up); +inf: the view has no windows
  float c1;               // kWinC1
};
static_assert(sizeof(WinRec) == 64, "WinRec is one cache line");
// What window_origin_kernel adds to a pair's anchor to reach the brick's eight corner voxels (corner c: bit 0 = i, 1 = j, 2 = k):
// (hx'', hy'', c.z) at voxel (7 or 0, 7 or 0, tk - 1 or 0) minus their values at (0, 0, 0), fp32, for 8- and 16-voxel columns;
// ferr: the centred rows' error bound cerr (4d.1), rounded up.  Wave-uniform: scalar operands of the kernel's packed adds.
struct alignas(64) FootRec {
  float s8[8][4];   // [corner] = (dhx'', dhy'', dcz, unused)
  float s16[8][4];
  float ferr, pad[15];
};
static_assert(sizeof(FootRec) == 320, "FootRec layout");
// The window column counts its coordinates from the window's CENTRE, first pixel + (kWinAnchorX, kWinAnchorY): |hw| <= (half the
// window + 1/2) * c.z, half of what the corner gave, and so are the c.z-proportional roundings that c1 has to absorb (4e.6).
// -DDMI_WIN_CORNER_ANCHOR counts from the first pixel again, with the wider band that needs (same results: an A/B switch for
// tools/gpu_exp.py, tools/exp_list_window_centre.txt).
#ifdef DMI_WIN_CORNER_ANCHOR
constexpr int kWinAnchorX = 0, kWinAnchorY = 0;
constexpr float kWinC1 = 0.5f - 0x1p-14f;
#else
constexpr int kWinAnchorX = kWindowCols / 2, kWinAnchorY = kWindowRows / 2;
constexpr float kWinC1 = 0.5f - 0x1p-15f;  // what is left of 1/2 after every c.z-proportional rounding of the window column (4e.6)
#endif
// an accepted candidate's magnitude stays below (this + 1/2) * kWinCzRatio + 3 (make_centred_rows)
constexpr int kWinReach = kWinAnchorY ? kWindowRows - kWinAnchorY : kWindowRows - 1;
// the brick's c.z may vary by this factor at most for the pair to get a window (bounds |hw| by the threshold's own c.z)
constexpr double kWinCzRatio = 1.25;

// How much of K's structure the uploaded views share; checked on the host, value-identical
// shortcuts proven in DESIGN.md ("K specialisation").
enum KMode : int {
  K_GENERAL = 0,       // any rows 0..2: the reference expression in full (cu:90-92)
  K_PINHOLE_SKEW = 1,  // [fx s cx 0; 0 fy cy 0; 0 0 1 0]
  K_PINHOLE = 2        // ... with s == 0
};

// ---- the host arithmetic ----------------------------------------------------------------------------

// All that the records' arithmetic reads of a context: the grid, the context's first cell layer (dmi_options::z_first) and the
// resident views' image size.
struct ViewFrame {
  dmi_grid_desc grid;
  int32_t z_first;
  int32_t W, H;
};

// What make_view_records forms of one view.  The records' pointer fields (TileMapRec::depth, valid, vbits, WinRec::vbits) are
// null: the caller owns the device buffers.
struct ViewRecords {
  TileMapRec tile;
  WinRec win;
  FootRec foot;
  int k_mode;    // KMode of the view's K
  bool finite;   // every entry of K and [R|T] is finite and within kMagnitudeLimit
  bool tile_ok;  // the view meets the tiled kernel's per-view preconditions (the other part: tile_eligible, dmi_capi.hip)
};

constexpr double kMagnitudeLimit = 1e60;  // see DESIGN.md "K specialisation": keeps every product finite

inline bool grid_axis_aligned(const dmi_grid_desc &g) {
  const double *m = g.grid_matrix;
  return m[1] == 0 && m[2] == 0 && m[4] == 0 && m[6] == 0 && m[8] == 0 && m[9] == 0;
}

inline bool bounded(double v) { return std::isfinite(v) && std::fabs(v) <= kMagnitudeLimit; }

inline int classify_k(const double *K, const double *RT) {
  for (int i = 0; i < 12; ++i)
    if (!bounded(K[i]) || !bounded(RT[i])) return dmi::K_GENERAL;
  const bool pinhole = K[3] == 0 && K[7] == 0 && K[11] == 0 && K[4] == 0 && K[8] == 0 && K[9] == 0 && K[10] == 1;
  if (!pinhole) return dmi::K_GENERAL;
  return K[1] == 0 ? dmi::K_PINHOLE : dmi::K_PINHOLE_SKEW;
}

// ---- tiled kernel support (fusion_tile.hip) --------------------------------------------------------

// (the bounds below were derived for columns of up to 32 voxels, not kMaxColumnHeight's 16: tightening it changes results, no part of a move)
constexpr int kMaxColumn = 32;  // tallest voxel column of any tile shape (error bound below uses it)

// rows 0..2 of the grid matrix applied to the centre of voxel (i, j, k): cu:78-83 + cu:168
inline void voxel_world(const dmi_grid_desc &g, int i, int j, int k, double w[3]) {
  const double p[3] = {g.origin[0] + (i + 0.5) * g.spacing[0], g.origin[1] + (j + 0.5) * g.spacing[1],
                       g.origin[2] + (k + 0.5) * g.spacing[2]};
  for (int r = 0; r < 3; ++r)
    w[r] = ((g.grid_matrix[4 * r] * p[0] + g.grid_matrix[4 * r + 1] * p[1]) + g.grid_matrix[4 * r + 2] * p[2]) +
           g.grid_matrix[4 * r + 3];
}

// Smallest float >= x (x >= 0, finite): the tier-1 margins are rounded up.
inline float float_not_below(double x) {
  float f = (float)x;
  if ((double)f < x) f = std::nextafterf(f, std::numeric_limits<float>::infinity());
  return f;
}

// The pixel selection of a pinhole view on an axis-aligned grid works in coordinates measured from the image centre
// (TileMapRec::cpx ...), in two tiers (fusion_tile.hip).  P, Q, S: rows 0..2 of K*[R|T]; Sx, Sy: magnitudes of
// the terms of h.x, h.y over the grid; M[2]: of c.z.
inline void make_centred_rows(const ViewFrame &f, const MapRec &r, const double P[4], const double Q[4], const double S[4],
                              double Sx, double Sy, const double M[3], double zabs, double zscale, bool general, bool aligned, TileMapRec *out,
                              dmi::WinRec *win, dmi::FootRec *foot) {
  TileMapRec &t = *out;
  std::memset(foot, 0, sizeof(*foot));
  std::memset(win, 0, sizeof(*win));
  win->e_abs = std::numeric_limits<float>::infinity();  // no windows unless everything below holds
  win->c1 = dmi::kWinC1;
  t.t1_ok = 0;
  t.t1_e1 = std::numeric_limits<float>::infinity();
  t.t1_c1 = 0.5f - 0x1p-20f;
  const double cxc = (double)(f.W / 2), cyc = (double)(f.H / 2);
  t.t1_cidx = (int32_t)((int64_t)f.W * (f.H / 2) + f.W / 2);
  if (general) return;  // those launches (GENK instantiations) read px .. q0 and errk
  double Pc[4], Qc[4];
  for (int c = 0; c < 4; ++c) {
    Pc[c] = P[c] - cxc * S[c];
    Qc[c] = Q[c] - cyc * S[c];
  }
  t.cpx = Pc[0]; t.cpy = Pc[1]; t.cpz = Pc[2]; t.cp0 = Pc[3];
  t.cqx = Qc[0]; t.cqy = Qc[1]; t.cqz = Qc[2]; t.cq0 = Qc[3];
  const double *g = f.grid.grid_matrix;
  const double sz = f.grid.spacing[2];
  t.cdhx = (Pc[0] * (g[2] * sz) + Pc[1] * (g[6] * sz)) + Pc[2] * (g[10] * sz);
  t.cdhy = (Qc[0] * (g[2] * sz) + Qc[1] * (g[6] * sz)) + Qc[2] * (g[10] * sz);
  // |hx''_ref - hx''_kernel|: the reference's h.x carries <= 11 ulp(Sx), cxc times its c.z <= 6 ulp(cxc * M[2]); the kernel's
  // affine value the 73 ulp of DESIGN.md 4.2 on the centred magnitudes (+ 2 per coefficient for the subtraction above);
  // 512 ulp of Sx + cxc * M[2] covers the sum five times over
  // Rotated grid: M and Sx are sums of magnitudes that also bound every intermediate of the reference's w (three products and
  // three sums per component instead of one of each); its w at two voxels of a column differs from the real, affine one by
  // <= 6 ulp(|w|) each, which the rows turn into <= 12 ulp of the magnitudes: twice the budget keeps the same margin.
  const double rot = aligned ? 1.0 : 2.0;
  const double Sxc = Sx + cxc * M[2], Syc = Sy + cyc * M[2];
  const double cerr = rot * std::max(Sxc, Syc) * 0x1p-44;
  t.cerrk = cerr + 0x1p-22 * zabs * (1.0 + 0x1p-20);  // (zabs >= |c.z| over the grid: make_tile_rec)
  t.t1_dhx = (float)t.cdhx;
  t.t1_dhy = (float)t.cdhy;
  const double dcz = t.dhz;  // pinhole: row 2 of [R|T] times the step of the world position per voxel along k
  t.t1_dcz = (float)dcz;
  t.t1_dthr = (float)(dcz * (double)t.t1_c1);
  if (!(cerr < 0x1p-12 * zscale)) return;  // (such a view fails the tiled kernel's per-view test anyway)
  // c.z over the voxels of the grid: at least czmin (the real-valued minimum over the box of voxel centres, less the
  // rounding of the computed value)
  // (affine in the voxel indices: the extremes are at the eight corner voxels of the grid, whatever its axes)
  double czmin = std::numeric_limits<double>::infinity(), Scx = 0.0, Scy = 0.0;
  for (int c = 0; c < 8; ++c) {
    double w[3];
    voxel_world(f.grid, (c & 1) ? f.grid.cell_dims[0] - 1 : 0, (c & 2) ? f.grid.cell_dims[1] - 1 : 0,
                f.z_first + ((c & 4) ? f.grid.cell_dims[2] - 1 : 0), w);
    czmin = std::min(czmin, ((r.rt[8] * w[0] + r.rt[9] * w[1]) + r.rt[10] * w[2]) + r.rt[11]);
    // |hx''|, |hy''| over the grid, from the centred rows themselves (for a principal point at the image centre the cz terms
    // of row 0 cancel: this is what keeps |u''| <= W / 2 instead of W)
    Scx = std::max(Scx, std::fabs(((Pc[0] * w[0] + Pc[1] * w[1]) + Pc[2] * w[2]) + Pc[3]));
    Scy = std::max(Scy, std::fabs(((Qc[0] * w[0] + Qc[1] * w[1]) + Qc[2] * w[2]) + Qc[3]));
  }
  czmin -= rot * 16.0 * 0x1p-52 * M[2];
  const double Sc = (std::max(Scx, Scy) + cerr) * (1.0 + 0x1p-20);               // bounds |hx''|, |hy''| and their fp32 images
  const double D = kMaxColumn * std::max(std::fabs(t.cdhx), std::fabs(t.cdhy));  // their change over a column
  const double Dz = kMaxColumn * std::fabs(dcz);
  const double nl = rot * 32.0 * 0x1p-53 * M[2];  // computed c.z against its affine model along a column (roundings of cu:80-92)
  if (!std::isfinite(czmin)) return;
  // The camera inside (or too near) the grid: no bound of |P| holds for the whole view; the kernel forms one per lane from its
  // column's own c.z (t1_ok = 2).  pmax enters e1 linearly: e1 = (A + B pmax)(1 + 2^-10).
  const bool per_lane = !(czmin > 0.0) || !(Sc / czmin + 1.0 < 0x1p22);
  const double pmax = per_lane ? 0.0 : Sc / czmin + 1.0;  // bounds every accepted tier-1 candidate |P|
  // W*py'' + px'' and the validity map's byte index yt*(8W - 8) + (8 px'' + py'') (|.| <= H*W + 4W + H/2) exact in fp32
  // (of the padded image: every pixel the FREE column may ask for lies within the margin, 4b.9)
  const bool index_exact = ((int64_t)f.H + 2 * dmi::kValidMargin + 8) * ((int64_t)f.W + 2 * dmi::kValidMargin) + f.H +
                               2 * dmi::kValidMargin < (int64_t(1) << 24);
  // e1 = e_abs + e_rel * HB, HB = the lane's bound on |hx''|, |hy''| along its column
  double e1 = cerr + 3.0 * 0x1p-24 * Dz * pmax + 0x1p-22 * Dz + nl * (pmax + 2.0) + 0x1p-53 * std::max(Sx, Sy);
  e1 *= 1.0 + 0x1p-10;
  t.t1_erel = 0x1p-22f * (1.0f + 0x1p-10f);
  t.t1_hspan = float_not_below(D * (1.0 + 0x1p-20));
  if (!(pmax < 0x1p22) || !index_exact || !(e1 > 0x1p-100) || !(Sc < 0x1p60) || !std::isfinite(e1)) return;
  t.t1_e1 = float_not_below(e1);  // (per_lane: the part of e1 that does not depend on pmax)
  t.t1_ok = 1;
  {
    // The window form of the FREE column (WinRec).  Steps of the centred numerators and of c.z
    // per voxel along i, j, k: the rows times the grid matrix's columns times the spacings (as cdhx above for k).
    const double *sp = f.grid.spacing;
    double d[3][2], c[3];
    for (int ax = 0; ax < 3; ++ax) {
      const double wxs = g[ax] * sp[ax], wys = g[4 + ax] * sp[ax], wzs = g[8 + ax] * sp[ax];
      d[ax][0] = (Pc[0] * wxs + Pc[1] * wys) + Pc[2] * wzs;
      d[ax][1] = (Qc[0] * wxs + Qc[1] * wys) + Qc[2] * wzs;
      c[ax] = (S[0] * wxs + S[1] * wys) + S[2] * wzs;
    }
    // |hw_ref - model| <= cerr + Xmax * nl2: the centred numerator within cerr of the affine model anchored at the brick's first
    // voxel (the budget of 4d.1 covers the anchor's FMA chain and seven steps each way: < 100 of its 512 ulp), the reference's
    // c.z within nl2 of ITS model (two computed values, 8 ulp(M[2]) each, rotated grids twice that), times the window's anchor
    // pixel Xc: its first pixel (|.| <= xpix) plus (kWinAnchorX, kWinAnchorY)
    const double xpix = (double)(std::max(f.W, f.H) / 2 + dmi::kValidMargin + 1);
    const double xmax = xpix + (double)std::max(dmi::kWinAnchorX, dmi::kWinAnchorY);
    const double nl2 = 2.0 * nl;
    const double pwin = (dmi::kWinReach + 0.5) * dmi::kWinCzRatio + 3.0;  // bounds an accepted candidate: |P| < |h| / z + 1/2
    // the steps as the kernel forms them, fl32(d32 - Xc * c32): each within 2^-23 (|d| + |Xc c|) of the real one; a lane takes up
    // to 7 along i and j and kMaxColumn - 1 along k
    const double steps[3] = {7.0, 7.0, (double)(kMaxColumn - 1)};
    double e_step = 0.0;
    for (int xy = 0; xy < 2; ++xy) {
      double e = 0.0;
      for (int ax = 0; ax < 3; ++ax) e += steps[ax] * (std::fabs(d[ax][xy]) + xmax * std::fabs(c[ax]));
      e_step = std::max(e_step, e * 0x1p-23);
    }
    double ew = (cerr + xmax * nl2) + e_step + pwin * nl2 + 0x1p-53 * std::max(Sx, Sy);
    ew *= 1.0 + 0x1p-10;
    bool ok = std::isfinite(ew) && ew > 0x1p-100 && ew < 0x1p60;
    for (int ax = 0; ax < 3; ++ax) ok = ok && std::fabs(d[ax][0]) < 0x1p60 && std::fabs(d[ax][1]) < 0x1p60 && std::fabs(c[ax]) < 0x1p60;
    if (ok) {
      for (int xy = 0; xy < 2; ++xy) {
        win->di[xy] = (float)d[0][xy];
        win->dj[xy] = (float)d[1][xy];
        win->dk[xy] = (float)d[2][xy];
      }
      win->ci[0] = (float)c[0]; win->ci[1] = (float)(c[0] * (double)dmi::kWinC1);
      win->cj[0] = (float)c[1]; win->cj[1] = (float)(c[1] * (double)dmi::kWinC1);
      win->ck[0] = (float)c[2]; win->ck[1] = (float)(c[2] * (double)dmi::kWinC1);
      win->e_abs = float_not_below(ew);
      // the brick's corner voxels relative to its first one (FootRec), for 8- and 16-voxel columns
      for (int cnr = 0; cnr < 8; ++cnr) {
        const double ni = (cnr & 1) ? 7.0 : 0.0, nj = (cnr & 2) ? 7.0 : 0.0;
        for (int v = 0; v < 2; ++v) {
          const double nk = (cnr & 4) ? (v ? 15.0 : 7.0) : 0.0;
          float *dst = v ? foot->s16[cnr] : foot->s8[cnr];
          dst[0] = (float)((ni * d[0][0] + nj * d[1][0]) + nk * d[2][0]);
          dst[1] = (float)((ni * d[0][1] + nj * d[1][1]) + nk * d[2][1]);
          dst[2] = (float)((ni * c[0] + nj * c[1]) + nk * c[2]);
        }
      }
      foot->ferr = float_not_below(cerr + xpix * nl2);  // (times a pixel's |u''|, not an anchor's)
    }
  }
  if (per_lane) {
    // the coefficient of pmax, rounded up, with one more factor (1 + 2^-10) for the roundings of the lane's own p
    const double B = (3.0 * 0x1p-24 * Dz + nl) * (1.0 + 0x1p-10) * (1.0 + 0x1p-10);
    if (!(B < 0x1p60) || !(B >= 0.0)) {
      t.t1_ok = 0;
      t.t1_e1 = std::numeric_limits<float>::infinity();
      return;
    }
    t.t1_b = float_not_below(B);
    t.t1_ok = 2;
  }
}

// Per-map record of the tiled kernel: row 2 of RT for the exact c.z, rows 0 and 1 of K*[R|T] for the
// pixel selection, and `err`, a bound on the absolute difference between the reference's computed
// h.x / h.y and the kernel's affine evaluation anywhere in the grid (DESIGN.md "Tiled kernel: proof
// obligations" derives the 73-ulp budget this bound covers seven times over).
inline TileMapRec make_tile_rec(const ViewFrame &f, const MapRec &r, dmi::WinRec *win, dmi::FootRec *foot, double *zscale_out) {
  TileMapRec t;
  std::memset(&t, 0, sizeof(t));
  const double *rt = r.rt, *k = r.k;
  t.rz0 = rt[8];
  t.rz1 = rt[9];
  t.rz3 = rt[11];
  // rows of K * [R|T]: h.x, h.y (and, for a K whose third row is not 0 0 1 0, h.z) as affine functions of the world
  // position.  A pinhole K keeps the shorter sums it always had (the dropped terms are exact zeros).
  const bool general = classify_k(r.k, r.rt) == dmi::K_GENERAL;
  double P[4], Q[4], S[4];
  for (int c = 0; c < 4; ++c) {
    if (general) {
      P[c] = (k[0] * rt[c] + k[1] * rt[4 + c]) + k[2] * rt[8 + c];
      Q[c] = (k[4] * rt[c] + k[5] * rt[4 + c]) + k[6] * rt[8 + c];
      S[c] = (k[8] * rt[c] + k[9] * rt[4 + c]) + k[10] * rt[8 + c];
    } else {
      P[c] = k[0] * rt[c] + k[1] * rt[4 + c] + k[2] * rt[8 + c];  // row 0 of K (fx s cx0 0) times [R|T]
      Q[c] = k[5] * rt[4 + c] + k[6] * rt[8 + c];                 // row 1 of K (0 fy cy0 0)
      S[c] = rt[8 + c];                                           // row 2 of K (0 0 1 0): h.z == c.z
    }
  }
  if (general) {  // the fourth column of K multiplies the homogeneous 1 (cu:90-92)
    P[3] += k[3];
    Q[3] += k[7];
    S[3] += k[11];
  }
  t.px = P[0]; t.py = P[1]; t.pz = P[2]; t.p0 = P[3];
  t.qx = Q[0]; t.qy = Q[1]; t.qz = Q[2]; t.q0 = Q[3];
  t.sx = S[0]; t.sy = S[1]; t.sz = S[2]; t.s0 = S[3];
  // step of the world position per voxel along k: column 2 of the grid matrix times the spacing (for an axis-aligned
  // grid only its z component is non-zero)
  const double *g = f.grid.grid_matrix;
  const double sz = f.grid.spacing[2];
  t.dhx = (P[0] * (g[2] * sz) + P[1] * (g[6] * sz)) + P[2] * (g[10] * sz);
  t.dhy = (Q[0] * (g[2] * sz) + Q[1] * (g[6] * sz)) + Q[2] * (g[10] * sz);
  t.dhz = (S[0] * (g[2] * sz) + S[1] * (g[6] * sz)) + S[2] * (g[10] * sz);
  // magnitudes of the world coordinates over the grid (plus one column height)
  double wm[3];
  const bool aligned = grid_axis_aligned(f.grid);
  if (aligned) {
    // |w| is largest at a grid corner (each w component is monotone in its own index)
    double lo[3], hi[3];
    voxel_world(f.grid, 0, 0, f.z_first, lo);
    voxel_world(f.grid, f.grid.cell_dims[0] - 1, f.grid.cell_dims[1] - 1,
                f.z_first + f.grid.cell_dims[2] - 1 + kMaxColumn, hi);
    for (int a = 0; a < 3; ++a) wm[a] = std::max(std::fabs(lo[a]), std::fabs(hi[a]));
  } else {
    // sum of magnitudes: also bounds every intermediate of the evaluation
    double gm[3];
    for (int a = 0; a < 3; ++a)
      gm[a] = std::fabs(f.grid.origin[a]) +
              (f.grid.cell_dims[a] + 1.0 + (a == 2 ? f.z_first + kMaxColumn : 0)) * std::fabs(f.grid.spacing[a]);
    for (int a = 0; a < 3; ++a)
      wm[a] = std::fabs(g[4 * a]) * gm[0] + std::fabs(g[4 * a + 1]) * gm[1] + std::fabs(g[4 * a + 2]) * gm[2] + std::fabs(g[4 * a + 3]);
  }
  double M[3];
  for (int row = 0; row < 3; ++row)
    M[row] = std::fabs(rt[4 * row]) * wm[0] + std::fabs(rt[4 * row + 1]) * wm[1] + std::fabs(rt[4 * row + 2]) * wm[2] +
             std::fabs(rt[4 * row + 3]);
  // magnitudes of the terms of h.x, h.y, h.z: every row of K against (|c.x|, |c.y|, |c.z|, 1)
  const double Sx = std::fabs(k[0]) * M[0] + std::fabs(k[1]) * M[1] + std::fabs(k[2]) * M[2] + (general ? std::fabs(k[3]) : 0.0);
  const double Sy = (general ? std::fabs(k[4]) * M[0] : 0.0) + std::fabs(k[5]) * M[1] + std::fabs(k[6]) * M[2] +
                    (general ? std::fabs(k[7]) : 0.0);
  const double Sz = general ? std::fabs(k[8]) * M[0] + std::fabs(k[9]) * M[1] + std::fabs(k[10]) * M[2] + std::fabs(k[11]) : M[2];
  t.err = std::max(Sx, Sy) * 0x1p-44;  // 512 ulps of the term magnitudes
  // general K: the same bound for the affine h.z.  0 for a pinhole K, where the kernel's h.z is the reference's own c.z
  t.errz = general ? Sz * 0x1p-44 : 0.0;
  // rotated grid: the computed c.z (9 + 6 rounded operations on terms bounded by M[2]) is within 8 ulp(M[2]) of the
  // real, exactly affine one; four times that as the margin of the brick classification
  t.cz_err = aligned ? 0.0 : M[2] * 0x1p-47;
  // The kernel accepts a pixel iff |frac| + errk * r < 1/2 with r = (1 +- 2^-39) / h.z.  errk * r covers
  //   err / h.z                      the error of h.x, h.y,
  //   2^16 * errz / h.z              that of h.z, times |u| < 2^16 (beyond that both are outside any map),
  //   2^-22                          the slack of DESIGN.md 4.4, because Sz bounds |h.z| everywhere in the grid
  //                                  (Sz * r >= 1 - 2^-39).
  // Z >= |h.z| over the grid's voxels (and one column above).  General K: the sum of magnitudes.  Pinhole: c.z is affine in the
  // voxel indices, so its extremes are at the grid's corner voxels -- their computed values, widened by the computed c.z's
  // distance from the real one (16 ulp of the term magnitudes, twice that on a rotated grid).  (Until round 5 the sum of
  // magnitudes served both: in a geo-referenced frame, where |T| ~ 1e6 cancels against R w, it overstates |c.z| a millionfold and
  // the fp64 tier accepted next to nothing.)
  double zabs = Sz, czlo = std::numeric_limits<double>::infinity(), czhi = -czlo;
  if (!general) {
    zabs = 0.0;
    for (int c = 0; c < 8; ++c) {
      double w[3];
      voxel_world(f.grid, (c & 1) ? f.grid.cell_dims[0] - 1 : 0, (c & 2) ? f.grid.cell_dims[1] - 1 : 0,
                  f.z_first + ((c & 4) ? f.grid.cell_dims[2] - 1 + kMaxColumn : 0), w);
      const double cz = ((rt[8] * w[0] + rt[9] * w[1]) + rt[10] * w[2]) + rt[11];
      zabs = std::max(zabs, std::fabs(cz));
      czlo = std::min(czlo, cz);
      czhi = std::max(czhi, cz);
    }
    zabs = zabs * (1.0 + 0x1p-20) + (aligned ? 1.0 : 2.0) * 32.0 * 0x1p-52 * M[2];
    if (!std::isfinite(zabs)) zabs = Sz;
  }
  // What "far below a pixel" is measured against: the bounds err, cerr are absolute (units of h.x), a voxel's share of a pixel is
  // bound / c.z.  zscale: the depth of most of the grid as the view sees it -- its nearest corner, but no less than a sixteenth
  // of its farthest (a camera inside the volume) and no less than 1.
  double zscale = 1.0;
  if (!general && std::isfinite(czlo) && std::isfinite(czhi)) zscale = std::max(1.0, std::max(czlo, czhi / 16.0));
  t.errk = (t.err + 65536.0 * t.errz) + 0x1p-22 * zabs * (1.0 + 0x1p-20);
  t.depth = r.depth;
  make_centred_rows(f, r, P, Q, S, Sx, Sy, M, zabs, zscale, general, aligned, &t, win, foot);
  if (zscale_out) *zscale_out = zscale;
  return t;
}

// The records of one view: rt, k are rows 0..2 of its row-major 4x4 [R|T] and K.
inline ViewRecords make_view_records(const ViewFrame &f, const double rt[12], const double k[12]) {
  MapRec r;
  std::memset(&r, 0, sizeof(r));
  std::memcpy(r.rt, rt, 12 * sizeof(double));
  std::memcpy(r.k, k, 12 * sizeof(double));
  ViewRecords v;
  bool finite = true;
  for (int q = 0; q < 12; ++q) finite = finite && bounded(r.k[q]) && bounded(r.rt[q]);
  v.finite = finite;
  const int km = classify_k(r.k, r.rt);
  v.k_mode = km;
  double zscale = 1.0;
  v.tile = make_tile_rec(f, r, &v.win, &v.foot, &zscale);
  TileMapRec &t = v.tile;
  t.vm_c0 = ((float)(f.H / 2 + dmi::kValidMargin) - 3.5f) * 0.125f;
  t.vm_w8 = (float)(8 * (f.W + 2 * dmi::kValidMargin) - 8);
  t.vm_base = 8 * (f.W / 2 + dmi::kValidMargin) + f.H / 2 + dmi::kValidMargin;
  t.vm_bytes = (int32_t)std::min<int64_t>(dmi::valid_map_bytes(f.W, f.H), 0x7fffffff);
  t.vb_bytes = (int32_t)std::min<int64_t>(dmi::valid_bits_bytes(f.W, f.H), 0x7fffffff);
  t.vb_rowskip = (dmi::valid_bits_tiles_x(f.W) - 1) * 128;
  t.vb_mx = 0x4B400000 + dmi::kValidMargin + f.W / 2;
  t.vb_my = 0x4B400000 + dmi::kValidMargin + f.H / 2;
  // pixel selection must be provable for nearly every lane: the error bounds over h.z must stay far below one pixel at the
  // depth of most of the grid (zscale, make_tile_rec): err / c.z < 2^-12 pixels sends about a voxel in a thousand to the exact
  // expression -- a few per cent of a wave's voxels redone, against the general kernel's 6 x.  (Until round 5 the test was
  // err < 2^-14 whatever the depth: a survey in a UTM frame with a long lens left the tiled kernel at offsets of 1e5.)
  v.tile_ok = finite && t.err < 0x1p-12 * zscale && 65536.0 * t.errz < 0x1p-14 && t.cerrk < 0x1p-11 * zscale;
  return v;
}

// Which path a resident view takes (dmi_get_view_paths): the index 0 .. 4 of the counter it adds to -- 0: the general kernel;
// 1: the tiled kernel's general-K instantiation; 2 + t1_ok: pinhole, by its tier 1 -- and *windows: it also has a window record
// (counter 5).  tiled_possible: tile_eligible, the part of the tiled kernel's preconditions that does not depend on the view.
inline int view_path(bool tiled_possible, bool tile_ok, int k_mode, const TileMapRec &t, const WinRec &win, bool *windows) {
  *windows = false;
  if (!tiled_possible || !tile_ok) return 0;
  if (k_mode == dmi::K_GENERAL) return 1;
  *windows = t.t1_ok != 0 && std::isfinite(win.e_abs);
  return 2 + std::min(std::max(t.t1_ok, 0), 2);
}

}  // namespace dmi
