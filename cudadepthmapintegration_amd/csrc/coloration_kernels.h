// coloration_kernels.h -- what dmi_capi_color.hip (the owner of dmi_color_context) sees of the coloration kernels in
// coloration_kernels.hip: the records host and device share, and one launch per step of a chunk.  Every launch goes to the given
// stream and returns the first error of its calls.  Private: never installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace dmi {

struct ColorView {
  double rt[12];           // rows 0..2 of [R|T]
  double k[9];             // rows 0..2, columns 0..2 of the 4x4 K (TransformVector ignores column 3)
  const uchar4 *color;     // [H][W] RGBA, TOP image row first (the reference's vtk order is flipped at upload)
  double p[12];            // rows 0..2 of K3 * [R|T]: the pixel selection's shortcut (project_color_kernel)
  double mag[12];          // |K3| * |[R|T]|, the same product of magnitudes: what bounds the shortcut's error
};

// Per view and chunk of vertices (launch_chunk_margins): how far the shortcut's homogeneous
// coordinates can be from the reference's, as (ex, ey) = E0 + 65537 E2, E1 + 65537 E2 with Ei = 2^-47 * sum_j mag[i][j] *
// max|p_j| over the chunk (p_3 = 1): the reference's d_i carries at most 11 roundings of terms bounded by that sum, the
// host's product K3*[R|T] three, the FMA chain four (see round_to_pixel_near).
struct ViewMargin {
  double ex, ey;
};

// What the median pass needs from the projection pass when the medians are found by nibble histograms: for each channel
// and each of the two middle ranks, the upper nibble of the median (4 bits each in .x) and the rank that remains inside
// that nibble's bin (16 bits each in .y .z .w).
struct MedianSeed {
  uint32_t hi, rest01, rest23, rest45;
};

// Are consecutive vertices neighbours in space, as a mesh's are?  A sample of up to 512 consecutive pairs against the same
// number of pairs half the array apart (dmi_capi_color.hip judges it).  Sample t of `samples` reads the rows i, i + 1 and
// (i + n / 2) % n with i = coherence_row(t, n, samples).
constexpr int64_t kCoherenceSamples = 512;
inline int64_t coherence_samples(int64_t n) { return std::min<int64_t>(kCoherenceSamples, n / 2); }
__host__ __device__ inline int64_t coherence_row(int64_t t, int64_t n, int64_t samples) { return t * ((n - 1) / samples); }
// rows[t] = the three rows of sample t, [samples][3][3], of vertices that are on the device
hipError_t launch_coherence_sample(const double *points, int64_t n, int64_t samples, double *rows, hipStream_t stream);

// n_pixels_total pixels of [n][H][W][3] u8 / [n][H][W] f64 in vtk point order -> [n] tiled planes, top row first
hipError_t launch_pack_color(const uint8_t *rgb, uchar4 *rgba, int W, int H, int64_t n_pixels_total, hipStream_t stream);
hipError_t launch_pack_depth(const double *src, double *dst, int W, int H, int64_t n_pixels_total, hipStream_t stream);

// ---- the steps of a chunk of nv vertices, in this order ----
// pmax (4 words) = the chunk's largest coordinate magnitudes, margins[view] = the ViewMargin they give
hipError_t launch_chunk_margins(const double *points, int64_t nv, const ColorView *views, int n_views, unsigned long long *pmax,
                                ViewMargin *margins, hipStream_t stream);
// The order of work along a Z-order curve of the chunk's bounding box: perm[position] = vertex.  keys, keys_sorted, index and
// perm hold a u32 per vertex, box six words; temp is what zorder_sort_temp_bytes asked for at the buffers' capacity.
struct ZOrderBuffers {
  unsigned long long *box;
  uint32_t *keys, *keys_sorted, *index, *perm;
  void *temp; size_t temp_bytes;
};
hipError_t zorder_sort_temp_bytes(size_t capacity, size_t *bytes, hipStream_t stream);
hipError_t launch_zorder_sort(const double *points, int64_t nv, const ZOrderBuffers &order, hipStream_t stream);
// The projection pass.  The depth policy: none, the context's tiled f64 planes, or a fusion context's [H][W] tables.  With
// histogram medians, vertices in a coherent order -- the caller's (coherent) or the Z-order pass's (perm) -- take the pipelined
// view loop, scattered ones the plain one.
enum class ColorDepth { none, planes, fused_f32, fused_f64 };
struct ProjectArgs {
  const double *points; int64_t nv;
  const uint32_t *perm;  // or null: the caller's order
  const ColorView *views; int n_views, W, H;
  uchar4 *scratch;       // [view][vertex]
  uint8_t *mean; int32_t *count; MedianSeed *seeds;
  const ViewMargin *margins;
  bool histogram_medians, coherent;
  unsigned extra_lds;    // tuning builds
  ColorDepth depth; const void *depth_tables; double tol;  // depth_tables: [view] -> plane or table, device
};
hipError_t launch_project_color(const ProjectArgs &a, hipStream_t stream);
// seeds: the projection pass's (histogram medians), or null: the bit-by-bit selection
hipError_t launch_color_median(const uchar4 *scratch, int64_t nv, int n_views, const uint32_t *perm, const int32_t *count,
                               const MedianSeed *seeds, uint8_t *median, hipStream_t stream);

}  // namespace dmi
