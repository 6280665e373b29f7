// mesh_depth_render.h -- what dmi_capi_color.hip (the owner of dmi_color_context) sees of the z-buffer rasteriser in
// mesh_depth_render.hip, and the texel layout that the rasteriser and coloration_kernels.hip share.  Private: never installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// A colour or depth plane in HBM: texels, top image row first, in TILES of 8 x 4 texels (texel (x, y) at
// ((y >> 2) * tiles_x + (x >> 3)) * 32 + (y & 3) * 8 + (x & 7)); coloration_kernels.hip says why.
#ifndef DMI_TEX_TILE_LOG_W
#define DMI_TEX_TILE_LOG_W 3
#define DMI_TEX_TILE_LOG_H 2
#endif

namespace dmi {

constexpr int kTexLogW = DMI_TEX_TILE_LOG_W, kTexLogH = DMI_TEX_TILE_LOG_H;
constexpr int kTexTileW = 1 << kTexLogW, kTexTileH = 1 << kTexLogH, kTexTile = kTexTileW * kTexTileH;
__host__ __device__ inline int64_t color_plane_texels(int W, int H) {
  return (int64_t)((W + kTexTileW - 1) / kTexTileW) * ((H + kTexTileH - 1) / kTexTileH) * kTexTile;
}
__host__ __device__ __forceinline__ int64_t texel_index(int x, int y, int tiles_x) {
  return ((int64_t)(y >> kTexLogH) * tiles_x + (x >> kTexLogW)) * kTexTile + ((y & (kTexTileH - 1)) << kTexLogW) + (x & (kTexTileW - 1));
}

// The camera of one view as the rasteriser reads it: ColorView's rt and k, nothing else.
struct RenderView {
  double rt[12];  // rows 0..2 of [R|T]
  double k[9];    // rows 0..2, columns 0..2 of the 4x4 K
};

// A (triangle, view) pair whose pixel range is too large for one lane: the large pass gives it a wave.
struct RenderPair {
  int64_t triangle;
  int32_t view;  // index into the views of the CALL (not of the group)
  int32_t pad;
};

constexpr int kRenderViewGroup = 16;  // views per launch of the small pass: one queue fill, one large pass
constexpr int kRenderLaneCap = 64;    // pixels of a clipped range that a lane of the small pass walks itself

struct RenderMesh {
  const double *points;      // [n_points][3], device
  const int64_t *triangles;  // [n_triangles][3], device
  int64_t n_points, n_triangles;
};

// *flag (a zeroed u32) becomes 1 if any id of any triangle is outside [0, n_points)
hipError_t launch_render_check_ids(const RenderMesh &mesh, uint32_t *flag, hipStream_t stream);
// every texel of n_texels becomes the bits of +inf: nothing covers it
hipError_t launch_render_init(double *planes, int64_t n_texels, hipStream_t stream);
// The views [m0, m0 + n) of `views` into planes + m * plane_texels (m counted over the call's views).  Small pass, then the
// large pass over what the small pass queued: *counter (zeroed here) ends as the number of pairs that WANTED a queue entry;
// those beyond `capacity` were dropped, and the caller runs the group again with a queue of that size (a minimum is idempotent).
// `between` (or null) is recorded between the two passes: with an event of the caller's on either side, the passes' times.
hipError_t launch_render_group(const RenderMesh &mesh, const RenderView *views, int m0, int n, int W, int H, double *planes,
                               RenderPair *queue, uint32_t capacity, uint32_t *counter, hipEvent_t between, hipStream_t stream);
// one tiled plane -> [H][W] f64 in vtk point order (row 0 = the bottom image row), -1 where the plane holds +inf
hipError_t launch_unpack_depth(const double *plane, double *dst, int W, int H, hipStream_t stream);

}  // namespace dmi
