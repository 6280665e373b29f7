// fan_triangulate.h -- polygons (VTK "Polys": connectivity and offsets) as the triangles the z-buffer rasteriser takes
// (dmi_color_render_depths): a polygon of k corners becomes the k - 2 triangles (c0, c_i, c_i+1), fanned from its first corner;
// polygons of fewer than three corners give none.  For the rendering only: what a tool writes keeps the polygons as they came.
#pragma once

#include <cstdint>
#include <vector>

namespace dmi {
namespace host {

// offsets[i] = end of polygon i in connectivity (polygon 0 starts at 0), increasing and within n_connectivity -- what
// vtp::ReadPolyData has checked; a polygon that breaks this is skipped all the same.
inline std::vector<int64_t> FanTriangulate(const int64_t *connectivity, int64_t n_connectivity, const int64_t *offsets, int64_t n_polys) {
  std::vector<int64_t> triangles;
  int64_t begin = 0;
  for (int64_t p = 0; p < n_polys; ++p) {
    const int64_t end = offsets[p];
    if (end < begin || end > n_connectivity) break;
    for (int64_t i = begin + 1; i + 1 < end; ++i) {
      triangles.push_back(connectivity[begin]);
      triangles.push_back(connectivity[i]);
      triangles.push_back(connectivity[i + 1]);
    }
    begin = end;
  }
  return triangles;
}

}  // namespace host
}  // namespace dmi
