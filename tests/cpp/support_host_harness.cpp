// Stand-alone host program around csrc/isosurface_support.hip itself (compiled as C++ against tests/cpp/support_host/): reads a
// mesh and views from a directory of raw arrays, runs the counting launch and, for min_views > 0, the filter launch, and writes what
// they left.  Every buffer has its exact size on the heap, so AddressSanitizer reports any access past one.
//   support_host_harness DIR N_VIEWS W H DEPTH_IS_F64 FACING MIN_VIEWS TOLERANCE
#include "isosurface_support.hip"

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

template <typename T>
std::vector<T> read_all(const std::string &path) {
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) {
    perror(path.c_str());
    exit(2);
  }
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<T> v((size_t)n / sizeof(T));
  if (n && fread(v.data(), 1, (size_t)n, f) != (size_t)n) exit(2);
  fclose(f);
  return v;
}
template <typename T>
void write_all(const std::string &path, const T *p, size_t n) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f || (n && fwrite(p, sizeof(T), n, f) != n)) exit(2);
  fclose(f);
}

int main(int argc, char **argv) {
  if (argc != 9) return 2;
  const std::string d = argv[1];
  const int n_views = atoi(argv[2]), W = atoi(argv[3]), H = atoi(argv[4]), f64 = atoi(argv[5]), facing = atoi(argv[6]), min_views = atoi(argv[7]);
  const double tolerance = atof(argv[8]);
  const auto verts = read_all<double>(d + "/vertices.bin");
  const auto tris = read_all<int64_t>(d + "/triangles.bin");
  const auto normals = read_all<float>(d + "/normals.bin");
  const auto K = read_all<double>(d + "/K4.bin"), RT = read_all<double>(d + "/RT4.bin");
  const auto depth64 = read_all<double>(d + "/depth_top_row_first.bin");  // [n][H][W]
  const std::vector<float> depth32(depth64.begin(), depth64.end());
  const uint64_t nv = verts.size() / 3, nt = tris.size() / 3;
  std::vector<dmi::MapRec> maps((size_t)n_views);
  for (int m = 0; m < n_views; ++m) {
    memset(&maps[m], 0, sizeof(dmi::MapRec));
    memcpy(maps[m].rt, &RT[16 * (size_t)m], 12 * sizeof(double));
    memcpy(maps[m].k, &K[16 * (size_t)m], 12 * sizeof(double));
    maps[m].depth = f64 ? (const void *)(depth64.data() + (size_t)m * W * H) : (const void *)(depth32.data() + (size_t)m * W * H);
  }
  std::vector<int32_t> support(nv), out_support(nv);
  std::vector<uint32_t> mark(nv + 1), vmap(nv + 1), tmap(nt + 1);
  std::vector<double> out_verts(3 * nv);
  std::vector<float> out_normals(3 * nv);
  std::vector<int64_t> out_tris(3 * std::max<uint64_t>(nt, 1));
  const dmi::SupportMesh m{nv, nt, verts.data(), normals.data(), tris.data(), out_verts.data(), out_normals.data(), out_tris.data()};
  const dmi::SupportViews views{maps.data(), n_views, W, H, f64};
  size_t temp = 0;
  dmi::support_scan_temp_bytes(nv, nt, &temp);
  std::vector<char> scan(temp);
  const dmi::SupportScratch s{support.data(), out_support.data(), mark.data(), vmap.data(), tmap.data(), scan.data(), temp};
  if (dmi::launch_isosurface_support_counts(m, views, tolerance, facing, s, nullptr, nullptr) != hipSuccess) return 1;
  write_all(d + "/support.out", support.data(), nv);
  if (min_views > 0) {
    if (dmi::launch_isosurface_support_filter(m, min_views, s, nullptr, nullptr) != hipSuccess) return 1;
    const uint32_t kv = vmap[nv], kt = tmap[nt];
    write_all(d + "/vertices.out", out_verts.data(), 3 * (size_t)kv);
    write_all(d + "/normals.out", out_normals.data(), 3 * (size_t)kv);
    write_all(d + "/triangles.out", out_tris.data(), 3 * (size_t)kt);
    write_all(d + "/support_compacted.out", out_support.data(), kv);
    printf("kept %u %u\n", kv, kt);
  }
  return 0;
}
