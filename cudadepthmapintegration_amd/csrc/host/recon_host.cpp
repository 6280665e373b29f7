// recon_host.cpp -- host side of the fusion path above the C ABI; see recon_host.h for what each piece
// mirrors in the reference.  Calls only include/dmi.h entry points; no TSDF arithmetic lives here.
#include "recon_host.h"
#include "vti_reader.h"

#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <ctime>
#include <fstream>
#include <condition_variable>
#include <exception>
#include <functional>
#include <iostream>
#include <mutex>
#include <thread>
#include <sstream>
#include <string_view>

namespace dmi {
namespace host {

// ====================================================================================================
// Sources/Helper.h
// ====================================================================================================
namespace help {

namespace {

// The whole file as one string; false when it cannot be opened.
bool slurp(const std::string &path, std::string *out) {
  std::ifstream in(path.c_str(), std::ios::binary);
  if (!in.is_open()) return false;
  in.seekg(0, std::ios::end);
  const std::streamoff size = in.tellg();
  in.seekg(0, std::ios::beg);
  out->resize(size > 0 ? (size_t)size : 0);
  if (size > 0) in.read(&(*out)[0], size);
  out->resize((size_t)in.gcount());
  return true;
}

// visit(line) for every line of `text`.  Lines end in "\n" or "\r\n" (a list written on Windows reads the same); a
// last line without a terminator counts, an empty remainder after the last terminator does not.
template <typename Visit>
void for_each_line(std::string_view text, Visit &&visit) {
  while (!text.empty()) {
    const size_t nl = text.find('\n');
    std::string_view line = text.substr(0, nl);
    text.remove_prefix(nl == std::string_view::npos ? text.size() : nl + 1);
    if (!line.empty() && line.back() == '\r') line.remove_suffix(1);
    visit(line);
  }
}

// Up to `want` numbers from the front of `line` into out[]; the ones that are not there stay 0 (what a failed
// operator>> leaves behind in the reference's loops, Helper.h:124-128).
void leading_numbers(std::string_view line, int want, double *out) {
  const std::string z(line);  // strtod needs a terminator
  const char *p = z.c_str();
  for (int i = 0; i < want; ++i) {
    out[i] = 0.0;
    char *end = nullptr;
    const double v = std::strtod(p, &end);
    if (end == p) {
      for (int j = i; j < want; ++j) out[j] = 0.0;
      return;
    }
    out[i] = v;
    p = end;
  }
}

}  // namespace

void SplitString(const std::string &s, char delim, std::vector<std::string> &elems) {
  // std::getline semantics (Helper.h:18-27): a piece per delimiter, no piece for a trailing delimiter
  size_t from = 0;
  while (from < s.size()) {
    const size_t at = s.find(delim, from);
    elems.emplace_back(s, from, at == std::string::npos ? std::string::npos : at - from);
    if (at == std::string::npos) break;
    from = at + 1;
  }
}

std::string GetFilenamePath(const std::string &filename) {
  // directory part with '/' separators (Helper.h:32-55): "" when there is none, "X:/" for a drive root, "/" for the root
  std::string unix_style = filename;
  for (char &c : unix_style)
    if (c == '\\') c = '/';
  const size_t cut = unix_style.rfind('/');
  if (cut == std::string::npos) return std::string();
  unix_style.resize(cut);
  if (unix_style.size() == 2 && unix_style[1] == ':') unix_style.push_back('/');
  if (unix_style.empty()) unix_style = "/";
  return unix_style;
}

std::vector<std::string> ExtractAllFilePath(const char *globalPath) {
  std::vector<std::string> entries;
  std::string listing;
  if (!globalPath || !slurp(globalPath, &listing)) {
    std::cerr << "Unable to open : " << (globalPath ? globalPath : "(null)") << std::endl;  // Helper.h:66-70
    return entries;
  }
  std::string base = GetFilenamePath(globalPath);
  if (base.empty()) {  // a bare file name: relative to the working directory (Helper.h:76-79)
    char cwd[4096];
    base = getcwd(cwd, sizeof(cwd)) ? cwd : ".";
  }
  for_each_line(listing, [&](std::string_view line) {
    // the entry is the last blank-separated token (Helper.h:86-96: "<index> <file>" or just "<file>"); trailing blanks
    // are not a token, and a line of nothing but blanks is an empty line
    while (!line.empty() && line.back() == ' ') line.remove_suffix(1);
    if (line.empty()) return;
    const size_t blank = line.rfind(' ');
    const std::string_view token = blank == std::string_view::npos ? line : line.substr(blank + 1);
    entries.push_back(base + "/" + std::string(token));
  });
  return entries;
}

bool ReadKrtdFile(const std::string &filename, double K3[9], double RT[16]) {
  std::string text;
  if (!slurp(filename, &text)) {
    std::cerr << "Unable to open krtd file : " << filename << std::endl;  // Helper.h:110-114
    return false;
  }
  // Helper.h:117-158: line 0-2 = rows of K, 3 skipped, 4-6 = rows of R, 7 skipped, 8 = T; whatever follows is ignored
  // and lines that are missing read as zeros.  RT = [R | T; 0 0 0 1] (Helper.h:160-165).
  for (int i = 0; i < 9; ++i) K3[i] = 0.0;
  for (int i = 0; i < 16; ++i) RT[i] = 0.0;
  RT[15] = 1.0;
  int index = 0;
  for_each_line(text, [&](std::string_view line) {
    double v[3];
    if (index <= 2) {
      leading_numbers(line, 3, v);
      for (int c = 0; c < 3; ++c) K3[3 * index + c] = v[c];
    } else if (index >= 4 && index <= 6) {
      leading_numbers(line, 3, v);
      for (int c = 0; c < 3; ++c) RT[4 * (index - 4) + c] = v[c];
    } else if (index == 8) {
      leading_numbers(line, 3, v);
      for (int r = 0; r < 3; ++r) RT[4 * r + 3] = v[r];
    }
    ++index;
  });
  return true;
}

}  // namespace help

// ====================================================================================================
// Sources/ReconstructionData
// ====================================================================================================
ReconstructionData::ReconstructionData() {
  std::memset(MatrixK, 0, sizeof(MatrixK));
  std::memset(Matrix4K, 0, sizeof(Matrix4K));
  std::memset(MatrixTR, 0, sizeof(MatrixTR));
}

ReconstructionData::ReconstructionData(const std::string &depthPath, const std::string &matrixPath)
    : ReconstructionData(depthPath, matrixPath, false) {}

ReconstructionData::ReconstructionData(const std::string &depthPath, const std::string &matrixPath, bool depthsOptional)
    : ReconstructionData() {
  HasDepthMap = ReadDepthMap(depthPath, &DepthMap, depthsOptional);  // RD.cxx:60-61
  double K[9], RT[16];
  std::memset(K, 0, sizeof(K));
  std::memset(RT, 0, sizeof(RT));
  help::ReadKrtdFile(matrixPath, K, RT);  // RD.cxx:73; the reference ignores its result too
  SetMatrixK(K);                          // RD.cxx:76
  SetMatrixTR(RT);                        // RD.cxx:77
}

int *ReconstructionData::GetDepthMapDimensions() { return DepthMap.dims; }
DepthImage *ReconstructionData::GetDepthMap() { return HasDepthMap ? &DepthMap : nullptr; }
const double *ReconstructionData::Get3MatrixK() const { return MatrixK; }
const double *ReconstructionData::Get4MatrixK() const { return Matrix4K; }
const double *ReconstructionData::GetMatrixTR() const { return MatrixTR; }

void ReconstructionData::SetDepthMap(const DepthImage &data) {
  DepthMap = data;
  HasDepthMap = true;
}

void ReconstructionData::SetMatrixK(const double K3[9]) {
  std::memcpy(MatrixK, K3, sizeof(MatrixK));
  // RD.cxx:201-209: identity, then the 3x3 in the top-left
  for (int i = 0; i < 16; ++i) Matrix4K[i] = (i % 5 == 0) ? 1.0 : 0.0;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Matrix4K[4 * i + j] = MatrixK[3 * i + j];
}

void ReconstructionData::SetMatrixTR(const double RT[16]) { std::memcpy(MatrixTR, RT, sizeof(MatrixTR)); }

bool ReconstructionData::GetColorValue(const int pixelPosition[2], double rgb[3]) const {
  if (!HasDepthMap || DepthMap.color.empty()) {
    std::cerr << "Error, no 'Color' array exists" << std::endl;  // RD.cxx:97-101
    return false;
  }
  const int W = DepthMap.dims[0], H = DepthMap.dims[1];
  const size_t id = ((size_t)(H - 1 - pixelPosition[1]) * W + (size_t)pixelPosition[0]) * 3;  // RD.cxx:105-110
  for (int i = 0; i < 3; ++i) rgb[i] = DepthMap.color[id + i];
  return true;
}

void ReconstructionData::TransformWorldToDepthMapPosition(const double *w, int pixelCoordinate[2]) const {
  // vtkTransform::TransformPoint / TransformVector restated (see oracle/coloration_oracle.c header)
  double c[3], d[3];
  for (int i = 0; i < 3; ++i) c[i] = MatrixTR[4 * i] * w[0] + MatrixTR[4 * i + 1] * w[1] + MatrixTR[4 * i + 2] * w[2] + MatrixTR[4 * i + 3];
  for (int i = 0; i < 3; ++i) d[i] = Matrix4K[4 * i] * c[0] + Matrix4K[4 * i + 1] * c[1] + Matrix4K[4 * i + 2] * c[2];
  d[0] = d[0] / d[2];
  d[1] = d[1] / d[2];
  const double ru = std::round(d[0]), rv = std::round(d[1]);
  // out-of-range conversions are undefined in the reference; here they land outside every image
  pixelCoordinate[0] = (ru > -2147483648.0 && ru < 2147483648.0) ? (int)ru : -1;
  pixelCoordinate[1] = (rv > -2147483648.0 && rv < 2147483648.0) ? (int)rv : -1;
}

void ReconstructionData::ApplyDepthThresholdFilter(double thresholdBestCost) {
  if (!HasDepthMap) return;  // RD.cxx:140-141
  if (DepthMap.depths.empty()) {
    std::cerr << "Error during threshold, depths is empty" << std::endl;  // RD.cxx:148-152
    return;
  }
  const size_t nbTuples = DepthMap.depths.size();
  if (DepthMap.best_cost.size() != nbTuples) return;  // RD.cxx:156-157
  for (size_t i = 0; i < nbTuples; i++)
    if (DepthMap.best_cost[i] > thresholdBestCost) DepthMap.depths[i] = -1;  // RD.cxx:159-166
}

bool ReconstructionData::ReadDepthMap(const std::string &path, DepthImage *out) { return ReadDepthMap(path, out, false); }

bool ReconstructionData::ReadDepthMap(const std::string &path, DepthImage *out, bool depthsOptional) {
  // RD.cxx:223-229 (vtkXMLImageDataReader) through the VTK-free reader; the arrays are then taken by name and
  // type exactly as the reference does: "Depths" and "Best Cost Values" must be vtkDoubleArrays (SafeDownCast,
  // RD.cxx:143-146, cu:249-250), "Color" a vtkUnsignedCharArray with 3 components (RD.cxx:94-95).
  vti::Image img;
  std::string err;
  if (!vti::ReadImageData(path, {"Depths", "Best Cost Values", "Color"}, &img, &err)) {
    std::cerr << "Unable to read depth map : " << err << std::endl;
    return false;
  }
  for (int a = 0; a < 3; ++a) out->dims[a] = img.dims(a);
  const size_t n = (size_t)out->dims[0] * out->dims[1] * out->dims[2];
  out->depths.clear();
  out->best_cost.clear();
  out->color.clear();
  for (const vti::Array &a : img.point_data) {
    if (a.name == "Color") {
      if (a.type != "UInt8" || a.components != 3) {
        std::cerr << "ReadDepthMap: array 'Color' is " << a.type << " x " << a.components << ", not UInt8 x 3" << std::endl;
        return false;
      }
      out->color = a.bytes;
      continue;
    }
    std::vector<double> *dst = a.name == "Depths" ? &out->depths : &out->best_cost;
    if (a.type != "Float64" || a.components != 1) {
      std::cerr << "ReadDepthMap: array '" << a.name << "' is " << a.type << " x " << a.components
                << ", not a 1-component Float64 array (the reference down-casts to vtkDoubleArray)" << std::endl;
      return false;
    }
    dst->resize(n);
    std::memcpy(dst->data(), a.bytes.data(), n * sizeof(double));
  }
  return depthsOptional || !out->depths.empty();
}

// ====================================================================================================
// CudaInitialize / ProcessDepthMap
// ====================================================================================================
FusionDriver::FusionDriver() {
  std::memset(&Grid, 0, sizeof(Grid));
  std::memset(&Ray, 0, sizeof(Ray));
  DepthDims[0] = DepthDims[1] = 0;
}
FusionDriver::~FusionDriver() {
  if (KeptContext) dmi_destroy(KeptContext);
}

void FusionDriver::CudaInitialize(const double i_gridMatrix[16], const int h_gridDims[3], const double h_gridOrig[3],
                                  const double h_gridSpacing[3], double h_rayPThick, double h_rayPRho, double h_rayPEta,
                                  double h_rayPDelta, const int h_depthMapDim[2]) {
  // cu:282-294: the nine constant uploads + ch_gridDims, kept in this object instead of global symbols
  std::memcpy(Grid.grid_matrix, i_gridMatrix, sizeof(Grid.grid_matrix));
  for (int a = 0; a < 3; ++a) {
    Grid.cell_dims[a] = h_gridDims[a] - 1;  // cells = points - 1 (cu:330-331, cu:128-129)
    Grid.origin[a] = h_gridOrig[a];
    Grid.spacing[a] = h_gridSpacing[a];
  }
  Ray.thickness = h_rayPThick;
  Ray.rho = h_rayPRho;
  Ray.eta = h_rayPEta;
  Ray.delta = h_rayPDelta;
  DepthDims[0] = h_depthMapDim[0];
  DepthDims[1] = h_depthMapDim[1];
  Initialized = true;
}

int64_t FusionDriver::NumberOfCells() const {
  return (int64_t)Grid.cell_dims[0] * Grid.cell_dims[1] * Grid.cell_dims[2];
}

namespace {

// One pinned structure-of-arrays chunk of views ([n][H][W] depth, [n][H][W] best cost, [n][16] K, [n][16] RT) and its
// place in the hand-over between the thread that fills chunks and the thread that uploads and fuses them.
struct Chunk {
  double *depth = nullptr, *cost = nullptr;  // pinned (dmi_alloc_pinned)
  std::vector<double> K4, RT;
  std::vector<char> has_cost;
  std::vector<unsigned char> color;  // [n][H][W][3] "Color" planes, only with a colour sink
  size_t first = 0, count = 0;
  bool filled = false;  // guarded by Feed::lock
  bool failed = false;
  std::string error;
};

struct Feed {
  std::mutex lock;
  std::condition_variable changed;
  Chunk slot[2];
  bool abandon = false;  // the consumer gave up: the filler stops at its next hand-over
};

}  // namespace

using ViewFill = ViewSource;

bool FusionDriver::ProcessDepthMap(size_t n_views, const ViewSource &fill, double thresholdBestCost, double *io_scalar) {
  Error.clear();
  if (!Initialized) {
    Error = "ProcessDepthMap: CudaInitialize has not been called";
    return false;
  }
  if (n_views == 0) {  // cu:304-308
    Error = "Error, no depthMap or KRTD matrix have been loaded";
    std::cerr << Error << std::endl;
    return false;
  }
  if (!io_scalar) {
    Error = "ProcessDepthMap: io_scalar is null";
    return false;
  }
  const int W = DepthDims[0], H = DepthDims[1];
  if (W < 1 || H < 1) {
    Error = "ProcessDepthMap: CudaInitialize was given an empty depth-map size";
    return false;
  }
  const size_t npix = (size_t)W * H;
  const bool multi = !Devices.empty();
  if (multi && (ColorSink || KeepContext || ResidentSet)) {
    Error = "ProcessDepthMap: a colour sink, a kept context and a resident view set need a single GPU";
    return false;
  }
  if (KeptContext) dmi_destroy(KeptContext);
  KeptContext = nullptr;

  // cu:323-327: the accumulator starts from io_scalar.  +0.0 everywhere (all bits zero)?  The filter knows (RequestData
  // has just filled the array, filt.cxx:133); other callers' arrays are scanned, eight bytes at a time.
  bool all_zero = InitialGridIsZero;
  InitialGridIsZero = false;
  const int64_t nvox = NumberOfCells();
  if (!all_zero) {
    uint64_t any = 0;
    for (int64_t i = 0; i < nvox; ++i) {
      uint64_t bits;
      std::memcpy(&bits, io_scalar + i, 8);
      any |= bits;
    }
    all_zero = any == 0;
  }

  dmi_context *ctx = nullptr;
  dmi_multi_context *mctx = nullptr;
  if (multi) {
    if (!all_zero) {
      Error = "ProcessDepthMap: a fusion over several GPUs (SetDevices) starts from a zero grid, as RequestData provides (filt.cxx:133)";
      return false;
    }
    dmi_multi_options mo;
    dmi_multi_default_options(&mo);
    mo.partition = Partition;
    // depth-map shards: the north star's float grid, summed by one RCCL all-reduce; z-slabs: the reference's f64, exact
    mo.grid_dtype = Partition == DMI_PARTITION_Z_SLABS ? DMI_F64 : DMI_F32;
    mo.kernel_variant = KernelVariant;
    std::vector<int32_t> devs(Devices.begin(), Devices.end());
    if (dmi_multi_create(&Grid, &Ray, &mo, devs.data(), (int32_t)devs.size(), &mctx) != DMI_OK) {
      Error = dmi_multi_last_error(nullptr);
      return false;
    }
  } else {
    dmi_options opt;
    dmi_default_options(&opt);
    opt.device = Device;
    opt.grid_dtype = DMI_F64;  // ProcessDepthMap<double>, filt.cxx:175
    opt.kernel_variant = KernelVariant;
    if (dmi_create(&Grid, &Ray, &opt, &ctx) != DMI_OK) {
      Error = dmi_last_error(nullptr);
      return false;
    }
    if (!all_zero && dmi_upload_grid(ctx, io_scalar) != DMI_OK) {
      Error = std::string("dmi_upload_grid: ") + dmi_last_error(ctx);
      dmi_destroy(ctx);
      return false;
    }
  }
  auto last_error = [&]() -> std::string { return multi ? dmi_multi_last_error(mctx) : dmi_last_error(ctx); };
  auto destroy = [&]() {
    if (ctx) dmi_destroy(ctx);
    if (mctx) dmi_multi_destroy(mctx);
  };

  // Views go up as pinned structure-of-arrays chunks of at most ~256 MiB.  Two chunks exist: while this thread copies
  // chunk i to the device (dmi_add_views: hipMemcpyAsync on the upload stream, returns when the chunk is resident) and
  // queues its fusion (dmi_fuse_range, asynchronous on the compute stream), a second thread fills chunk i+1 -- reading
  // and parsing the .vti / .krtd files when the views come from list files, as the reference does one view at a time
  // inside its loop (cu:343-353).  Host residency is two chunks whatever the number of views; every voxel still
  // accumulates its views in order (cu:211), and the f64 grid makes the chunking invisible in the result.
  const size_t chunk = std::max<size_t>(1, std::min(n_views, HostChunkBytes / std::max<size_t>(1, npix * 16)));
  Feed feed;
  bool ok = true;
  int32_t last_first = (int32_t)n_views, last_count = 0;  // the chunk whose fusion is left to dmi_fuse_range_download
  constexpr int32_t kDownloadSlabs = 8;
  for (Chunk &c : feed.slot) {
    void *pd = nullptr, *pc = nullptr;
    if (dmi_alloc_pinned(chunk * npix * 8, &pd) != DMI_OK || dmi_alloc_pinned(chunk * npix * 8, &pc) != DMI_OK) {
      if (pd) dmi_free_pinned(pd);
      Error = "ProcessDepthMap: dmi_alloc_pinned failed";
      ok = false;
      break;
    }
    c.depth = static_cast<double *>(pd);
    c.cost = static_cast<double *>(pc);
    c.K4.resize(chunk * 16);
    c.RT.resize(chunk * 16);
    c.has_cost.resize(chunk);
    if (ColorSink) c.color.resize(chunk * npix * 3);
  }
  auto free_chunks = [&]() {
    for (Chunk &c : feed.slot) {
      if (c.depth) dmi_free_pinned(c.depth);
      if (c.cost) dmi_free_pinned(c.cost);
      c.depth = c.cost = nullptr;
    }
  };
  if (!ok) {
    free_chunks();
    destroy();
    return false;
  }

  const size_t n_chunks = (n_views + chunk - 1) / chunk;
  // fills chunk q (on the filler thread, or on this one just before the chunk is needed)
  auto fill_chunk = [&](size_t q) {
      Chunk &c = feed.slot[q & 1];
      c.first = q * chunk;
      c.count = std::min(chunk, n_views - c.first);
      c.failed = false;
      for (size_t v = 0; v < c.count && !c.failed; ++v) {
        bool has_cost = false;
        FillColor = ColorSink ? c.color.data() + v * npix * 3 : nullptr;  // (one thread fills at a time)
        try {
          if (!fill(c.first + v, c.depth + v * npix, c.cost + v * npix, &has_cost, &c.K4[v * 16], &c.RT[v * 16], &c.error)) c.failed = true;
        } catch (const std::exception &e) {
          c.error = std::string("view ") + std::to_string(c.first + v) + ": " + e.what();
          c.failed = true;
        }
        c.has_cost[v] = has_cost ? 1 : 0;
      }
  };
  std::thread filler;
  if (!FillOnCallingThread)
    filler = std::thread([&]() {
      for (size_t q = 0; q < n_chunks; ++q) {
        Chunk &c = feed.slot[q & 1];
        {
          std::unique_lock<std::mutex> hold(feed.lock);
          feed.changed.wait(hold, [&] { return !c.filled || feed.abandon; });
          if (feed.abandon) return;
        }
        fill_chunk(q);
        {
          std::lock_guard<std::mutex> hold(feed.lock);
          c.filled = true;
        }
        feed.changed.notify_all();
        if (c.failed) return;
      }
    });

  for (size_t q = 0; ok && q < n_chunks; ++q) {
    Chunk &c = feed.slot[q & 1];
    if (FillOnCallingThread) {
      fill_chunk(q);  // the previous chunk's fusion is still running on the device meanwhile
    } else {
      std::unique_lock<std::mutex> hold(feed.lock);
      feed.changed.wait(hold, [&] { return c.filled; });
    }
    if (c.failed) {
      Error = c.error;
      ok = false;
      break;
    }
    // RD.cxx:156-157: the filter is skipped for a view whose cost array does not match.  A chunk whose views all have
    // costs is thresholded on the device (fused into the upload kernel); a mixed chunk on this copy, view by view.
    bool every_view_has_cost = true;
    for (size_t v = 0; v < c.count; ++v) every_view_has_cost = every_view_has_cost && c.has_cost[v];
    if (!every_view_has_cost && !ResidentSet)
      for (size_t v = 0; v < c.count; ++v)
        if (c.has_cost[v])
          for (size_t i = 0; i < npix; ++i)
            if (c.cost[v * npix + i] > thresholdBestCost) c.depth[v * npix + i] = -1;  // RD.cxx:159-166
    const double *cost = every_view_has_cost ? c.cost : nullptr;
    int rc;
    if (multi) {
      rc = dmi_multi_add_views(mctx, c.depth, cost, thresholdBestCost, c.K4.data(), c.RT.data(), (int32_t)c.count, W, H);
    } else {
      // (a resident set holds the chunk's depths, thresholded when it was loaded: they go from its planes to the context's)
      rc = ResidentSet ? dmi_add_views_from_set(ctx, ResidentSet, (int32_t)c.first, (int32_t)c.count)
                       : dmi_add_views(ctx, c.depth, cost, thresholdBestCost, c.K4.data(), c.RT.data(), (int32_t)c.count, W, H);
      // replaces the kernel launches of these views (cu:363); runs while the next chunk is filled and copied.  The LAST chunk
      // is fused together with the copy back, below: slab by slab, each slab on its way to the host under the next one's fusion
      if (c.first + c.count == n_views) {
        last_first = (int32_t)c.first;
        last_count = (int32_t)c.count;
      } else if (rc == DMI_OK) {
        rc = dmi_fuse_range(ctx, (int32_t)c.first, (int32_t)c.count);
      }
      // the same chunk's colour planes, while that fusion runs
      if (rc == DMI_OK && ColorSink && dmi_color_add_views(ColorSink, c.color.data(), c.K4.data(), c.RT.data(), (int32_t)c.count, W, H) != DMI_OK) {
        Error = std::string("dmi_color_add_views: ") + dmi_color_last_error();
        ok = false;
        break;
      }
    }
    if (rc != DMI_OK) {
      Error = std::string(multi ? "dmi_multi_add_views: " : "dmi_add_views / dmi_fuse_range: ") + last_error();
      ok = false;
      break;
    }
    {
      std::lock_guard<std::mutex> hold(feed.lock);
      c.filled = false;  // the chunk is resident on the device: its buffers may be refilled
    }
    feed.changed.notify_all();
  }
  {
    std::lock_guard<std::mutex> hold(feed.lock);
    feed.abandon = !ok;
  }
  feed.changed.notify_all();
  if (filler.joinable()) filler.join();
  free_chunks();
  if (!ok) {
    destroy();
    return false;
  }
  if (multi) {
    // the whole fusion: every device fuses its share of the views, the library sums the grids (one RCCL all-reduce,
    // overlapped slab by slab) or, for z-slabs, there is nothing to exchange
    if (dmi_multi_fuse(mctx) != DMI_OK || dmi_multi_download_grid_f64(mctx, io_scalar, nullptr, nullptr) != DMI_OK) {
      Error = std::string("dmi_multi_fuse / download: ") + last_error();
      destroy();
      return false;
    }
    dmi_multi_timings t;
    if (dmi_multi_get_timings(mctx, &t) == DMI_OK) FuseKernelMs = t.last_step_ms;
  } else {
    // cu:363 for the last chunk's views and cu:368-371 (synchronises)
    if (dmi_fuse_range_download(ctx, last_first, last_count, io_scalar, DMI_F64, kDownloadSlabs) != DMI_OK) {
      Error = std::string("dmi_fuse_range_download: ") + last_error();
      destroy();
      return false;
    }
    dmi_timings t;
    if (dmi_get_timings(ctx, &t) == DMI_OK) FuseKernelMs = t.total_fuse_kernel_ms;
    if (KeepContext) {
      KeptContext = ctx;
      ctx = nullptr;
    }
  }
  destroy();
  return true;
}

bool FusionDriver::ProcessDepthMap(const std::vector<ReconstructionData *> &views, double thresholdBestCost,
                                   double *io_scalar) {
  const int W = DepthDims[0], H = DepthDims[1];
  const size_t npix = (size_t)W * H;
  const ViewFill fill = [&](size_t index, double *depth, double *cost, bool *has_cost, double K4[16], double RT[16],
                            std::string *error) {
    ReconstructionData *d = views[index];
    DepthImage *img = d ? d->GetDepthMap() : nullptr;
    if (!img || img->dims[0] != W || img->dims[1] != H || img->depths.size() != npix) {
      // the reference takes the depth-map size from view 0 only (filt.cxx:167-168) and would read past the end of a
      // smaller table; here a mismatch is an error
      *error = "ProcessDepthMap: view " + std::to_string(index) + " has no depth map of the size given to CudaInitialize";
      return false;
    }
    if (!ResidentSet) std::memcpy(depth, img->depths.data(), npix * 8);  // (a resident set holds the depths: nothing to stage)
    *has_cost = !ResidentSet && img->best_cost.size() == npix;
    if (*has_cost) std::memcpy(cost, img->best_cost.data(), npix * 8);
    if (FillColor) {
      if (img->color.size() != npix * 3) {
        *error = "ProcessDepthMap: view " + std::to_string(index) + " has no UInt8 x 3 'Color' array of the views' size";
        return false;
      }
      std::memcpy(FillColor, img->color.data(), npix * 3);
    }
    std::memcpy(K4, d->Get4MatrixK(), 16 * 8);  // cu:352
    std::memcpy(RT, d->GetMatrixTR(), 16 * 8);  // cu:353
    return true;
  };
  if (ResidentSet) {
    dmi_views_info info;
    if (dmi_views_get_info(ResidentSet, &info) != DMI_OK || (size_t)info.n != views.size() || info.W != W || info.H != H) {
      Error = "ProcessDepthMap: the resident view set does not hold these views (their number or their size differs)";
      return false;
    }
  }
  return ProcessDepthMap(views.size(), fill, thresholdBestCost, io_scalar);
}

bool FusionDriver::ProcessDepthMap(const std::vector<std::string> &vtiList, const std::vector<std::string> &krtdList,
                                   double thresholdBestCost, double *io_scalar) {
  if (vtiList.size() == 0 || krtdList.size() == 0) {  // cu:304-308
    Error = "Error, no depthMap or KRTD matrix have been loaded";
    std::cerr << Error << std::endl;
    return false;
  }
  const size_t n = vtiList.size();  // cu:310
  if (krtdList.size() < n) {
    Error = "ProcessDepthMap: fewer krtd files than depth maps";
    return false;
  }
  const int W = DepthDims[0], H = DepthDims[1];
  const size_t npix = (size_t)W * H;
  // one view at a time, read where the reference reads it (cu:347), straight into the pinned chunk: no view outlives
  // the chunk it travels in
  const ViewFill fill = [&](size_t index, double *depth, double *cost, bool *has_cost, double K4[16], double RT[16],
                            std::string *error) {
    ReconstructionData data(vtiList[index], krtdList[index]);
    DepthImage *img = data.GetDepthMap();
    if (!img) {
      *error = "ProcessDepthMap: cannot read depth map " + vtiList[index];
      return false;
    }
    if (img->dims[0] != W || img->dims[1] != H || img->depths.size() != npix) {
      *error = "ProcessDepthMap: depth map " + vtiList[index] + " does not have the size given to CudaInitialize";
      return false;
    }
    std::memcpy(depth, img->depths.data(), npix * 8);
    *has_cost = img->best_cost.size() == npix;
    if (*has_cost) std::memcpy(cost, img->best_cost.data(), npix * 8);
    if (FillColor) {
      if (img->color.size() != npix * 3) {
        *error = "ProcessDepthMap: depth map " + vtiList[index] + " has no UInt8 x 3 'Color' array of the views' size (--meshColoration needs it)";
        return false;
      }
      std::memcpy(FillColor, img->color.data(), npix * 3);
    }
    std::memcpy(K4, data.Get4MatrixK(), 16 * 8);
    std::memcpy(RT, data.GetMatrixTR(), 16 * 8);
    return true;
  };
  return ProcessDepthMap(n, fill, thresholdBestCost, io_scalar);
}

// ---- what the depth-map filters below and DepthViewSet::Load share: the views checked and gathered, the planes put back ----
namespace {

// The views' common size: view 0 has a depth map and there are not too many of them.  false: *error says why, in `caller`'s name.
bool CommonViewSize(const char *caller, const std::vector<ReconstructionData *> &views, int *W, int *H, std::string *error) {
  const size_t n = views.size();
  DepthImage *first = n && views[0] ? views[0]->GetDepthMap() : nullptr;
  if (!first) {
    *error = std::string(caller) + ": no views, or view 0 has no depth map";
    return false;
  }
  if (n > 0x7fffffffu) {
    *error = std::string(caller) + ": too many views";
    return false;
  }
  *W = first->dims[0];
  *H = first->dims[1];
  return true;
}

// view m has a depth map of that size
bool ViewHasSize(const char *caller, const std::vector<ReconstructionData *> &views, size_t m, int W, int H, std::string *error) {
  DepthImage *img = views[m] ? views[m]->GetDepthMap() : nullptr;
  if (img && img->dims[0] == W && img->dims[1] == H && img->depths.size() == (size_t)W * H) return true;
  *error = std::string(caller) + ": view " + std::to_string(m) + " has no depth map of the size of view 0";
  return false;
}

struct GatheredViews {
  int W = 0, H = 0;
  size_t npix = 0;
  std::vector<double> depth;   // [n][H][W], thresholded
  std::vector<double> K4, RT;  // [n][16] each, where asked for
};

// View after view: checked, thresholded (ApplyDepthThresholdFilter) and copied; a view that fails leaves the ones before it
// thresholded.
bool GatherViews(const char *caller, const std::vector<ReconstructionData *> &views, double thresholdBestCost, bool withCameras,
                 GatheredViews *g, std::string *error) {
  if (!CommonViewSize(caller, views, &g->W, &g->H, error)) return false;
  const size_t n = views.size(), npix = g->npix = (size_t)g->W * g->H;
  g->depth.resize(n * npix);
  if (withCameras) {
    g->K4.resize(n * 16);
    g->RT.resize(n * 16);
  }
  for (size_t m = 0; m < n; ++m) {
    if (!ViewHasSize(caller, views, m, g->W, g->H, error)) return false;
    views[m]->ApplyDepthThresholdFilter(thresholdBestCost);
    std::memcpy(g->depth.data() + m * npix, views[m]->GetDepthMap()->depths.data(), npix * 8);
    if (withCameras) {
      std::memcpy(g->K4.data() + m * 16, views[m]->Get4MatrixK(), 16 * 8);
      std::memcpy(g->RT.data() + m * 16, views[m]->GetMatrixTR(), 16 * 8);
    }
  }
  return true;
}

// The planes back into the views; perView(m, before, &after) -- the view's map as it was and as it is about to be set -- where given.
void ScatterViews(const std::vector<ReconstructionData *> &views, const GatheredViews &g,
                  const std::function<void(size_t, const DepthImage &, DepthImage *)> &perView = nullptr) {
  for (size_t m = 0; m < views.size(); ++m) {
    const DepthImage &before = *views[m]->GetDepthMap();
    DepthImage after = before;
    after.depths.assign(g.depth.begin() + (ptrdiff_t)(m * g.npix), g.depth.begin() + (ptrdiff_t)((m + 1) * g.npix));
    if (perView) perView(m, before, &after);
    views[m]->SetDepthMap(after);
  }
}

bool LastError(std::string *error) {
  *error = dmi_last_error(nullptr);
  return false;
}

}  // namespace

// Not in the reference (recon_host.h)
bool FilterDepthConsistency(const std::vector<ReconstructionData *> &views, double thresholdBestCost, int minViews,
                            double absTolerance, double relTolerance, int device, DepthConsistencyReport *report, std::string *error) {
  GatheredViews g;
  if (!GatherViews("FilterDepthConsistency", views, thresholdBestCost, true, &g, error)) return false;
  DepthConsistencyReport r;
  r.views = views.size();
  for (const double d : g.depth) r.validPixels += d > 0.0 && d < HUGE_VAL ? 1 : 0;
  if (dmi_filter_depth_consistency(g.depth.data(), nullptr, 0.0, g.K4.data(), g.RT.data(), (int32_t)views.size(), g.W, g.H, absTolerance,
                                   relTolerance, minViews, device, g.depth.data(), nullptr, &r.kernelMs) != DMI_OK)
    return LastError(error);
  for (const double d : g.depth) r.keptPixels += d > 0.0 ? 1 : 0;
  ScatterViews(views, g);
  if (report) *report = r;
  return true;
}

// Not in the reference (recon_host.h)
bool FilterDepthSpeckles(const std::vector<ReconstructionData *> &views, double thresholdBestCost, long long minPixels,
                         double absTolerance, double relTolerance, int device, DepthSpeckleReport *report, std::string *error) {
  GatheredViews g;
  if (!GatherViews("FilterDepthSpeckles", views, thresholdBestCost, false, &g, error)) return false;
  const size_t npix = g.npix;
  DepthSpeckleReport r;
  r.views = views.size();
  for (const double d : g.depth) r.validPixels += d > 0.0 && d < HUGE_VAL ? 1 : 0;
  std::vector<int32_t> size(g.depth.size());
  if (dmi_filter_depth_speckles(g.depth.data(), nullptr, 0.0, (int32_t)views.size(), g.W, g.H, absTolerance, relTolerance, minPixels, device,
                                g.depth.data(), size.data(), &r.kernelMs) != DMI_OK)
    return LastError(error);
  for (const double d : g.depth) r.keptPixels += d > 0.0 ? 1 : 0;
  // a segment of s pixels shows s times in the sizes: the pixels of size s, over s, are the segments of that size
  std::vector<uint64_t> pixelsOfSize(npix + 1, 0);
  for (const int32_t s : size)
    if (s > 0 && (size_t)s <= npix) ++pixelsOfSize[(size_t)s];
  for (size_t s = 1; s <= npix; ++s) {
    r.segments += pixelsOfSize[s] / s;
    if ((long long)s >= minPixels) r.keptSegments += pixelsOfSize[s] / s;
  }
  ScatterViews(views, g);
  if (report) *report = r;
  return true;
}

// Not in the reference (recon_host.h)
bool FillDepthHoles(const std::vector<ReconstructionData *> &views, double thresholdBestCost, long long maxPixels, double absTolerance,
                    double relTolerance, int device, DepthHolesReport *report, std::string *error) {
  GatheredViews g;
  if (!GatherViews("FillDepthHoles", views, thresholdBestCost, false, &g, error)) return false;
  const size_t npix = g.npix;
  const std::vector<double> &depth = g.depth;
  DepthHolesReport r;
  r.views = views.size();
  std::vector<int32_t> size(depth.size());
  if (dmi_fill_depth_holes(g.depth.data(), nullptr, 0.0, (int32_t)views.size(), g.W, g.H, absTolerance, relTolerance, maxPixels, device,
                           g.depth.data(), size.data(), &r.kernelMs) != DMI_OK)
    return LastError(error);
  // a hole of s pixels shows s times in the sizes, and a filled hole is filled at every pixel: the pixels of size s, over s, are
  // the holes of that size
  std::vector<uint64_t> pixelsOfSize(npix + 1, 0), filledOfSize(npix + 1, 0);
  for (size_t i = 0; i < size.size(); ++i) {
    const int32_t s = size[i];
    if (s <= 0 || (size_t)s > npix) continue;
    ++pixelsOfSize[(size_t)s];
    if (depth[i] != -1.0) {
      ++filledOfSize[(size_t)s];
      ++r.filledPixels;
    }
  }
  for (size_t s = 1; s <= npix; ++s) {
    r.holes += pixelsOfSize[s] / s;
    r.filledHoles += filledOfSize[s] / s;
  }
  // a pixel the threshold had dropped and the fill gave a depth again must pass the threshold from now on: the consistency
  // filter, the bounds estimate and the fusion all apply it once more
  ScatterViews(views, g, [&](size_t, const DepthImage &, DepthImage *filled) {
    if (filled->best_cost.size() == npix)
      for (size_t i = 0; i < npix; ++i)
        if (filled->depths[i] != -1.0 && filled->best_cost[i] > thresholdBestCost) filled->best_cost[i] = thresholdBestCost;
  });
  if (report) *report = r;
  return true;
}

// Not in the reference (recon_host.h)
bool SmoothDepths(const std::vector<ReconstructionData *> &views, double thresholdBestCost, double sigma, double truncate,
                  double absTolerance, double relTolerance, int iterations, int device, DepthSmoothReport *report, std::string *error) {
  GatheredViews g;
  if (!GatherViews("SmoothDepths", views, thresholdBestCost, false, &g, error)) return false;
  const size_t npix = g.npix;
  DepthSmoothReport r;
  r.views = views.size();
  std::vector<int32_t> count(g.depth.size());
  if (dmi_smooth_depths(g.depth.data(), nullptr, 0.0, (int32_t)views.size(), g.W, g.H, sigma, truncate, absTolerance, relTolerance,
                        (int32_t)iterations, device, g.depth.data(), count.data(), &r.kernelMs) != DMI_OK)
    return LastError(error);
  uint64_t taps = 0;
  ScatterViews(views, g, [&](size_t m, const DepthImage &before, DepthImage *smoothed) {
    for (size_t i = 0; i < npix; ++i) {
      if (smoothed->depths[i] == -1.0) continue;  // what is not valid comes out as -1, and nothing else does
      ++r.validPixels;
      taps += (uint64_t)count[m * npix + i];
      if (smoothed->depths[i] != before.depths[i]) ++r.changedPixels;
    }
  });
  r.meanTaps = r.validPixels ? (double)taps / (double)r.validPixels : 0.0;
  if (report) *report = r;
  return true;
}

// Not in the reference (recon_host.h)
bool EstimateSceneBounds(const std::vector<ReconstructionData *> &views, double thresholdBestCost, const double axes[9],
                         double trimFraction, int pixelStep, int device, SceneBoundsReport *report, std::string *error) {
  GatheredViews g;
  if (!GatherViews("EstimateSceneBounds", views, thresholdBestCost, true, &g, error)) return false;
  SceneBoundsReport r;
  r.views = views.size();
  if (dmi_estimate_scene_bounds(g.depth.data(), nullptr, 0.0, g.K4.data(), g.RT.data(), (int32_t)views.size(), g.W, g.H, axes, trimFraction,
                                pixelStep, device, r.lo, r.hi, &r.points, &r.kernelMs) != DMI_OK)
    return LastError(error);
  if (report) *report = r;
  return true;
}

// Not in the reference (recon_host.h)
bool DepthViewSet::Fail(const char *what) {
  Error = std::string(what) + ": " + dmi_views_last_error(Set);
  return false;
}

void DepthViewSet::Release() {
  if (Set) dmi_views_destroy(Set);
  Set = nullptr;
  NViews = 0;
}

bool DepthViewSet::Load(const std::vector<ReconstructionData *> &views, double thresholdBestCost, int device) {
  Release();
  Code = DMI_ERR_INVALID_ARGUMENT;
  const size_t n = views.size();
  if (!CommonViewSize("DepthViewSet", views, &W, &H, &Error)) return false;
  Dev = device;
  const size_t npix = (size_t)W * H;
  for (size_t m = 0; m < n; ++m)
    if (!ViewHasSize("DepthViewSet", views, m, W, H, &Error)) return false;
  if ((Code = dmi_views_create(device, W, H, &Set)) != DMI_OK) {
    Error = std::string("dmi_views_create: ") + dmi_views_last_error(nullptr);
    Set = nullptr;
    return false;
  }
  const size_t chunk = std::max<size_t>(1, std::min(n, (size_t(256) << 20) / std::max<size_t>(1, npix * 8)));
  std::vector<double> depth(chunk * npix), cost(chunk * npix), K4(chunk * 16), RT(chunk * 16);
  for (size_t m0 = 0; m0 < n; m0 += chunk) {
    const size_t cnt = std::min(chunk, n - m0);
    bool every_view_has_cost = true;
    for (size_t v = 0; v < cnt; ++v) every_view_has_cost = every_view_has_cost && views[m0 + v]->GetDepthMap()->best_cost.size() == npix;
    for (size_t v = 0; v < cnt; ++v) {
      const DepthImage *img = views[m0 + v]->GetDepthMap();
      std::memcpy(depth.data() + v * npix, img->depths.data(), npix * 8);
      if (every_view_has_cost) {
        std::memcpy(cost.data() + v * npix, img->best_cost.data(), npix * 8);
      } else if (img->best_cost.size() == npix) {  // a mixed piece: on this copy, view by view (RD.cxx:159-166)
        for (size_t i = 0; i < npix; ++i)
          if (img->best_cost[i] > thresholdBestCost) depth[v * npix + i] = -1;
      }
      std::memcpy(K4.data() + v * 16, views[m0 + v]->Get4MatrixK(), 16 * 8);
      std::memcpy(RT.data() + v * 16, views[m0 + v]->GetMatrixTR(), 16 * 8);
    }
    Code = dmi_views_add(Set, depth.data(), every_view_has_cost ? cost.data() : nullptr, thresholdBestCost, K4.data(), RT.data(), (int32_t)cnt);
    if (Code != DMI_OK) {
      Fail("dmi_views_add");
      Release();
      return false;
    }
  }
  NViews = n;
  return true;
}

bool DepthViewSet::FilterSpeckles(long long minPixels, double absTolerance, double relTolerance, DepthSpeckleReport *report) {
  dmi_views_step_report r;
  if ((Code = dmi_views_filter_speckles(Set, absTolerance, relTolerance, minPixels, nullptr, &r)) != DMI_OK)
    return Fail("dmi_views_filter_speckles");
  if (report) {
    *report = DepthSpeckleReport();
    report->views = NViews;
    report->validPixels = r.valid_before;
    report->keptPixels = r.valid_after;
    report->segments = r.groups;
    report->keptSegments = r.groups_kept;
    report->kernelMs = r.kernel_ms;
  }
  return true;
}

bool DepthViewSet::FillHoles(long long maxPixels, double absTolerance, double relTolerance, DepthHolesReport *report) {
  dmi_views_step_report r;
  if ((Code = dmi_views_fill_holes(Set, absTolerance, relTolerance, maxPixels, nullptr, &r)) != DMI_OK) return Fail("dmi_views_fill_holes");
  if (report) {
    *report = DepthHolesReport();
    report->views = NViews;
    report->holes = r.groups;
    report->filledHoles = r.groups_kept;
    report->filledPixels = r.changed;
    report->kernelMs = r.kernel_ms;
  }
  return true;
}

bool DepthViewSet::Smooth(double sigma, double truncate, double absTolerance, double relTolerance, int iterations,
                          DepthSmoothReport *report) {
  dmi_views_step_report r;
  if ((Code = dmi_views_smooth(Set, sigma, truncate, absTolerance, relTolerance, (int32_t)iterations, nullptr, &r)) != DMI_OK)
    return Fail("dmi_views_smooth");
  if (report) {
    *report = DepthSmoothReport();
    report->views = NViews;
    report->validPixels = r.valid_after;
    report->changedPixels = r.changed;
    report->meanTaps = r.valid_after ? (double)r.aux_sum / (double)r.valid_after : 0.0;
    report->kernelMs = r.kernel_ms;
  }
  return true;
}

bool DepthViewSet::FilterConsistency(int minViews, double absTolerance, double relTolerance, DepthConsistencyReport *report) {
  dmi_views_step_report r;
  if ((Code = dmi_views_filter_consistency(Set, absTolerance, relTolerance, (int32_t)minViews, nullptr, &r)) != DMI_OK)
    return Fail("dmi_views_filter_consistency");
  if (report) {
    *report = DepthConsistencyReport();
    report->views = NViews;
    report->validPixels = r.valid_before;
    report->keptPixels = r.valid_after;
    report->kernelMs = r.kernel_ms;
  }
  return true;
}

bool DepthViewSet::EstimateBounds(const double axes[9], double trimFraction, int pixelStep, SceneBoundsReport *report) {
  SceneBoundsReport r;
  r.views = NViews;
  if ((Code = dmi_views_estimate_bounds(Set, axes, trimFraction, (int32_t)pixelStep, r.lo, r.hi, &r.points, &r.kernelMs)) != DMI_OK)
    return Fail("dmi_views_estimate_bounds");
  if (report) *report = r;
  return true;
}

bool DepthViewSet::BuildPoints(double absTolerance, double relTolerance, double normalAbsTolerance, double normalRelTolerance, int minViews,
                               int pixelStep, bool dedupe, DepthPointsReport *report) {
  dmi_views_points_report r;
  uint64_t n = 0;
  if ((Code = dmi_views_build_points(Set, absTolerance, relTolerance, normalAbsTolerance, normalRelTolerance, (int32_t)minViews,
                                     (int32_t)pixelStep, dedupe ? 1 : 0, &n, &r)) != DMI_OK)
    return Fail("dmi_views_build_points");
  NPoints = n;
  Filtered = false;
  Fitted = false;
  if (report) {
    *report = DepthPointsReport();
    report->views = NViews;
    report->validPixels = r.valid;
    report->candidates = r.candidates;
    report->owned = r.owned;
    report->points = r.points;
    report->withNormal = r.with_normal;
    report->kernelMs = r.kernel_ms;
  }
  return true;
}

bool DepthViewSet::ThinPoints(double cellSize, int minPoints, DepthThinReport *report) {
  dmi_points_thin_report r;
  uint64_t n = 0;
  if ((Code = dmi_views_thin_points(Set, cellSize, (int32_t)minPoints, &n, &r)) != DMI_OK) return Fail("dmi_views_thin_points");
  NPoints = n;
  Filtered = false;
  Fitted = false;
  if (report) {
    *report = DepthThinReport();
    report->pointsIn = r.points_in;
    report->cells = r.cells;
    report->cellsKept = r.cells_kept;
    report->multiViewCells = r.multi_view_cells;
    report->largestCell = r.largest_cell;
    report->withNormal = r.with_normal;
    report->kernelMs = r.kernel_ms;
  }
  return true;
}

bool DepthViewSet::FilterPointsRadius(double radius, int minNeighbors, DepthRadiusReport *report) {
  dmi_points_radius_report r;
  uint64_t n = 0;
  if ((Code = dmi_views_filter_points_radius(Set, radius, (int32_t)minNeighbors, &n, &r)) != DMI_OK)
    return Fail("dmi_views_filter_points_radius");
  NPoints = n;
  Filtered = true;
  Fitted = false;
  if (report) {
    *report = DepthRadiusReport();
    report->pointsIn = r.points_in;
    report->pointsKept = r.points_kept;
    report->isolated = r.isolated;
    report->maxNeighbors = r.max_neighbors;
    report->neighborSum = r.neighbor_sum;
    report->distanceTests = r.distance_tests;
    report->kernelMs = r.kernel_ms;
  }
  return true;
}

bool DepthViewSet::FitPointPlanes(double radius, int minNeighbors, bool move, bool normals, DepthPlaneFitReport *report) {
  dmi_points_planes_report r;
  const int32_t flags = (move ? DMI_PLANE_FIT_MOVE : 0) | (normals ? DMI_PLANE_FIT_NORMALS : 0);
  if ((Code = dmi_views_fit_point_planes(Set, radius, (int32_t)minNeighbors, flags, &r)) != DMI_OK)
    return Fail("dmi_views_fit_point_planes");
  Fitted = true;
  if (report) {
    *report = DepthPlaneFitReport();
    report->pointsIn = r.points_in;
    report->fitted = r.fitted;
    report->unsupported = r.unsupported;
    report->crowded = r.crowded;
    report->maxNeighbors = r.max_neighbors;
    report->neighborSum = r.neighbor_sum;
    report->distanceTests = r.distance_tests;
    report->maxShift = r.max_shift;
    report->kernelMs = r.kernel_ms;
  }
  return true;
}

bool DepthViewSet::DownloadPoints(DepthPoints *points) {
  const size_t n = (size_t)NPoints;
  points->plane_rms.resize(Fitted ? n : 0);
  if (Fitted && (Code = dmi_views_download_point_plane_rms(Set, 0, NPoints, points->plane_rms.data())) != DMI_OK)
    return Fail("dmi_views_download_point_plane_rms");
  points->neighbors.resize(Filtered ? n : 0);
  if (Filtered && (Code = dmi_views_download_point_neighbors(Set, 0, NPoints, points->neighbors.data())) != DMI_OK)
    return Fail("dmi_views_download_point_neighbors");
  points->members.resize(n);
  if ((Code = dmi_views_download_point_members(Set, 0, NPoints, points->members.data())) != DMI_OK)
    return Fail("dmi_views_download_point_members");
  points->xyz.resize(3 * n);
  points->normal.resize(3 * n);
  points->view.resize(n);
  points->pixel.resize(n);
  points->count.resize(n);
  if ((Code = dmi_views_download_points(Set, 0, NPoints, points->xyz.data(), points->normal.data(), points->view.data(),
                                        points->pixel.data(), points->count.data())) != DMI_OK)
    return Fail("dmi_views_download_points");
  return true;
}

bool DepthViewSet::Store(const std::vector<ReconstructionData *> &views, double thresholdBestCost) {
  if (!Set || views.size() != NViews) {
    Code = DMI_ERR_INVALID_ARGUMENT;
    Error = "DepthViewSet: these are not the views the set was loaded from";
    return false;
  }
  const size_t npix = (size_t)W * H;
  std::vector<double> depth(npix);
  for (size_t m = 0; m < NViews; ++m) {  // (a view at a time: host memory holds one plane more)
    if ((Code = dmi_views_download(Set, (int32_t)m, 1, depth.data())) != DMI_OK) return Fail("dmi_views_download");
    DepthImage stored = *views[m]->GetDepthMap();
    stored.depths = depth;
    if (stored.best_cost.size() == npix)
      for (size_t i = 0; i < npix; ++i)
        if (stored.depths[i] != -1.0 && stored.best_cost[i] > thresholdBestCost) stored.best_cost[i] = thresholdBestCost;
    views[m]->SetDepthMap(stored);
  }
  return true;
}

// ====================================================================================================
// vtkCudaReconstructionFilter
// ====================================================================================================
ReconstructionFilter::ReconstructionFilter() {
  // filt.cxx:76-85
  std::memset(GridMatrix, 0, sizeof(GridMatrix));
  RayPotentialRho = RayPotentialThickness = RayPotentialDelta = RayPotentialEta = ThresholdBestCost = 0;
  ExecutionTime = 0;
  InDims[0] = InDims[1] = InDims[2] = 0;
  for (int a = 0; a < 3; ++a) InOrigin[a] = InSpacing[a] = 0;
}
ReconstructionFilter::~ReconstructionFilter() {
  if (KeptContext) dmi_destroy(KeptContext);
}

void ReconstructionFilter::SetFilePathKRTD(const char *path) {
  HasKRTD = path != nullptr;
  FilePathKRTD = path ? path : "";
}
void ReconstructionFilter::SetFilePathVTI(const char *path) {
  HasVTI = path != nullptr;
  FilePathVTI = path ? path : "";
}
void ReconstructionFilter::SetGridMatrix(const double gridMatrix[16]) {
  HasGridMatrix = gridMatrix != nullptr;
  if (gridMatrix) std::memcpy(GridMatrix, gridMatrix, sizeof(GridMatrix));
}
void ReconstructionFilter::SetInputData(const int dims[3], const double origin[3], const double spacing[3]) {
  for (int a = 0; a < 3; ++a) {
    InDims[a] = dims[a];
    InOrigin[a] = origin[a];
    InSpacing[a] = spacing[a];
  }
  HasInput = true;
}

int64_t ReconstructionFilter::GetNumberOfCells() const {
  if (!HasInput) return 0;
  int64_t n = 1;
  for (int a = 0; a < 3; ++a) n *= std::max(InDims[a] - 1, 0);  // vtkImageData::GetNumberOfCells for a 3-D image
  return n;
}

int ReconstructionFilter::Update() { return RequestData(); }

int ReconstructionFilter::RequestData() {
  ExecutionTime = -1;  // filt.cxx:101
  const clock_t start = clock();
  Error.clear();
  if (!HasInput) {
    Error = "Error, no input grid has been set.";
    std::cerr << Error << std::endl;
    return 0;
  }
  if (!HasKRTD || !HasVTI) {  // filt.cxx:114-118
    Error = "Error, some inputs have not been set.";
    std::cerr << Error << std::endl;
    return 0;
  }
  int gridDims[3];
  double gridOrig[3], gridSpacing[3];
  for (int a = 0; a < 3; ++a) {  // filt.cxx:121-126
    gridOrig[a] = InOrigin[a];
    gridDims[a] = InDims[a];
    gridSpacing[a] = InSpacing[a];
  }
  OutScalar.assign((size_t)GetNumberOfCells(), 0.0);  // filt.cxx:129-133
  if (RayPotentialRho == 0 && RayPotentialThickness == 0) {  // filt.cxx:138-142
    Error = "Error : Ray potential Rho or Thickness or both have not been set";
    std::cerr << Error << std::endl;
    return 0;
  }
  const int rc = Compute(gridDims, gridOrig, gridSpacing, &OutScalar);
  const clock_t end = clock();
  ExecutionTime = (double)(end - start) / CLOCKS_PER_SEC;  // filt.cxx:147-148 (CPU time, as the reference)
  return rc == 0 ? 1 : 0;
}

int ReconstructionFilter::Compute(int gridDims[3], double gridOrig[3], double gridSpacing[3], std::vector<double> *outScalar) {
  if (!HasGridMatrix) {
    // the reference dereferences a null GridMatrix in CudaInitialize (cu:280); here it is an error
    Error = "Error : GridMatrix has not been set";
    std::cerr << Error << std::endl;
    return -1;
  }
  FusionDriver driver;
  driver.SetDevice(Device);
  driver.SetDevices(Devices);
  driver.SetPartition(Partition);
  driver.SetKernelVariant(KernelVariant);
  driver.SetHostChunkBytes(HostChunkBytes);
  driver.SetFillOnCallingThread(FillOnCallingThread);
  driver.SetColorSink(ColorSink);
  driver.SetKeepContext(KeepContext);
  if (KeptContext) dmi_destroy(KeptContext);
  KeptContext = nullptr;
  driver.SetInitialGridIsZero(true);  // RequestData zero-filled outScalar just before (filt.cxx:133)
  bool result;
  if (Resident && !Views.empty()) {
    if (!Resident->Loaded() || Resident->Views() != Views.size()) {
      Error = "Error : the resident view set does not hold the views that were set";
      return -1;
    }
    if (!Devices.empty()) {  // several GPUs: the depths come down once and the views go the staged way
      if (!Resident->Store(Views, ThresholdBestCost)) {
        Error = Resident->LastError();
        return -1;
      }
    } else {
      driver.SetResidentSet(Resident->Handle());
    }
  }
  if (!Views.empty()) {
    int *depthMapGrid = Views[0]->GetDepthMapDimensions();  // filt.cxx:167-168: sizes from view 0
    driver.CudaInitialize(GridMatrix, gridDims, gridOrig, gridSpacing, RayPotentialThickness, RayPotentialRho,
                          RayPotentialEta, RayPotentialDelta, depthMapGrid);  // filt.cxx:171-173
    result = driver.ProcessDepthMap(Views, ThresholdBestCost, outScalar->data());  // filt.cxx:175-176
  } else {
    const std::vector<std::string> vtiList = help::ExtractAllFilePath(FilePathVTI.c_str());    // filt.cxx:158
    const std::vector<std::string> krtdList = help::ExtractAllFilePath(FilePathKRTD.c_str());  // filt.cxx:159
    if (vtiList.size() == 0 || krtdList.size() < vtiList.size()) {  // filt.cxx:161-165
      Error = "Error : There is no enough vti files, please check your vtiList.txt and krtdList.txt";
      std::cerr << Error << std::endl;
      return -1;
    }
    int depthMapGrid[2];
    {
      ReconstructionData data0(vtiList[0], krtdList[0]);  // filt.cxx:167: the first view, for the depth-map size only
      if (!data0.GetDepthMap()) {
        Error = "Error : cannot read depth map " + vtiList[0];
        std::cerr << Error << std::endl;
        return -1;
      }
      depthMapGrid[0] = data0.GetDepthMapDimensions()[0];  // filt.cxx:168
      depthMapGrid[1] = data0.GetDepthMapDimensions()[1];
    }
    driver.CudaInitialize(GridMatrix, gridDims, gridOrig, gridSpacing, RayPotentialThickness, RayPotentialRho,
                          RayPotentialEta, RayPotentialDelta, depthMapGrid);  // filt.cxx:171-173
    // the views are read chunk by chunk inside the driver, as the reference reads them inside its loop (cu:343-353)
    result = driver.ProcessDepthMap(vtiList, krtdList, ThresholdBestCost, outScalar->data());  // filt.cxx:175-176
  }
  FuseKernelMs = driver.LastFuseKernelMs();
  KeptContext = driver.TakeContext();
  if (!result) {
    Error = driver.LastError();
    return -1;
  }
  return 0;
}

// ====================================================================================================
// Coloration/MeshColoration
// ====================================================================================================
MeshColoration::MeshColoration() {}

MeshColoration::MeshColoration(const double *meshPoints, int64_t nbMeshPoint, const std::string &vti, const std::string &krtd) {
  SetInput(meshPoints, nbMeshPoint);
  ReadViews(vti, krtd, false);
}

MeshColoration::MeshColoration(const double *meshPoints, int64_t nbMeshPoint, const int64_t *triangles, int64_t nbTriangles, const std::string &vti,
                               const std::string &krtd) {
  SetInput(meshPoints, nbMeshPoint);
  SetDepthFromMesh(triangles, nbTriangles);
  ReadViews(vti, krtd, true);
}

void MeshColoration::ReadViews(const std::string &vti, const std::string &krtd, bool depthsOptional) {
  const std::vector<std::string> vtiList = help::ExtractAllFilePath(vti.c_str());
  const std::vector<std::string> krtdList = help::ExtractAllFilePath(krtd.c_str());
  if (krtdList.size() < vtiList.size()) {  // MC.cxx:59-63
    std::cerr << "Error, not enough krtd file for each vti file" << std::endl;
    return;
  }
  for (size_t id = 0; id < vtiList.size(); id++) {  // MC.cxx:67-71
    ReconstructionData *data = new ReconstructionData(vtiList[id], krtdList[id], depthsOptional);
    Owned.push_back(data);
    DataList.push_back(data);
  }
}

MeshColoration::~MeshColoration() {
  for (ReconstructionData *d : Owned) delete d;
}

void MeshColoration::SetInput(const double *meshPoints, int64_t nbMeshPoint) {
  Points.assign(meshPoints, meshPoints + 3 * nbMeshPoint);
  HasInput = true;
}

void MeshColoration::AddView(ReconstructionData *data) { DataList.push_back(data); }

bool MeshColoration::ProcessColoration() {
  Error.clear();
  const int nbDepthMap = (int)DataList.size();
  if (!HasInput || nbDepthMap == 0) {  // MC.cxx:102-106
    Error = "Error when input has been set or during reading vti/krtd file path";
    std::cerr << Error << std::endl;
    return false;
  }
  const int64_t nv = (int64_t)Points.size() / 3;
  DepthImage *first = DataList[0]->GetDepthMap();
  if (!first) {
    Error = "MeshColoration: view 0 has no image";
    return false;
  }
  const int W = first->dims[0], H = first->dims[1];  // MC.cxx:111: dimensions of view 0
  const size_t npix = (size_t)W * H;
  if (DepthTest && !(DepthTolerance >= 0.0 && std::isfinite(DepthTolerance))) {
    Error = "MeshColoration: the depth tolerance must be finite and >= 0";
    return false;
  }
  std::vector<unsigned char> colors(npix * 3 * (size_t)nbDepthMap);
  const bool uploadDepths = DepthTest && !DepthFromMesh;  // (a rendered depth replaces the "Depths" arrays: they are not read)
  std::vector<double> depths(uploadDepths ? npix * (size_t)nbDepthMap : 0);
  std::vector<double> K4(16 * (size_t)nbDepthMap), RT(16 * (size_t)nbDepthMap);
  for (int m = 0; m < nbDepthMap; ++m) {
    DepthImage *img = DataList[m]->GetDepthMap();
    if (!img || img->dims[0] != W || img->dims[1] != H || img->color.size() != npix * 3) {
      Error = "MeshColoration: view " + std::to_string(m) + " has no 'Color' array of the size of view 0";  // RD.cxx:97-101
      std::cerr << Error << std::endl;
      return false;
    }
    if (uploadDepths) {
      if (img->depths.size() != npix) {  // (ReadDepthMap already requires a Float64 "Depths" array, RD.cxx:143-146)
        Error = "MeshColoration: view " + std::to_string(m) + " has no 'Depths' array of the size of view 0 (the depth test needs it)";
        std::cerr << Error << std::endl;
        return false;
      }
      std::memcpy(&depths[(size_t)m * npix], img->depths.data(), npix * sizeof(double));
    }
    std::memcpy(&colors[(size_t)m * npix * 3], img->color.data(), npix * 3);
    std::memcpy(&K4[16 * (size_t)m], DataList[m]->Get4MatrixK(), 16 * sizeof(double));
    std::memcpy(&RT[16 * (size_t)m], DataList[m]->GetMatrixTR(), 16 * sizeof(double));
  }
  Mean.assign((size_t)nv * 3, 0);   // MC.cxx:113-133: arrays start at 0
  Median.assign((size_t)nv * 3, 0);
  std::vector<int32_t> count((size_t)nv, 0);
  int rc = DMI_OK;
  if (nv == 0) {
    // no vertex: nothing to colour, no device needed
  } else if (!DepthTest) {
    rc = dmi_color_mesh(Points.data(), nv, colors.data(), K4.data(), RT.data(), nbDepthMap, W, H, Device, Mean.data(), Median.data(),
                        count.data());
  } else {
    dmi_color_context *ctx = nullptr;
    rc = dmi_color_create(Device, &ctx);
    if (rc == DMI_OK && uploadDepths) rc = dmi_color_add_views_with_depth(ctx, colors.data(), depths.data(), K4.data(), RT.data(), nbDepthMap, W, H);
    if (rc == DMI_OK && !uploadDepths) {
      rc = dmi_color_add_views(ctx, colors.data(), K4.data(), RT.data(), nbDepthMap, W, H);
      if (rc == DMI_OK) rc = dmi_color_render_depths(ctx, Points.data(), nv, Triangles.data(), (int64_t)Triangles.size() / 3);
      if (rc == DMI_OK) rc = dmi_color_get_render_kernel_ms(ctx, &RenderKernelMs);
    }
    if (rc == DMI_OK) rc = dmi_color_set_depth_test(ctx, 1, DepthTolerance);
    if (rc == DMI_OK) rc = dmi_color_process(ctx, Points.data(), nv, Mean.data(), Median.data(), count.data());
    if (ctx) dmi_color_destroy(ctx);  // (the message stays in dmi_color_last_error)
  }
  if (rc != DMI_OK) {
    Error = dmi_color_last_error();
    return false;
  }
  Count.assign(count.begin(), count.end());
  return true;
}

}  // namespace host
}  // namespace dmi
