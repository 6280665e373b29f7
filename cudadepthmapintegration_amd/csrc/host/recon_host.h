// recon_host.h -- host side of the fusion path, above the C ABI (include/dmi.h): a VTK-free mirror of the
// reference's operator interface for this path.  Same names, argument meaning and error behaviour as
//   Reconstruction/vtkCudaReconstructionFilter.{h,cxx}   (class, setters, RequestData, Compute)
//   Reconstruction/CudaReconstruction.cu:269-386          (CudaInitialize, ProcessDepthMap<T>)
//   Sources/ReconstructionData.{h,cxx}                    (depth map + K + RT container, best-cost filter)
//   Sources/Helper.h:60-168                               (list files, .krtd files)
// with plain C++ containers where the reference uses VTK objects (there is no VTK in the build image;
// INTEGRATION.md shows the few lines that bind these to vtkImageData / vtkMatrix4x4 / vtkDoubleArray).
//
// Nothing here computes TSDF values: all arithmetic of the path is in the HIP library behind dmi.h.
#pragma once

#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../../include/dmi.h"

namespace dmi {
namespace host {

// ---- Sources/Helper.h ------------------------------------------------------------------------------
namespace help {
// Helper.h:18-27
void SplitString(const std::string &s, char delim, std::vector<std::string> &elems);
// Helper.h:32-55 (vtksys::SystemTools::ConvertToUnixSlashes is restated: '\\' -> '/')
std::string GetFilenamePath(const std::string &filename);
// Helper.h:60-100: one entry per line, last space-separated token, relative to the list file's directory,
// empty lines skipped.  Returns an empty vector (and prints to stderr) when the file cannot be opened.
std::vector<std::string> ExtractAllFilePath(const char *globalPath);
// Helper.h:105-168: 3 lines K, 1 skipped, 3 lines R, 1 skipped, 1 line T.  K3 row-major 3x3, RT row-major 4x4
// with last row 0 0 0 1.  false (and a message on stderr) when the file cannot be opened.
bool ReadKrtdFile(const std::string &filename, double K3[9], double RT[16]);
}  // namespace help

// The part of a depth-map vtkImageData the path reads: point arrays "Depths" and "Best Cost Values"
// (both f64, RD.cxx:143-146), W x H x 1 points, vtk point order (row 0 = bottom image row, cu:141-149).
struct DepthImage {
  int dims[3] = {0, 0, 1};
  std::vector<double> depths;     // "Depths"
  std::vector<double> best_cost;  // "Best Cost Values"; may be empty
  std::vector<unsigned char> color;  // "Color", 3 components per point (RD.cxx:94-95); may be empty
};

// Sources/ReconstructionData.h:40-79, minus the colour helpers of the Coloration tool.
class ReconstructionData {
 public:
  ReconstructionData();
  // RD.cxx:55-78.  matrixPath is a .krtd file; depthPath a .vti file (see ReadDepthMap for what is read).
  ReconstructionData(const std::string &depthPath, const std::string &matrixPath);
  // Not in the reference: the same for a colouring that renders its own depth (MeshColoration::SetDepthFromMesh): a file without a
  // "Depths" array is then an image too (its "Color" array is what is wanted).
  ReconstructionData(const std::string &depthPath, const std::string &matrixPath, bool depthsOptional);

  int *GetDepthMapDimensions();  // {W, H, 1}
  DepthImage *GetDepthMap();     // RD.cxx:118-121
  const double *Get3MatrixK() const;   // row-major 3x3, RD.cxx:123-126
  const double *Get4MatrixK() const;   // row-major 4x4, RD.cxx:128-131
  const double *GetMatrixTR() const;   // row-major 4x4, RD.cxx:133-136

  void SetDepthMap(const DepthImage &data);  // RD.cxx:184-190
  void SetMatrixK(const double K3[9]);       // RD.cxx:192-212: also builds the identity-padded 4x4
  void SetMatrixTR(const double RT[16]);     // RD.cxx:214-221

  // RD.cxx:92-116: RGB of image pixel (x, y) = vtk point (x, H-1-y); false (and a message) without a "Color" array.
  bool GetColorValue(const int pixelPosition[2], double rgb[3]) const;
  // RD.cxx:169-182: RT as a point transform, K as a vector transform, divide, std::round.  No z-sign test.
  void TransformWorldToDepthMapPosition(const double *worldCoordinate, int pixelCoordinate[2]) const;

  // RD.cxx:138-167: best cost > threshold => depth = -1.  No-op without depths or when the two arrays
  // differ in length (the reference dereferences a null "Best Cost Values"; here that is a no-op too).
  void ApplyDepthThresholdFilter(double thresholdBestCost);

  // RD.cxx:223-229 uses vtkXMLImageDataReader.  Without VTK this reads the subset of .vti the path needs:
  // <ImageData WholeExtent=...> with point-data arrays "Depths" / "Best Cost Values" of type Float64 in
  // format="ascii" (other encodings need VTK: returns false).  See INTEGRATION.md.
  static bool ReadDepthMap(const std::string &path, DepthImage *out);
  // depthsOptional: a file without "Depths" is read all the same (out->depths stays empty)
  static bool ReadDepthMap(const std::string &path, DepthImage *out, bool depthsOptional);

 private:
  DepthImage DepthMap;
  bool HasDepthMap = false;
  double MatrixK[9];
  double Matrix4K[16];
  double MatrixTR[16];
};

// Where ProcessDepthMap gets view `index` from: fills depth (and best cost when the view has one; *has_cost says so) as
// W*H doubles in vtk point order, the identity-padded 4x4 K (cu:352) and [R|T] (cu:353); false + *error to abort.
// Lets a caller keep its own way of reading views -- the VTK binding reads them with the reference's own
// ReconstructionData / vtkXMLImageDataReader (vtk/vtkCudaReconstructionFilter.cxx) -- and still get the chunked,
// pinned, overlapped upload.
using ViewSource = std::function<bool(size_t index, double *depth, double *best_cost, bool *has_cost, double K4[16],
                                      double RT[16], std::string *error)>;

// Not in the reference: the views filtered by cross-view consistency on the GPU before they are fused (dmi_filter_depth_consistency,
// include/dmi.h states the definition).  Every view is thresholded first (ApplyDepthThresholdFilter), then all of them are packed --
// host memory holds every depth plane twice for the duration of the call --, filtered on `device`, and the filtered depths stored
// back with SetDepthMap: a depth stays only where at least minViews other views hold a depth within absTolerance + relTolerance * z
// of the same world point's camera z; everything else becomes -1.  The views must share one size and have depth maps.
struct DepthConsistencyReport {
  uint64_t views = 0;
  uint64_t validPixels = 0;  // after the threshold: depths > 0 and finite
  uint64_t keptPixels = 0;   // of those, the ones the filter kept
  double kernelMs = 0.0;     // hipEvent time of the pass's kernels
};
bool FilterDepthConsistency(const std::vector<ReconstructionData *> &views, double thresholdBestCost, int minViews,
                            double absTolerance, double relTolerance, int device, DepthConsistencyReport *report, std::string *error);

// Not in the reference: the views without their small depth segments, filtered on the GPU before they are fused
// (dmi_filter_depth_speckles, include/dmi.h states the definition).  It works as FilterDepthConsistency does: every view is
// thresholded first (ApplyDepthThresholdFilter), all of them are packed, filtered in place on `device`, and the filtered depths
// stored back with SetDepthMap: a depth stays only where its connected segment -- 4-neighbours whose depths differ by at most
// absTolerance + relTolerance * the smaller one -- has at least minPixels pixels; everything else becomes -1.  The cameras are not
// read.  The views must share one size and have depth maps.
struct DepthSpeckleReport {
  uint64_t views = 0;
  uint64_t validPixels = 0;     // after the threshold: depths > 0 and finite
  uint64_t keptPixels = 0;      // of those, the ones the filter kept
  uint64_t segments = 0;        // the segments of all views before the filter ...
  uint64_t keptSegments = 0;    // ... and the ones of at least minPixels pixels
  double kernelMs = 0.0;        // hipEvent time of the pass's kernels
};
bool FilterDepthSpeckles(const std::vector<ReconstructionData *> &views, double thresholdBestCost, long long minPixels,
                         double absTolerance, double relTolerance, int device, DepthSpeckleReport *report, std::string *error);

// Not in the reference: the views with their small depth holes filled on the GPU before they are fused (dmi_fill_depth_holes,
// include/dmi.h states the definition).  It works as FilterDepthSpeckles does: every view is thresholded first, all of them are
// packed, filled in place on `device`, and the filled depths stored back with SetDepthMap: a connected component of pixels
// without a depth that has at most maxPixels pixels, does not touch the image's border and whose rim depths lo..hi satisfy
// hi - lo <= absTolerance + relTolerance * lo is interpolated from the nearest valid pixels of every pixel's row and column.
// The cameras are not read.  The views must share one size and have depth maps.  Where the threshold had made the hole, the
// stored best cost of a filled pixel becomes the threshold itself, so that the later steps, which threshold again, keep the depth.
struct DepthHolesReport {
  uint64_t views = 0;
  uint64_t holes = 0;          // the holes of all views ...
  uint64_t filledHoles = 0;    // ... and the ones that were filled
  uint64_t filledPixels = 0;   // their pixels
  double kernelMs = 0.0;       // hipEvent time of the pass's kernels
};
bool FillDepthHoles(const std::vector<ReconstructionData *> &views, double thresholdBestCost, long long maxPixels, double absTolerance,
                    double relTolerance, int device, DepthHolesReport *report, std::string *error);

// Not in the reference: the views' depths smoothed on the GPU, edges preserved, before they are fused (dmi_smooth_depths,
// include/dmi.h states the definition).  It works as FillDepthHoles does: every view is thresholded first, all of them are
// packed, smoothed in place on `device`, and the smoothed depths stored back with SetDepthMap: every valid depth moves to the
// weighted mean of the valid depths within ceil(truncate * sigma) pixels that differ from it by less than
// absTolerance + relTolerance * depth, `iterations` times.  No pixel gains or loses its depth, so the best costs are left alone.
// The cameras are not read.  The views must share one size and have depth maps.
struct DepthSmoothReport {
  uint64_t views = 0;
  uint64_t validPixels = 0;    // the pixels with a depth (before and after: the step changes no validity) ...
  uint64_t changedPixels = 0;  // ... and the ones whose depth is no longer what it was
  double meanTaps = 0.0;       // taps taken per valid pixel in the last iteration, the centre included
  double kernelMs = 0.0;       // hipEvent time of the kernels
};
bool SmoothDepths(const std::vector<ReconstructionData *> &views, double thresholdBestCost, double sigma, double truncate,
                  double absTolerance, double relTolerance, int iterations, int device, DepthSmoothReport *report, std::string *error);

// Not in the reference: the bounds of the scene the views see, along the rows of `axes` (row-major 3 x 3), on the GPU
// (dmi_estimate_scene_bounds, include/dmi.h states the definition): per axis the coordinate of rank k and of rank N-1-k of the
// back-projected valid pixels, k = min((uint64_t)(trimFraction * N), (N - 1) / 2), over every pixelStep-th pixel of every
// pixelStep-th row.  Every view is thresholded first (ApplyDepthThresholdFilter) and all of them are packed, as
// FilterDepthConsistency does; the views' depths are not changed beyond that.  points == 0 leaves lo and hi NaN.
struct SceneBoundsReport {
  uint64_t views = 0;
  uint64_t points = 0;    // N: the points that were ordered
  double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0};
  double kernelMs = 0.0;  // hipEvent time of the call's kernels
};
bool EstimateSceneBounds(const std::vector<ReconstructionData *> &views, double thresholdBestCost, const double axes[9],
                         double trimFraction, int pixelStep, int device, SceneBoundsReport *report, std::string *error);

// Not in the reference: the fused point cloud of a resident view set (dmi_views_build_points, include/dmi.h states the definition;
// DESIGN.md 8n): the report of a build, and the points as DepthViewSet::DownloadPoints brings them down.
struct DepthPointsReport {
  uint64_t views = 0;
  uint64_t validPixels = 0, candidates = 0, owned = 0, points = 0, withNormal = 0;
  double kernelMs = 0.0;  // hipEvent time of the build's kernels
};
struct DepthPoints {
  std::vector<double> xyz;    // [n][3]
  std::vector<float> normal;  // [n][3], zero where a point has none
  std::vector<int32_t> view, pixel, count;  // [n]: the view, py * W + px in image coordinates, the views that agree
  std::vector<uint32_t> members;            // [n]: the points each was merged from (1 unless DepthViewSet::ThinPoints has run)
  std::vector<uint32_t> neighbors;          // [n] where DepthViewSet::FilterPointsRadius made the cloud, else empty: the points within the radius
  std::vector<float> plane_rms;             // [n] where DepthViewSet::FitPointPlanes was the cloud's last step, else empty: -1 without a fit
};
// ... and the report of a thinning of it on a voxel grid (dmi_views_thin_points)
struct DepthThinReport {
  uint64_t pointsIn = 0, cells = 0, cellsKept = 0, multiViewCells = 0, largestCell = 0, withNormal = 0;
  double kernelMs = 0.0;  // hipEvent time of the thinning's kernels
};

// ... and of a radius outlier filter of it (dmi_views_filter_points_radius)
struct DepthRadiusReport {
  uint64_t pointsIn = 0, pointsKept = 0, isolated = 0, maxNeighbors = 0, neighborSum = 0, distanceTests = 0;
  double kernelMs = 0.0;  // hipEvent time of the filter's kernels
};

// ... and of a plane fit of it (dmi_views_fit_point_planes)
struct DepthPlaneFitReport {
  uint64_t pointsIn = 0, fitted = 0, unsupported = 0, crowded = 0, maxNeighbors = 0, neighborSum = 0, distanceTests = 0;
  double maxShift = 0.0;
  double kernelMs = 0.0;  // hipEvent time of the fit's kernels
};

// Not in the reference: the views' depths resident on one GPU from the first of the steps above to the fusion (dmi_view_set,
// include/dmi.h).  Load thresholds and uploads every view once; each step runs where the depths are and fills the
// report of its staged counterpart above from the counters the device returns, with the same numbers; ReconstructionFilter::
// SetResidentViews then fuses the depths without a host copy.  The host views keep their files' depths -- only Store writes the
// set's depths back into them.  Every method returns false on error: LastError() has the text, LastCode() the dmi_status.
class DepthViewSet {
 public:
  DepthViewSet() = default;
  ~DepthViewSet() { Release(); }
  DepthViewSet(const DepthViewSet &) = delete;
  DepthViewSet &operator=(const DepthViewSet &) = delete;

  // The views must share one size and have depth maps.  The threshold goes through dmi_views_add with the best costs where every
  // view of a piece has them, as FusionDriver does; a view without costs is not thresholded (RD.cxx:156-157).  The views go up in
  // pieces of at most 256 MiB of depths.
  bool Load(const std::vector<ReconstructionData *> &views, double thresholdBestCost, int device);
  bool Loaded() const { return Set != nullptr; }
  void Release();
  bool FilterSpeckles(long long minPixels, double absTolerance, double relTolerance, DepthSpeckleReport *report);
  bool FillHoles(long long maxPixels, double absTolerance, double relTolerance, DepthHolesReport *report);
  bool Smooth(double sigma, double truncate, double absTolerance, double relTolerance, int iterations, DepthSmoothReport *report);
  bool FilterConsistency(int minViews, double absTolerance, double relTolerance, DepthConsistencyReport *report);
  bool EstimateBounds(const double axes[9], double trimFraction, int pixelStep, SceneBoundsReport *report);
  // The point cloud of the set's current depths, built on the device and kept there until the depths change; then all of it
  bool BuildPoints(double absTolerance, double relTolerance, double normalAbsTolerance, double normalRelTolerance, int minViews,
                   int pixelStep, bool dedupe, DepthPointsReport *report);
  // The built cloud replaced, on the device, by one point per occupied cell of cellSize that holds at least minPoints points, at
  // their mean (once per build); DownloadPoints then brings the thinned cloud
  bool ThinPoints(double cellSize, int minPoints, DepthThinReport *report);
  // The cloud, built or thinned, replaced on the device by its points that have at least minNeighbors other points within radius,
  // in their order (any number of times); DownloadPoints then brings the kept points with their counts
  bool FilterPointsRadius(double radius, int minNeighbors, DepthRadiusReport *report);
  // The cloud, built, thinned or filtered, with every point that has at least minNeighbors others within radius moved onto the
  // plane fitted to them (move) and carrying that plane's normal (normals), in its order and layout (any number of times: each call
  // is a pass); DownloadPoints then brings plane_rms too
  bool FitPointPlanes(double radius, int minNeighbors, bool move, bool normals, DepthPlaneFitReport *report);
  bool DownloadPoints(DepthPoints *points);
  int Width() const { return W; }
  int Height() const { return H; }
  // The set's depths into the views they were loaded from (one download), so that the staged functions above and SetViews go on
  // from here: a depth whose best cost the threshold would drop again gets the threshold as its cost, as FillDepthHoles does.
  bool Store(const std::vector<ReconstructionData *> &views, double thresholdBestCost);
  dmi_view_set *Handle() const { return Set; }
  size_t Views() const { return NViews; }
  int Device() const { return Dev; }
  const std::string &LastError() const { return Error; }
  int LastCode() const { return Code; }

 private:
  bool Fail(const char *what);
  dmi_view_set *Set = nullptr;
  size_t NViews = 0;
  uint64_t NPoints = 0;  // of the last BuildPoints
  bool Filtered = false;  // the cloud came out of FilterPointsRadius
  bool Fitted = false;    // FitPointPlanes was the cloud's last step
  int W = 0, H = 0, Dev = 0;
  std::string Error;
  int Code = 0;
};

// ---- Reconstruction/CudaReconstruction.cu host driver -------------------------------------------------
// The reference keeps the grid description in global __constant__ state between the two calls (cu:55-64);
// here it lives in an object.  One FusionDriver = one CudaInitialize + ProcessDepthMap pair.
class FusionDriver {
 public:
  FusionDriver();
  ~FusionDriver();
  FusionDriver(const FusionDriver &) = delete;
  FusionDriver &operator=(const FusionDriver &) = delete;

  // cu:269-298.  h_gridDims are vtkImageData POINT dimensions (cells = dims - 1, cu:330-331);
  // i_gridMatrix row-major 4x4 (vtkMatrix4x4 order, cu:220-230).
  void CudaInitialize(const double i_gridMatrix[16], const int h_gridDims[3], const double h_gridOrig[3],
                      const double h_gridSpacing[3], double h_rayPThick, double h_rayPRho, double h_rayPEta,
                      double h_rayPDelta, const int h_depthMapDim[2]);

  // cu:302-386 with in-memory views: threshold (cu:348), upload as pinned SoA chunks (replaces cu:351-360), one fused
  // launch per chunk (replaces the per-map launches cu:363) overlapped with the filling of the next chunk, download
  // into io_scalar (cu:368-371).
  // io_scalar holds NumberOfCells doubles and is accumulated onto (cu:323-327).  Returns false on error
  // (message in LastError()); never calls exit() (the reference's gpuAssert does, cu:68-76).
  bool ProcessDepthMap(const std::vector<ReconstructionData *> &views, double thresholdBestCost, double *io_scalar);
  // same, from list files as the reference (vtiList[i], krtdList[i] -> ReconstructionData, cu:347): the files are read
  // one view at a time by a second thread while the previous chunk uploads and fuses, so host memory holds two chunks
  // (<= 2 x 256 MiB of depth + as much of best cost), never the whole set of views
  bool ProcessDepthMap(const std::vector<std::string> &vtiList, const std::vector<std::string> &krtdList,
                       double thresholdBestCost, double *io_scalar);

  // the general form behind both: n_views views, each produced by `source` when its chunk is being filled
  bool ProcessDepthMap(size_t n_views, const ViewSource &source, double thresholdBestCost, double *io_scalar);
  // true: views are produced on the thread that called ProcessDepthMap (for sources that must not run on another
  // thread; the fusion of a chunk still overlaps the filling of the next, only its host-to-device copy does not).
  // Default false: a second thread fills chunk i+1 while chunk i is copied and fused.
  void SetFillOnCallingThread(bool yes) { FillOnCallingThread = yes; }

  void SetDevice(int device) { Device = device; }
  // Several GPUs of the node for ONE fusion (none in the reference; north star: depth maps shard across the GPUs, one
  // RCCL all-reduce of the float TSDF grid).  Empty = single GPU (SetDevice).  Non-empty: ProcessDepthMap runs through
  // dmi_multi_* -- DMI_PARTITION_VIEWS (default): f32 grids summed over xGMI, |result - single GPU| within
  // 2*G*2^-24*sum|partials| per voxel; DMI_PARTITION_Z_SLABS: every GPU fuses all views into its own cell layers, f64,
  // no exchange, bit-identical to one GPU.  The grid must start from zeros (as RequestData provides, filt.cxx:133).
  void SetDevices(const std::vector<int> &devices) { Devices = devices; }
  void SetPartition(int partition) { Partition = partition; }
  void SetKernelVariant(int v) { KernelVariant = v; }
  // pinned host memory of ONE staging chunk (depth + best cost of as many views as fit, at least one); two chunks exist.
  // Default 256 MiB.
  void SetHostChunkBytes(size_t bytes) { HostChunkBytes = bytes < 1 ? 1 : bytes; }
  // the next ProcessDepthMap's io_scalar is known to hold +0.0 everywhere: skips the scan and the upload (cu:323-327)
  void SetInitialGridIsZero(bool yes) { InitialGridIsZero = yes; }
  // Not in the reference.  With a sink, every chunk's "Color" planes go to it with the chunk's K and RT (dmi_color_add_views)
  // right after the chunk's depths went to the fusion context: every file is read once.  A view without a UInt8 x 3 Color array
  // of the views' size fails the call with the file's name.  Single GPU only.
  void SetColorSink(dmi_color_context *sink) { ColorSink = sink; }
  // Not in the reference.  With a resident set, ProcessDepthMap(views, ...) takes the depths of views [first, first + count) of
  // every chunk from the set (dmi_add_views_from_set) instead of copying them from the host views -- the same chunks, so every voxel
  // accumulates its views in the same order -- and asks the views for their sizes, matrices and Color planes only.  The set must
  // hold as many views as the call is given.  Single GPU only.
  void SetResidentSet(dmi_view_set *set) { ResidentSet = set; }
  // Keep the (single-GPU) fusion context of a successful ProcessDepthMap instead of destroying it: its views stay resident and
  // its grid is the fused one.  TakeContext hands it over (the caller destroys it); the destructor destroys one nobody took.
  void SetKeepContext(bool keep) { KeepContext = keep; }
  dmi_context *TakeContext() {
    dmi_context *c = KeptContext;
    KeptContext = nullptr;
    return c;
  }
  const std::string &LastError() const { return Error; }
  double LastFuseKernelMs() const { return FuseKernelMs; }
  int64_t NumberOfCells() const;

 private:
  dmi_grid_desc Grid;
  dmi_ray_potential Ray;
  int DepthDims[2];
  bool Initialized = false;
  bool InitialGridIsZero = false;
  bool FillOnCallingThread = false;

  int Device = 0;
  std::vector<int> Devices;
  // several GPUs: z-slabs by default -- the reference's f64 grid, bit-identical to one GPU, no exchange; the north star's
  // depth-map shards + f32 all-reduce (DMI_PARTITION_VIEWS: tolerance include/dmi.h states) are an explicit choice
  int Partition = DMI_PARTITION_Z_SLABS;
  int KernelVariant = 0;
  size_t HostChunkBytes = size_t(256) << 20;
  double FuseKernelMs = 0.0;
  std::string Error;
  dmi_color_context *ColorSink = nullptr;
  dmi_view_set *ResidentSet = nullptr;
  bool KeepContext = false;
  dmi_context *KeptContext = nullptr;
  unsigned char *FillColor = nullptr;  // where the view being filled puts its colour plane (null: not wanted)
};

// ---- Reconstruction/vtkCudaReconstructionFilter ------------------------------------------------------
// vtkImageAlgorithm subclass in the reference (filt.h:48-120).  The input vtkImageData contributes only
// its geometry (filt.cxx:121-126), the output is its shallow copy plus the CELL array
// "reconstruction_scalar" (filt.cxx:129-135): here SetInputData takes the geometry and GetOutput...
// returns the array.
class ReconstructionFilter {
 public:
  ReconstructionFilter();   // filt.cxx:74-86: everything 0 / unset
  ~ReconstructionFilter();

  void SetRayPotentialThickness(double v) { RayPotentialThickness = v; }  // filt.h:57
  void SetRayPotentialRho(double v) { RayPotentialRho = v; }              // filt.h:60
  void SetRayPotentialEta(double v) { RayPotentialEta = v; }              // filt.h:63
  void SetRayPotentialDelta(double v) { RayPotentialDelta = v; }          // filt.h:66
  void SetThresholdBestCost(double v) { ThresholdBestCost = v; }          // filt.h:69
  void SetFilePathKRTD(const char *path);                                 // filt.h:73 (vtkSetStringMacro: copies)
  void SetFilePathVTI(const char *path);                                  // filt.h:77
  double GetExecutionTime() const { return ExecutionTime; }               // filt.h:81
  void SetGridMatrix(const double gridMatrix[16]);                        // filt.h:86, row-major vtkMatrix4x4

  // the input port: vtkImageData dimensions (points), origin, spacing (filt.cxx:121-126)
  void SetInputData(const int dims[3], const double origin[3], const double spacing[3]);
  // In-memory alternative to the two list files: when views are set, Compute uses them instead of reading
  // FilePathVTI / FilePathKRTD (the paths must still be set, as RequestData checks them first, filt.cxx:114).
  void SetViews(const std::vector<ReconstructionData *> &views) { Views = views; }
  // Not in the reference.  With SetViews: the views' depths are the ones resident in `set` (loaded from these views, in this order)
  // and reach the fusion by dmi_add_views_from_set, in the chunks SetViews alone would upload them in, so the grid is the same; the
  // views still give their matrices, and their Color planes to the colour sink.  With several devices (SetDevices) the set's depths
  // are stored into the views once (DepthViewSet::Store) and the SetViews path is taken.  Null: back to SetViews alone.
  void SetResidentViews(DepthViewSet *set) { Resident = set; }

  // RequestData (filt.cxx:96-151): 1 on success, 0 when a path is unset (filt.cxx:114-118) or rho and
  // thickness are both 0 (filt.cxx:138-142).  Unlike the reference, a failure inside Compute also
  // returns 0 (the reference ignores Compute's result, filt.cxx:144).
  int Update();

  static const char *OutputArrayName() { return "reconstruction_scalar"; }  // filt.cxx:130
  int64_t GetNumberOfCells() const;
  const std::vector<double> &GetOutputScalars() const { return OutScalar; }  // cell data, x fastest
  const std::string &LastError() const { return Error; }

  void SetDevice(int d) { Device = d; }
  // new, optional, default = the reference's single GPU: see FusionDriver::SetDevices / SetPartition
  void SetDevices(const std::vector<int> &devices) { Devices = devices; }
  void SetPartition(int partition) { Partition = partition; }
  void SetHostChunkBytes(size_t bytes) { HostChunkBytes = bytes < 1 ? 1 : bytes; }  // FusionDriver::SetHostChunkBytes
  void SetFillOnCallingThread(bool yes) { FillOnCallingThread = yes; }               // FusionDriver::SetFillOnCallingThread
  void SetKernelVariant(int v) { KernelVariant = v; }
  double GetFuseKernelMs() const { return FuseKernelMs; }
  // Not in the reference (the CLI's --meshColoration): see FusionDriver::SetColorSink / SetKeepContext; TakeContext hands over
  // the fusion context of the last Update (views resident, grid fused), or null; the caller destroys it
  void SetColorSink(dmi_color_context *sink) { ColorSink = sink; }
  void SetKeepContext(bool keep) { KeepContext = keep; }
  dmi_context *TakeContext() {
    dmi_context *c = KeptContext;
    KeptContext = nullptr;
    return c;
  }

 protected:
  int RequestData();
  // filt.cxx:155-179.  0 on success, -1 on error.
  int Compute(int gridDims[3], double gridOrig[3], double gridSpacing[3], std::vector<double> *outScalar);

 private:
  double GridMatrix[16];
  bool HasGridMatrix = false;
  double RayPotentialRho, RayPotentialThickness, RayPotentialEta, RayPotentialDelta, ThresholdBestCost;
  double ExecutionTime;
  std::string FilePathKRTD, FilePathVTI;
  bool HasKRTD = false, HasVTI = false;
  int InDims[3];
  double InOrigin[3], InSpacing[3];
  bool HasInput = false;
  std::vector<ReconstructionData *> Views;
  DepthViewSet *Resident = nullptr;
  std::vector<double> OutScalar;
  std::string Error;
  int Device = 0, KernelVariant = 0;
  dmi_color_context *ColorSink = nullptr;
  bool KeepContext = false;
  dmi_context *KeptContext = nullptr;
  std::vector<int> Devices;
  // several GPUs: z-slabs by default -- the reference's f64 grid, bit-identical to one GPU, no exchange; the north star's
  // depth-map shards + f32 all-reduce (DMI_PARTITION_VIEWS: tolerance include/dmi.h states) are an explicit choice
  int Partition = DMI_PARTITION_Z_SLABS;
  size_t HostChunkBytes = size_t(256) << 20;
  bool FillOnCallingThread = false;
  double FuseKernelMs = 0.0;
};

// ---- Coloration/MeshColoration ---------------------------------------------------------------------------
// MC.h:42-61.  The mesh contributes only its points (MC.cxx:109-110); the output is the three point-data arrays
// the reference adds to the mesh (MC.cxx:194-196).  ProcessColoration runs on the GPU (dmi_color_mesh; with the depth test
// the resident-view context: dmi_color_add_views_with_depth, dmi_color_set_depth_test).
class MeshColoration {
 public:
  MeshColoration();
  // MC.cxx:52-72: reads every view named by the two list files (needs "Color" arrays in the .vti files)
  MeshColoration(const double *meshPoints, int64_t nbMeshPoint, const std::string &vtiList, const std::string &krtdList);
  // Not in the reference: the same, with these triangles ([n][3] ids into the points) as SetDepthFromMesh: the views' .vti files
  // then need no "Depths" array at all (the files are read here, so the reader has to know now)
  MeshColoration(const double *meshPoints, int64_t nbMeshPoint, const int64_t *triangles, int64_t nbTriangles, const std::string &vtiList,
                 const std::string &krtdList);
  ~MeshColoration();
  void SetInput(const double *meshPoints, int64_t nbMeshPoint);  // MC.cxx:85-91 (vtkPolyData points, [n][3])
  void AddView(ReconstructionData *data);                        // in-memory alternative to the list files; not owned
  bool ProcessColoration();                                      // MC.cxx:98-199
  const std::vector<unsigned char> &GetMeanColoration() const { return Mean; }      // "MeanColoration", u8 x 3
  const std::vector<unsigned char> &GetMedianColoration() const { return Median; }  // "MedianColoration", u8 x 3
  const std::vector<int> &GetNbProjectedDepthMap() const { return Count; }          // "NbProjectedDepthMap"
  const std::string &LastError() const { return Error; }
  void SetDevice(int d) { Device = d; }
  // Not in the reference: the visibility test of dmi_color_set_depth_test (a pair counts only if the view's "Depths" value at
  // the pixel is within `tolerance` of the vertex's camera z, both > 0); needs every view's "Depths" array.  A NaN, infinite or
  // negative tolerance fails ProcessColoration.  ClearDepthTest: back to the reference's colouring.
  void SetDepthTolerance(double tolerance) {
    DepthTest = true;
    DepthTolerance = tolerance;
  }
  void ClearDepthTest() { DepthTest = false; }
  // Not in the reference: with the depth test on, the depth it compares against is THIS mesh's own -- the input points and these
  // triangles ([n][3] ids into them) rendered into every view (dmi_color_render_depths) -- and the views' "Depths" arrays are not
  // read.  ClearDepthFromMesh: back to the "Depths" arrays.
  void SetDepthFromMesh(const int64_t *triangles, int64_t nbTriangles) {
    DepthFromMesh = true;
    Triangles.assign(triangles, triangles + 3 * nbTriangles);
  }
  void ClearDepthFromMesh() { DepthFromMesh = false; }
  double GetRenderKernelMs() const { return RenderKernelMs; }  // of the last ProcessColoration that rendered

 private:
  bool DepthTest = false;
  double DepthTolerance = 0.0;
  bool DepthFromMesh = false;
  std::vector<int64_t> Triangles;
  double RenderKernelMs = 0.0;
  std::vector<double> Points;
  bool HasInput = false;
  std::vector<ReconstructionData *> DataList;
  std::vector<ReconstructionData *> Owned;
  std::vector<unsigned char> Mean, Median;
  std::vector<int> Count;
  std::string Error;
  int Device = 0;
  void ReadViews(const std::string &vtiList, const std::string &krtdList, bool depthsOptional);
};

}  // namespace host
}  // namespace dmi
