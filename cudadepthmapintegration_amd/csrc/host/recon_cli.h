// recon_cli.h -- the command line of the reference's `Reconstruction` tool (Reconstruction/main.cxx) on top of the host
// mirror: same flags, defaults and validation (rmain:216-343), the same derivation of spacing / dimensions from the
// grid's end point, the grid matrix from gridVecX/Y/Z (rmain:345-360), the filter run and the cell -> point pass
// (rmain:110-155), and the outputs that need no VTK algorithm: the point-data volume as a compressed MetaImage
// (rmain:157-161), the transformed volume as a .vts structured grid (rmain:189-198), the summary file (rmain:458-516).
// The iso-surface (vtkContourFilter + vtkTransformFilter, rmain:166-187) only with --extractMesh, which the reference does
// not have: dmi_extract_isosurface at --contour on the device, written to --outputMeshFilename as a .vtp of points and
// triangles; with --meshNormals as well (not in the reference either) dmi_extract_isosurface_normals, and the .vtp carries
// the point arrays Normals and reconstruction_scalar that vtkContourFilter attaches.  --meshMinComponentTriangles N and
// --meshLargestComponent (not in the reference: what a vtkPolyDataConnectivityFilter behind the contour would do) drop connected
// components of that mesh on the device before it is downloaded (dmi_filter_isosurface_components: by size, then the largest),
// and --meshRegionIds writes the point array RegionId (Int64: the kept components numbered by ascending label).
// --meshSmoothIterations N with --meshSmoothLambda / --meshSmoothMu (not in the reference: what a smoothing filter behind those
// would do) runs dmi_smooth_isosurface on the device after the component flags; with --meshNormals the Normals written are then
// the smoothed mesh's geometric ones.  --meshDecimateCellSize v (not in the reference: what a vtkQuadricClustering or a
// vtkCleanPolyData behind those would do) runs dmi_decimate_isosurface last, before the downloads; with --meshRegionIds the
// labelling then runs again on the decimated mesh; with --meshDecimateQuadric it is dmi_decimate_isosurface_placed with the quadric
// placement.  --meshMinSupportViews N with --meshSupportDepthTolerance T (not in the reference:
// the trim by observation support of every TSDF pipeline) runs dmi_filter_isosurface_support right after the extraction, before the
// component flags, which then remove the fragments it leaves; --meshSupportArray writes the final mesh's counts.
// --meshFillHoles N (not in the reference: what a vtkFillHolesFilter behind those would do) runs dmi_fill_isosurface_holes behind
// the component flags and in front of the smoothing, which then moves the patches and the former rims with the rest.
// --contourSmoothSigma S [S S] with --contourSmoothTruncate T (not in the reference: what a vtkImageGaussianSmooth in front of the
// contour would do) sets dmi_set_point_smoothing directly before the extraction, after the point data of the .mha has been
// downloaded and the active cells counted: the volume files hold what was fused, the smoothing belongs to the contour.
// --depthConsistencyMinViews N with --depthConsistencyTolerance / --depthConsistencyRelTolerance (not in the reference: the geometric
// consistency check of every depth-map fusion pipeline) reads all views into memory, filters their depths on the first device
// (dmi_filter_depth_consistency) and fuses the filtered views through ReconstructionFilter::SetViews.
// --depthSpeckleMinPixels N with --depthSpeckleTolerance / --depthSpeckleRelTolerance (not in the reference: the speckle filter of
// every stereo pipeline) takes the same in-memory path and runs FIRST (dmi_filter_depth_speckles), so that an island of wrong
// depths cannot vouch for another view's island; the consistency filter, the bounds estimate and the fusion see what it left.
// --depthFillHolesMaxPixels N with --depthFillHolesTolerance / --depthFillHolesRelTolerance (not in the reference: the gap
// interpolation of stereo pipelines) takes the same in-memory path and runs behind the speckle filter and in front of the
// consistency filter (dmi_fill_depth_holes): an island the first removed is refilled from its surroundings, and every invented
// depth still has to be confirmed by other views where the second is on.
// --depthSmoothSigma S with --depthSmoothTruncate / --depthSmoothTolerance / --depthSmoothRelTolerance / --depthSmoothIterations
// (not in the reference: the bilateral filter of TSDF pipelines) takes the same in-memory path and runs behind the hole fill and
// in front of the consistency filter (dmi_smooth_depths): invented depths are smoothed with their surroundings, and every
// smoothed depth still has to be confirmed by other views where the consistency filter is on.
// --gridAutoBounds (not in the reference, which needs --gridOrigin and --gridEnd from outside the data) takes the grid's box from the
// depth maps themselves: all views are read into memory -- and filtered first with --depthConsistencyMinViews --, the first device
// gives trimmed order statistics of the back-projected pixels along the grid's axes (dmi_estimate_scene_bounds;
// --gridAutoBoundsTrim, --gridAutoBoundsPixelStep), a margin is added (--gridAutoBoundsMargin), and spacing or dimensions follow
// as they do from a given box.  Without --extractMesh
// --outputMeshFilename is accepted and checked as the reference does, and nothing is written to it.
#pragma once

#include <cstdint>
#include <iosfwd>
#include <string>
#include <vector>

namespace dmi {
namespace host {
namespace cli {

struct Options {
  std::vector<int> gridDims;          // --gridDims (cells per axis, as the reference passes them to SetDimensions)
  std::vector<double> gridSpacing;    // --gridSpacing
  std::vector<double> gridOrigin;     // --gridOrigin
  std::vector<double> gridEnd;        // --gridEnd
  std::vector<double> gridVecX, gridVecY, gridVecZ;  // --gridVecX/Y/Z, defaults: the coordinate axes
  std::string outputGridFilename;     // --outputGridFilename (.vts)
  std::string outputMeshFilename;     // --outputMeshFilename (.vtp; checked; written with --extractMesh only)
  std::string dataFolder;             // --dataFolder
  std::string depthMapFile = "vtiList.txt";  // --depthMapFile
  std::string krtFile = "kList.txt";         // --KRTFile
  double rayThick = 2, rayRho = 0.8, rayEta = 0.03, rayDelta = 0.3;  // --rayThick / --rayRho / --rayEta / --rayDelta
  double threshBestCost = 0.14;       // --threshBestCost
  double contour = 1.0;               // --contour (recorded in the summary; no contour is extracted here)
  bool verbose = false, summary = false, forceCubicVoxel = false;
  bool extractMesh = false;           // not in the reference: write the iso-surface at --contour to --outputMeshFilename
  bool meshNormals = false;           // not in the reference: ... with its Normals and scalar arrays (needs --extractMesh)
  // not in the reference (all need --extractMesh): drop the mesh's connected components of fewer than N triangles (-1: flag not
  // given), keep only the largest one (after the former), write the point array RegionId
  long long meshMinComponentTriangles = -1;
  bool meshLargestComponent = false, meshRegionIds = false;
  // not in the reference (all need --extractMesh): Taubin smoothing of the mesh on the GPU after the component flags, N iterations
  // of a step with lambda and one with mu (0 iterations: off)
  long long meshSmoothIterations = 0;
  double meshSmoothLambda = 0.5, meshSmoothMu = -0.53;
  bool meshSmoothIterationsGiven = false, meshSmoothLambdaGiven = false, meshSmoothMuGiven = false;
  // not in the reference (needs --extractMesh): vertex clustering on the GPU after the smoothing, cells of this size (0: off)
  double meshDecimateCellSize = 0.0;
  bool meshDecimateCellSizeGiven = false;
  // not in the reference (needs --extractMesh): colour the final mesh on the GPU where it is (dmi_color_process_isosurface) from the
  // views' Color arrays and write MeanColoration, MedianColoration and NbProjectedDepthMap; with a tolerance, the visibility test
  // against the depths the fusion kept
  bool meshColoration = false;
  double meshColorationDepthTolerance = 0.0;
  bool meshColorationDepthToleranceGiven = false;
  bool meshColorationDepthFromMesh = false;  // the tolerance is measured against the final mesh's own rendered depth
  // not in the reference (all need --extractMesh and one GPU): trim the mesh by view support on the GPU right after the extraction
  // (dmi_filter_isosurface_support: -1 = flag not given), with this depth tolerance and, unless --meshSupportNoFacing, the facing
  // test; --meshSupportArray writes the counts of the final mesh as the point array NbSupportingViews
  long long meshMinSupportViews = -1;
  double meshSupportDepthTolerance = 0.0;
  bool meshSupportDepthToleranceGiven = false;
  bool meshSupportNoFacing = false, meshSupportArray = false;
  // not in the reference: which GPU(s); several = dmi_multi_* (FusionDriver::SetDevices)
  std::vector<int> devices;
  // not in the reference (needs --meshDecimateCellSize): the decimation places its vertices by quadric error
  // (dmi_decimate_isosurface_placed, DMI_DECIMATE_QUADRIC) instead of at the mean
  bool meshDecimateQuadric = false;
  // not in the reference: filter the depth maps by cross-view consistency on the GPU before they are fused
  // (dmi_filter_depth_consistency: -1 = flag not given), with an absolute and a relative depth tolerance
  long long depthConsistencyMinViews = -1;
  double depthConsistencyTolerance = 0.0, depthConsistencyRelTolerance = 0.01;
  bool depthConsistencyToleranceGiven = false, depthConsistencyRelToleranceGiven = false;
  // not in the reference: the grid's box from the depth maps (dmi_estimate_scene_bounds) instead of --gridOrigin / --gridEnd, which
  // then must be absent; ReadArguments leaves gridOrigin, gridEnd and whichever of gridDims / gridSpacing was not given empty, and Run
  // fills them in.  The share of the points cut off at either end of an axis, the margin added on either side as a share of the
  // trimmed extent, and the step between the pixels (and rows) that take part
  bool gridAutoBounds = false;
  double gridAutoBoundsTrim = 0.005, gridAutoBoundsMargin = 0.05;
  long long gridAutoBoundsPixelStep = 1;
  bool gridAutoBoundsTrimGiven = false, gridAutoBoundsMarginGiven = false, gridAutoBoundsPixelStepGiven = false;
  // not in the reference (needs --extractMesh): close the mesh's boundary loops of at most N edges on the GPU
  // (dmi_fill_isosurface_holes) behind the support trim and the component flags and in front of the smoothing (0: off)
  long long meshFillHoles = 0;
  bool meshFillHolesGiven = false;
  // not in the reference (needs --extractMesh): a Gaussian over the point data on the GPU right before the contour
  // (dmi_set_point_smoothing), sigma per grid axis in voxels (one value stands for all three; all 0: off) and its truncation
  std::vector<double> contourSmoothSigma;
  double contourSmoothTruncate = 3.0;
  bool contourSmoothTruncateGiven = false;
  // not in the reference: remove the depth maps' small segments on the GPU before anything else sees them
  // (dmi_filter_depth_speckles: -1 = flag not given), with an absolute and a relative depth tolerance between 4-neighbours
  long long depthSpeckleMinPixels = -1;
  // --depthStagedFilters (not in the reference): run the depth-map steps through the context-free calls, every step with its own
  // upload and download, instead of on a resident view set.  Needs one of the five flags that use the set.
  bool depthStagedFilters = false;
  double depthSpeckleTolerance = 0.0, depthSpeckleRelTolerance = 0.01;
  bool depthSpeckleToleranceGiven = false, depthSpeckleRelToleranceGiven = false;
  // not in the reference: fill the depth maps' small holes on the GPU behind the speckle filter (dmi_fill_depth_holes: -1 = flag
  // not given), with an absolute and a relative tolerance on the depths round a hole
  long long depthFillHolesMaxPixels = -1;
  double depthFillHolesTolerance = 0.0, depthFillHolesRelTolerance = 0.01;
  bool depthFillHolesToleranceGiven = false, depthFillHolesRelToleranceGiven = false;
  // not in the reference: smooth the depth maps on the GPU, edges preserved, behind the hole fill (dmi_smooth_depths: sigma in
  // pixels, -1 = flag not given), with the reach in sigmas, an absolute and a relative tolerance on the depth difference of a tap,
  // and the number of passes
  double depthSmoothSigma = -1.0, depthSmoothTruncate = 2.0, depthSmoothTolerance = 0.0, depthSmoothRelTolerance = 0.01;
  long long depthSmoothIterations = 1;
  bool depthSmoothSigmaGiven = false, depthSmoothTruncateGiven = false, depthSmoothToleranceGiven = false, depthSmoothRelToleranceGiven = false,
       depthSmoothIterationsGiven = false;
  // not in the reference: the fused point cloud of the depth maps that are fused (dmi_views_build_points), written to
  // this .vtp: the points at least pointCloudMinViews other views agree with, within the agreement tolerances (they default to the
  // --depthConsistency pair when that was given; otherwise one of them is required), each once unless pointCloudKeepDuplicates, with
  // a normal whose neighbours lie within the normal tolerances (they default to the agreement pair), of every k-th pixel of every
  // k-th row; with pointCloudColors the views' Color at each point's pixel
  std::string outputPointCloudFilename;
  long long pointCloudMinViews = 1, pointCloudPixelStep = 1;
  double pointCloudTolerance = 0.0, pointCloudRelTolerance = 0.0, pointCloudNormalTolerance = 0.0, pointCloudNormalRelTolerance = 0.0;
  bool pointCloudMinViewsGiven = false, pointCloudPixelStepGiven = false, pointCloudToleranceGiven = false,
       pointCloudRelToleranceGiven = false, pointCloudNormalToleranceGiven = false, pointCloudNormalRelToleranceGiven = false;
  bool pointCloudKeepDuplicates = false, pointCloudColors = false;
  // with pointCloudCellSize the cloud is thinned on the GPU behind the build, before it is written (dmi_views_thin_points,
  // DESIGN.md 8o): one point per occupied cell of this size that holds at least pointCloudMinCellPoints points, at their mean, and
  // the .vtp gets the point array NbMergedPoints.  pointCloudKeepDuplicates together with a cell size is what averages across views:
  // every view's points of one surface element fall into one cell, and the mean averages their independent depth noise
  double pointCloudCellSize = 0.0;
  long long pointCloudMinCellPoints = 1;
  bool pointCloudCellSizeGiven = false, pointCloudMinCellPointsGiven = false;
  // with pointCloudOutlierRadius the cloud loses, on the GPU behind the build and BEFORE the thinning -- strays never become cells
  // --, every point with fewer than pointCloudMinNeighbors other points within that radius (dmi_views_filter_points_radius,
  // DESIGN.md 8p); the .vtp gets the point array NbNeighbors when no thinning follows
  double pointCloudOutlierRadius = 0.0;
  long long pointCloudMinNeighbors = 1;
  bool pointCloudOutlierRadiusGiven = false, pointCloudMinNeighborsGiven = false;
  // with pointCloudPlaneFitRadius every point that has at least pointCloudPlaneFitMinNeighbors others within that radius is moved,
  // on the GPU behind the outlier filter and BEFORE the thinning, onto the plane fitted to them and takes that plane's normal
  // (dmi_views_fit_point_planes), pointCloudPlaneFitIterations times, each pass on the result of the one before;
  // KeepPositions and KeepNormals leave one of the two as it is; the .vtp gets the point array PlaneRms when no thinning follows
  double pointCloudPlaneFitRadius = 0.0;
  long long pointCloudPlaneFitMinNeighbors = 5, pointCloudPlaneFitIterations = 1;
  bool pointCloudPlaneFitKeepPositions = false, pointCloudPlaneFitKeepNormals = false;
  bool pointCloudPlaneFitRadiusGiven = false, pointCloudPlaneFitMinNeighborsGiven = false, pointCloudPlaneFitIterationsGiven = false;
};

// rmain:216-343.  false: do not run (an error or --help; the text went to `err`).
bool ReadArguments(int argc, const char *const *argv, Options *out, std::ostream &err);
// rmain:365-385: pairwise dot products within 1e-5 of zero
bool AreVectorsOrthogonal(const Options &o);
// rmain:345-360: rows 0..2 of the 4x4 are gridVecX, gridVecY, gridVecZ; row-major
void CreateGridMatrixFromInput(const Options &o, double m[16]);
std::string HelpText();

struct RunResult {
  double reconstructionSeconds = 0.0, totalSeconds = 0.0;
  // cells of the point lattice whose corners straddle --contour (dmi_iso_active_cells): what a marching cubes would visit
  unsigned long long contourActiveCells = 0;
  // --extractMesh: the size of the mesh written
  unsigned long long meshVertices = 0, meshTriangles = 0;
  // with a component flag: the mesh as extracted (as --meshMinSupportViews left it), and the connected components found in it and kept (meshVertices /
  // meshTriangles are then the filtered mesh's)
  unsigned long long meshVerticesExtracted = 0, meshTrianglesExtracted = 0, meshComponents = 0, meshComponentsKept = 0;
  double meshSmoothKernelMs = 0.0;  // --meshSmoothIterations: hipEvent time of the smoothing's kernels
  // --meshDecimateCellSize: the mesh that went into the decimation and the hipEvent time of its kernels
  unsigned long long meshVerticesBeforeDecimation = 0, meshTrianglesBeforeDecimation = 0;
  double meshDecimateKernelMs = 0.0;
  // --meshColoration: the views that coloured the mesh and the hipEvent time of the colouring's kernels
  unsigned long long meshColorationViews = 0;
  double meshColorationKernelMs = 0.0;
  double meshColorationRenderKernelMs = 0.0;  // --meshColorationDepthFromMesh: the rendering's kernels
  // --meshMinSupportViews: the mesh that went into the trim, the views that were asked and the hipEvent time of its kernels
  unsigned long long meshVerticesBeforeSupport = 0, meshTrianglesBeforeSupport = 0, meshSupportViews = 0;
  double meshSupportKernelMs = 0.0;
  // --depthConsistencyMinViews: the views filtered, their pixels with a depth after --threshBestCost, the pixels the filter kept
  // and the hipEvent time of its kernels
  unsigned long long depthConsistencyViews = 0, depthConsistencyValidPixels = 0, depthConsistencyKeptPixels = 0;
  double depthConsistencyKernelMs = 0.0;
  // --gridAutoBounds: the trimmed bounds along the grid's axes before the margin, the points they were taken from, the hipEvent time
  // of the estimate's kernels, and the box, spacing and dimensions the run then used
  double gridAutoBoundsLo[3] = {0.0, 0.0, 0.0}, gridAutoBoundsHi[3] = {0.0, 0.0, 0.0};
  unsigned long long gridAutoBoundsPoints = 0;
  double gridAutoBoundsKernelMs = 0.0;
  double gridOrigin[3] = {0.0, 0.0, 0.0}, gridEnd[3] = {0.0, 0.0, 0.0}, gridSpacing[3] = {0.0, 0.0, 0.0};
  int gridDims[3] = {0, 0, 0};
  std::string error;  // empty on success
  // --meshFillHoles: the loops filled, the boundary edges left and the hipEvent time of the fill's kernels
  unsigned long long meshHolesFilled = 0, meshBoundaryEdgesLeft = 0;
  double meshFillHolesKernelMs = 0.0;
  // --contourSmoothSigma: the radii per axis and the hipEvent time of the smoothing's kernels
  int contourSmoothRadius[3] = {0, 0, 0};
  double contourSmoothKernelMs = 0.0;
  // --depthSpeckleMinPixels: the views filtered, their pixels with a depth after --threshBestCost, the pixels the filter kept, the
  // segments it found and the ones it kept, and the hipEvent time of its kernels
  unsigned long long depthSpeckleViews = 0, depthSpeckleValidPixels = 0, depthSpeckleKeptPixels = 0, depthSpeckleSegments = 0,
                     depthSpeckleKeptSegments = 0;
  double depthSpeckleKernelMs = 0.0;
  // --depthFillHolesMaxPixels: the views filled, the holes found in them, the holes and the pixels filled, and the hipEvent time
  // of the kernels
  unsigned long long depthFillHolesViews = 0, depthFillHolesHoles = 0, depthFillHolesFilledHoles = 0, depthFillHolesFilledPixels = 0;
  double depthFillHolesKernelMs = 0.0;
  // --depthSmoothSigma: the views smoothed, their pixels with a depth, the ones whose depth changed, the taps taken per valid
  // pixel in the last iteration, and the hipEvent time of the kernels
  unsigned long long depthSmoothViews = 0, depthSmoothValidPixels = 0, depthSmoothChangedPixels = 0;
  double depthSmoothMeanTaps = 0.0, depthSmoothKernelMs = 0.0;
  // --outputPointCloudFilename: the report of the build (include/dmi.h: dmi_views_points_report) and the views it read
  unsigned long long pointCloudViews = 0, pointCloudValidPixels = 0, pointCloudCandidates = 0, pointCloudOwned = 0, pointCloudPoints = 0,
                     pointCloudWithNormal = 0;
  double pointCloudKernelMs = 0.0;
  // --pointCloudCellSize: the report of the thinning (include/dmi.h: dmi_points_thin_report); pointCloudPoints stays the build's
  unsigned long long pointCloudCells = 0, pointCloudCellsKept = 0, pointCloudMultiViewCells = 0, pointCloudLargestCell = 0,
                     pointCloudThinnedWithNormal = 0;
  double pointCloudThinKernelMs = 0.0;
  // --pointCloudOutlierRadius: the report of the filter (include/dmi.h: dmi_points_radius_report)
  unsigned long long pointCloudRadiusPointsIn = 0, pointCloudRadiusPointsKept = 0, pointCloudRadiusIsolated = 0,
                     pointCloudRadiusMaxNeighbors = 0, pointCloudRadiusNeighborSum = 0, pointCloudRadiusDistanceTests = 0;
  double pointCloudRadiusKernelMs = 0.0;
  // --pointCloudPlaneFitRadius: the report of the last pass (include/dmi.h: dmi_points_planes_report); the kernel time of all passes
  unsigned long long pointCloudPlaneFitPointsIn = 0, pointCloudPlaneFitFitted = 0, pointCloudPlaneFitUnsupported = 0,
                     pointCloudPlaneFitCrowded = 0, pointCloudPlaneFitMaxNeighbors = 0, pointCloudPlaneFitNeighborSum = 0,
                     pointCloudPlaneFitDistanceTests = 0;
  double pointCloudPlaneFitMaxShift = 0.0, pointCloudPlaneFitKernelMs = 0.0;
};
// rmain:97-213, the contour with --extractMesh only: 0 on success.  `log` receives what --verbose prints.
int Run(const Options &o, int argc, const char *const *argv, std::ostream &log, RunResult *result);

// writers (little-endian hosts)
bool WriteMetaImage(const std::string &path, const int pointDims[3], const double origin[3], const double spacing[3],
                    const double *pointScalars, std::string *error);
// a triangle mesh as VTK XML PolyData (what vtkXMLPolyDataWriter writes, rmain:184-187): appended raw data, UInt64 headers,
// Float64 Points, Polys with Int64 connectivity and offsets.  With `normals` ([nPoints][3] f32) also the point arrays of
// vtkContourFilter: <PointData Normals="Normals" Scalars="reconstruction_scalar">, Float32 x 3 and Float64 `contour` at every
// point, appended behind the offsets; without them the file is what it always was.  With `regionIds` ([nPoints] int64) the
// point array RegionId (Int64, one component) behind those; alone it is the section's Scalars.  With `mean` ([nPoints][3] u8),
// `median` ([nPoints][3] u8) and `count` ([nPoints] int32), all three or none, the arrays MeanColoration, MedianColoration and
// NbProjectedDepthMap of the Coloration tool behind every other array.  With `support` ([nPoints] int32) the point array
// NbSupportingViews (Int32, one component) behind RegionId and before those three.
bool WritePolyData(const std::string &path, const double *points, int64_t nPoints, const int64_t *triangles, int64_t nTriangles,
                   std::string *error, const float *normals = nullptr, double contour = 0.0, const int64_t *regionIds = nullptr,
                   const uint8_t *mean = nullptr, const uint8_t *median = nullptr, const int32_t *count = nullptr,
                   const int32_t *support = nullptr);
// a point cloud as VTK XML PolyData in the same conventions: Float64 Points, one Verts cell per point (Int64 connectivity 0, 1, 2
// ... and offsets 1, 2, 3 ...), the point arrays Normals (Float32 x 3, the section's Normals), ViewIndex and NbAgreeingViews (Int32)
// and, with `color` ([nPoints][3] u8), Color (UInt8 x 3) behind them; with `merged` ([nPoints] u32: the points each point of a thinned
// cloud was merged from) NbMergedPoints (UInt32) behind NbAgreeingViews.  Without `merged` the file is what it was before the array existed.
// With `neighbors` ([nPoints] u32: the points within the outlier filter's radius) NbNeighbors (UInt32) behind those and before Color;
// without it the file is what it was before that array existed.  With `planeRms` ([nPoints] f32: the RMS distance of each point's
// ball from its fitted plane, -1 without a fit) PlaneRms (Float32) behind those and before Color; without it likewise.
bool WritePointCloud(const std::string &path, const double *points, int64_t nPoints, const float *normals, const int32_t *view,
                     const int32_t *agreeing, const uint8_t *color, std::string *error, const uint32_t *merged = nullptr,
                     const uint32_t *neighbors = nullptr, const float *planeRms = nullptr);
bool WriteStructuredGrid(const std::string &path, const int pointDims[3], const double origin[3], const double spacing[3],
                         const double gridMatrix[16], const double *cellScalars, const char *arrayName, std::string *error);

}  // namespace cli
}  // namespace host
}  // namespace dmi
