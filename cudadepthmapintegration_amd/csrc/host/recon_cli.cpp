// recon_cli.cpp -- see recon_cli.h.  Reference: Reconstruction/main.cxx ("rmain").
#include "recon_cli.h"

#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <map>
#include <memory>
#include <ostream>
#include <sstream>

#include "../depth_smooth_rules.h"
#include "../point_smooth_rules.h"
#include "recon_host.h"

namespace dmi {
namespace host {
namespace cli {

namespace {

enum class Kind { kMulti, kValue, kFlag };

struct Spec {
  Kind kind;
  const char *help;
  std::function<bool(const std::vector<std::string> &)> store;  // false: a value did not parse
};

template <typename T>
bool parse_number(const std::string &text, T *out) {
  std::istringstream in(text);
  in >> *out;
  return !in.fail() && in.eof();
}

template <typename T>
std::function<bool(const std::vector<std::string> &)> into_vector(std::vector<T> *dst) {
  return [dst](const std::vector<std::string> &values) {
    for (const std::string &v : values) {
      T x;
      if (!parse_number(v, &x)) return false;
      dst->push_back(x);
    }
    return true;
  };
}

std::function<bool(const std::vector<std::string> &)> into_double(double *dst) {
  return [dst](const std::vector<std::string> &values) { return values.size() == 1 && parse_number(values[0], dst); };
}

std::function<bool(const std::vector<std::string> &)> into_string(std::string *dst) {
  return [dst](const std::vector<std::string> &values) {
    if (values.size() != 1) return false;
    *dst = values[0];
    return true;
  };
}

// a non-negative integer: digits only ("-3", "+3", "3.5" and "" are errors)
std::function<bool(const std::vector<std::string> &)> into_count(long long *dst) {
  return [dst](const std::vector<std::string> &values) {
    if (values.size() != 1 || values[0].empty() || values[0].size() > 18) return false;
    long long n = 0;
    for (const char c : values[0]) {
      if (c < '0' || c > '9') return false;
      n = 10 * n + (c - '0');
    }
    *dst = n;
    return true;
  };
}

// a number the predicate accepts (a NaN, an infinity or a value out of range is an error like a word); *given notes the flag
std::function<bool(const std::vector<std::string> &)> into_checked_double(double *dst, bool *given, bool (*ok)(double)) {
  return [dst, given, ok](const std::vector<std::string> &values) {
    double x = 0.0;
    if (values.size() != 1 || !parse_number(values[0], &x) || !std::isfinite(x) || !ok(x)) return false;
    *dst = x;
    *given = true;
    return true;
  };
}

std::function<bool(const std::vector<std::string> &)> into_flag(bool *dst) {
  return [dst](const std::vector<std::string> &) {
    *dst = true;
    return true;
  };
}

// the table of rmain:224-247, in the reference's order; `help` is what --help prints for the flag
std::vector<std::pair<std::string, Spec>> flag_table(Options *o, bool *help) {
  return {
      {"--gridDims", {Kind::kMulti, "grid dimensions, one or three integers", into_vector(&o->gridDims)}},
      {"--gridSpacing", {Kind::kMulti, "voxel size per axis (not together with --gridDims)", into_vector(&o->gridSpacing)}},
      {"--gridOrigin", {Kind::kMulti, "first corner of the grid", into_vector(&o->gridOrigin)}},
      {"--gridVecX", {Kind::kMulti, "direction of the grid's x axis (default 1 0 0)", into_vector(&o->gridVecX)}},
      {"--gridVecY", {Kind::kMulti, "direction of the grid's y axis (default 0 1 0)", into_vector(&o->gridVecY)}},
      {"--gridVecZ", {Kind::kMulti, "direction of the grid's z axis (default 0 0 1)", into_vector(&o->gridVecZ)}},
      {"--outputGridFilename", {Kind::kValue, "where the fused volume goes (.vts, required)", into_string(&o->outputGridFilename)}},
      {"--dataFolder", {Kind::kValue, "folder holding the two list files (required)", into_string(&o->dataFolder)}},
      {"--depthMapFile", {Kind::kValue, "list of depth-map .vti files inside the data folder (default vtiList.txt)", into_string(&o->depthMapFile)}},
      {"--KRTFile", {Kind::kValue, "list of .krtd files inside the data folder (default kList.txt)", into_string(&o->krtFile)}},
      {"--rayThick", {Kind::kValue, "ray potential: half width of the ramp around a surface (default 2)", into_double(&o->rayThick)}},
      {"--rayRho", {Kind::kValue, "ray potential: plateau value (default 0.8)", into_double(&o->rayRho)}},
      {"--rayEta", {Kind::kValue, "ray potential: free-space value as a share of rho, 0..1 (default 0.03)", into_double(&o->rayEta)}},
      {"--rayDelta", {Kind::kValue, "ray potential: reach around a surface, not below --rayThick (default 0.3)", into_double(&o->rayDelta)}},
      {"--threshBestCost", {Kind::kValue, "depths whose best cost exceeds this are dropped (default 0.14)", into_double(&o->threshBestCost)}},
      {"--gridEnd", {Kind::kMulti, "last corner of the grid (required)", into_vector(&o->gridEnd)}},
      {"--contour", {Kind::kValue, "iso value (default 1.0; a surface is extracted only with --extractMesh)", into_double(&o->contour)}},
      {"--outputMeshFilename", {Kind::kValue, "mesh file name (.vtp, required by the reference's checks; written only with --extractMesh)", into_string(&o->outputMeshFilename)}},
      {"--verbose", {Kind::kFlag, "print progress and the parameters", into_flag(&o->verbose)}},
      {"--summary", {Kind::kFlag, "write summary.txt into the data folder", into_flag(&o->summary)}},
      {"--forceCubicVoxel", {Kind::kFlag, "use the smallest of the three spacings on every axis", into_flag(&o->forceCubicVoxel)}},
      {"--device", {Kind::kMulti, "HIP device ordinal(s); several = one fusion over several GPUs (not in the reference)", into_vector(&o->devices)}},
      {"--extractMesh", {Kind::kFlag, "extract the iso-surface at --contour on the GPU and write it to --outputMeshFilename: points and "
                                      "triangles only, without the Normals and scalar arrays VTK's contour filter adds unless --meshNormals "
                                      "is given (not in the reference)",
                         into_flag(&o->extractMesh)}},
      {"--meshNormals", {Kind::kFlag, "with --extractMesh: compute the mesh's normals on the GPU and write them and the scalar array "
                                      "reconstruction_scalar (the contour value) as point data, as VTK's contour filter does (not in the "
                                      "reference)",
                         into_flag(&o->meshNormals)}},
      {"--meshMinComponentTriangles", {Kind::kValue, "with --extractMesh: drop every connected component of the mesh that has fewer "
                                                     "than this many triangles, on the GPU (a non-negative integer; 0 drops "
                                                     "nothing; not in the reference)",
                                       into_count(&o->meshMinComponentTriangles)}},
      {"--meshLargestComponent", {Kind::kFlag, "with --extractMesh: keep only the connected component with the most triangles, on the GPU "
                                               "(after --meshMinComponentTriangles when both are given; not in the reference)",
                                  into_flag(&o->meshLargestComponent)}},
      {"--meshRegionIds", {Kind::kFlag, "with --extractMesh: write the point array RegionId, the number of each vertex's connected component "
                                        "(components numbered by their smallest vertex id; not in the reference)",
                           into_flag(&o->meshRegionIds)}},
      {"--meshSmoothIterations", {Kind::kValue, "with --extractMesh: smooth the mesh on the GPU, after the component flags, with this "
                                                "many Taubin iterations (a step with --meshSmoothLambda, then one with --meshSmoothMu; "
                                                "vertices on the mesh's boundary stay; an integer in 0..1000, default 0 = off); with "
                                                "--meshNormals the Normals written are then the smoothed mesh's geometric normals, not the "
                                                "field's gradient (not in the reference)",
                                  [o](const std::vector<std::string> &values) {
                                    long long n = 0;
                                    if (!into_count(&n)(values) || n > 1000) return false;
                                    o->meshSmoothIterations = n;
                                    o->meshSmoothIterationsGiven = true;
                                    return true;
                                  }}},
      {"--meshSmoothLambda", {Kind::kValue, "with --extractMesh: the smoothing's positive factor, in (0, 1] (default 0.5; not in the reference)",
                              into_checked_double(&o->meshSmoothLambda, &o->meshSmoothLambdaGiven, [](double x) { return x > 0.0 && x <= 1.0; })}},
      {"--meshSmoothMu", {Kind::kValue, "with --extractMesh: the smoothing's negative factor, <= 0 (default -0.53; 0 = plain Laplacian "
                                        "smoothing; not in the reference)",
                          into_checked_double(&o->meshSmoothMu, &o->meshSmoothMuGiven, [](double x) { return x <= 0.0; })}},
      {"--meshDecimateCellSize", {Kind::kValue, "with --extractMesh: decimate the mesh on the GPU by vertex clustering, after the component "
                                                "flags and the smoothing: the vertices of one cubic cell of this size (world units, "
                                                "finite and > 0) become their mean, collapsed and duplicate triangles go; a tiny value "
                                                "only welds coincident vertices; with --meshNormals the Normals written are then the "
                                                "decimated mesh's geometric normals, with --meshRegionIds the components are labelled again "
                                                "on the decimated mesh (default 0 = off; not in the reference)",
                                  into_checked_double(&o->meshDecimateCellSize, &o->meshDecimateCellSizeGiven, [](double x) { return x > 0.0; })}},
      {"--meshDecimateQuadric", {Kind::kFlag, "with --meshDecimateCellSize: place every cell's vertex by the quadric error of the cell's "
                                              "triangles, as vtkQuadricClustering does, instead of at the mean of its vertices: creases "
                                              "and corners inside a cell stay sharp and convex shapes do not shrink; the triangles are the "
                                              "same either way (not in the reference)",
                                 into_flag(&o->meshDecimateQuadric)}},
      {"--meshFillHoles", {Kind::kValue, "with --extractMesh: close the mesh's small holes on the GPU, after --meshMinSupportViews and the "
                                         "component flags and before the smoothing: every boundary loop of at most this many edges (an "
                                         "integer in 3..1048576) gets a triangle, or a vertex at the mean of its rim and a fan round "
                                         "it, as vtkFillHolesFilter closes holes; loops through a non-manifold vertex stay open; with "
                                         "--meshNormals the new vertices get geometric normals, with --meshRegionIds the components "
                                         "are labelled again on the filled mesh (default 0 = off; not in the reference)",
                           [o](const std::vector<std::string> &values) {
                             long long n = 0;
                             if (!into_count(&n)(values) || n < 3 || n > 1048576) return false;
                             o->meshFillHoles = n;
                             o->meshFillHolesGiven = true;
                             return true;
                           }}},
      {"--meshColoration", {Kind::kFlag, "with --extractMesh, on one GPU: colour the mesh on the GPU where it is, last of all, from the "
                                         "Color arrays of the depth-map files (UInt8 x 3, read in the same pass as the depths), and "
                                         "write the point arrays MeanColoration, MedianColoration and NbProjectedDepthMap as the "
                                         "Coloration tool does (not in the reference)",
                            into_flag(&o->meshColoration)}},
      {"--meshColorationDepthTolerance", {Kind::kValue, "with --meshColoration: a view colours a vertex only if the vertex lies in "
                                                        "front of the camera and within this distance (finite, >= 0) of the depth "
                                                        "the fusion kept at its pixel, i.e. after --threshBestCost; without the "
                                                        "flag every view whose image holds the vertex counts, as in the reference "
                                                        "(not in the reference)",
                                          into_checked_double(&o->meshColorationDepthTolerance, &o->meshColorationDepthToleranceGiven,
                                                              [](double x) { return x >= 0.0; })}},
      {"--meshColorationDepthFromMesh", {Kind::kFlag, "with --meshColoration and --meshColorationDepthTolerance: the depth that "
                                                     "tolerance is measured against is the final mesh's own -- rendered into every "
                                                     "view on the GPU after the last mesh operation -- instead of the depth the "
                                                     "fusion kept: no holes, and still the surface after smoothing or decimation. "
                                                     "A triangle that crosses a camera's plane does not occlude (not in the reference)",
                                         into_flag(&o->meshColorationDepthFromMesh)}},
      {"--meshMinSupportViews", {Kind::kValue, "with --extractMesh, on one GPU: trim the mesh by view support on the GPU, right after "
                                               "the extraction and before the component flags (which then remove the fragments it "
                                               "leaves): a view supports a vertex that lies in front of its camera, inside its image, "
                                               "within --meshSupportDepthTolerance of the depth the fusion kept at its pixel (after "
                                               "--threshBestCost) and whose normal points towards the camera; only the triangles whose "
                                               "three vertices have at least this many supporting views stay, with the vertices they "
                                               "name (a non-negative integer; 0 drops nothing; needs --meshSupportDepthTolerance; not "
                                               "in the reference)",
                                 into_count(&o->meshMinSupportViews)}},
      {"--meshSupportDepthTolerance", {Kind::kValue, "the depth tolerance of --meshMinSupportViews and --meshSupportArray (world units, "
                                                     "finite, >= 0; required with either; not in the reference)",
                                       into_checked_double(&o->meshSupportDepthTolerance, &o->meshSupportDepthToleranceGiven,
                                                           [](double x) { return x >= 0.0; })}},
      {"--meshSupportNoFacing", {Kind::kFlag, "with --meshMinSupportViews or --meshSupportArray: a view supports a vertex whichever way "
                                              "its normal points (without the flag the normals are computed for the test even when "
                                              "--meshNormals is not given, and then not written; not in the reference)",
                                 into_flag(&o->meshSupportNoFacing)}},
      {"--meshSupportArray", {Kind::kFlag, "with --extractMesh, on one GPU: write the point array NbSupportingViews (Int32), the number of "
                                           "supporting views of every vertex of the mesh as written, counted after every other mesh "
                                           "operation (needs --meshSupportDepthTolerance, works without --meshMinSupportViews; not in "
                                           "the reference)",
                              into_flag(&o->meshSupportArray)}},
      {"--depthConsistencyMinViews", {Kind::kValue, "filter the depth maps by cross-view consistency on the GPU before they are fused: a "
                                                    "depth stays only if at least this many other views, looking at the same world "
                                                    "point, hold a depth that agrees with the point's distance from their camera; every "
                                                    "other depth is dropped like one that fails --threshBestCost (a non-negative "
                                                    "integer; 0 drops nothing).  All views are then read into host memory at once (at "
                                                    "256 views of 1280 x 720 with costs and colours about 4.5 GB) and filtered on the "
                                                    "first --device; the support trim and the fused test of the coloration see "
                                                    "the filtered depths (not in the reference)",
                                      into_count(&o->depthConsistencyMinViews)}},
      {"--depthConsistencyTolerance", {Kind::kValue, "with --depthConsistencyMinViews: two depths agree within this distance (world "
                                                     "units, finite, >= 0, default 0) plus the relative tolerance (not in the reference)",
                                       into_checked_double(&o->depthConsistencyTolerance, &o->depthConsistencyToleranceGiven,
                                                           [](double x) { return x >= 0.0; })}},
      {"--depthConsistencyRelTolerance", {Kind::kValue, "with --depthConsistencyMinViews: ... plus this share of the distance from the "
                                                        "other view's camera (finite, >= 0, default 0.01; not in the reference)",
                                          into_checked_double(&o->depthConsistencyRelTolerance, &o->depthConsistencyRelToleranceGiven,
                                                              [](double x) { return x >= 0.0; })}},
      {"--depthSpeckleMinPixels", {Kind::kValue, "remove the small segments of the depth maps on the GPU before they are fused, and "
                                                 "before --depthConsistencyMinViews and --gridAutoBounds see them: neighbouring pixels "
                                                 "(left, right, above, below) whose depths agree form a segment, and the depths of a "
                                                 "segment of fewer than this many pixels are dropped like ones that fail "
                                                 "--threshBestCost (a non-negative integer; 0 drops nothing).  All views are then read "
                                                 "into host memory at once, as with --depthConsistencyMinViews, and filtered on the "
                                                 "first --device (not in the reference)",
                                   into_count(&o->depthSpeckleMinPixels)}},
      {"--depthSpeckleTolerance", {Kind::kValue, "with --depthSpeckleMinPixels: two neighbouring depths agree within this distance "
                                                 "(world units, finite, >= 0, default 0) plus the relative tolerance (not in the reference)",
                                   into_checked_double(&o->depthSpeckleTolerance, &o->depthSpeckleToleranceGiven,
                                                       [](double x) { return x >= 0.0; })}},
      {"--depthSpeckleRelTolerance", {Kind::kValue, "with --depthSpeckleMinPixels: ... plus this share of the smaller of the two depths "
                                                    "(finite, >= 0, default 0.01).  The value must fit the image resolution: on a "
                                                    "slanted surface the depth steps from pixel to pixel by an amount that grows as "
                                                    "the image gets coarser, and a tolerance below that step cuts the surface into "
                                                    "rows that are then dropped as small segments (0.01 suits 640 x 480 and above; "
                                                    "images of 80 x 60 need about 0.05; not in the reference)",
                                      into_checked_double(&o->depthSpeckleRelTolerance, &o->depthSpeckleRelToleranceGiven,
                                                          [](double x) { return x >= 0.0; })}},
      {"--depthFillHolesMaxPixels", {Kind::kValue, "fill the small holes of the depth maps on the GPU before they are fused, behind "
                                                   "--depthSpeckleMinPixels and before --depthConsistencyMinViews and --gridAutoBounds "
                                                   "see them: neighbouring pixels (left, right, above, below) without a depth form a "
                                                   "hole, and a hole of at most this many pixels that does not touch the image's border "
                                                   "and whose surrounding depths agree gets depths interpolated from the nearest pixels "
                                                   "of every pixel's row and column (a non-negative integer; 0 fills nothing).  All "
                                                   "views are then read into host memory at once, as with --depthSpeckleMinPixels, and "
                                                   "filled on the first --device (not in the reference)",
                                     into_count(&o->depthFillHolesMaxPixels)}},
      {"--depthFillHolesTolerance", {Kind::kValue, "with --depthFillHolesMaxPixels: the depths round a hole agree if the largest "
                                                   "exceeds the smallest by at most this distance (world units, finite, >= 0, default "
                                                   "0) plus the relative tolerance (not in the reference)",
                                     into_checked_double(&o->depthFillHolesTolerance, &o->depthFillHolesToleranceGiven,
                                                         [](double x) { return x >= 0.0; })}},
      {"--depthFillHolesRelTolerance", {Kind::kValue, "with --depthFillHolesMaxPixels: ... plus this share of the smallest depth "
                                                      "round the hole (finite, >= 0, default 0.01; not in the reference)",
                                        into_checked_double(&o->depthFillHolesRelTolerance, &o->depthFillHolesRelToleranceGiven,
                                                            [](double x) { return x >= 0.0; })}},
      {"--depthSmoothSigma", {Kind::kValue, "smooth the depth maps on the GPU before they are fused, their edges preserved, behind "
                                            "--depthFillHolesMaxPixels and before --depthConsistencyMinViews and --gridAutoBounds see "
                                            "them: every depth moves to a weighted mean of the depths round it that differ from it by "
                                            "less than the tolerance, the weight falling off with the distance as a Gaussian of this "
                                            "sigma in pixels and with the depth difference (finite, >= 0; the radius "
                                            "ceil(truncate * sigma) is at most 8).  No pixel gains or loses its depth.  All views are "
                                            "then read into host memory at once, as with --depthSpeckleMinPixels, and smoothed on the "
                                            "first --device (not in the reference)",
                              into_checked_double(&o->depthSmoothSigma, &o->depthSmoothSigmaGiven, [](double x) { return x >= 0.0; })}},
      {"--depthSmoothTruncate", {Kind::kValue, "with --depthSmoothSigma: the Gaussian is cut off at this many sigmas (finite, in (0, 4], "
                                               "default 2; not in the reference)",
                                 into_checked_double(&o->depthSmoothTruncate, &o->depthSmoothTruncateGiven,
                                                     [](double x) { return x > 0.0 && x <= 4.0; })}},
      {"--depthSmoothTolerance", {Kind::kValue, "with --depthSmoothSigma: a neighbouring depth takes part if it differs from the pixel's "
                                                "by less than this distance (world units, finite, >= 0, default 0) plus the relative "
                                                "tolerance; a step higher than that is not smoothed across (not in the reference)",
                                  into_checked_double(&o->depthSmoothTolerance, &o->depthSmoothToleranceGiven,
                                                      [](double x) { return x >= 0.0; })}},
      {"--depthSmoothRelTolerance", {Kind::kValue, "with --depthSmoothSigma: ... plus this share of the pixel's depth (finite, >= 0, "
                                                   "default 0.01; not in the reference)",
                                     into_checked_double(&o->depthSmoothRelTolerance, &o->depthSmoothRelToleranceGiven,
                                                         [](double x) { return x >= 0.0; })}},
      {"--depthSmoothIterations", {Kind::kValue, "with --depthSmoothSigma: smooth this many times, each pass on the result of the one "
                                                 "before (an integer in [1, 16], default 1; not in the reference)",
                                   [o](const std::vector<std::string> &values) {
                                     o->depthSmoothIterationsGiven = true;
                                     return into_count(&o->depthSmoothIterations)(values) && o->depthSmoothIterations >= 1 &&
                                            o->depthSmoothIterations <= dmi::kDepthSmoothMaxIterations;
                                   }}},
      {"--outputPointCloudFilename", {Kind::kValue, "write the fused point cloud of the depth maps to this .vtp: the points the views "
                                                    "agree on, each once, with a normal taken from its own depth map -- built on the GPU "
                                                    "from the depth maps that are fused, behind every --depth... step.  Points "
                                                    "(Float64), one vertex cell per point, and the point arrays Normals, ViewIndex and "
                                                    "NbAgreeingViews.  Needs --pointCloudTolerance or --pointCloudRelTolerance unless "
                                                    "--depthConsistencyMinViews gives the tolerances; the depth maps stay on the GPU, so "
                                                    "--depthStagedFilters is refused (not in the reference)",
                                      into_string(&o->outputPointCloudFilename)}},
      {"--pointCloudMinViews", {Kind::kValue, "with --outputPointCloudFilename: a pixel becomes a point only if at least this many other "
                                              "views agree with its depth (a non-negative integer, default 1; not in the reference)",
                                [o](const std::vector<std::string> &values) {
                                  o->pointCloudMinViewsGiven = true;
                                  return into_count(&o->pointCloudMinViews)(values) && o->pointCloudMinViews <= 0x7fffffffLL;
                                }}},
      {"--pointCloudTolerance", {Kind::kValue, "with --outputPointCloudFilename: two depths agree within this distance (world units, "
                                               "finite, >= 0) plus the relative tolerance; default: --depthConsistencyTolerance when "
                                               "--depthConsistencyMinViews is given (not in the reference)",
                                 into_checked_double(&o->pointCloudTolerance, &o->pointCloudToleranceGiven, [](double x) { return x >= 0.0; })}},
      {"--pointCloudRelTolerance", {Kind::kValue, "with --outputPointCloudFilename: ... plus this share of the distance from the other "
                                                  "view's camera (finite, >= 0); default: --depthConsistencyRelTolerance when "
                                                  "--depthConsistencyMinViews is given (not in the reference)",
                                    into_checked_double(&o->pointCloudRelTolerance, &o->pointCloudRelToleranceGiven,
                                                        [](double x) { return x >= 0.0; })}},
      {"--pointCloudNormalTolerance", {Kind::kValue, "with --outputPointCloudFilename: a neighbouring pixel enters a point's normal only "
                                                     "if its depth lies within this distance (finite, >= 0) plus the relative normal "
                                                     "tolerance of the point's; default: the agreement tolerance (not in the reference)",
                                       into_checked_double(&o->pointCloudNormalTolerance, &o->pointCloudNormalToleranceGiven,
                                                           [](double x) { return x >= 0.0; })}},
      {"--pointCloudNormalRelTolerance", {Kind::kValue, "with --outputPointCloudFilename: ... plus this share of the point's depth "
                                                        "(finite, >= 0); default: the relative agreement tolerance (not in the reference)",
                                          into_checked_double(&o->pointCloudNormalRelTolerance, &o->pointCloudNormalRelToleranceGiven,
                                                              [](double x) { return x >= 0.0; })}},
      {"--pointCloudPixelStep", {Kind::kValue, "with --outputPointCloudFilename: only every k-th pixel of every k-th row becomes a point "
                                               "(an integer >= 1, default 1; not in the reference)",
                                 [o](const std::vector<std::string> &values) {
                                   o->pointCloudPixelStepGiven = true;
                                   return into_count(&o->pointCloudPixelStep)(values) && o->pointCloudPixelStep >= 1 &&
                                          o->pointCloudPixelStep <= 0x7fffffffLL;
                                 }}},
      {"--pointCloudKeepDuplicates", {Kind::kFlag, "with --outputPointCloudFilename: every view keeps its points; without the flag a "
                                                   "point that a lower view holds already is dropped.  Together with "
                                                   "--pointCloudCellSize this is what averages across views: the views' points of one "
                                                   "surface element are merged into their mean (not in the reference)",
                                      into_flag(&o->pointCloudKeepDuplicates)}},
      {"--pointCloudCellSize", {Kind::kValue, "with --outputPointCloudFilename: thin the cloud on the GPU before it is written, to one "
                                              "point per occupied cell of a grid of this size (world units, finite, > 0): the mean of "
                                              "the cell's points, their normals merged, the first one's view, the largest "
                                              "NbAgreeingViews, and the point array NbMergedPoints (not in the reference)",
                                into_checked_double(&o->pointCloudCellSize, &o->pointCloudCellSizeGiven, [](double x) { return x > 0.0; })}},
      {"--pointCloudMinCellPoints", {Kind::kValue, "with --pointCloudCellSize: drop the cells that hold fewer points than this (an "
                                                   "integer >= 1, default 1; not in the reference)",
                                     [o](const std::vector<std::string> &values) {
                                       o->pointCloudMinCellPointsGiven = true;
                                       return into_count(&o->pointCloudMinCellPoints)(values) && o->pointCloudMinCellPoints >= 1 &&
                                              o->pointCloudMinCellPoints <= 0x7fffffffLL;
                                     }}},
      {"--pointCloudOutlierRadius", {Kind::kValue, "with --outputPointCloudFilename: drop, on the GPU behind the build and before "
                                                   "--pointCloudCellSize, every point that has fewer than --pointCloudMinNeighbors other "
                                                   "points within this distance (world units, finite, > 0); without a thinning behind "
                                                   "it the file gets the point array NbNeighbors (not in the reference)",
                                     into_checked_double(&o->pointCloudOutlierRadius, &o->pointCloudOutlierRadiusGiven, [](double x) {
                                       const double r2 = x * x;  // a normal number: dmi_views_filter_points_radius asks for it
                                       return x > 0.0 && r2 >= 2.2250738585072014e-308 && r2 <= 1.7976931348623157e308;
                                     })}},
      {"--pointCloudMinNeighbors", {Kind::kValue, "with --pointCloudOutlierRadius: the points a point needs within the radius to stay (a "
                                                  "non-negative integer, default 1; 0 drops nothing and only counts; not in the reference)",
                                    [o](const std::vector<std::string> &values) {
                                      o->pointCloudMinNeighborsGiven = true;
                                      return into_count(&o->pointCloudMinNeighbors)(values) && o->pointCloudMinNeighbors >= 0 &&
                                             o->pointCloudMinNeighbors <= 0x7fffffffLL;
                                    }}},
      {"--pointCloudPlaneFitRadius", {Kind::kValue, "with --outputPointCloudFilename: fit, on the GPU behind --pointCloudOutlierRadius and "
                                                    "before --pointCloudCellSize, a plane to the points within this distance of every "
                                                    "point (world units, finite, > 0), move the point onto it and give it the plane's "
                                                    "normal; without a thinning behind it the file gets the point array PlaneRms, -1 "
                                                    "where a point had too few neighbours (not in the reference)",
                                      into_checked_double(&o->pointCloudPlaneFitRadius, &o->pointCloudPlaneFitRadiusGiven, [](double x) {
                                        const double r2 = x * x;  // a normal number: dmi_views_fit_point_planes asks for it
                                        return x > 0.0 && r2 >= 2.2250738585072014e-308 && r2 <= 1.7976931348623157e308;
                                      })}},
      {"--pointCloudPlaneFitMinNeighbors", {Kind::kValue, "with --pointCloudPlaneFitRadius: the other points a point needs within the "
                                                          "radius for a fit (an integer >= 2, default 5; not in the reference)",
                                            [o](const std::vector<std::string> &values) {
                                              o->pointCloudPlaneFitMinNeighborsGiven = true;
                                              return into_count(&o->pointCloudPlaneFitMinNeighbors)(values) &&
                                                     o->pointCloudPlaneFitMinNeighbors >= 2 && o->pointCloudPlaneFitMinNeighbors <= 0x7fffffffLL;
                                            }}},
      {"--pointCloudPlaneFitIterations", {Kind::kValue, "with --pointCloudPlaneFitRadius: the passes, each on the result of the one "
                                                        "before (an integer in [1, 100], default 1; not in the reference)",
                                          [o](const std::vector<std::string> &values) {
                                            o->pointCloudPlaneFitIterationsGiven = true;
                                            return into_count(&o->pointCloudPlaneFitIterations)(values) &&
                                                   o->pointCloudPlaneFitIterations >= 1 && o->pointCloudPlaneFitIterations <= 100;
                                          }}},
      {"--pointCloudPlaneFitKeepPositions", {Kind::kFlag, "with --pointCloudPlaneFitRadius: leave the points where they are, only "
                                                          "replace the normals (not in the reference)",
                                             into_flag(&o->pointCloudPlaneFitKeepPositions)}},
      {"--pointCloudPlaneFitKeepNormals", {Kind::kFlag, "with --pointCloudPlaneFitRadius: leave the normals as they are, only move the "
                                                        "points (not in the reference)",
                                           into_flag(&o->pointCloudPlaneFitKeepNormals)}},
      {"--pointCloudColors", {Kind::kFlag, "with --outputPointCloudFilename: the point array Color (UInt8 RGB), each point's pixel of its "
                                           "view's Color array; every depth map file must carry one (not in the reference)",
                              into_flag(&o->pointCloudColors)}},
      {"--depthStagedFilters", {Kind::kFlag, "with --depthSpeckleMinPixels, --depthFillHolesMaxPixels, --depthSmoothSigma, "
                                             "--depthConsistencyMinViews or --gridAutoBounds: run these steps through the staged "
                                             "calls, each with an upload and a download of its own, instead of keeping the depth "
                                             "maps on the GPU from the first step to the fusion; every output is the same, only the "
                                             "times differ (the tool takes this path by itself when the GPU's memory cannot hold the "
                                             "resident depth maps; not in the reference)",
                               into_flag(&o->depthStagedFilters)}},
      {"--gridAutoBounds", {Kind::kFlag, "take the grid's box from the depth maps instead of --gridOrigin and --gridEnd, which then must "
                                         "not be given (one of --gridDims / --gridSpacing still is): every valid pixel is "
                                         "back-projected on the GPU, and along each of the grid's axes the box runs from the "
                                         "coordinate below which the share --gridAutoBoundsTrim of the points lies to the one above "
                                         "which the same share lies, plus the margin -- a handful of wild depths does not decide "
                                         "it.  All views are then read into host memory at once, on the first --device, and with "
                                         "--depthConsistencyMinViews the filtered depths are what is measured (not in the reference)",
                           into_flag(&o->gridAutoBounds)}},
      {"--gridAutoBoundsTrim", {Kind::kValue, "with --gridAutoBounds: the share of the points left outside the box at either end of "
                                              "each axis (in [0, 0.5], default 0.005; 0 is the plain minimum and maximum; not in "
                                              "the reference)",
                                into_checked_double(&o->gridAutoBoundsTrim, &o->gridAutoBoundsTrimGiven,
                                                    [](double x) { return x >= 0.0 && x <= 0.5; })}},
      {"--gridAutoBoundsMargin", {Kind::kValue, "with --gridAutoBounds: what is added on either side of each axis, as a share of the "
                                                "trimmed extent (finite, >= 0, default 0.05; not in the reference)",
                                  into_checked_double(&o->gridAutoBoundsMargin, &o->gridAutoBoundsMarginGiven,
                                                      [](double x) { return x >= 0.0; })}},
      {"--gridAutoBoundsPixelStep", {Kind::kValue, "with --gridAutoBounds: only every s-th pixel of every s-th row is measured (an "
                                                   "integer >= 1, default 1; not in the reference)",
                                     [o](const std::vector<std::string> &values) {
                                       o->gridAutoBoundsPixelStepGiven = true;
                                       return into_count(&o->gridAutoBoundsPixelStep)(values) && o->gridAutoBoundsPixelStep >= 1 &&
                                              o->gridAutoBoundsPixelStep <= 0x7fffffffLL;
                                     }}},
      {"--contourSmoothSigma", {Kind::kMulti, "with --extractMesh: smooth the point data on the GPU with a Gaussian right before the "
                                              "contour, as a vtkImageGaussianSmooth in front of vtkContourFilter does: sigma in voxels, "
                                              "one value or one per grid axis (finite, >= 0; 0 skips the axis; the radius "
                                              "ceil(truncate * sigma) is at most 16).  The .mha and .vts volumes and the count of "
                                              "active cells stay what was fused (default 0 = off; not in the reference)",
                                [o](const std::vector<std::string> &values) {
                                  if (values.size() != 1 && values.size() != 3) return false;
                                  o->contourSmoothSigma.clear();
                                  for (const std::string &v : values) {
                                    double x = 0.0;
                                    if (!parse_number(v, &x) || !std::isfinite(x) || x < 0.0) return false;
                                    o->contourSmoothSigma.push_back(x);
                                  }
                                  o->contourSmoothSigma.resize(3, o->contourSmoothSigma[0]);
                                  return true;
                                }}},
      {"--contourSmoothTruncate", {Kind::kValue, "with --contourSmoothSigma: the Gaussian is cut off at this many sigmas (finite, in "
                                                 "(0, 4], default 3; not in the reference)",
                                   into_checked_double(&o->contourSmoothTruncate, &o->contourSmoothTruncateGiven,
                                                       [](double x) { return x > 0.0 && x <= 4.0; })}},
      {"--help", {Kind::kFlag, "print this text", into_flag(help)}},
  };
}

// rmain:310-344: the extent decides whichever of spacing / dimensions was not given, then --forceCubicVoxel
void derive_spacing_or_dimensions(Options *o) {
  double size[3];
  for (int a = 0; a < 3; ++a) size[a] = o->gridEnd[a] - o->gridOrigin[a];
  if (o->gridSpacing.empty()) {
    o->gridSpacing.resize(3);
    for (int a = 0; a < 3; ++a) o->gridSpacing[a] = size[a] / (double)o->gridDims[a];
  }
  if (o->gridDims.empty()) {
    o->gridDims.resize(3);
    for (int a = 0; a < 3; ++a) o->gridDims[a] = (int)(size[a] / o->gridSpacing[a]);
  }
  if (o->forceCubicVoxel) {  // rmain:337-344
    const double smallest = *std::min_element(o->gridSpacing.begin(), o->gridSpacing.end());
    o->gridSpacing.assign(3, smallest);
  }
}

double dot3(const std::vector<double> &a, const std::vector<double> &b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

bool ends_with_or_contains(const std::string &name, const std::string &extension) {
  return name.find(extension) != std::string::npos;  // rmain:296-297 looks for the extension anywhere in the name
}

}  // namespace

std::string HelpText() {
  Options scratch;
  bool help = false;
  std::ostringstream out;
  out << "dmi_reconstruction: fuses the depth maps of a data folder into a TSDF volume on an MI355X.\n";
  for (const auto &entry : flag_table(&scratch, &help)) {
    out << "  " << entry.first;
    if (entry.second.kind == Kind::kMulti) out << " v [v ...]";
    if (entry.second.kind == Kind::kValue) out << " v";
    out << "\n      " << entry.second.help << "\n";
  }
  return out.str();
}

bool ReadArguments(int argc, const char *const *argv, Options *o, std::ostream &err) {
  bool help = false;
  auto table = flag_table(o, &help);
  std::map<std::string, const Spec *> by_name;
  for (const auto &entry : table) by_name[entry.first] = &entry.second;
  for (int i = 1; i < argc;) {
    const std::string flag = argv[i];
    const auto hit = by_name.find(flag);
    if (hit == by_name.end()) {  // vtksys's parser fails on an argument nobody registered
      err << "Unknown argument: " << flag << "\n" << HelpText();
      return false;
    }
    ++i;
    std::vector<std::string> values;
    if (hit->second->kind == Kind::kValue) {
      if (i >= argc) {
        err << flag << " needs a value\n" << HelpText();
        return false;
      }
      values.push_back(argv[i++]);
    } else if (hit->second->kind == Kind::kMulti) {
      while (i < argc && by_name.find(argv[i]) == by_name.end()) values.push_back(argv[i++]);  // "-2.29" is a value
    }
    if (!hit->second->store(values)) {
      err << "Bad value for " << flag << "\n" << HelpText();
      return false;
    }
  }
  if (help) {
    err << HelpText();
    return false;
  }
  if (o->meshNormals && !o->extractMesh) {
    err << "Error : --meshNormals needs --extractMesh (the normals belong to the extracted mesh).\n" << HelpText();
    return false;
  }
  if (o->meshMinComponentTriangles >= 0 && !o->extractMesh) {
    err << "Error : --meshMinComponentTriangles needs --extractMesh (the components belong to the extracted mesh).\n" << HelpText();
    return false;
  }
  if (o->meshLargestComponent && !o->extractMesh) {
    err << "Error : --meshLargestComponent needs --extractMesh (the components belong to the extracted mesh).\n" << HelpText();
    return false;
  }
  if (o->meshRegionIds && !o->extractMesh) {
    err << "Error : --meshRegionIds needs --extractMesh (the region ids belong to the extracted mesh).\n" << HelpText();
    return false;
  }
  for (const auto &flag : {std::make_pair("--meshSmoothIterations", o->meshSmoothIterationsGiven),
                           std::make_pair("--meshSmoothLambda", o->meshSmoothLambdaGiven), std::make_pair("--meshSmoothMu", o->meshSmoothMuGiven)})
    if (flag.second && !o->extractMesh) {
      err << "Error : " << flag.first << " needs --extractMesh (the smoothing belongs to the extracted mesh).\n" << HelpText();
      return false;
    }
  if (o->meshFillHolesGiven && !o->extractMesh) {
    err << "Error : --meshFillHoles needs --extractMesh (the holes belong to the extracted mesh).\n" << HelpText();
    return false;
  }
  for (const auto &flag : {std::make_pair("--contourSmoothSigma", !o->contourSmoothSigma.empty()),
                           std::make_pair("--contourSmoothTruncate", o->contourSmoothTruncateGiven)})
    if (flag.second && !o->extractMesh) {
      err << "Error : " << flag.first << " needs --extractMesh (the smoothing belongs to the contour).\n" << HelpText();
      return false;
    }
  for (const double sigma : o->contourSmoothSigma) {  // the library's own rule: ceil(truncate * sigma) <= 16
    int32_t radius = 0;
    double weights[17];
    if (dmi::point_smoothing_weights(sigma, o->contourSmoothTruncate, &radius, weights) != 0) {
      err << "Bad value for --contourSmoothSigma: the radius ceil(truncate * sigma) must not exceed 16\n" << HelpText();
      return false;
    }
  }
  if (o->meshDecimateCellSizeGiven && !o->extractMesh) {
    err << "Error : --meshDecimateCellSize needs --extractMesh (the decimation belongs to the extracted mesh).\n" << HelpText();
    return false;
  }
  if (o->meshDecimateQuadric && !o->meshDecimateCellSizeGiven) {
    err << "Error : --meshDecimateQuadric needs --meshDecimateCellSize (it places the decimation's vertices).\n" << HelpText();
    return false;
  }
  if (o->meshColoration && !o->extractMesh) {
    err << "Error : --meshColoration needs --extractMesh (the colours belong to the extracted mesh).\n" << HelpText();
    return false;
  }
  if (o->meshColorationDepthToleranceGiven && !o->meshColoration) {
    err << "Error : --meshColorationDepthTolerance needs --meshColoration.\n" << HelpText();
    return false;
  }
  if (o->meshColorationDepthFromMesh && !(o->meshColoration && o->meshColorationDepthToleranceGiven)) {
    err << "Error : --meshColorationDepthFromMesh needs --meshColoration and --meshColorationDepthTolerance.\n" << HelpText();
    return false;
  }
  if (o->meshColoration && o->devices.size() > 1) {
    err << "Error : --meshColoration takes one --device (the mesh of a fusion over several GPUs is not coloured).\n" << HelpText();
    return false;
  }
  for (const auto &flag : {std::make_pair("--meshMinSupportViews", o->meshMinSupportViews >= 0), std::make_pair("--meshSupportArray", o->meshSupportArray)}) {
    if (!flag.second) continue;
    if (!o->extractMesh) {
      err << "Error : " << flag.first << " needs --extractMesh (the support belongs to the extracted mesh).\n" << HelpText();
      return false;
    }
    if (!o->meshSupportDepthToleranceGiven) {
      err << "Error : " << flag.first << " needs --meshSupportDepthTolerance.\n" << HelpText();
      return false;
    }
    if (o->devices.size() > 1) {
      err << "Error : " << flag.first << " takes one --device (the mesh of a fusion over several GPUs is not trimmed).\n" << HelpText();
      return false;
    }
  }
  for (const auto &flag : {std::make_pair("--meshSupportDepthTolerance", o->meshSupportDepthToleranceGiven),
                           std::make_pair("--meshSupportNoFacing", o->meshSupportNoFacing)})
    if (flag.second && o->meshMinSupportViews < 0 && !o->meshSupportArray) {
      err << "Error : " << flag.first << " needs --meshMinSupportViews or --meshSupportArray.\n" << HelpText();
      return false;
    }
  for (const auto &flag : {std::make_pair("--depthConsistencyTolerance", o->depthConsistencyToleranceGiven),
                           std::make_pair("--depthConsistencyRelTolerance", o->depthConsistencyRelToleranceGiven)})
    if (flag.second && o->depthConsistencyMinViews < 0) {
      err << "Error : " << flag.first << " needs --depthConsistencyMinViews.\n" << HelpText();
      return false;
    }
  if (o->depthConsistencyMinViews > 0x7fffffffLL) {
    err << "Bad value for --depthConsistencyMinViews\n" << HelpText();
    return false;
  }
  const bool pointCloud = !o->outputPointCloudFilename.empty();
  for (const auto &flag : {std::make_pair("--pointCloudMinViews", o->pointCloudMinViewsGiven),
                           std::make_pair("--pointCloudTolerance", o->pointCloudToleranceGiven),
                           std::make_pair("--pointCloudRelTolerance", o->pointCloudRelToleranceGiven),
                           std::make_pair("--pointCloudNormalTolerance", o->pointCloudNormalToleranceGiven),
                           std::make_pair("--pointCloudNormalRelTolerance", o->pointCloudNormalRelToleranceGiven),
                           std::make_pair("--pointCloudPixelStep", o->pointCloudPixelStepGiven),
                           std::make_pair("--pointCloudKeepDuplicates", o->pointCloudKeepDuplicates),
                           std::make_pair("--pointCloudColors", o->pointCloudColors),
                           std::make_pair("--pointCloudCellSize", o->pointCloudCellSizeGiven),
                           std::make_pair("--pointCloudOutlierRadius", o->pointCloudOutlierRadiusGiven),
                           std::make_pair("--pointCloudPlaneFitRadius", o->pointCloudPlaneFitRadiusGiven)})
    if (flag.second && !pointCloud) {
      err << "Error : " << flag.first << " needs --outputPointCloudFilename.\n" << HelpText();
      return false;
    }
  if (o->pointCloudMinCellPointsGiven && !o->pointCloudCellSizeGiven) {
    err << "Error : --pointCloudMinCellPoints needs --pointCloudCellSize.\n" << HelpText();
    return false;
  }
  if (o->pointCloudMinNeighborsGiven && !o->pointCloudOutlierRadiusGiven) {
    err << "Error : --pointCloudMinNeighbors needs --pointCloudOutlierRadius.\n" << HelpText();
    return false;
  }
  for (const auto &flag : {std::make_pair("--pointCloudPlaneFitMinNeighbors", o->pointCloudPlaneFitMinNeighborsGiven),
                           std::make_pair("--pointCloudPlaneFitIterations", o->pointCloudPlaneFitIterationsGiven),
                           std::make_pair("--pointCloudPlaneFitKeepPositions", o->pointCloudPlaneFitKeepPositions),
                           std::make_pair("--pointCloudPlaneFitKeepNormals", o->pointCloudPlaneFitKeepNormals)})
    if (flag.second && !o->pointCloudPlaneFitRadiusGiven) {
      err << "Error : " << flag.first << " needs --pointCloudPlaneFitRadius.\n" << HelpText();
      return false;
    }
  if (o->pointCloudPlaneFitKeepPositions && o->pointCloudPlaneFitKeepNormals) {
    err << "Error : --pointCloudPlaneFitKeepPositions and --pointCloudPlaneFitKeepNormals together leave the fit nothing to do.\n" << HelpText();
    return false;
  }
  if (pointCloud) {
    if (!ends_with_or_contains(o->outputPointCloudFilename, ".vtp")) {
      err << "Error : --outputPointCloudFilename must name a .vtp file.\n" << HelpText();
      return false;
    }
    if (o->depthStagedFilters) {
      err << "Error : --outputPointCloudFilename builds the points on the resident depth maps, which --depthStagedFilters does not "
             "keep.\n"
          << HelpText();
      return false;
    }
    if (!o->pointCloudToleranceGiven && !o->pointCloudRelToleranceGiven && o->depthConsistencyMinViews < 0) {
      err << "Error : --outputPointCloudFilename needs --pointCloudTolerance or --pointCloudRelTolerance when "
             "--depthConsistencyMinViews does not give the tolerances.\n"
          << HelpText();
      return false;
    }
    // the agreement pair from the consistency filter's where that was given, the normal pair from the agreement pair
    if (o->depthConsistencyMinViews >= 0) {
      if (!o->pointCloudToleranceGiven) o->pointCloudTolerance = o->depthConsistencyTolerance;
      if (!o->pointCloudRelToleranceGiven) o->pointCloudRelTolerance = o->depthConsistencyRelTolerance;
    }
    if (!o->pointCloudNormalToleranceGiven) o->pointCloudNormalTolerance = o->pointCloudTolerance;
    if (!o->pointCloudNormalRelToleranceGiven) o->pointCloudNormalRelTolerance = o->pointCloudRelTolerance;
  }
  if (o->depthStagedFilters && o->depthSpeckleMinPixels < 0 && o->depthFillHolesMaxPixels < 0 && !o->depthSmoothSigmaGiven &&
      o->depthConsistencyMinViews < 0 && !o->gridAutoBounds) {
    err << "Error : --depthStagedFilters needs --depthSpeckleMinPixels, --depthFillHolesMaxPixels, --depthSmoothSigma, "
           "--depthConsistencyMinViews or --gridAutoBounds.\n"
        << HelpText();
    return false;
  }
  for (const auto &flag : {std::make_pair("--depthSpeckleTolerance", o->depthSpeckleToleranceGiven),
                           std::make_pair("--depthSpeckleRelTolerance", o->depthSpeckleRelToleranceGiven)})
    if (flag.second && o->depthSpeckleMinPixels < 0) {
      err << "Error : " << flag.first << " needs --depthSpeckleMinPixels.\n" << HelpText();
      return false;
    }
  for (const auto &flag : {std::make_pair("--depthFillHolesTolerance", o->depthFillHolesToleranceGiven),
                           std::make_pair("--depthFillHolesRelTolerance", o->depthFillHolesRelToleranceGiven)})
    if (flag.second && o->depthFillHolesMaxPixels < 0) {
      err << "Error : " << flag.first << " needs --depthFillHolesMaxPixels.\n" << HelpText();
      return false;
    }
  for (const auto &flag : {std::make_pair("--depthSmoothTruncate", o->depthSmoothTruncateGiven),
                           std::make_pair("--depthSmoothTolerance", o->depthSmoothToleranceGiven),
                           std::make_pair("--depthSmoothRelTolerance", o->depthSmoothRelToleranceGiven),
                           std::make_pair("--depthSmoothIterations", o->depthSmoothIterationsGiven)})
    if (flag.second && !o->depthSmoothSigmaGiven) {
      err << "Error : " << flag.first << " needs --depthSmoothSigma.\n" << HelpText();
      return false;
    }
  if (o->depthSmoothSigmaGiven) {  // the library's own rule: ceil(truncate * sigma) <= 8
    int32_t radius = 0;
    double weights[dmi::kDepthSmoothMaxRadius + 1];
    if (dmi::depth_smoothing_weights(o->depthSmoothSigma, o->depthSmoothTruncate, &radius, weights) != 0) {
      err << "Bad value for --depthSmoothSigma: the radius ceil(truncate * sigma) must not exceed " << dmi::kDepthSmoothMaxRadius << "\n"
          << HelpText();
      return false;
    }
  }
  for (const auto &flag : {std::make_pair("--gridAutoBoundsTrim", o->gridAutoBoundsTrimGiven),
                           std::make_pair("--gridAutoBoundsMargin", o->gridAutoBoundsMarginGiven),
                           std::make_pair("--gridAutoBoundsPixelStep", o->gridAutoBoundsPixelStepGiven)})
    if (flag.second && !o->gridAutoBounds) {
      err << "Error : " << flag.first << " needs --gridAutoBounds.\n" << HelpText();
      return false;
    }
  if (o->gridAutoBounds && (!o->gridOrigin.empty() || !o->gridEnd.empty())) {
    err << "Error : --gridAutoBounds takes the grid's box from the depth maps: --gridOrigin and --gridEnd must not be given.\n"
        << HelpText();
    return false;
  }
  // rmain:257-262
  if (!o->gridSpacing.empty() && !o->gridDims.empty()) {
    err << "Error : Spacing and dimensions can't be both set\n" << HelpText();
    return false;
  }
  // rmain:265-269: one dimension stands for all three
  if (o->gridDims.size() == 1) o->gridDims.resize(3, o->gridDims[0]);
  // rmain:272-278
  if (o->outputGridFilename.empty() || o->outputMeshFilename.empty() || o->depthMapFile.empty() || o->krtFile.empty() ||
      o->rayDelta < o->rayThick || o->rayEta < 0 || o->rayEta > 1) {
    err << "Error arguments.\n" << HelpText();
    return false;
  }
  if (o->gridVecX.empty()) o->gridVecX = {1, 0, 0};
  if (o->gridVecY.empty()) o->gridVecY = {0, 1, 0};
  if (o->gridVecZ.empty()) o->gridVecZ = {0, 0, 1};
  // rmain:294-301
  if (!ends_with_or_contains(o->outputGridFilename, ".vts") || !ends_with_or_contains(o->outputMeshFilename, ".vtp")) {
    err << "Error : Bad output extension.\n";
    return false;
  }
  // The reference indexes these vectors without looking at their length (rmain:311-313, 345-360): a missing
  // --gridOrigin / --gridEnd or a two-component axis is undefined behaviour there and an error here.
  // (with --gridAutoBounds the two corners are absent: Run takes them from the depth maps)
  const size_t corner = o->gridAutoBounds ? 0 : 3;
  if (o->gridVecX.size() != 3 || o->gridVecY.size() != 3 || o->gridVecZ.size() != 3 || o->gridOrigin.size() != corner ||
      o->gridEnd.size() != corner || (!o->gridDims.empty() && o->gridDims.size() != 3) ||
      (!o->gridSpacing.empty() && o->gridSpacing.size() != 3) || (o->gridDims.empty() && o->gridSpacing.empty())) {
    err << "Error : --gridOrigin, --gridEnd and the three axes take three values each, and one of --gridDims / "
           "--gridSpacing is required.\n";
    return false;
  }
  if (!AreVectorsOrthogonal(*o)) {
    err << "Given vectors are not orthogonals.\n";
    return false;
  }
  if (o->gridAutoBounds) return true;  // the box is not known yet: Run estimates it and derives the rest
  derive_spacing_or_dimensions(o);
  return true;
}

bool AreVectorsOrthogonal(const Options &o) {
  // vtkMathUtilities::FuzzyCompare(x, 0.0, 10e-6): |x| < 1e-5
  const double epsilon = 10e-6;
  return std::fabs(dot3(o.gridVecX, o.gridVecY)) < epsilon && std::fabs(dot3(o.gridVecY, o.gridVecZ)) < epsilon &&
         std::fabs(dot3(o.gridVecZ, o.gridVecX)) < epsilon;
}

void CreateGridMatrixFromInput(const Options &o, double m[16]) {
  for (int i = 0; i < 16; ++i) m[i] = (i % 5 == 0) ? 1.0 : 0.0;
  for (int c = 0; c < 3; ++c) {
    m[0 * 4 + c] = o.gridVecX[c];
    m[1 * 4 + c] = o.gridVecY[c];
    m[2 * 4 + c] = o.gridVecZ[c];
  }
}

// ---- writers -----------------------------------------------------------------------------------------------------------

bool WriteMetaImage(const std::string &path, const int pointDims[3], const double origin[3], const double spacing[3],
                    const double *pointScalars, std::string *error) {
  // MetaImage with local, zlib-compressed element data (vtkMetaImageWriter with SetCompression(true), rmain:157-161)
  const uint64_t n = (uint64_t)pointDims[0] * pointDims[1] * pointDims[2];
  const uint64_t raw_bytes = n * sizeof(double);
  if (raw_bytes > (uint64_t)1 << 40) {
    *error = "WriteMetaImage: volume too large";
    return false;
  }
  std::ofstream out(path, std::ios::binary);
  if (!out) {
    *error = "WriteMetaImage: cannot open " + path;
    return false;
  }
  // compress in pieces of 256 MiB: one deflate stream
  std::vector<unsigned char> packed;
  z_stream z;
  std::memset(&z, 0, sizeof(z));
  if (deflateInit(&z, Z_BEST_SPEED) != Z_OK) {
    *error = "WriteMetaImage: zlib initialisation failed";
    return false;
  }
  std::vector<unsigned char> chunk(size_t(4) << 20);
  const unsigned char *src = reinterpret_cast<const unsigned char *>(pointScalars);
  uint64_t done = 0;
  int rc = Z_OK;
  do {
    const uint64_t piece = std::min<uint64_t>(raw_bytes - done, uint64_t(256) << 20);
    z.next_in = const_cast<unsigned char *>(src + done);
    z.avail_in = (uInt)piece;
    done += piece;
    const int flush = done == raw_bytes ? Z_FINISH : Z_NO_FLUSH;
    do {
      z.next_out = chunk.data();
      z.avail_out = (uInt)chunk.size();
      rc = deflate(&z, flush);
      packed.insert(packed.end(), chunk.data(), chunk.data() + (chunk.size() - z.avail_out));
    } while (z.avail_out == 0);
  } while (done < raw_bytes);
  deflateEnd(&z);
  if (rc != Z_STREAM_END) {
    *error = "WriteMetaImage: compression failed";
    return false;
  }
  out << "ObjectType = Image\nNDims = 3\nBinaryData = True\nBinaryDataByteOrderMSB = False\nCompressedData = True\n"
      << "CompressedDataSize = " << packed.size() << "\nTransformMatrix = 1 0 0 0 1 0 0 0 1\n";
  out.precision(17);
  out << "Offset = " << origin[0] << " " << origin[1] << " " << origin[2] << "\nCenterOfRotation = 0 0 0\n"
      << "ElementSpacing = " << spacing[0] << " " << spacing[1] << " " << spacing[2] << "\n"
      << "DimSize = " << pointDims[0] << " " << pointDims[1] << " " << pointDims[2] << "\nAnatomicalOrientation = ???\n"
      << "ElementType = MET_DOUBLE\nElementDataFile = LOCAL\n";
  out.write(reinterpret_cast<const char *>(packed.data()), (std::streamsize)packed.size());
  if (!out) {
    *error = "WriteMetaImage: write failed: " + path;
    return false;
  }
  return true;
}

bool WriteStructuredGrid(const std::string &path, const int pointDims[3], const double origin[3], const double spacing[3],
                         const double gridMatrix[16], const double *cellScalars, const char *arrayName, std::string *error) {
  // What vtkTransformFilter makes of the filter's vtkImageData (rmain:189-198): a structured grid whose points are the
  // image's points under the grid matrix, cell data carried along.  VTK XML, appended raw data, UInt64 headers.
  const int nx = pointDims[0], ny = pointDims[1], nz = pointDims[2];
  if (nx < 2 || ny < 2 || nz < 2) {
    *error = "WriteStructuredGrid: at least two points per axis";
    return false;
  }
  const uint64_t n_cells = (uint64_t)(nx - 1) * (ny - 1) * (nz - 1), n_points = (uint64_t)nx * ny * nz;
  std::ofstream out(path, std::ios::binary);
  if (!out) {
    *error = "WriteStructuredGrid: cannot open " + path;
    return false;
  }
  const uint64_t cell_bytes = n_cells * sizeof(double), point_bytes = n_points * 3 * sizeof(double);
  out << "<?xml version=\"1.0\"?>\n<VTKFile type=\"StructuredGrid\" version=\"1.0\" byte_order=\"LittleEndian\" "
         "header_type=\"UInt64\">\n  <StructuredGrid WholeExtent=\"0 "
      << nx - 1 << " 0 " << ny - 1 << " 0 " << nz - 1 << "\">\n    <Piece Extent=\"0 " << nx - 1 << " 0 " << ny - 1 << " 0 " << nz - 1
      << "\">\n      <PointData/>\n      <CellData Scalars=\"" << arrayName << "\">\n        <DataArray type=\"Float64\" Name=\""
      << arrayName << "\" format=\"appended\" offset=\"0\"/>\n      </CellData>\n      <Points>\n        <DataArray type=\"Float64\" "
         "Name=\"Points\" NumberOfComponents=\"3\" format=\"appended\" offset=\""
      << cell_bytes + sizeof(uint64_t) << "\"/>\n      </Points>\n    </Piece>\n  </StructuredGrid>\n  <AppendedData encoding=\"raw\">\n   _";
  out.write(reinterpret_cast<const char *>(&cell_bytes), sizeof(cell_bytes));
  out.write(reinterpret_cast<const char *>(cellScalars), (std::streamsize)cell_bytes);
  out.write(reinterpret_cast<const char *>(&point_bytes), sizeof(point_bytes));
  std::vector<double> row((size_t)nx * 3);
  for (int k = 0; k < nz; ++k)
    for (int j = 0; j < ny; ++j) {
      for (int i = 0; i < nx; ++i) {
        // vtkTransform::TransformPoint: M * (x, y, z, 1), left to right
        const double p[3] = {origin[0] + i * spacing[0], origin[1] + j * spacing[1], origin[2] + k * spacing[2]};
        for (int r = 0; r < 3; ++r)
          row[(size_t)i * 3 + r] = gridMatrix[4 * r + 0] * p[0] + gridMatrix[4 * r + 1] * p[1] + gridMatrix[4 * r + 2] * p[2] + gridMatrix[4 * r + 3];
      }
      out.write(reinterpret_cast<const char *>(row.data()), (std::streamsize)(row.size() * sizeof(double)));
    }
  out << "\n  </AppendedData>\n</VTKFile>\n";
  if (!out) {
    *error = "WriteStructuredGrid: write failed: " + path;
    return false;
  }
  return true;
}

bool WritePointCloud(const std::string &path, const double *points, int64_t nPoints, const float *normals, const int32_t *view,
                     const int32_t *agreeing, const uint8_t *color, std::string *error, const uint32_t *merged, const uint32_t *neighbors,
                     const float *planeRms) {
  if (nPoints < 0) {
    *error = "WritePointCloud: negative count";
    return false;
  }
  std::ofstream out(path, std::ios::binary);
  if (!out) {
    *error = "WritePointCloud: cannot open " + path;
    return false;
  }
  const uint64_t n = (uint64_t)nPoints, header = sizeof(uint64_t);
  const uint64_t point_bytes = n * 3 * sizeof(double), cell_bytes = n * sizeof(int64_t), normal_bytes = n * 3 * sizeof(float),
                 int_bytes = n * sizeof(int32_t), rgb_bytes = n * 3;
  // the raw block: Points, connectivity, offsets, Normals, ViewIndex, NbAgreeingViews, NbMergedPoints, NbNeighbors, PlaneRms, Color -- [UInt64
  // byte count] bytes each
  const uint64_t conn_offset = header + point_bytes, offsets_offset = conn_offset + header + cell_bytes;
  const uint64_t normal_offset = offsets_offset + header + cell_bytes, view_offset = normal_offset + header + normal_bytes;
  const uint64_t agreeing_offset = view_offset + header + int_bytes, merged_offset = agreeing_offset + header + int_bytes;
  const uint64_t neighbors_offset = merged ? merged_offset + header + int_bytes : merged_offset;
  const uint64_t rms_offset = neighbors ? neighbors_offset + header + int_bytes : neighbors_offset;
  const uint64_t color_offset = planeRms ? rms_offset + header + int_bytes : rms_offset;
  out << "<?xml version=\"1.0\"?>\n<VTKFile type=\"PolyData\" version=\"1.0\" byte_order=\"LittleEndian\" "
         "header_type=\"UInt64\">\n  <PolyData>\n    <Piece NumberOfPoints=\""
      << nPoints << "\" NumberOfVerts=\"" << nPoints << "\" NumberOfLines=\"0\" NumberOfStrips=\"0\" NumberOfPolys=\"0\">\n"
      << "      <PointData Normals=\"Normals\">\n        <DataArray type=\"Float32\" Name=\"Normals\" NumberOfComponents=\"3\" "
         "format=\"appended\" offset=\""
      << normal_offset << "\"/>\n        <DataArray type=\"Int32\" Name=\"ViewIndex\" format=\"appended\" offset=\"" << view_offset
      << "\"/>\n        <DataArray type=\"Int32\" Name=\"NbAgreeingViews\" format=\"appended\" offset=\"" << agreeing_offset << "\"/>\n";
  if (merged)
    out << "        <DataArray type=\"UInt32\" Name=\"NbMergedPoints\" format=\"appended\" offset=\"" << merged_offset << "\"/>\n";
  if (neighbors)
    out << "        <DataArray type=\"UInt32\" Name=\"NbNeighbors\" format=\"appended\" offset=\"" << neighbors_offset << "\"/>\n";
  if (planeRms)
    out << "        <DataArray type=\"Float32\" Name=\"PlaneRms\" format=\"appended\" offset=\"" << rms_offset << "\"/>\n";
  if (color)
    out << "        <DataArray type=\"UInt8\" Name=\"Color\" NumberOfComponents=\"3\" format=\"appended\" offset=\"" << color_offset
        << "\"/>\n";
  out << "      </PointData>\n      <Points>\n        <DataArray type=\"Float64\" Name=\"Points\" NumberOfComponents=\"3\" "
         "format=\"appended\" offset=\"0\"/>\n      </Points>\n      <Verts>\n        <DataArray type=\"Int64\" Name=\"connectivity\" "
         "format=\"appended\" offset=\""
      << conn_offset << "\"/>\n        <DataArray type=\"Int64\" Name=\"offsets\" format=\"appended\" offset=\"" << offsets_offset
      << "\"/>\n      </Verts>\n    </Piece>\n  </PolyData>\n  <AppendedData encoding=\"raw\">\n   _";
  auto write = [&](const void *data, uint64_t bytes) {
    out.write(reinterpret_cast<const char *>(&bytes), sizeof(bytes));
    out.write(reinterpret_cast<const char *>(data), (std::streamsize)bytes);
  };
  write(points, point_bytes);
  for (const int64_t first : {int64_t(0), int64_t(1)}) {  // connectivity 0, 1, 2 ...; offsets 1, 2, 3 ...: in pieces
    out.write(reinterpret_cast<const char *>(&cell_bytes), sizeof(cell_bytes));
    std::vector<int64_t> run((size_t)std::min<int64_t>(nPoints, int64_t(1) << 20));
    for (int64_t done = 0; done < nPoints;) {
      const int64_t count = std::min<int64_t>(nPoints - done, (int64_t)run.size());
      for (int64_t q = 0; q < count; ++q) run[(size_t)q] = first + done + q;
      out.write(reinterpret_cast<const char *>(run.data()), (std::streamsize)(count * sizeof(int64_t)));
      done += count;
    }
  }
  write(normals, normal_bytes);
  write(view, int_bytes);
  write(agreeing, int_bytes);
  if (merged) write(merged, int_bytes);
  if (neighbors) write(neighbors, int_bytes);
  if (planeRms) write(planeRms, int_bytes);
  if (color) write(color, rgb_bytes);
  out << "\n  </AppendedData>\n</VTKFile>\n";
  if (!out) {
    *error = "WritePointCloud: write failed: " + path;
    return false;
  }
  return true;
}

bool WritePolyData(const std::string &path, const double *points, int64_t nPoints, const int64_t *triangles, int64_t nTriangles,
                   std::string *error, const float *normals, double contour, const int64_t *regionIds, const uint8_t *mean,
                   const uint8_t *median, const int32_t *count, const int32_t *support) {
  const bool colors = mean && median && count;
  if (nPoints < 0 || nTriangles < 0) {
    *error = "WritePolyData: negative count";
    return false;
  }
  std::ofstream out(path, std::ios::binary);
  if (!out) {
    *error = "WritePolyData: cannot open " + path;
    return false;
  }
  const uint64_t point_bytes = (uint64_t)nPoints * 3 * sizeof(double), conn_bytes = (uint64_t)nTriangles * 3 * sizeof(int64_t),
                 offset_bytes = (uint64_t)nTriangles * sizeof(int64_t);
  const uint64_t normal_bytes = (uint64_t)nPoints * 3 * sizeof(float), scalar_bytes = (uint64_t)nPoints * sizeof(double);
  const uint64_t normal_offset = 3 * sizeof(uint64_t) + point_bytes + conn_bytes + offset_bytes;  // behind the offsets
  const uint64_t region_bytes = (uint64_t)nPoints * sizeof(int64_t);
  const uint64_t region_offset = normal_offset + (normals ? 2 * sizeof(uint64_t) + normal_bytes + scalar_bytes : 0);
  const uint64_t rgb_bytes = (uint64_t)nPoints * 3, count_bytes = (uint64_t)nPoints * sizeof(int32_t);
  const uint64_t support_offset = region_offset + (regionIds ? sizeof(uint64_t) + region_bytes : 0);
  const uint64_t color_offset = support_offset + (support ? sizeof(uint64_t) + count_bytes : 0);  // behind every other array
  out << "<?xml version=\"1.0\"?>\n<VTKFile type=\"PolyData\" version=\"1.0\" byte_order=\"LittleEndian\" "
         "header_type=\"UInt64\">\n  <PolyData>\n    <Piece NumberOfPoints=\""
      << nPoints << "\" NumberOfVerts=\"0\" NumberOfLines=\"0\" NumberOfStrips=\"0\" NumberOfPolys=\"" << nTriangles << "\">\n";
  if (normals)  // vtkContourFilter's point data (ComputeNormals, ComputeScalars)
    out << "      <PointData Normals=\"Normals\" Scalars=\"reconstruction_scalar\">\n        <DataArray type=\"Float32\" "
           "Name=\"Normals\" NumberOfComponents=\"3\" format=\"appended\" offset=\""
        << normal_offset << "\"/>\n        <DataArray type=\"Float64\" Name=\"reconstruction_scalar\" format=\"appended\" offset=\""
        << normal_offset + sizeof(uint64_t) + normal_bytes << "\"/>\n";
  else if (regionIds)
    out << "      <PointData Scalars=\"RegionId\">\n";
  else if (colors || support)
    out << "      <PointData>\n";
  if (regionIds)  // vtkPolyDataConnectivityFilter's (ColorRegionsOn)
    out << "        <DataArray type=\"Int64\" Name=\"RegionId\" format=\"appended\" offset=\"" << region_offset << "\"/>\n";
  if (support)
    out << "        <DataArray type=\"Int32\" Name=\"NbSupportingViews\" format=\"appended\" offset=\"" << support_offset << "\"/>\n";
  if (colors)  // the Coloration tool's three (MC.cxx:194-196)
    out << "        <DataArray type=\"UInt8\" Name=\"MeanColoration\" NumberOfComponents=\"3\" format=\"appended\" offset=\"" << color_offset
        << "\"/>\n        <DataArray type=\"UInt8\" Name=\"MedianColoration\" NumberOfComponents=\"3\" format=\"appended\" offset=\""
        << color_offset + sizeof(uint64_t) + rgb_bytes << "\"/>\n        <DataArray type=\"Int32\" Name=\"NbProjectedDepthMap\" format=\"appended\" offset=\""
        << color_offset + 2 * (sizeof(uint64_t) + rgb_bytes) << "\"/>\n";
  if (normals || regionIds || colors || support) out << "      </PointData>\n";
  out << "      <Points>\n        <DataArray type=\"Float64\" Name=\"Points\" NumberOfComponents=\"3\" format=\"appended\" "
         "offset=\"0\"/>\n      </Points>\n      <Polys>\n        <DataArray type=\"Int64\" Name=\"connectivity\" format=\"appended\" offset=\""
      << sizeof(uint64_t) + point_bytes << "\"/>\n        <DataArray type=\"Int64\" Name=\"offsets\" format=\"appended\" offset=\""
      << 2 * sizeof(uint64_t) + point_bytes + conn_bytes
      << "\"/>\n      </Polys>\n    </Piece>\n  </PolyData>\n  <AppendedData encoding=\"raw\">\n   _";
  out.write(reinterpret_cast<const char *>(&point_bytes), sizeof(point_bytes));
  out.write(reinterpret_cast<const char *>(points), (std::streamsize)point_bytes);
  out.write(reinterpret_cast<const char *>(&conn_bytes), sizeof(conn_bytes));
  out.write(reinterpret_cast<const char *>(triangles), (std::streamsize)conn_bytes);
  out.write(reinterpret_cast<const char *>(&offset_bytes), sizeof(offset_bytes));
  std::vector<int64_t> offsets((size_t)std::min<int64_t>(nTriangles, int64_t(1) << 20));
  for (int64_t done = 0; done < nTriangles;) {  // 3, 6, 9, ... in pieces
    const int64_t n = std::min<int64_t>(nTriangles - done, (int64_t)offsets.size());
    for (int64_t q = 0; q < n; ++q) offsets[(size_t)q] = 3 * (done + q + 1);
    out.write(reinterpret_cast<const char *>(offsets.data()), (std::streamsize)(n * sizeof(int64_t)));
    done += n;
  }
  if (normals) {
    out.write(reinterpret_cast<const char *>(&normal_bytes), sizeof(normal_bytes));
    out.write(reinterpret_cast<const char *>(normals), (std::streamsize)normal_bytes);
    out.write(reinterpret_cast<const char *>(&scalar_bytes), sizeof(scalar_bytes));
    const std::vector<double> scalars((size_t)std::min<int64_t>(nPoints, int64_t(1) << 20), contour);
    for (int64_t done = 0; done < nPoints;) {
      const int64_t n = std::min<int64_t>(nPoints - done, (int64_t)scalars.size());
      out.write(reinterpret_cast<const char *>(scalars.data()), (std::streamsize)(n * sizeof(double)));
      done += n;
    }
  }
  if (regionIds) {
    out.write(reinterpret_cast<const char *>(&region_bytes), sizeof(region_bytes));
    out.write(reinterpret_cast<const char *>(regionIds), (std::streamsize)region_bytes);
  }
  if (support) {
    out.write(reinterpret_cast<const char *>(&count_bytes), sizeof(count_bytes));
    out.write(reinterpret_cast<const char *>(support), (std::streamsize)count_bytes);
  }
  if (colors) {
    out.write(reinterpret_cast<const char *>(&rgb_bytes), sizeof(rgb_bytes));
    out.write(reinterpret_cast<const char *>(mean), (std::streamsize)rgb_bytes);
    out.write(reinterpret_cast<const char *>(&rgb_bytes), sizeof(rgb_bytes));
    out.write(reinterpret_cast<const char *>(median), (std::streamsize)rgb_bytes);
    out.write(reinterpret_cast<const char *>(&count_bytes), sizeof(count_bytes));
    out.write(reinterpret_cast<const char *>(count), (std::streamsize)count_bytes);
  }
  out << "\n  </AppendedData>\n</VTKFile>\n";
  if (!out) {
    *error = "WritePolyData: write failed: " + path;
    return false;
  }
  return true;
}

namespace {

void describe(const Options &o, std::ostream &out, bool with_sketch) {
  const double mean_voxel = (o.gridSpacing[0] + o.gridSpacing[1] + o.gridSpacing[2]) / 3.0;
  out << "grid\n  dimensions   " << o.gridDims[0] << " x " << o.gridDims[1] << " x " << o.gridDims[2] << " ("
      << (long long)o.gridDims[0] * o.gridDims[1] * o.gridDims[2] << " voxels)\n  spacing      " << o.gridSpacing[0] << " "
      << o.gridSpacing[1] << " " << o.gridSpacing[2] << "\n  origin       " << o.gridOrigin[0] << " " << o.gridOrigin[1] << " "
      << o.gridOrigin[2] << "\n  end          " << o.gridEnd[0] << " " << o.gridEnd[1] << " " << o.gridEnd[2] << "\n  extent       "
      << o.gridDims[0] * o.gridSpacing[0] << " " << o.gridDims[1] * o.gridSpacing[1] << " " << o.gridDims[2] * o.gridSpacing[2]
      << "\n  axes (rows)  " << o.gridVecX[0] << " " << o.gridVecX[1] << " " << o.gridVecX[2] << " | " << o.gridVecY[0] << " "
      << o.gridVecY[1] << " " << o.gridVecY[2] << " | " << o.gridVecZ[0] << " " << o.gridVecZ[1] << " " << o.gridVecZ[2]
      << "\ndepth maps\n  best-cost threshold  " << o.threshBestCost << "\nray potential\n";
  if (with_sketch)
    out << "  value   rho ........................ /''''|\n"
           "            0 .......................  /    |________\n"
           "     -eta*rho ______________          /\n"
           "                            |________/\n"
           "                          -delta  -thick  0  +thick  (distance behind the surface)\n";
  out << "  thickness  " << o.rayThick << " (about " << o.rayThick / mean_voxel << " voxels)\n  rho        " << o.rayRho
      << "\n  eta        " << o.rayEta << "\n  delta      " << o.rayDelta << " (about " << o.rayDelta / mean_voxel
      << " voxels)\nother\n  contour value  " << o.contour
      << (o.extractMesh ? " (surface extracted: --extractMesh)\n" : " (no surface is extracted by this tool)\n");
}

// --contourSmoothSigma with a sigma that is not 0
bool contourSmoothed(const Options &o) {
  return std::any_of(o.contourSmoothSigma.begin(), o.contourSmoothSigma.end(), [](double s) { return s > 0.0; });
}

}  // namespace

int Run(const Options &given, int argc, const char *const *argv, std::ostream &log, RunResult *result) {
  const auto start = std::chrono::steady_clock::now();
  Options resolved = given;  // --gridAutoBounds fills in the box and what follows from it
  const Options &o = resolved;
  auto say = [&](const std::string &what) {
    if (o.verbose) log << what << "\n" << std::endl;
  };
  say("---START---");
  const std::string vti_list = o.dataFolder + "/" + o.depthMapFile, krtd_list = o.dataFolder + "/" + o.krtFile;
  // --depthConsistencyMinViews and --gridAutoBounds: every view is read once and held in memory; the filter then fuses them from
  // there (SetViews: the path that thresholds again, which changes nothing, and forwards the Color planes to the colour sink)
  std::vector<std::unique_ptr<ReconstructionData>> memoryViews;
  std::vector<ReconstructionData *> views;
  auto read_views = [&](const std::string &flag) {
    if (!views.empty()) return true;  // (an earlier filter of this run has read them)
    const std::vector<std::string> vtis = help::ExtractAllFilePath(vti_list.c_str()), krtds = help::ExtractAllFilePath(krtd_list.c_str());
    if (vtis.empty() || krtds.size() < vtis.size()) {  // filt.cxx:161-165
      result->error = "Error : There is no enough vti files, please check your vtiList.txt and krtdList.txt";
      return false;
    }
    for (size_t m = 0; m < vtis.size(); ++m) {
      memoryViews.emplace_back(new ReconstructionData(vtis[m], krtds[m]));
      if (!memoryViews.back()->GetDepthMap()) {
        result->error = flag + ": cannot read depth map " + vtis[m];
        return false;
      }
      views.push_back(memoryViews.back().get());
    }
    return true;
  };
  // The steps below run on a resident view set: the views go up once, every step works where they are, and the
  // filter fuses them from there.  --depthStagedFilters keeps the staged calls; so does, from then on, a set that the device's
  // memory cannot hold: its depths are stored into the host views and the step that failed is run again the staged way.
  DepthViewSet resident;
  bool staged = o.depthStagedFilters;
  const int stepDevice = o.devices.empty() ? 0 : o.devices[0];
  // true: the step is to run on the set, which is loaded
  auto on_set = [&]() {
    if (staged || resident.Loaded()) return !staged;
    if (resident.Load(views, o.threshBestCost, stepDevice)) return true;
    if (resident.LastCode() == DMI_ERR_OUT_OF_MEMORY) {
      say("the depth maps do not fit the GPU's memory as a resident set: the staged filters are used (" + resident.LastError() + ")");
      staged = true;
      return false;
    }
    if (resident.LastCode() == DMI_ERR_INVALID_ARGUMENT) {  // views the set cannot take: the staged call says what is wrong with them
      say("the depth maps cannot form a resident set: the staged filters are used (" + resident.LastError() + ")");
      staged = true;
      return false;
    }
    return true;  // (another failure: run_step reports it)
  };
  // a step on the set has failed: true if the staged path is to take over (out of memory, and the depths are back on the host)
  auto taken_over = [&](const std::string &flag, std::string *error) {
    *error = resident.LastError();
    if (resident.LastCode() != DMI_ERR_OUT_OF_MEMORY || !resident.Loaded()) return false;
    if (!resident.Store(views, o.threshBestCost)) {
      *error = resident.LastError();
      return false;
    }
    say(flag + ": the GPU's memory does not hold this step on the resident set: the staged filters are used from here (" + *error + ")");
    resident.Release();
    staged = true;
    return true;
  };
  // runs `on_resident` on the set or `on_host` the staged way; false: `error` says why
  auto run_step = [&](const std::string &flag, const std::function<bool()> &on_resident, const std::function<bool(std::string *)> &on_host,
                      std::string *error) {
    if (on_set()) {
      if (!resident.Loaded()) {
        *error = resident.LastError();
        return false;
      }
      if (on_resident()) return true;
      if (!taken_over(flag, error)) return false;
    }
    return on_host(error);
  };
  // the small segments of all views removed on the first device: before the consistency filter, so that an island cannot vouch for
  // another view's island
  auto speckle_views = [&]() {
    say("** Remove the small segments of the depth maps...");
    if (!read_views("--depthSpeckleMinPixels")) return false;
    DepthSpeckleReport report;
    std::string error;
    if (!run_step("--depthSpeckleMinPixels",
                  [&]() { return resident.FilterSpeckles(o.depthSpeckleMinPixels, o.depthSpeckleTolerance, o.depthSpeckleRelTolerance, &report); },
                  [&](std::string *why) {
                    return FilterDepthSpeckles(views, o.threshBestCost, o.depthSpeckleMinPixels, o.depthSpeckleTolerance,
                                               o.depthSpeckleRelTolerance, stepDevice, &report, why);
                  },
                  &error)) {
      result->error = "--depthSpeckleMinPixels: " + error;
      return false;
    }
    result->depthSpeckleViews = report.views;
    result->depthSpeckleValidPixels = report.validPixels;
    result->depthSpeckleKeptPixels = report.keptPixels;
    result->depthSpeckleSegments = report.segments;
    result->depthSpeckleKeptSegments = report.keptSegments;
    result->depthSpeckleKernelMs = report.kernelMs;
    std::ostringstream line;
    line << "depth speckles: segments of at least " << o.depthSpeckleMinPixels << " pixels, tolerance " << o.depthSpeckleTolerance << " + "
         << o.depthSpeckleRelTolerance << " z; " << report.views << " views, " << report.validPixels << " pixels with a depth, "
         << report.keptPixels << " kept; " << report.segments << " segments, " << report.keptSegments << " kept; " << report.kernelMs
         << " ms of GPU kernels";
    say(line.str());
    return true;
  };
  // the small holes of all views filled on the first device: behind the speckle filter, so that a removed island is refilled from
  // its surroundings, and in front of the consistency filter, so that every invented depth still has to be confirmed
  auto fill_views = [&]() {
    say("** Fill the small holes of the depth maps...");
    if (!read_views("--depthFillHolesMaxPixels")) return false;
    DepthHolesReport report;
    std::string error;
    if (!run_step("--depthFillHolesMaxPixels",
                  [&]() { return resident.FillHoles(o.depthFillHolesMaxPixels, o.depthFillHolesTolerance, o.depthFillHolesRelTolerance, &report); },
                  [&](std::string *why) {
                    return FillDepthHoles(views, o.threshBestCost, o.depthFillHolesMaxPixels, o.depthFillHolesTolerance,
                                          o.depthFillHolesRelTolerance, stepDevice, &report, why);
                  },
                  &error)) {
      result->error = "--depthFillHolesMaxPixels: " + error;
      return false;
    }
    result->depthFillHolesViews = report.views;
    result->depthFillHolesHoles = report.holes;
    result->depthFillHolesFilledHoles = report.filledHoles;
    result->depthFillHolesFilledPixels = report.filledPixels;
    result->depthFillHolesKernelMs = report.kernelMs;
    std::ostringstream line;
    line << "depth holes: holes of at most " << o.depthFillHolesMaxPixels << " pixels, tolerance " << o.depthFillHolesTolerance << " + "
         << o.depthFillHolesRelTolerance << " z; " << report.views << " views, " << report.holes << " holes, " << report.filledHoles
         << " filled; " << report.filledPixels << " pixels filled; " << report.kernelMs << " ms of GPU kernels";
    say(line.str());
    return true;
  };
  // the depths of all views smoothed on the first device: behind the hole fill, so that invented depths are smoothed with their
  // surroundings, and in front of the consistency filter, so that every smoothed depth still has to be confirmed
  auto smooth_views = [&]() {
    say("** Smooth the depth maps...");
    if (!read_views("--depthSmoothSigma")) return false;
    DepthSmoothReport report;
    std::string error;
    if (!run_step("--depthSmoothSigma",
                  [&]() {
                    return resident.Smooth(o.depthSmoothSigma, o.depthSmoothTruncate, o.depthSmoothTolerance, o.depthSmoothRelTolerance,
                                           (int)o.depthSmoothIterations, &report);
                  },
                  [&](std::string *why) {
                    return SmoothDepths(views, o.threshBestCost, o.depthSmoothSigma, o.depthSmoothTruncate, o.depthSmoothTolerance,
                                        o.depthSmoothRelTolerance, (int)o.depthSmoothIterations, stepDevice, &report, why);
                  },
                  &error)) {
      result->error = "--depthSmoothSigma: " + error;
      return false;
    }
    result->depthSmoothViews = report.views;
    result->depthSmoothValidPixels = report.validPixels;
    result->depthSmoothChangedPixels = report.changedPixels;
    result->depthSmoothMeanTaps = report.meanTaps;
    result->depthSmoothKernelMs = report.kernelMs;
    std::ostringstream line;
    line << "depth smoothing: sigma " << o.depthSmoothSigma << " pixels, truncate " << o.depthSmoothTruncate << ", tolerance "
         << o.depthSmoothTolerance << " + " << o.depthSmoothRelTolerance << " z, " << o.depthSmoothIterations << " iterations; "
         << report.views << " views, " << report.validPixels << " pixels with a depth, " << report.changedPixels << " changed; "
         << report.meanTaps << " taps per pixel; " << report.kernelMs << " ms of GPU kernels";
    say(line.str());
    return true;
  };
  // all views filtered on the first device
  auto filter_views = [&]() {
    say("** Filter the depth maps by cross-view consistency...");
    if (!read_views("--depthConsistencyMinViews")) return false;
    DepthConsistencyReport report;
    std::string error;
    if (!run_step("--depthConsistencyMinViews",
                  [&]() {
                    return resident.FilterConsistency((int)o.depthConsistencyMinViews, o.depthConsistencyTolerance,
                                                      o.depthConsistencyRelTolerance, &report);
                  },
                  [&](std::string *why) {
                    return FilterDepthConsistency(views, o.threshBestCost, (int)o.depthConsistencyMinViews, o.depthConsistencyTolerance,
                                                  o.depthConsistencyRelTolerance, stepDevice, &report, why);
                  },
                  &error)) {
      result->error = "--depthConsistencyMinViews: " + error;
      return false;
    }
    result->depthConsistencyViews = report.views;
    result->depthConsistencyValidPixels = report.validPixels;
    result->depthConsistencyKeptPixels = report.keptPixels;
    result->depthConsistencyKernelMs = report.kernelMs;
    std::ostringstream line;
    line << "depth consistency: at least " << o.depthConsistencyMinViews << " of " << report.views - 1 << " other views, tolerance "
         << o.depthConsistencyTolerance << " + " << o.depthConsistencyRelTolerance << " z; " << report.validPixels
         << " pixels with a depth, " << report.keptPixels << " kept; " << report.kernelMs << " ms of GPU kernels";
    say(line.str());
    return true;
  };
  // the point cloud of the depth maps that are fused: built on the resident set behind the last depth-map step, written at once
  auto point_cloud = [&]() {
    say("** Build the point cloud of the depth maps...");
    const std::string flag = "--outputPointCloudFilename";
    if (!read_views(flag)) return false;
    if (!on_set() || !resident.Loaded()) {
      result->error = flag + ": the points are built on the resident depth maps, and " +
                      (staged ? "the staged filters have taken over (" + resident.LastError() + ")" : resident.LastError());
      return false;
    }
    DepthPointsReport report;
    DepthThinReport thinned;
    DepthRadiusReport sifted;
    DepthPlaneFitReport fitted;
    double fit_ms = 0.0;
    auto fit_planes = [&]() {  // each pass on the result of the one before; the report is the last one's
      for (long long pass = 0; pass < o.pointCloudPlaneFitIterations; ++pass) {
        if (!resident.FitPointPlanes(o.pointCloudPlaneFitRadius, (int)o.pointCloudPlaneFitMinNeighbors, !o.pointCloudPlaneFitKeepPositions,
                                     !o.pointCloudPlaneFitKeepNormals, &fitted))
          return false;
        fit_ms += fitted.kernelMs;
      }
      return true;
    };
    DepthPoints points;
    if (!resident.BuildPoints(o.pointCloudTolerance, o.pointCloudRelTolerance, o.pointCloudNormalTolerance, o.pointCloudNormalRelTolerance,
                              (int)o.pointCloudMinViews, (int)o.pointCloudPixelStep, !o.pointCloudKeepDuplicates, &report) ||
        (o.pointCloudOutlierRadiusGiven &&
         !resident.FilterPointsRadius(o.pointCloudOutlierRadius, (int)o.pointCloudMinNeighbors, &sifted)) ||  // strays never become cells
        (o.pointCloudPlaneFitRadiusGiven && !fit_planes()) ||  // ... nor pull a plane; the cells then average denoised points
        (o.pointCloudCellSizeGiven && !resident.ThinPoints(o.pointCloudCellSize, (int)o.pointCloudMinCellPoints, &thinned)) ||
        !resident.DownloadPoints(&points)) {
      result->error = flag + ": " + resident.LastError();
      return false;
    }
    std::vector<uint8_t> color;
    if (o.pointCloudColors) {  // each point's pixel of its view's Color array: image row py is vtk row H-1-py
      const int64_t W = resident.Width(), H = resident.Height();
      for (size_t m = 0; m < views.size(); ++m)
        if (views[m]->GetDepthMap()->color.size() != (size_t)(W * H * 3)) {
          result->error = "--pointCloudColors: view " + std::to_string(m) + " has no Color array of three UInt8 per pixel";
          return false;
        }
      color.resize(3 * points.view.size());
      for (size_t q = 0; q < points.view.size(); ++q) {
        const int64_t py = points.pixel[q] / W, px = points.pixel[q] - py * W;
        const unsigned char *const rgb = views[(size_t)points.view[q]]->GetDepthMap()->color.data() + 3 * ((H - 1 - py) * W + px);
        std::copy(rgb, rgb + 3, color.begin() + 3 * (std::ptrdiff_t)q);
      }
    }
    std::string error;
    if (!WritePointCloud(o.outputPointCloudFilename, points.xyz.data(), (int64_t)points.view.size(), points.normal.data(), points.view.data(),
                         points.count.data(), o.pointCloudColors ? color.data() : nullptr, &error,
                         o.pointCloudCellSizeGiven ? points.members.data() : nullptr,
                         o.pointCloudOutlierRadiusGiven && !o.pointCloudCellSizeGiven ? points.neighbors.data() : nullptr,
                         o.pointCloudPlaneFitRadiusGiven && !o.pointCloudCellSizeGiven ? points.plane_rms.data() : nullptr)) {
      result->error = error;
      return false;
    }
    result->pointCloudViews = report.views;
    result->pointCloudValidPixels = report.validPixels;
    result->pointCloudCandidates = report.candidates;
    result->pointCloudOwned = report.owned;
    result->pointCloudPoints = report.points;
    result->pointCloudWithNormal = report.withNormal;
    result->pointCloudKernelMs = report.kernelMs;
    std::ostringstream line;
    line << "point cloud: at least " << o.pointCloudMinViews << " agreeing views, tolerance " << o.pointCloudTolerance << " + "
         << o.pointCloudRelTolerance << " z, normal tolerance " << o.pointCloudNormalTolerance << " + " << o.pointCloudNormalRelTolerance
         << " z, pixel step " << o.pointCloudPixelStep << (o.pointCloudKeepDuplicates ? ", duplicates kept; " : "; ") << report.views
         << " views, " << report.validPixels << " pixels with a depth, " << report.candidates << " candidates, " << report.owned
         << " held by a lower view, " << report.points << " points, " << report.withNormal << " with a normal; " << report.kernelMs
         << " ms of GPU kernels";
    say(line.str());
    if (o.pointCloudOutlierRadiusGiven) {
      result->pointCloudRadiusPointsIn = sifted.pointsIn;
      result->pointCloudRadiusPointsKept = sifted.pointsKept;
      result->pointCloudRadiusIsolated = sifted.isolated;
      result->pointCloudRadiusMaxNeighbors = sifted.maxNeighbors;
      result->pointCloudRadiusNeighborSum = sifted.neighborSum;
      result->pointCloudRadiusDistanceTests = sifted.distanceTests;
      result->pointCloudRadiusKernelMs = sifted.kernelMs;
      std::ostringstream sift;
      sift << "point cloud outliers: radius " << o.pointCloudOutlierRadius << ", at least " << o.pointCloudMinNeighbors << " neighbours; "
           << sifted.pointsIn << " points, " << sifted.pointsKept << " kept, " << sifted.isolated << " without a neighbour, at most "
           << sifted.maxNeighbors << " neighbours, " << sifted.neighborSum << " in all from " << sifted.distanceTests
           << " distance tests; " << sifted.kernelMs << " ms of GPU kernels";
      say(sift.str());
    }
    if (o.pointCloudPlaneFitRadiusGiven) {
      result->pointCloudPlaneFitPointsIn = fitted.pointsIn;
      result->pointCloudPlaneFitFitted = fitted.fitted;
      result->pointCloudPlaneFitUnsupported = fitted.unsupported;
      result->pointCloudPlaneFitCrowded = fitted.crowded;
      result->pointCloudPlaneFitMaxNeighbors = fitted.maxNeighbors;
      result->pointCloudPlaneFitNeighborSum = fitted.neighborSum;
      result->pointCloudPlaneFitDistanceTests = fitted.distanceTests;
      result->pointCloudPlaneFitMaxShift = fitted.maxShift;
      result->pointCloudPlaneFitKernelMs = fit_ms;
      std::ostringstream fit;
      fit << "point cloud plane fit: radius " << o.pointCloudPlaneFitRadius << ", at least " << o.pointCloudPlaneFitMinNeighbors
          << " neighbours, " << o.pointCloudPlaneFitIterations << " passes"
          << (o.pointCloudPlaneFitKeepPositions ? ", positions kept" : o.pointCloudPlaneFitKeepNormals ? ", normals kept" : "") << "; "
          << fitted.pointsIn << " points, " << fitted.fitted << " fitted, " << fitted.unsupported << " with too few neighbours, "
          << fitted.crowded << " crowded, at most " << fitted.maxNeighbors << " neighbours, " << fitted.neighborSum << " in all from "
          << fitted.distanceTests << " distance tests, the largest shift " << fitted.maxShift << "; " << fit_ms << " ms of GPU kernels";
      say(fit.str());
    }
    if (o.pointCloudCellSizeGiven) {
      result->pointCloudCells = thinned.cells;
      result->pointCloudCellsKept = thinned.cellsKept;
      result->pointCloudMultiViewCells = thinned.multiViewCells;
      result->pointCloudLargestCell = thinned.largestCell;
      result->pointCloudThinnedWithNormal = thinned.withNormal;
      result->pointCloudThinKernelMs = thinned.kernelMs;
      std::ostringstream thin;
      thin << "point cloud thinning: cells of " << o.pointCloudCellSize << ", at least " << o.pointCloudMinCellPoints << " points; "
           << thinned.pointsIn << " points in " << thinned.cells << " cells, " << thinned.cellsKept << " kept, " << thinned.multiViewCells
           << " fed by more than one view, the largest of " << thinned.largestCell << " points, " << thinned.withNormal
           << " with a normal; " << thinned.kernelMs << " ms of GPU kernels";
      say(thin.str());
    }
    return true;
  };
  if (o.gridAutoBounds) {
    // the box before anything is described or set up: filtered depths if a filter was asked for, measured along the grid's axes
    if (o.depthSpeckleMinPixels >= 0 && !speckle_views()) return 1;
    if (o.depthFillHolesMaxPixels >= 0 && !fill_views()) return 1;
    if (o.depthSmoothSigmaGiven && !smooth_views()) return 1;
    if (o.depthConsistencyMinViews >= 0 ? !filter_views() : !read_views("--gridAutoBounds")) return 1;
    say("** Estimate the grid's bounds from the depth maps...");
    // axes[j][i] = M[i][j] / |row_i|^2, M's rows the grid's axes: the inverse of the grid matrix for orthogonal rows, so that the
    // bounds are in the coordinates --gridOrigin uses
    const std::vector<double> *rows[3] = {&o.gridVecX, &o.gridVecY, &o.gridVecZ};
    double axes[9];
    for (int i = 0; i < 3; ++i) {
      const double norm2 = dot3(*rows[i], *rows[i]);
      for (int j = 0; j < 3; ++j) axes[j * 3 + i] = (*rows[i])[(size_t)j] / norm2;
    }
    for (const double v : axes)
      if (!std::isfinite(v)) {
        result->error = "--gridAutoBounds: an axis of the grid has no length";
        return 1;
      }
    SceneBoundsReport bounds;
    std::string error;
    if (!run_step("--gridAutoBounds",
                  [&]() { return resident.EstimateBounds(axes, o.gridAutoBoundsTrim, (int)o.gridAutoBoundsPixelStep, &bounds); },
                  [&](std::string *why) {
                    return EstimateSceneBounds(views, o.threshBestCost, axes, o.gridAutoBoundsTrim, (int)o.gridAutoBoundsPixelStep, stepDevice,
                                               &bounds, why);
                  },
                  &error)) {
      result->error = "--gridAutoBounds: " + error;
      return 1;
    }
    if (bounds.points == 0) {
      result->error = "--gridAutoBounds: no pixel of the depth maps holds a depth, there is nothing to put a box around";
      return 1;
    }
    resolved.gridOrigin.resize(3);
    resolved.gridEnd.resize(3);
    for (int a = 0; a < 3; ++a) {
      if (bounds.hi[a] == bounds.lo[a]) {
        result->error = "--gridAutoBounds: the depth maps' points have no extent along axis " + std::to_string(a) + " of the grid";
        return 1;
      }
      const double pad = o.gridAutoBoundsMargin * (bounds.hi[a] - bounds.lo[a]);
      resolved.gridOrigin[(size_t)a] = bounds.lo[a] - pad;
      resolved.gridEnd[(size_t)a] = bounds.hi[a] + pad;
      result->gridAutoBoundsLo[a] = bounds.lo[a];
      result->gridAutoBoundsHi[a] = bounds.hi[a];
    }
    derive_spacing_or_dimensions(&resolved);
    result->gridAutoBoundsPoints = bounds.points;
    result->gridAutoBoundsKernelMs = bounds.kernelMs;
    std::ostringstream line;
    line.precision(17);
    line << "grid bounds: trim " << o.gridAutoBoundsTrim << ", margin " << o.gridAutoBoundsMargin << ", pixel step "
         << o.gridAutoBoundsPixelStep << "; " << bounds.points << " points of " << bounds.views << " views; trimmed bounds " << bounds.lo[0]
         << " " << bounds.lo[1] << " " << bounds.lo[2] << " to " << bounds.hi[0] << " " << bounds.hi[1] << " " << bounds.hi[2]
         << "; --gridOrigin " << o.gridOrigin[0] << " " << o.gridOrigin[1] << " " << o.gridOrigin[2] << " --gridEnd " << o.gridEnd[0]
         << " " << o.gridEnd[1] << " " << o.gridEnd[2] << "; " << bounds.kernelMs << " ms of GPU kernels";
    say(line.str());
  }
  for (int a = 0; a < 3; ++a) {
    result->gridOrigin[a] = o.gridOrigin[(size_t)a];
    result->gridEnd[a] = o.gridEnd[(size_t)a];
    result->gridSpacing[a] = o.gridSpacing[(size_t)a];
    result->gridDims[a] = o.gridDims[(size_t)a];
  }
  if (o.verbose) describe(o, log, true);
  double matrix[16];
  CreateGridMatrixFromInput(o, matrix);

  say("** Launch reconstruction...");
  ReconstructionFilter filter;
  filter.SetFilePathKRTD(krtd_list.c_str());
  filter.SetFilePathVTI(vti_list.c_str());
  filter.SetRayPotentialRho(o.rayRho);
  filter.SetRayPotentialThickness(o.rayThick);
  filter.SetRayPotentialEta(o.rayEta);
  filter.SetRayPotentialDelta(o.rayDelta);
  filter.SetThresholdBestCost(o.threshBestCost);
  const int dims[3] = {o.gridDims[0], o.gridDims[1], o.gridDims[2]};
  const double origin[3] = {o.gridOrigin[0], o.gridOrigin[1], o.gridOrigin[2]};
  const double spacing[3] = {o.gridSpacing[0], o.gridSpacing[1], o.gridSpacing[2]};
  filter.SetInputData(dims, origin, spacing);
  filter.SetGridMatrix(matrix);
  if (o.devices.size() == 1) filter.SetDevice(o.devices[0]);
  if (o.devices.size() > 1) filter.SetDevices(o.devices);
  // --meshColoration: the driver hands every chunk's Color planes to this context while it reads the files, and keeps its fusion
  // context (the views' thresholded depths stay resident for the fused visibility test; the mesh is extracted in it)
  struct ColorContextHolder {
    dmi_color_context *c = nullptr;
    ~ColorContextHolder() {
      if (c) dmi_color_destroy(c);
    }
  } coloring;
  if (o.meshColoration) {
    if (dmi_color_create(o.devices.empty() ? 0 : o.devices[0], &coloring.c) != DMI_OK) {
      result->error = std::string("--meshColoration: ") + dmi_color_last_error();
      return 1;
    }
    filter.SetColorSink(coloring.c);
    filter.SetKeepContext(true);
  }
  // the support trim and the support array read the depths the fusion kept: the same context, its views resident
  const bool supportMesh = o.meshMinSupportViews >= 0 || o.meshSupportArray;
  const bool supportFacing = supportMesh && !o.meshSupportNoFacing;
  if (supportMesh) filter.SetKeepContext(true);
  if (o.depthSpeckleMinPixels >= 0 && !o.gridAutoBounds && !speckle_views()) return 1;
  if (o.depthFillHolesMaxPixels >= 0 && !o.gridAutoBounds && !fill_views()) return 1;
  if (o.depthSmoothSigmaGiven && !o.gridAutoBounds && !smooth_views()) return 1;
  if (o.depthConsistencyMinViews >= 0 && !o.gridAutoBounds && !filter_views()) return 1;
  if (!o.outputPointCloudFilename.empty() && !point_cloud()) return 1;
  if (!views.empty()) filter.SetViews(views);
  if (resident.Loaded()) filter.SetResidentViews(&resident);
  if (!filter.Update()) {
    result->error = filter.LastError().empty() ? "the reconstruction filter refused its parameters" : filter.LastError();
    return 1;
  }
  result->reconstructionSeconds = filter.GetExecutionTime();
  say("Reconstruction execution time : " + std::to_string(result->reconstructionSeconds) + " s");

  say("** Transform cell data to point data...");
  const std::vector<double> &cells = filter.GetOutputScalars();
  std::vector<double> points((size_t)dims[0] * dims[1] * dims[2]);
  std::vector<double> meshVertices;    // --extractMesh
  std::vector<int64_t> meshTriangles;
  std::vector<float> meshNormals;      // --meshNormals
  std::vector<int64_t> meshRegionIds;  // --meshRegionIds
  const bool filterMesh = o.meshMinComponentTriangles >= 0 || o.meshLargestComponent || o.meshRegionIds;
  double dummyVertex = 0.0;            // a valid pointer for an empty mesh
  int64_t dummyTriangle = 0;
  float dummyNormal = 0.f;
  int64_t dummyRegion = 0;
  std::vector<uint8_t> meshMean, meshMedian;  // --meshColoration
  std::vector<int32_t> meshCount;
  uint8_t dummyRgb[3] = {0, 0, 0};
  int32_t dummyCount = 0;
  std::vector<int32_t> meshSupport;  // --meshSupportArray
  {
    // vtkCellDataToPointData (rmain:151-155) on the GPU: the cell grid goes up once more, the point grid comes back
    dmi_grid_desc grid;
    std::memset(&grid, 0, sizeof(grid));
    for (int a = 0; a < 3; ++a) {
      grid.cell_dims[a] = dims[a] - 1;
      grid.origin[a] = origin[a];
      grid.spacing[a] = spacing[a];
    }
    std::memcpy(grid.grid_matrix, matrix, sizeof(matrix));
    dmi_ray_potential ray = {o.rayThick, o.rayRho, o.rayEta, o.rayDelta};
    dmi_options opt;
    dmi_default_options(&opt);
    opt.device = o.devices.empty() ? 0 : o.devices[0];
    opt.grid_dtype = DMI_F64;
    // (with --meshColoration: the context that fused, its views resident; the grid goes up the same way, so that every array
    // written is what it is without the flag)
    dmi_context *ctx = o.meshColoration || supportMesh ? filter.TakeContext() : nullptr;  // (destroyed below like a fresh one)
    int rc = ctx ? DMI_OK : dmi_create(&grid, &ray, &opt, &ctx);
    if (rc == DMI_OK) rc = dmi_upload_grid(ctx, cells.data());
    if (rc == DMI_OK) rc = dmi_cell_to_point(ctx);
    if (rc == DMI_OK) rc = dmi_download_point_data_f64(ctx, points.data());
    // the contour filter's pre-pass (rmain:169-173): the cells whose corners straddle --contour
    uint64_t active = 0;
    if (rc == DMI_OK) rc = dmi_iso_active_cells(ctx, o.contour, &active, nullptr, 0);
    result->contourActiveCells = active;
    if (rc != DMI_OK) result->error = std::string("cell data -> point data: ") + dmi_last_error(ctx);
    if (rc == DMI_OK && o.extractMesh) {
      // vtkContourFilter + vtkTransformFilter (rmain:166-182) on the device; vtkXMLPolyDataWriter (rmain:184-187) below
      uint64_t nv = 0, nt = 0;
      // --contourSmoothSigma: set here, behind the download and the pre-pass above, so that the volume files and the count of
      // active cells are what they are without the flag; the extraction recomputes the point data and smooths it
      const bool contourSmooth = contourSmoothed(o);
      if (contourSmooth) {
        rc = dmi_set_point_smoothing(ctx, o.contourSmoothSigma.data(), o.contourSmoothTruncate);
        double weights[17];
        for (int a = 0; a < 3; ++a)  // (the radii, for the log: the parser has checked the parameters)
          (void)dmi::point_smoothing_weights(o.contourSmoothSigma[(size_t)a], o.contourSmoothTruncate, &result->contourSmoothRadius[a], weights);
      }
      // (the facing test needs the normals whether they are written or not)
      if (rc == DMI_OK) rc = o.meshNormals || supportFacing ? dmi_extract_isosurface_normals(ctx, o.contour, &nv, &nt) : dmi_extract_isosurface(ctx, o.contour, &nv, &nt);
      if (rc == DMI_OK && contourSmooth) rc = dmi_get_point_smoothing_kernel_ms(ctx, &result->contourSmoothKernelMs);
      if (rc == DMI_OK && o.meshMinSupportViews > 0) {  // first: the fragments it leaves are the component flags' to remove
        result->meshVerticesBeforeSupport = nv;
        result->meshTrianglesBeforeSupport = nt;
        rc = dmi_filter_isosurface_support(ctx, (int32_t)std::min(o.meshMinSupportViews, 0x7fffffffLL), o.meshSupportDepthTolerance,
                                           supportFacing ? 1 : 0, &nv, &nt);
        if (rc == DMI_OK) rc = dmi_get_isosurface_support_kernel_ms(ctx, &result->meshSupportKernelMs);
      }
      if (supportMesh) {
        dmi_info info;
        if (rc == DMI_OK && dmi_get_info(ctx, &info) == DMI_OK) result->meshSupportViews = (unsigned long long)info.n_views;
      }
      result->meshVerticesExtracted = nv;
      result->meshTrianglesExtracted = nt;
      if (rc == DMI_OK && filterMesh) {
        // vtkPolyDataConnectivityFilter's part, on the device before anything is downloaded: by size, then the largest; with
        // --meshRegionIds alone everything is kept and only labelled
        uint64_t found = 0, kept = 0, found2 = 0;
        if (o.meshMinComponentTriangles >= 0 || !o.meshLargestComponent)
          rc = dmi_filter_isosurface_components(ctx, DMI_COMPONENTS_MIN_TRIANGLES, (uint64_t)std::max(o.meshMinComponentTriangles, 0LL),
                                                &nv, &nt, &found, &kept);
        if (rc == DMI_OK && o.meshLargestComponent) {
          const bool first = o.meshMinComponentTriangles < 0;
          rc = dmi_filter_isosurface_components(ctx, DMI_COMPONENTS_LARGEST, 0, &nv, &nt, first ? &found : &found2, &kept);
        }
        result->meshComponents = found;
        result->meshComponentsKept = kept;
      }
      if (rc == DMI_OK && o.meshFillHoles > 0) {  // behind the trim and the component flags: the smoothing then moves the former rims
        uint64_t filled = 0, left = 0;
        rc = dmi_fill_isosurface_holes(ctx, (uint64_t)o.meshFillHoles, &nv, &nt, &filled, &left);
        if (rc == DMI_OK) rc = dmi_get_isosurface_holes_kernel_ms(ctx, &result->meshFillHolesKernelMs);
        result->meshHolesFilled = filled;
        result->meshBoundaryEdgesLeft = left;
        // the fill has dropped the regions: labelled anew, nothing dropped (behind a decimation that happens there)
        if (rc == DMI_OK && o.meshRegionIds && filled > 0 && !(o.meshDecimateCellSize > 0)) {
          uint64_t found = 0, kept = 0;
          rc = dmi_filter_isosurface_components(ctx, DMI_COMPONENTS_MIN_TRIANGLES, 0, &nv, &nt, &found, &kept);
        }
      }
      if (rc == DMI_OK && o.meshSmoothIterations > 0) {  // on the mesh the component flags left, before anything is downloaded
        rc = dmi_smooth_isosurface(ctx, (int32_t)o.meshSmoothIterations, o.meshSmoothLambda, o.meshSmoothMu);
        if (rc == DMI_OK) rc = dmi_get_isosurface_smooth_kernel_ms(ctx, &result->meshSmoothKernelMs);
      }
      if (rc == DMI_OK && o.meshDecimateCellSize > 0) {  // last: on the mesh the component flags and the smoothing left
        result->meshVerticesBeforeDecimation = nv;
        result->meshTrianglesBeforeDecimation = nt;
        rc = o.meshDecimateQuadric ? dmi_decimate_isosurface_placed(ctx, o.meshDecimateCellSize, DMI_DECIMATE_QUADRIC, &nv, &nt)
                                   : dmi_decimate_isosurface(ctx, o.meshDecimateCellSize, &nv, &nt);
        if (rc == DMI_OK) rc = dmi_get_isosurface_decimate_kernel_ms(ctx, &result->meshDecimateKernelMs);
        if (rc == DMI_OK && o.meshRegionIds) {  // a cluster may have joined components: RegionId is labelled anew, nothing dropped
          uint64_t found = 0, kept = 0;
          rc = dmi_filter_isosurface_components(ctx, DMI_COMPONENTS_MIN_TRIANGLES, 0, &nv, &nt, &found, &kept);
        }
      }
      if (rc == DMI_OK && o.meshSupportArray) {  // the counts of the mesh as it will be written: nothing changes it from here on
        uint64_t same_nv = 0, same_nt = 0;
        rc = dmi_filter_isosurface_support(ctx, 0, o.meshSupportDepthTolerance, supportFacing ? 1 : 0, &same_nv, &same_nt);
        if (rc == DMI_OK) {
          meshSupport.resize((size_t)nv);
          rc = dmi_download_isosurface_support(ctx, meshSupport.data() ? meshSupport.data() : &dummyCount);
        }
      }
      if (rc == DMI_OK && o.meshColoration) {  // last of all: the mesh as it will be written, where it is
        uint64_t colored = 0;
        if (o.meshColorationDepthFromMesh) {
          // the mesh's own z-buffer in the colour context's planes, then the colour context's own test against them
          rc = dmi_color_render_isosurface_depths(coloring.c, ctx);
          // (neither of the next two can fail on a context that has just rendered and a tolerance the parser has checked)
          if (rc == DMI_OK) rc = dmi_color_get_render_kernel_ms(coloring.c, &result->meshColorationRenderKernelMs);
          if (rc == DMI_OK) rc = dmi_color_set_depth_test(coloring.c, 1, o.meshColorationDepthTolerance);
          if (rc == DMI_OK) rc = dmi_color_process_isosurface(coloring.c, ctx, 0, 0.0, &colored);
        } else {
          rc = dmi_color_process_isosurface(coloring.c, ctx, o.meshColorationDepthToleranceGiven ? 1 : 0, o.meshColorationDepthTolerance, &colored);
        }
        if (rc == DMI_OK) rc = dmi_get_isosurface_color_kernel_ms(ctx, &result->meshColorationKernelMs);
        if (rc == DMI_OK) {
          meshMean.resize((size_t)nv * 3);
          meshMedian.resize((size_t)nv * 3);
          meshCount.resize((size_t)nv);
          rc = dmi_download_isosurface_colors(ctx, meshMean.data(), meshMedian.data(), meshCount.data());
        }
        dmi_info info;
        if (rc == DMI_OK && dmi_get_info(ctx, &info) == DMI_OK) result->meshColorationViews = (unsigned long long)info.n_views;
      }
      if (rc == DMI_OK) {
        meshVertices.resize((size_t)nv * 3);
        meshTriangles.resize((size_t)nt * 3);
        rc = dmi_download_isosurface(ctx, meshVertices.data() ? meshVertices.data() : &dummyVertex,
                                     meshTriangles.data() ? meshTriangles.data() : &dummyTriangle);
      }
      if (rc == DMI_OK && o.meshNormals) {
        meshNormals.resize((size_t)nv * 3);
        rc = dmi_download_isosurface_normals(ctx, meshNormals.data() ? meshNormals.data() : &dummyNormal);
      }
      if (rc == DMI_OK && o.meshRegionIds) {
        meshRegionIds.resize((size_t)nv);
        rc = dmi_download_isosurface_regions(ctx, meshRegionIds.data() ? meshRegionIds.data() : &dummyRegion, nullptr);
      }
      if (rc != DMI_OK) result->error = std::string("iso-surface: ") + dmi_last_error(ctx);
      result->meshVertices = nv;
      result->meshTriangles = nt;
    }
    if (ctx) dmi_destroy(ctx);
    if (rc != DMI_OK) return 1;
  }
  std::string error;
  if (!WriteMetaImage("meta_image_volume.mha", dims, origin, spacing, points.data(), &error)) {  // rmain:157-161: that name, here
    result->error = error;
    return 1;
  }
  if (o.extractMesh) {
    say("** Save mesh...");
    if (!WritePolyData(o.outputMeshFilename, meshVertices.data(), (int64_t)result->meshVertices, meshTriangles.data(),
                       (int64_t)result->meshTriangles, &error, o.meshNormals ? (meshNormals.empty() ? &dummyNormal : meshNormals.data()) : nullptr, o.contour,
                       o.meshRegionIds ? (meshRegionIds.empty() ? &dummyRegion : meshRegionIds.data()) : nullptr,
                       o.meshColoration ? (meshMean.empty() ? dummyRgb : meshMean.data()) : nullptr,
                       o.meshColoration ? (meshMedian.empty() ? dummyRgb : meshMedian.data()) : nullptr,
                       o.meshColoration ? (meshCount.empty() ? &dummyCount : meshCount.data()) : nullptr,
                       o.meshSupportArray ? (meshSupport.empty() ? &dummyCount : meshSupport.data()) : nullptr)) {
      result->error = error;
      return 1;
    }
    // said whatever --verbose is, like the warning below without the flag
    log << "mesh: " << o.outputMeshFilename << ": " << result->meshVertices << " vertices, " << result->meshTriangles
        << " triangles at the contour value " << o.contour << " (" << result->contourActiveCells << " of "
        << (long long)(dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1) << " cells straddle it)" << std::endl;
    if (contourSmoothed(o))
      log << "contour smoothing: sigma " << o.contourSmoothSigma[0] << " " << o.contourSmoothSigma[1] << " " << o.contourSmoothSigma[2]
          << " voxels, truncate " << o.contourSmoothTruncate << ", radii " << result->contourSmoothRadius[0] << " "
          << result->contourSmoothRadius[1] << " " << result->contourSmoothRadius[2] << "; " << result->contourSmoothKernelMs
          << " ms of GPU kernels" << std::endl;
    if (o.meshMinSupportViews > 0)
      log << "mesh support: at least " << o.meshMinSupportViews << " of " << result->meshSupportViews << " views, depth tolerance "
          << o.meshSupportDepthTolerance << (supportFacing ? ", facing" : ", any facing") << "; " << result->meshVerticesBeforeSupport
          << " vertices, " << result->meshTrianglesBeforeSupport << " triangles before, " << result->meshVerticesExtracted << " vertices, "
          << result->meshTrianglesExtracted << " triangles after; " << result->meshSupportKernelMs << " ms of GPU kernels" << std::endl;
    if (filterMesh)
      log << "mesh components: " << result->meshComponents << " found, " << result->meshComponentsKept << " kept; "
          << result->meshVerticesExtracted << " vertices, " << result->meshTrianglesExtracted << " triangles before, "
          << result->meshVertices << " vertices, " << result->meshTriangles << " triangles after" << std::endl;
    if (o.meshFillHoles > 0)
      log << "mesh holes: at most " << o.meshFillHoles << " edges; " << result->meshHolesFilled << " filled, "
          << result->meshBoundaryEdgesLeft << " boundary edges left; " << result->meshFillHolesKernelMs << " ms of GPU kernels" << std::endl;
    if (o.meshSmoothIterations > 0)
      log << "mesh smoothing: " << o.meshSmoothIterations << " iterations, lambda " << o.meshSmoothLambda << ", mu " << o.meshSmoothMu
          << "; " << result->meshSmoothKernelMs << " ms of GPU kernels" << std::endl;
    if (o.meshDecimateCellSize > 0)
      log << "mesh decimation: cell size " << o.meshDecimateCellSize << (o.meshDecimateQuadric ? ", quadric placement" : "") << "; "
          << result->meshVerticesBeforeDecimation << " vertices, "
          << result->meshTrianglesBeforeDecimation << " triangles before, " << result->meshVertices << " vertices, "
          << result->meshTriangles << " triangles after; " << result->meshDecimateKernelMs << " ms of GPU kernels" << std::endl;
    if (o.meshColoration) {
      log << "mesh coloration: " << result->meshVertices << " vertices, " << result->meshColorationViews << " views, depth tolerance ";
      if (o.meshColorationDepthToleranceGiven) log << o.meshColorationDepthTolerance; else log << "none";
      if (o.meshColorationDepthFromMesh) log << " against the mesh's own rendered depth (" << result->meshColorationRenderKernelMs << " ms of GPU kernels to render)";
      log << "; " << result->meshColorationKernelMs << " ms of GPU kernels" << std::endl;
    }
  } else {
    // Said whatever --verbose is: the reference writes a mesh here (rmain:166-187) and this tool does not.
    log << "warning: " << o.outputMeshFilename << " is NOT written: the iso-surface (vtkContourFilter) is not part of this tool; "
        << result->contourActiveCells << " of " << (long long)(dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1)
        << " cells straddle the contour value " << o.contour << std::endl;
  }
  say("** Save volume...");
  if (!WriteStructuredGrid(o.outputGridFilename, dims, origin, spacing, matrix, cells.data(), ReconstructionFilter::OutputArrayName(),
                           &error)) {
    result->error = error;
    return 1;
  }
  result->totalSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
  if (o.summary) {  // rmain:201-206, 458-516
    say("** Save summary file...");
    std::ofstream out(o.dataFolder + "/summary.txt");
    out << "command line\n ";
    for (int i = 0; i < argc; ++i) out << " " << argv[i];
    out << "\noutput volume  " << o.outputGridFilename << "\n";
    describe(o, out, false);
    if (o.gridAutoBounds) {
      const std::streamsize digits = out.precision(17);
      out << "grid bounds from the depth maps\n  trim  " << o.gridAutoBoundsTrim << "\n  margin  " << o.gridAutoBoundsMargin
          << "\n  pixel step  " << o.gridAutoBoundsPixelStep << "\n  points  " << result->gridAutoBoundsPoints << "\n  trimmed lower bounds  "
          << result->gridAutoBoundsLo[0] << " " << result->gridAutoBoundsLo[1] << " " << result->gridAutoBoundsLo[2]
          << "\n  trimmed upper bounds  " << result->gridAutoBoundsHi[0] << " " << result->gridAutoBoundsHi[1] << " "
          << result->gridAutoBoundsHi[2] << "\n  --gridOrigin  " << o.gridOrigin[0] << " " << o.gridOrigin[1] << " " << o.gridOrigin[2]
          << "\n  --gridEnd  " << o.gridEnd[0] << " " << o.gridEnd[1] << " " << o.gridEnd[2] << "\n  GPU kernels  "
          << result->gridAutoBoundsKernelMs << " ms\n";
      out.precision(digits);
    }
    if (o.depthSpeckleMinPixels >= 0)
      out << "depth speckles\n  minimum segment pixels  " << o.depthSpeckleMinPixels << "\n  tolerance  " << o.depthSpeckleTolerance << " + "
          << o.depthSpeckleRelTolerance << " z\n  views  " << result->depthSpeckleViews << "\n  pixels with a depth  "
          << result->depthSpeckleValidPixels << "\n  pixels kept  " << result->depthSpeckleKeptPixels << "\n  segments  "
          << result->depthSpeckleSegments << "\n  segments kept  " << result->depthSpeckleKeptSegments << "\n  GPU kernels  "
          << result->depthSpeckleKernelMs << " ms\n";
    if (o.depthFillHolesMaxPixels >= 0)
      out << "depth holes\n  maximum hole pixels  " << o.depthFillHolesMaxPixels << "\n  tolerance  " << o.depthFillHolesTolerance << " + "
          << o.depthFillHolesRelTolerance << " z\n  views  " << result->depthFillHolesViews << "\n  holes  " << result->depthFillHolesHoles
          << "\n  holes filled  " << result->depthFillHolesFilledHoles << "\n  pixels filled  " << result->depthFillHolesFilledPixels
          << "\n  GPU kernels  " << result->depthFillHolesKernelMs << " ms\n";
    if (o.depthSmoothSigmaGiven)
      out << "depth smoothing\n  sigma  " << o.depthSmoothSigma << " pixels\n  truncate  " << o.depthSmoothTruncate << "\n  tolerance  "
          << o.depthSmoothTolerance << " + " << o.depthSmoothRelTolerance << " z\n  iterations  " << o.depthSmoothIterations
          << "\n  views  " << result->depthSmoothViews << "\n  pixels with a depth  " << result->depthSmoothValidPixels
          << "\n  pixels changed  " << result->depthSmoothChangedPixels << "\n  taps per pixel  " << result->depthSmoothMeanTaps
          << "\n  GPU kernels  " << result->depthSmoothKernelMs << " ms\n";
    if (o.depthConsistencyMinViews >= 0)
      out << "depth consistency\n  minimum agreeing views  " << o.depthConsistencyMinViews << "\n  tolerance  " << o.depthConsistencyTolerance
          << " + " << o.depthConsistencyRelTolerance << " z\n  views  " << result->depthConsistencyViews << "\n  pixels with a depth  "
          << result->depthConsistencyValidPixels << "\n  pixels kept  " << result->depthConsistencyKeptPixels << "\n  GPU kernels  "
          << result->depthConsistencyKernelMs << " ms\n";
    if (!o.outputPointCloudFilename.empty())
      out << "point cloud\n  file  " << o.outputPointCloudFilename << "\n  minimum agreeing views  " << o.pointCloudMinViews
          << "\n  tolerance  " << o.pointCloudTolerance << " + " << o.pointCloudRelTolerance << " z\n  normal tolerance  "
          << o.pointCloudNormalTolerance << " + " << o.pointCloudNormalRelTolerance << " z\n  pixel step  " << o.pointCloudPixelStep
          << "\n  duplicates  " << (o.pointCloudKeepDuplicates ? "kept" : "dropped") << "\n  views  " << result->pointCloudViews
          << "\n  pixels with a depth  " << result->pointCloudValidPixels << "\n  candidates  " << result->pointCloudCandidates
          << "\n  held by a lower view  " << result->pointCloudOwned << "\n  points  " << result->pointCloudPoints
          << "\n  points with a normal  " << result->pointCloudWithNormal << "\n  GPU kernels  " << result->pointCloudKernelMs << " ms\n";
    if (!o.outputPointCloudFilename.empty() && o.pointCloudOutlierRadiusGiven)
      out << "point cloud outliers\n  radius  " << o.pointCloudOutlierRadius << "\n  minimum neighbours  " << o.pointCloudMinNeighbors
          << "\n  points in  " << result->pointCloudRadiusPointsIn << "\n  points kept  " << result->pointCloudRadiusPointsKept
          << "\n  points without a neighbour  " << result->pointCloudRadiusIsolated << "\n  most neighbours  "
          << result->pointCloudRadiusMaxNeighbors << "\n  neighbours in all  " << result->pointCloudRadiusNeighborSum
          << "\n  distance tests  " << result->pointCloudRadiusDistanceTests << "\n  GPU kernels  " << result->pointCloudRadiusKernelMs
          << " ms\n";
    if (!o.outputPointCloudFilename.empty() && o.pointCloudPlaneFitRadiusGiven)
      out << "point cloud plane fit\n  radius  " << o.pointCloudPlaneFitRadius << "\n  minimum neighbours  " << o.pointCloudPlaneFitMinNeighbors
          << "\n  passes  " << o.pointCloudPlaneFitIterations << "\n  positions  " << (o.pointCloudPlaneFitKeepPositions ? "kept" : "moved")
          << "\n  normals  " << (o.pointCloudPlaneFitKeepNormals ? "kept" : "replaced") << "\n  points in  "
          << result->pointCloudPlaneFitPointsIn << "\n  points fitted  " << result->pointCloudPlaneFitFitted
          << "\n  points with too few neighbours  " << result->pointCloudPlaneFitUnsupported << "\n  crowded points  "
          << result->pointCloudPlaneFitCrowded << "\n  most neighbours  " << result->pointCloudPlaneFitMaxNeighbors
          << "\n  neighbours in all  " << result->pointCloudPlaneFitNeighborSum << "\n  distance tests  "
          << result->pointCloudPlaneFitDistanceTests << "\n  largest shift  " << result->pointCloudPlaneFitMaxShift << "\n  GPU kernels  "
          << result->pointCloudPlaneFitKernelMs << " ms\n";
    if (!o.outputPointCloudFilename.empty() && o.pointCloudCellSizeGiven)
      out << "point cloud thinning\n  cell size  " << o.pointCloudCellSize << "\n  minimum points per cell  " << o.pointCloudMinCellPoints
          << "\n  occupied cells  " << result->pointCloudCells << "\n  cells kept  " << result->pointCloudCellsKept
          << "\n  cells fed by more than one view  " << result->pointCloudMultiViewCells << "\n  largest cell  "
          << result->pointCloudLargestCell << "\n  points with a normal  " << result->pointCloudThinnedWithNormal << "\n  GPU kernels  "
          << result->pointCloudThinKernelMs << " ms\n";
    if (o.extractMesh)
      out << "contour\n  cells straddling the value  " << result->contourActiveCells << "\n  mesh  " << o.outputMeshFilename << "\n  mesh vertices  "
          << result->meshVertices << "\n  mesh triangles  " << result->meshTriangles << "\n";
    if (contourSmoothed(o))  // (only with --extractMesh)
      out << "  contour smoothing  sigma " << o.contourSmoothSigma[0] << " " << o.contourSmoothSigma[1] << " " << o.contourSmoothSigma[2]
          << " voxels, truncate " << o.contourSmoothTruncate << ", radii " << result->contourSmoothRadius[0] << " "
          << result->contourSmoothRadius[1] << " " << result->contourSmoothRadius[2] << ", " << result->contourSmoothKernelMs
          << " ms of GPU kernels\n";
    if (o.meshMinSupportViews > 0)  // (only with --extractMesh)
      out << "  mesh support  at least " << o.meshMinSupportViews << " of " << result->meshSupportViews << " views, depth tolerance "
          << o.meshSupportDepthTolerance << (supportFacing ? ", facing" : ", any facing") << ", " << result->meshVerticesBeforeSupport
          << " vertices, " << result->meshTrianglesBeforeSupport << " triangles before, " << result->meshVerticesExtracted << " vertices, "
          << result->meshTrianglesExtracted << " triangles after, " << result->meshSupportKernelMs << " ms of GPU kernels\n";
    if (filterMesh)  // (only with --extractMesh)
      out << "  mesh components found  " << result->meshComponents << "\n  mesh components kept  " << result->meshComponentsKept
          << "\n  mesh vertices before the component filter  " << result->meshVerticesExtracted
          << "\n  mesh triangles before the component filter  " << result->meshTrianglesExtracted << "\n";
    if (o.meshFillHoles > 0)  // (only with --extractMesh)
      out << "  mesh holes  at most " << o.meshFillHoles << " edges, " << result->meshHolesFilled << " filled, "
          << result->meshBoundaryEdgesLeft << " boundary edges left, " << result->meshFillHolesKernelMs << " ms of GPU kernels\n";
    if (o.meshSmoothIterations > 0)  // (only with --extractMesh)
      out << "  mesh smoothing  " << o.meshSmoothIterations << " iterations, lambda " << o.meshSmoothLambda << ", mu " << o.meshSmoothMu
          << ", " << result->meshSmoothKernelMs << " ms of GPU kernels\n";
    if (o.meshDecimateCellSize > 0)  // (only with --extractMesh)
      out << "  mesh decimation  cell size " << o.meshDecimateCellSize << (o.meshDecimateQuadric ? ", quadric placement" : "") << ", "
          << result->meshVerticesBeforeDecimation << " vertices, "
          << result->meshTrianglesBeforeDecimation << " triangles before, " << result->meshVertices << " vertices, "
          << result->meshTriangles << " triangles after, " << result->meshDecimateKernelMs << " ms of GPU kernels\n";
    if (o.meshColoration) {  // (only with --extractMesh)
      out << "  mesh coloration  " << result->meshVertices << " vertices, " << result->meshColorationViews << " views, depth tolerance ";
      if (o.meshColorationDepthToleranceGiven) out << o.meshColorationDepthTolerance; else out << "none";
      if (o.meshColorationDepthFromMesh) out << " against the mesh's own rendered depth (" << result->meshColorationRenderKernelMs << " ms of GPU kernels to render)";
      out << ", " << result->meshColorationKernelMs << " ms of GPU kernels\n";
    }
    if (!o.extractMesh)
      out << "contour\n  cells straddling the value  " << result->contourActiveCells << " (no surface extracted)\n";
    out << "time\n  reconstruction  " << result->reconstructionSeconds << " s\n  total           " << result->totalSeconds << " s\n";
  }
  say("---END---");
  return 0;
}

}  // namespace cli
}  // namespace host
}  // namespace dmi
