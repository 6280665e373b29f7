/*
 * dmi_host.h -- C bindings of the host-side mirror of the reference's operator interface
 * (cudadepthmapintegration_amd/csrc/host/recon_host.h), for callers without a C++ toolchain that matches
 * (tests and bench bind it with ctypes).  Each function names the reference member it stands for:
 *   filt.h / filt.cxx = Reconstruction/vtkCudaReconstructionFilter.{h,cxx}
 *   RD.cxx            = Sources/ReconstructionData.cxx
 *   Helper.h          = Sources/Helper.h
 * The compute entry points proper are in dmi.h; nothing here does TSDF arithmetic.
 */
#ifndef DMI_HOST_H_
#define DMI_HOST_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dmi_filter dmi_filter; /* a vtkCudaReconstructionFilter (filt.h:48) */

dmi_filter *dmi_filter_new(void);                                    /* vtkCudaReconstructionFilter::New, filt.cxx:74-86 */
void dmi_filter_delete(dmi_filter *f);
void dmi_filter_set_ray_potential_thickness(dmi_filter *f, double v); /* filt.h:57 */
void dmi_filter_set_ray_potential_rho(dmi_filter *f, double v);       /* filt.h:60 */
void dmi_filter_set_ray_potential_eta(dmi_filter *f, double v);       /* filt.h:63 */
void dmi_filter_set_ray_potential_delta(dmi_filter *f, double v);     /* filt.h:66 */
void dmi_filter_set_threshold_best_cost(dmi_filter *f, double v);     /* filt.h:69 */
void dmi_filter_set_file_path_krtd(dmi_filter *f, const char *path);  /* filt.h:73; NULL unsets */
void dmi_filter_set_file_path_vti(dmi_filter *f, const char *path);   /* filt.h:77; NULL unsets */
void dmi_filter_set_grid_matrix(dmi_filter *f, const double m[16]);   /* filt.h:86; row-major vtkMatrix4x4; NULL unsets */
/* SetInputData(vtkImageData*): only dimensions (POINTS), origin and spacing are read (filt.cxx:121-126) */
void dmi_filter_set_input_data(dmi_filter *f, const int32_t dims[3], const double origin[3], const double spacing[3]);
/* In-memory views in place of the two list files: one ReconstructionData each (RD.cxx:55-78):
 * depths / best_cost [H][W] f64 in vtk point order (best_cost may be NULL), K 3x3 and RT 4x4 row-major. */
int dmi_filter_add_view(dmi_filter *f, const double *depths, const double *best_cost, int32_t width, int32_t height,
                        const double K3[9], const double RT[16]);
void dmi_filter_clear_views(dmi_filter *f);
void dmi_filter_set_device(dmi_filter *f, int32_t device);
void dmi_filter_set_kernel_variant(dmi_filter *f, int32_t variant);
/* New and optional (the reference drives one GPU): fuse on several GPUs of the node through dmi_multi_* (dmi.h).
 * n == 0 (the default) = single GPU.  partition: DMI_PARTITION_VIEWS (depth-map shards + one RCCL all-reduce of the
 * f32 grid; the default) or DMI_PARTITION_Z_SLABS (no exchange, f64, bit-identical to one GPU). */
void dmi_filter_set_devices(dmi_filter *f, const int32_t *devices, int32_t n);
void dmi_filter_set_partition(dmi_filter *f, int32_t partition);
/* Pinned host memory of one staging chunk of views (two exist; default 256 MiB): bounds the filter's host memory
 * whatever the number of views -- the list files are read chunk by chunk, as the reference reads them view by view
 * inside its loop (cu:343-353). */
void dmi_filter_set_host_chunk_bytes(dmi_filter *f, uint64_t bytes);
/* != 0: views are read / copied into the staging chunks on the thread that calls Update() (what the VTK binding uses,
 * vtk/vtkCudaReconstructionFilter.cxx: its view source creates VTK readers); 0 (default): on a second thread, while the
 * previous chunk is copied to the device. */
void dmi_filter_set_fill_on_calling_thread(dmi_filter *f, int32_t yes);
/* Update() -> RequestData (filt.cxx:96-151): 1 on success, 0 on error */
int dmi_filter_update(dmi_filter *f);
double dmi_filter_get_execution_time(const dmi_filter *f);            /* filt.h:81 */
double dmi_filter_get_fuse_kernel_ms(const dmi_filter *f);
int64_t dmi_filter_get_number_of_cells(const dmi_filter *f);
/* copies the "reconstruction_scalar" cell array (filt.cxx:129-135) into out[number_of_cells]; returns the count */
int64_t dmi_filter_get_output(const dmi_filter *f, double *out);
const char *dmi_filter_last_error(const dmi_filter *f);

/* Helper.h:105-168.  1 on success, 0 when the file cannot be opened. */
int dmi_read_krtd_file(const char *path, double K3[9], double RT[16]);
/* Helper.h:60-100.  Writes the resolved paths separated by '\n' into buf (NUL-terminated, truncated to
 * buflen) and returns how many entries the list file holds. */
int dmi_extract_all_file_path(const char *list_path, char *buf, size_t buflen);
/* RD.cxx:192-212: 3x3 K into the top-left of a 4x4 identity. */
void dmi_k3_to_k4(const double K3[9], double K4[16]);
/* RD.cxx:138-167 on a bare table; returns how many depths were set to -1. */
int64_t dmi_apply_depth_threshold(double *depths, const double *best_cost, int64_t n, double threshold);
/* RD.cxx:223-229 (vtkXMLImageDataReader) without VTK: every data mode vtkXMLImageDataWriter produces (ascii, binary,
 * appended raw / base64; with or without vtkZLibDataCompressor; UInt32 / UInt64 headers; either byte order), see
 * csrc/host/vti_reader.h.  1 on success.  dims[3]; depths / best_cost sized by the caller (width*height each,
 * best_cost may be NULL); pass depths == NULL to query dims only. */
int dmi_read_depth_map(const char *path, int32_t dims[3], double *depths, double *best_cost, int32_t *has_best_cost);
/* The "Color" array of the same file (RD.cxx:94-95: unsigned char x 3, vtk point order): color sized by the caller
 * (width*height*3) or NULL to query; *has_color = 0 when the file has none.  1 on success. */
int dmi_read_depth_map_color(const char *path, int32_t dims[3], uint8_t *color, int32_t *has_color);

/* MeshColoration(mesh, vtiList, krtdList) + ProcessColoration() (Coloration/MeshColoration.cxx:52-72, :98-199) on mesh
 * points [n_points][3]; fills mean / median [n_points][3] and count [n_points].  1 on success, 0 on error (message in
 * err, truncated to errlen). */
int dmi_mesh_coloration_from_lists(const double *points, int64_t n_points, const char *vti_list, const char *krtd_list,
                                   int32_t device, uint8_t *mean, uint8_t *median, int32_t *count, char *err, size_t errlen);

/* ---- the `Reconstruction` command line (Reconstruction/main.cxx; csrc/host/recon_cli.h) ----
 * What ReadArguments (rmain:216-343) makes of a command line: flags, defaults, validation and the derived grid. */
typedef struct dmi_cli_options {
  int32_t grid_dims[3];       /* POINT dimensions handed to the filter (rmain:118) */
  double grid_spacing[3], grid_origin[3], grid_end[3];
  double grid_matrix[16];     /* CreateGridMatrixFromInput (rmain:345-360), row-major */
  double ray_thick, ray_rho, ray_eta, ray_delta, thresh_best_cost, contour;
  int32_t verbose, summary, force_cubic_voxel;
  int32_t extract_mesh;       /* --extractMesh (not in the reference): write the iso-surface to --outputMeshFilename */
  int32_t mesh_normals;       /* --meshNormals (not in the reference; only with --extractMesh): with its Normals and scalar */
  /* not in the reference, only with --extractMesh (dmi_filter_isosurface_components, dmi.h): */
  int32_t mesh_largest_component;        /* --meshLargestComponent: keep the connected component with the most triangles */
  int32_t mesh_region_ids;               /* --meshRegionIds: write the point array RegionId */
  int64_t mesh_min_component_triangles;  /* --meshMinComponentTriangles N: drop components of fewer triangles; -1: not given */
  /* not in the reference, only with --extractMesh (dmi_smooth_isosurface, dmi.h); appended to the struct: */
  int64_t mesh_smooth_iterations;        /* --meshSmoothIterations N: Taubin iterations after the component flags; 0: off */
  double mesh_smooth_lambda;             /* --meshSmoothLambda (default 0.5) */
  double mesh_smooth_mu;                 /* --meshSmoothMu (default -0.53) */
  /* not in the reference, only with --extractMesh (dmi_decimate_isosurface, dmi.h); appended to the struct: */
  double mesh_decimate_cell_size;        /* --meshDecimateCellSize v: vertex clustering after the smoothing, world units; 0: off */
  /* not in the reference, only with --extractMesh (dmi_color_process_isosurface, dmi.h); appended to the struct: */
  int32_t mesh_coloration;               /* --meshColoration: colour the final mesh on the device and write the three arrays */
  int32_t mesh_coloration_fused;         /* --meshColorationDepthTolerance was given: the visibility test */
  double mesh_coloration_depth_tolerance; /* ... its tolerance (finite, >= 0) */
  /* (dmi_color_render_isosurface_depths, dmi.h); appended to the struct: */
  int32_t mesh_coloration_depth_from_mesh; /* --meshColorationDepthFromMesh: that test against the mesh's own rendered depth */
  /* (dmi_decimate_isosurface_placed, dmi.h); appended to the struct: */
  int32_t mesh_decimate_quadric;         /* --meshDecimateQuadric: the decimation places its vertices by quadric error */
  /* not in the reference (dmi_filter_depth_consistency, dmi.h); appended to the struct: */
  int64_t depth_consistency_min_views;   /* --depthConsistencyMinViews N: filter the depth maps before the fusion; -1: not given */
  double depth_consistency_tolerance;    /* --depthConsistencyTolerance (default 0) */
  double depth_consistency_rel_tolerance; /* --depthConsistencyRelTolerance (default 0.01) */
  /* not in the reference (dmi_estimate_scene_bounds, dmi.h); appended to the struct.  With --gridAutoBounds grid_origin and grid_end
   * are zero here, and so is whichever of grid_dims / grid_spacing was not given: the run derives them from the depth maps */
  int32_t grid_auto_bounds;              /* --gridAutoBounds: the grid's box from the depth maps */
  double grid_auto_bounds_trim;          /* --gridAutoBoundsTrim (default 0.005) */
  double grid_auto_bounds_margin;        /* --gridAutoBoundsMargin (default 0.05) */
  int64_t grid_auto_bounds_pixel_step;   /* --gridAutoBoundsPixelStep (default 1) */
  /* not in the reference, only with --extractMesh (dmi_fill_isosurface_holes, dmi.h); appended to the struct: */
  int64_t mesh_fill_holes;               /* --meshFillHoles N: close boundary loops of at most N edges before the smoothing; 0: off */
  /* not in the reference, only with --extractMesh (dmi_set_point_smoothing, dmi.h); appended to the struct: */
  double contour_smooth_sigma[3];        /* --contourSmoothSigma S [S S]: Gaussian over the point data before the contour, voxels; 0: off */
  double contour_smooth_truncate;        /* --contourSmoothTruncate (default 3) */
  /* not in the reference (dmi_filter_depth_speckles, dmi.h); appended to the struct: */
  int64_t depth_speckle_min_pixels;      /* --depthSpeckleMinPixels N: drop depth-map segments of fewer pixels before the fusion; -1: not given */
  double depth_speckle_tolerance;        /* --depthSpeckleTolerance (default 0) */
  double depth_speckle_rel_tolerance;    /* --depthSpeckleRelTolerance (default 0.01) */
  /* not in the reference (dmi_fill_depth_holes, dmi.h); appended to the struct: */
  int64_t depth_fill_holes_max_pixels;   /* --depthFillHolesMaxPixels N: fill depth-map holes of at most N pixels before the fusion; -1: not given */
  double depth_fill_holes_tolerance;     /* --depthFillHolesTolerance (default 0) */
  double depth_fill_holes_rel_tolerance; /* --depthFillHolesRelTolerance (default 0.01) */
  /* not in the reference (dmi_smooth_depths, dmi.h); appended to the struct: */
  double depth_smooth_sigma;             /* --depthSmoothSigma S: smooth the depth maps, edges preserved, before the fusion; -1: not given */
  double depth_smooth_truncate;          /* --depthSmoothTruncate (default 2) */
  double depth_smooth_tolerance;         /* --depthSmoothTolerance (default 0) */
  double depth_smooth_rel_tolerance;     /* --depthSmoothRelTolerance (default 0.01) */
  int64_t depth_smooth_iterations;       /* --depthSmoothIterations (default 1) */
  int32_t depth_staged_filters;          /* --depthStagedFilters: the depth-map steps through the staged calls, not on a resident view set */
  /* not in the reference, only with --outputPointCloudFilename (dmi_views_thin_points, dmi.h); appended to the struct: */
  double point_cloud_cell_size;          /* --pointCloudCellSize v: thin the point cloud on a voxel grid before it is written; 0: not given */
  int64_t point_cloud_min_cell_points;   /* --pointCloudMinCellPoints N (default 1) */
  /* not in the reference, only with --outputPointCloudFilename (dmi_views_filter_points_radius, dmi.h); appended to the struct: */
  double point_cloud_outlier_radius;     /* --pointCloudOutlierRadius r: drop the points with too few neighbours within r, before the thinning; 0: not given */
  int64_t point_cloud_min_neighbors;     /* --pointCloudMinNeighbors N (default 1) */
  /* not in the reference, only with --outputPointCloudFilename (dmi_views_fit_point_planes, dmi.h); appended to the struct: */
  double point_cloud_plane_fit_radius;            /* --pointCloudPlaneFitRadius r: fit planes within r, behind the outlier filter and before the thinning; 0: not given */
  int64_t point_cloud_plane_fit_min_neighbors;    /* --pointCloudPlaneFitMinNeighbors N (default 5) */
  int64_t point_cloud_plane_fit_iterations;       /* --pointCloudPlaneFitIterations k (default 1) */
  int32_t point_cloud_plane_fit_keep_positions;   /* --pointCloudPlaneFitKeepPositions */
  int32_t point_cloud_plane_fit_keep_normals;     /* --pointCloudPlaneFitKeepNormals */
} dmi_cli_options;
/* 1: the run may proceed, *out filled.  0: an error or --help; the text (what the tool would print) in err. */
int dmi_cli_read_arguments(int32_t argc, const char *const *argv, dmi_cli_options *out, char *err, size_t errlen);
/* The whole tool: ReadArguments, the filter, cell -> point data, meta_image_volume.mha (in the working directory, as the
 * reference), the .vts volume, the summary file.  Process exit code: 0 on success.  The iso-surface (rmain:166-187) only
 * with --extractMesh: dmi_extract_isosurface at --contour, written to --outputMeshFilename by dmi_write_polydata; with
 * --meshNormals too, dmi_extract_isosurface_normals and dmi_write_polydata_with_normals.  With --meshMinComponentTriangles
 * and / or --meshLargestComponent the mesh goes through dmi_filter_isosurface_components first (by size, then the largest), and
 * with --meshRegionIds the file is dmi_write_polydata_with_arrays' with RegionId.  With --meshSmoothIterations N the mesh goes
 * through dmi_smooth_isosurface after those (the Normals of --meshNormals are then the smoothed mesh's geometric ones).  With
 * --meshDecimateCellSize v it goes through dmi_decimate_isosurface last (Normals: the decimated mesh's geometric ones; RegionId:
 * from the labelling run again on the decimated mesh; with --meshDecimateQuadric dmi_decimate_isosurface_placed and the quadric
 * placement).  With --meshColoration (one device) the views' Color arrays go to a
 * dmi_color_context in the same pass that reads the depths, the mesh is extracted in the context that fused (its views stay
 * resident) and coloured last by dmi_color_process_isosurface -- with --meshColorationDepthTolerance T the fused visibility
 * test -- and the file is dmi_write_polydata_with_colors'.  A view without a UInt8 x 3 Color array of the views' size ends the
 * run non-zero with the file's name.  With --meshMinSupportViews N --meshSupportDepthTolerance T (one device) the mesh is extracted
 * in the context that fused and trimmed by dmi_filter_isosurface_support before the component flags; --meshSupportArray writes the
 * final mesh's counts as the Int32 point array NbSupportingViews, behind RegionId and before the colours.  With
 * --depthConsistencyMinViews N every view is read into memory, the depths are filtered by dmi_filter_depth_consistency on the first
 * device and the filter fuses the filtered views (ReconstructionFilter::SetViews).  With --gridAutoBounds (--gridOrigin and
 * --gridEnd absent) every view is read into memory as well, filtered first if that was asked for, and the grid's box is what
 * dmi_estimate_scene_bounds gives along the grid's axes, plus a margin.  With --meshFillHoles N the mesh goes through
 * dmi_fill_isosurface_holes behind the support trim and the component flags and in front of the smoothing (RegionId: from the
 * labelling run again on the filled mesh, unless a decimation behind it does that).  With --contourSmoothSigma S the context's
 * point smoothing is set (dmi_set_point_smoothing) directly before the extraction: the .mha, the .vts and the count of active cells
 * are what they are without the flag.  With --depthSpeckleMinPixels N every view is read into memory as with
 * --depthConsistencyMinViews and the depths go through dmi_filter_depth_speckles first of all: the consistency filter, the bounds
 * estimate and the fusion see what it left.  With --depthFillHolesMaxPixels N the depths then go through
 * dmi_fill_depth_holes: behind the speckle filter, in front of the consistency filter, the bounds estimate and the fusion.  With
 * --depthSmoothSigma S they then go through dmi_smooth_depths: behind the hole fill, in front of the same three. */
int dmi_cli_main(int32_t argc, const char *const *argv);

/* What vtkXMLPolyDataWriter makes of a triangle mesh (rmain:184-187), without VTK: a VTK XML PolyData file in the layout of
 * the .vts writer (appended raw data, UInt64 headers, little-endian): Float64 Points [n_points][3], Polys with Int64
 * connectivity [n_triangles][3] and offsets 3, 6, 9, ...  No point or cell arrays (VTK's contour filter would add Normals
 * and the scalar: dmi_write_polydata_with_normals).  1 on success, 0 when the file cannot be written or a count is negative. */
int dmi_write_polydata(const char *path, const double *points, int64_t n_points, const int64_t *triangles, int64_t n_triangles);
/* dmi_write_polydata's file plus the point data vtkContourFilter attaches: <PointData Normals="Normals"
 * Scalars="reconstruction_scalar"> with Normals, Float32 x 3 ([n_points][3], dmi_download_isosurface_normals), and
 * reconstruction_scalar, Float64, `contour` at every point; both in the appended raw block behind the offsets.  1 on success,
 * 0 when the file cannot be written, a count is negative or a pointer is null while its count is not zero. */
int dmi_write_polydata_with_normals(const char *path, const double *points, int64_t n_points, const int64_t *triangles,
                                    int64_t n_triangles, const float *normals, double contour);

/* Either file with the point array RegionId (Int64, one component: region_id[n_points], dmi_download_isosurface_regions)
 * appended behind everything else.  normals == NULL: dmi_write_polydata's file plus <PointData Scalars="RegionId">; otherwise
 * dmi_write_polydata_with_normals' with RegionId as the third array of its <PointData>.  region_id == NULL: exactly the file of
 * dmi_write_polydata (normals == NULL) or dmi_write_polydata_with_normals.  1 on success; 0 as those two. */
int dmi_write_polydata_with_arrays(const char *path, const double *points, int64_t n_points, const int64_t *triangles,
                                   int64_t n_triangles, const float *normals, double contour, const int64_t *region_id);

/* dmi_write_polydata_with_arrays' file with the Coloration tool's point arrays MeanColoration (UInt8 x 3), MedianColoration
 * (UInt8 x 3) and NbProjectedDepthMap (Int32) appended behind every array it writes: mean, median [n_points][3], count [n_points]
 * (dmi_download_isosurface_colors), all three or none (none: exactly dmi_write_polydata_with_arrays' file).  A function of its
 * own because the older one's signature is part of the ABI.  1 on success; 0 as those. */
int dmi_write_polydata_with_colors(const char *path, const double *points, int64_t n_points, const int64_t *triangles,
                                   int64_t n_triangles, const float *normals, double contour, const int64_t *region_id,
                                   const uint8_t *mean, const uint8_t *median, const int32_t *count);

/* dmi_mesh_coloration_from_lists with the visibility test of dmi_color_set_depth_test (dmi.h) at `depth_tolerance`
 * (MeshColoration::SetDepthTolerance; needs the views' "Depths" arrays).  1 on success, 0 on error (message in err). */
int dmi_mesh_coloration_from_lists_with_depth(const double *points, int64_t n_points, const char *vti_list, const char *krtd_list,
                                              int32_t device, double depth_tolerance, uint8_t *mean, uint8_t *median, int32_t *count,
                                              char *err, size_t errlen);
/* The same test against the MESH'S OWN depth: points and triangles ([n_triangles][3] ids into the points) are rendered into every
 * view (dmi_color_render_depths, dmi.h; MeshColoration::SetDepthFromMesh) and the views' "Depths" arrays are neither read nor
 * needed -- a .vti file with a "Color" array alone will do.  render_kernel_ms (nullable) receives the rendering's kernel time.
 * 1 on success, 0 on error (message in err). */
int dmi_mesh_coloration_from_lists_with_mesh_depth(const double *points, int64_t n_points, const int64_t *triangles, int64_t n_triangles,
                                                   const char *vti_list, const char *krtd_list, int32_t device, double depth_tolerance,
                                                   uint8_t *mean, uint8_t *median, int32_t *count, double *render_kernel_ms, char *err,
                                                   size_t errlen);

/* ---- VTK XML PolyData without VTK (csrc/host/vtp_reader.h): what vtkXMLPolyDataReader gives the Coloration tool ----
 * One piece; Points Float32 / Float64; Polys with Int32 / Int64 connectivity and offsets; every point- and cell-data array as
 * stored (host byte order), with its section's designations.  Every data mode of the format (see dmi_read_depth_map).
 * dmi_read_polydata: NULL on failure, the reason in err (truncated to errlen). */
typedef struct dmi_polydata dmi_polydata;
dmi_polydata *dmi_read_polydata(const char *path, char *err, size_t errlen);
void dmi_polydata_free(dmi_polydata *pd);
/* out[0] points, out[1] polys, out[2] connectivity length, out[3] point-data arrays, out[4] cell-data arrays.  1 on success. */
int dmi_polydata_counts(const dmi_polydata *pd, int64_t out[5]);
/* One array: kind 0 = Points, 1 = Polys connectivity, 2 = Polys offsets, 3 = point-data array `index`, 4 = cell-data array
 * `index`.  Pointers into pd (valid until dmi_polydata_free); any out pointer may be NULL.  1 on success. */
int dmi_polydata_array(const dmi_polydata *pd, int32_t kind, int32_t index, const char **name, const char **type, int32_t *components,
                       int64_t *n_tuples, const void **data);
/* the attributes of <PointData> (cell == 0) or <CellData> (cell != 0), "key=value" per line: Scalars=..., Normals=... */
const char *dmi_polydata_designations(const dmi_polydata *pd, int32_t cell);

/* ---- the `Coloration` command line (Coloration/main.cxx; csrc/host/color_cli.h) ----
 * What ReadArguments (cmain:105-135) makes of a command line.  --device, --depthTolerance and --depthFromMesh are not in the
 * reference. */
typedef struct dmi_color_cli_options {
  char input[4096], output[4096], krtd[4096], vti[4096]; /* --input, --output, --krtd, --vti (NUL-terminated, truncated) */
  int32_t verbose;
  int32_t device;             /* --device (default 0) */
  int32_t depth_test;         /* --depthTolerance given: the visibility test of dmi_color_set_depth_test */
  double depth_tolerance;
  int32_t depth_from_mesh;    /* --depthFromMesh: that test against the input mesh's own rendered depth (appended to the struct) */
} dmi_color_cli_options;
/* 1: the run may proceed, *out filled.  0: an error or --help; the text (what the tool would print) in err. */
int dmi_color_cli_read_arguments(int32_t argc, const char *const *argv, dmi_color_cli_options *out, char *err, size_t errlen);
/* The whole tool: read --input, colour its points from the views of the two list files, write --output with the input's
 * points, polys and arrays plus MeanColoration, MedianColoration and NbProjectedDepthMap.  Process exit code: 0 on success,
 * 1 on any error -- including a failed colouring, after which the reference returns 0 and writes nothing (cmain:82-99). */
int dmi_color_cli_main(int32_t argc, const char *const *argv);

#ifdef __cplusplus
}
#endif

#endif /* DMI_HOST_H_ */
