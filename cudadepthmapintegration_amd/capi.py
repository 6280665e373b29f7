"""ctypes binding of the C ABI (include/dmi.h) -- used by tests, smoke and bench.

There is NO CPU fallback: if libdmi_hip.so is missing or no HIP device is present every
entry point raises.  The library is built in-tree by cudadepthmapintegration_amd.build.
"""
from __future__ import annotations

import ctypes
import os
import sys
from typing import NamedTuple

import numpy as np

from . import build as _build
from .scene import GridDesc, RayPotential, Views

DMI_OK = 0
DMI_F32, DMI_F64 = 0, 1
DMI_DEPTH_AUTO, DMI_DEPTH_F32, DMI_DEPTH_F64 = 0, 1, 2
DMI_COMPONENTS_MIN_TRIANGLES, DMI_COMPONENTS_LARGEST = 0, 1

# kernel_variant bits (tuning knobs)
VARIANT_EXACT_DIVISION = 1  # disable the checked-reciprocal fast path
VARIANT_GENERAL_K = 2  # ignore K structure, evaluate the full 4x4 rows
VARIANT_FORCE_GENERAL = 16  # never use the register-tiled kernel
VARIANT_NO_BRICK_CLASSES = 256  # tiled kernel without the proven per-brick shortcuts
VARIANT_KEEP_BEHIND_ADDS = 1024  # tiled kernel: perform +0.0 adds even when they cannot change a sum
VARIANT_NO_INTERIOR = 2048  # tiled kernel: keep the in-front / in-image tests for every mixed pair
VARIANT_XCD_RUNS = 8192  # tiled kernel: ordered bricks dealt to the XCDs in runs (round 1) instead of an eighth of a level each
VARIANT_ZMAJOR_SLOTS = 16384  # tiled kernel: super-bricks enumerated x, y, z (until r03h) instead of in Z-order
VARIANT_PERSISTENT_ALWAYS = 32768  # tiled kernel: persistent one-wave workgroups whatever the number of views (default: from 96 on)
VARIANT_PERSISTENT_NEVER = 65536  # tiled kernel: one workgroup per brick whatever the number of views
VARIANT_NO_WINDOWS = 262144  # tiled kernel: the FREE column always gathers from the validity maps (no bit windows)
VARIANT_WINDOWS_ALWAYS = 524288  # tiled kernel: bit windows whatever the depth maps look like (default: maps with scattered holes)
VARIANT_COST_ORDER = 1048576  # tiled kernel: bricks ordered by their number of mixed views whatever the grid's size (default: up to 2^16 bricks)
VARIANT_NO_COST_ORDER = 2097152  # tiled kernel: never (four work levels, an eighth of each per XCD)
VARIANT_BRICK_CLASSES_ALWAYS = 131072  # tiled kernel: brick classes for tiny grids too (default: none up to 1024 bricks per launch)
VARIANT_FIXED_TILE_SHAPE = 4096  # tile-shape bits 0 mean shape 0 (tk16_w5) whatever the grid size; without it grids
                                 # below 512^3 pick tk8_w7 on their own
VARIANT_SPATIAL_ORDER = 512  # tiled kernel: workgroups in spatial order instead of heaviest bricks first
VARIANT_TILE_SHAPE = {"tk16_w5_g8_1x1": 0, "tk8_w6_g8_2x2": 32, "tk16_w5_g8_2x2": 64, "tk8_w6": 96, "tk8_w7_g8": 128, "tk16_w5_g4": 160,
                      "tk16_w6_g2": 192, "tk8_w6_g8_1x1": 224}  # tiled kernel: column height / compiler register budget / load group


class GridDescC(ctypes.Structure):
    _fields_ = [("cell_dims", ctypes.c_int32 * 3), ("origin", ctypes.c_double * 3),
                ("spacing", ctypes.c_double * 3), ("grid_matrix", ctypes.c_double * 16)]


class RayPotentialC(ctypes.Structure):
    _fields_ = [("thickness", ctypes.c_double), ("rho", ctypes.c_double), ("eta", ctypes.c_double),
                ("delta", ctypes.c_double)]


class OptionsC(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("grid_dtype", ctypes.c_int32), ("depth_storage", ctypes.c_int32),
                ("count_hits", ctypes.c_int32), ("kernel_variant", ctypes.c_int32), ("z_first", ctypes.c_int32),
                ("stream", ctypes.c_void_p), ("external_grid", ctypes.c_void_p)]


class TimingsC(ctypes.Structure):
    _fields_ = [("last_fuse_kernel_ms", ctypes.c_double), ("total_fuse_kernel_ms", ctypes.c_double),
                ("fuse_launches", ctypes.c_uint64), ("last_upload_ms", ctypes.c_double),
                ("last_download_ms", ctypes.c_double), ("last_cell_to_point_ms", ctypes.c_double),
                ("last_fuse_main_kernel_ms", ctypes.c_double), ("total_fuse_main_kernel_ms", ctypes.c_double)]


class InfoC(ctypes.Structure):
    _fields_ = [("n_voxels", ctypes.c_int64), ("n_views", ctypes.c_int32), ("depth_width", ctypes.c_int32),
                ("depth_height", ctypes.c_int32), ("depth_storage_in_use", ctypes.c_int32),
                ("grid_dtype", ctypes.c_int32), ("k_mode", ctypes.c_int32), ("kernel_variant", ctypes.c_int32),
                ("tiled_kernel", ctypes.c_int32), ("device_bytes", ctypes.c_uint64), ("pixels_without_depth", ctypes.c_uint64)]


class ViewsInfoC(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("W", ctypes.c_int32), ("H", ctypes.c_int32), ("device", ctypes.c_int32),
                ("device_bytes", ctypes.c_uint64), ("steps", ctypes.c_uint64), ("h2d_plane_bytes", ctypes.c_uint64),
                ("d2h_plane_bytes", ctypes.c_uint64), ("last_report_kernel_ms", ctypes.c_double)]


class ViewsStepReportC(ctypes.Structure):
    _fields_ = [("valid_before", ctypes.c_uint64), ("valid_after", ctypes.c_uint64), ("changed", ctypes.c_uint64),
                ("groups", ctypes.c_uint64), ("groups_kept", ctypes.c_uint64), ("aux_sum", ctypes.c_uint64),
                ("kernel_ms", ctypes.c_double)]


class ViewsPointsReportC(ctypes.Structure):
    _fields_ = [("valid", ctypes.c_uint64), ("candidates", ctypes.c_uint64), ("owned", ctypes.c_uint64), ("points", ctypes.c_uint64),
                ("with_normal", ctypes.c_uint64), ("kernel_ms", ctypes.c_double)]


class PointsThinReportC(ctypes.Structure):
    _fields_ = [("points_in", ctypes.c_uint64), ("cells", ctypes.c_uint64), ("cells_kept", ctypes.c_uint64),
                ("multi_view_cells", ctypes.c_uint64), ("largest_cell", ctypes.c_uint64), ("with_normal", ctypes.c_uint64),
                ("kernel_ms", ctypes.c_double)]


class PointsRadiusReportC(ctypes.Structure):
    _fields_ = [("points_in", ctypes.c_uint64), ("points_kept", ctypes.c_uint64), ("isolated", ctypes.c_uint64),
                ("max_neighbors", ctypes.c_uint64), ("neighbor_sum", ctypes.c_uint64), ("distance_tests", ctypes.c_uint64),
                ("kernel_ms", ctypes.c_double)]


class PointsPlanesReportC(ctypes.Structure):
    _fields_ = [("points_in", ctypes.c_uint64), ("fitted", ctypes.c_uint64), ("unsupported", ctypes.c_uint64),
                ("crowded", ctypes.c_uint64), ("max_neighbors", ctypes.c_uint64), ("neighbor_sum", ctypes.c_uint64),
                ("distance_tests", ctypes.c_uint64), ("max_shift", ctypes.c_double), ("kernel_ms", ctypes.c_double)]


PLANE_FIT_MOVE, PLANE_FIT_NORMALS = 1, 2   # DMI_PLANE_FIT_MOVE, DMI_PLANE_FIT_NORMALS


class MultiOptionsC(ctypes.Structure):
    _fields_ = [("grid_dtype", ctypes.c_int32), ("depth_storage", ctypes.c_int32), ("kernel_variant", ctypes.c_int32),
                ("partition", ctypes.c_int32), ("exchange", ctypes.c_int32), ("n_slabs", ctypes.c_int32)]


class MultiInfoC(ctypes.Structure):
    _fields_ = [("world", ctypes.c_int32), ("n_local", ctypes.c_int32), ("first_rank", ctypes.c_int32),
                ("rccl_ranks", ctypes.c_int32), ("rccl_version", ctypes.c_int32), ("partition", ctypes.c_int32),
                ("exchange", ctypes.c_int32), ("n_slabs", ctypes.c_int32), ("n_voxels", ctypes.c_int64),
                ("n_views_total", ctypes.c_int64), ("n_views_local", ctypes.c_int64)]


class MultiTimingsC(ctypes.Structure):
    _fields_ = [("last_step_ms", ctypes.c_double), ("last_fuse_kernel_ms", ctypes.c_double),
                ("total_step_ms", ctypes.c_double), ("steps", ctypes.c_uint64)]


DMI_PARTITION_VIEWS, DMI_PARTITION_Z_SLABS = 0, 1
DMI_EXCHANGE_ALL_REDUCE, DMI_EXCHANGE_REDUCE_SCATTER, DMI_EXCHANGE_PEER_COPY = 0, 1, 2
DMI_UNIQUE_ID_BYTES = 128
# the rasteriser's compile-time shape (csrc/mesh_depth_render.h: kRenderViewGroup, kRenderLaneCap), for tests that aim at its edges
RENDER_VIEW_GROUP, RENDER_LANE_CAP = 16, 64

# dmi_decimate_isosurface_placed's placements (DMI_DECIMATE_MEAN, DMI_DECIMATE_QUADRIC)
DMI_DECIMATE_MEAN, DMI_DECIMATE_QUADRIC = 0, 1
DECIMATE_PLACEMENTS = {"mean": DMI_DECIMATE_MEAN, "quadric": DMI_DECIMATE_QUADRIC}

# every symbol include/dmi.h declares (tests/test_abi.py checks the library exports them all)
ABI_SYMBOLS = [
    "dmi_default_options", "dmi_create", "dmi_destroy", "dmi_last_error", "dmi_add_views", "dmi_add_views_f32",
    "dmi_clear_views", "dmi_reset_grid", "dmi_upload_grid", "dmi_fuse", "dmi_fuse_range", "dmi_fuse_slab", "dmi_fuse_range_download", "dmi_synchronize",
    "dmi_download_grid_f64", "dmi_download_grid_f32", "dmi_download_hits", "dmi_grid_device_pointer",
    "dmi_get_brick_class_histogram", "dmi_get_timings", "dmi_get_info", "dmi_alloc_pinned", "dmi_free_pinned", "dmi_pcie_probe", "dmi_fp64_probe", "dmi_abi_version", "dmi_device_count",
    "dmi_color_mesh", "dmi_color_last_error", "dmi_cell_to_point", "dmi_download_point_data_f64",
    "dmi_point_data_device_pointer", "dmi_color_create", "dmi_color_destroy", "dmi_color_add_views",
    "dmi_color_clear_views", "dmi_color_process", "dmi_color_get_kernel_ms", "dmi_get_mixed_reason_histogram", "dmi_get_window_pair_count", "dmi_get_view_paths", "dmi_get_upload_kernel_ms", "dmi_sizeof_info", "dmi_sizeof_timings",
    "dmi_color_set_scratch_budget", "dmi_color_set_vertex_reorder", "dmi_color_add_views_with_depth", "dmi_color_set_depth_test",
    "dmi_iso_active_cells",
    "dmi_extract_isosurface", "dmi_download_isosurface", "dmi_get_isosurface_kernel_ms",
    "dmi_extract_isosurface_normals", "dmi_download_isosurface_normals",
    "dmi_filter_isosurface_components", "dmi_download_isosurface_regions", "dmi_get_isosurface_filter_kernel_ms",
    "dmi_get_isosurface_filter_pass_ms", "dmi_get_isosurface_filter_cas_retries",
    "dmi_smooth_isosurface", "dmi_get_isosurface_smooth_kernel_ms", "dmi_get_isosurface_smooth_pass_ms",
    "dmi_decimate_isosurface", "dmi_get_isosurface_decimate_kernel_ms", "dmi_get_isosurface_decimate_pass_ms",
    "dmi_color_process_isosurface", "dmi_download_isosurface_colors", "dmi_get_isosurface_color_kernel_ms",
    "dmi_filter_isosurface_support", "dmi_download_isosurface_support", "dmi_get_isosurface_support_kernel_ms",
    "dmi_get_isosurface_support_pass_ms", "dmi_decimate_isosurface_placed",
    "dmi_fill_isosurface_holes", "dmi_get_isosurface_holes_kernel_ms", "dmi_get_isosurface_holes_pass_ms",
    "dmi_color_render_depths", "dmi_color_render_isosurface_depths", "dmi_color_download_depths", "dmi_color_get_render_kernel_ms",
    "dmi_color_set_render_queue_capacity", "dmi_color_get_render_pass_ms", "dmi_color_get_render_queued_pairs",
    "dmi_filter_depth_consistency", "dmi_estimate_scene_bounds", "dmi_filter_depth_speckles", "dmi_fill_depth_holes",
    "dmi_depth_smoothing_weights", "dmi_smooth_depths",
    "dmi_views_create", "dmi_views_destroy", "dmi_views_last_error", "dmi_views_add", "dmi_views_clear", "dmi_views_get_info",
    "dmi_sizeof_views_info", "dmi_views_set_piece_bytes", "dmi_views_filter_speckles", "dmi_views_fill_holes", "dmi_views_smooth",
    "dmi_views_filter_consistency", "dmi_views_estimate_bounds", "dmi_views_download", "dmi_add_views_from_set",
    "dmi_views_build_points", "dmi_views_download_points", "dmi_views_get_points_pass_ms",
    "dmi_thin_point_cloud", "dmi_views_thin_points", "dmi_views_download_point_members", "dmi_views_get_thin_pass_ms",
    "dmi_views_set_thin_wave_cell_points",
    "dmi_count_point_neighbors", "dmi_views_filter_points_radius", "dmi_views_download_point_neighbors", "dmi_views_get_radius_pass_ms",
    "dmi_views_set_radius_group_points",
    "dmi_fit_point_planes", "dmi_views_fit_point_planes", "dmi_views_download_point_plane_rms", "dmi_views_get_plane_fit_pass_ms",
    "dmi_point_smoothing_weights", "dmi_set_point_smoothing", "dmi_get_point_smoothing", "dmi_get_point_smoothing_kernel_ms",
    "dmi_multi_default_options", "dmi_multi_view_shard", "dmi_multi_z_slab", "dmi_multi_slab_ranges", "dmi_multi_peer_chunk", "dmi_multi_create",
    "dmi_multi_get_unique_id", "dmi_multi_create_rank", "dmi_multi_destroy", "dmi_multi_last_error", "dmi_multi_add_views",
    "dmi_multi_add_views_f32", "dmi_multi_add_local_views", "dmi_multi_add_local_views_f32", "dmi_multi_clear_views", "dmi_multi_fuse", "dmi_multi_synchronize",
    "dmi_multi_download_grid_f32", "dmi_multi_download_grid_f64", "dmi_multi_get_info", "dmi_multi_get_timings",
    "dmi_multi_local_context",
]

_lib = None


def point_smoothing_weights(sigma: float, truncate: float = 3.0) -> np.ndarray:
    """k_0..k_r, the normalised weights of one axis of the point smoothing with r = ceil(truncate * sigma), as the library
    computes them (dmi_point_smoothing_weights; no GPU needed).  DmiError with code 1 for parameters outside the definition."""
    L = load()
    r, k = ctypes.c_int32(0), np.zeros(17, dtype=np.float64)
    code = L.dmi_point_smoothing_weights(float(sigma), float(truncate), ctypes.byref(r), _dp(k))
    if code != 0:
        raise DmiError(code, (L.dmi_last_error(None) or b"").decode())
    return k[:int(r.value) + 1].copy()


class DmiError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"dmi error {code}: {message}")
        self.code = code


def library_path() -> str:
    return _build.LIB_PATH


def load() -> ctypes.CDLL:
    """Load libdmi_hip.so (building it with hipcc if the sources are newer).  Raises if it cannot."""
    global _lib
    if _lib is not None:
        return _lib
    if "torch" not in sys.modules:
        # torch ships its own libamdhip64 / librccl (same SONAMEs as ROCm's).  Whichever is loaded first serves the whole
        # process; if ROCm's came first, a later `import torch` finds no GPU.  So when torch exists it goes first and this
        # library, bench.py and torch.distributed all share one HIP runtime.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    path = _build.build()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: the HIP extension is required, there is no CPU fallback")
    L = ctypes.CDLL(path)
    vp, i32, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    dp = ctypes.POINTER(ctypes.c_double)
    L.dmi_default_options.argtypes = [ctypes.POINTER(OptionsC)]
    L.dmi_default_options.restype = None
    L.dmi_create.argtypes = [ctypes.POINTER(GridDescC), ctypes.POINTER(RayPotentialC), ctypes.POINTER(OptionsC),
                             ctypes.POINTER(vp)]
    L.dmi_destroy.argtypes = [vp]
    L.dmi_destroy.restype = None
    L.dmi_last_error.argtypes = [vp]
    L.dmi_last_error.restype = ctypes.c_char_p
    L.dmi_add_views.argtypes = [vp, dp, dp, dbl, dp, dp, i32, i32, i32]
    L.dmi_add_views_f32.argtypes = [vp, ctypes.POINTER(ctypes.c_float), dp, dp, i32, i32, i32]
    L.dmi_clear_views.argtypes = [vp]
    L.dmi_reset_grid.argtypes = [vp]
    L.dmi_upload_grid.argtypes = [vp, dp]
    L.dmi_fuse.argtypes = [vp]
    L.dmi_fuse_range.argtypes = [vp, i32, i32]
    L.dmi_fuse_slab.argtypes = [vp, i32, i32]
    if hasattr(L, "dmi_fuse_range_download"):  # (absent from an older prebuilt library loaded for an A/B timing, tools/gpu_exp.py)
        L.dmi_fuse_range_download.argtypes = [vp, i32, i32, vp, i32, i32]
    L.dmi_synchronize.argtypes = [vp]
    L.dmi_download_grid_f64.argtypes = [vp, dp]
    L.dmi_download_grid_f32.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    L.dmi_download_hits.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)]
    L.dmi_grid_device_pointer.argtypes = [vp, ctypes.POINTER(vp)]
    L.dmi_cell_to_point.argtypes = [vp]
    L.dmi_download_point_data_f64.argtypes = [vp, dp]
    L.dmi_point_data_device_pointer.argtypes = [vp, ctypes.POINTER(vp)]
    if hasattr(L, "dmi_iso_active_cells"):  # (an older build loaded for an A/B, tools/gpu_exp.py, lacks the newest entry points)
        L.dmi_iso_active_cells.argtypes = [vp, ctypes.c_double, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int64),
                                           ctypes.c_uint64]
    if hasattr(L, "dmi_extract_isosurface"):
        L.dmi_extract_isosurface.argtypes = [vp, ctypes.c_double, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
        L.dmi_download_isosurface.argtypes = [vp, dp, ctypes.POINTER(ctypes.c_int64)]
        L.dmi_get_isosurface_kernel_ms.argtypes = [vp, dp]
    if hasattr(L, "dmi_extract_isosurface_normals"):
        L.dmi_extract_isosurface_normals.argtypes = [vp, ctypes.c_double, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
        L.dmi_download_isosurface_normals.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    if hasattr(L, "dmi_filter_isosurface_components"):
        u64p = ctypes.POINTER(ctypes.c_uint64)
        L.dmi_filter_isosurface_components.argtypes = [vp, ctypes.c_int, ctypes.c_uint64, u64p, u64p, u64p, u64p]
        L.dmi_download_isosurface_regions.argtypes = [vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
        L.dmi_get_isosurface_filter_kernel_ms.argtypes = [vp, dp]
        L.dmi_get_isosurface_filter_pass_ms.argtypes = [vp, dp]
        L.dmi_get_isosurface_filter_cas_retries.argtypes = [vp, u64p]
    if hasattr(L, "dmi_smooth_isosurface"):
        L.dmi_smooth_isosurface.argtypes = [vp, i32, dbl, dbl]
        L.dmi_get_isosurface_smooth_kernel_ms.argtypes = [vp, dp]
        L.dmi_get_isosurface_smooth_pass_ms.argtypes = [vp, dp]
    if hasattr(L, "dmi_decimate_isosurface"):
        L.dmi_decimate_isosurface.argtypes = [vp, dbl, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
        L.dmi_get_isosurface_decimate_kernel_ms.argtypes = [vp, dp]
        L.dmi_get_isosurface_decimate_pass_ms.argtypes = [vp, dp]
    if hasattr(L, "dmi_decimate_isosurface_placed"):
        L.dmi_decimate_isosurface_placed.argtypes = [vp, dbl, i32, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    if hasattr(L, "dmi_fill_isosurface_holes"):
        L.dmi_fill_isosurface_holes.argtypes = [vp, ctypes.c_uint64] + [ctypes.POINTER(ctypes.c_uint64)] * 4
        L.dmi_get_isosurface_holes_kernel_ms.argtypes = [vp, dp]
        L.dmi_get_isosurface_holes_pass_ms.argtypes = [vp, dp]
    if hasattr(L, "dmi_filter_isosurface_support"):
        L.dmi_filter_isosurface_support.argtypes = [vp, i32, dbl, i32, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
        L.dmi_download_isosurface_support.argtypes = [vp, ctypes.POINTER(ctypes.c_int32)]
        L.dmi_get_isosurface_support_kernel_ms.argtypes = [vp, dp]
        L.dmi_get_isosurface_support_pass_ms.argtypes = [vp, dp]
    if hasattr(L, "dmi_set_point_smoothing"):
        L.dmi_point_smoothing_weights.argtypes = [dbl, dbl, ctypes.POINTER(i32), dp]
        L.dmi_set_point_smoothing.argtypes = [vp, dp, dbl]
        L.dmi_get_point_smoothing.argtypes = [vp, dp, dp]
        L.dmi_get_point_smoothing_kernel_ms.argtypes = [vp, dp]
    L.dmi_get_brick_class_histogram.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    L.dmi_get_mixed_reason_histogram.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    if hasattr(L, "dmi_get_window_pair_count"):  # (absent from an older prebuilt library loaded for an A/B timing, tools/gpu_exp.py)
        L.dmi_get_window_pair_count.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    if hasattr(L, "dmi_get_view_paths"):
        L.dmi_get_view_paths.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    if hasattr(L, "dmi_get_upload_kernel_ms"):
        L.dmi_get_upload_kernel_ms.argtypes = [vp, dp, dp]
    for name in ("dmi_sizeof_info", "dmi_sizeof_timings"):
        if hasattr(L, name):
            getattr(L, name).restype = ctypes.c_size_t
    L.dmi_get_timings.argtypes = [vp, ctypes.POINTER(TimingsC)]
    L.dmi_get_info.argtypes = [vp, ctypes.POINTER(InfoC)]
    L.dmi_alloc_pinned.argtypes = [ctypes.c_size_t, ctypes.POINTER(vp)]
    L.dmi_free_pinned.argtypes = [vp]
    L.dmi_pcie_probe.argtypes = [i32, ctypes.c_size_t, dp, dp]
    L.dmi_fp64_probe.argtypes = [i32, ctypes.c_double, dp]
    u8p = ctypes.POINTER(ctypes.c_uint8)
    L.dmi_color_mesh.argtypes = [dp, ctypes.c_int64, u8p, dp, dp, i32, i32, i32, i32, u8p, u8p, ctypes.POINTER(ctypes.c_int32)]
    L.dmi_color_create.argtypes = [i32, ctypes.POINTER(vp)]
    L.dmi_color_destroy.argtypes = [vp]
    L.dmi_color_destroy.restype = None
    L.dmi_color_add_views.argtypes = [vp, u8p, dp, dp, i32, i32, i32]
    L.dmi_color_clear_views.argtypes = [vp]
    L.dmi_color_process.argtypes = [vp, dp, ctypes.c_int64, u8p, u8p, ctypes.POINTER(ctypes.c_int32)]
    L.dmi_color_get_kernel_ms.argtypes = [vp, dp]
    L.dmi_color_set_scratch_budget.argtypes = [vp, ctypes.c_uint64]
    L.dmi_color_set_vertex_reorder.argtypes = [vp, i32]
    L.dmi_color_add_views_with_depth.argtypes = [vp, u8p, dp, dp, dp, i32, i32, i32]
    L.dmi_color_set_depth_test.argtypes = [vp, i32, ctypes.c_double]
    L.dmi_color_last_error.argtypes = []
    L.dmi_color_process_isosurface.argtypes = [vp, vp, i32, dbl, ctypes.POINTER(ctypes.c_uint64)]
    L.dmi_download_isosurface_colors.argtypes = [vp, u8p, u8p, ctypes.POINTER(ctypes.c_int32)]
    L.dmi_get_isosurface_color_kernel_ms.argtypes = [vp, dp]
    L.dmi_color_last_error.restype = ctypes.c_char_p
    L.dmi_color_render_depths.argtypes = [vp, dp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.c_int64]
    L.dmi_color_render_isosurface_depths.argtypes = [vp, vp]
    L.dmi_color_download_depths.argtypes = [vp, i32, i32, dp]
    L.dmi_color_get_render_kernel_ms.argtypes = [vp, dp]
    L.dmi_color_set_render_queue_capacity.argtypes = [vp, ctypes.c_uint64]
    L.dmi_color_get_render_pass_ms.argtypes = [vp, dp]
    L.dmi_color_get_render_queued_pairs.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    i64, i64p, i32p = ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    if hasattr(L, "dmi_filter_depth_consistency"):
        L.dmi_filter_depth_consistency.argtypes = [dp, dp, dbl, dp, dp, i32, i32, i32, dbl, dbl, i32, i32, dp, i32p, dp]
    if hasattr(L, "dmi_estimate_scene_bounds"):
        L.dmi_estimate_scene_bounds.argtypes = [dp, dp, dbl, dp, dp, i32, i32, i32, dp, dbl, i32, i32, dp, dp,
                                                ctypes.POINTER(ctypes.c_uint64), dp]
    if hasattr(L, "dmi_filter_depth_speckles"):  # (DMI_LIB_OVERRIDE may name an older library)
        L.dmi_filter_depth_speckles.argtypes = [dp, dp, dbl, i32, i32, i32, dbl, dbl, i64, i32, dp, i32p, dp]
    if hasattr(L, "dmi_fill_depth_holes"):
        L.dmi_fill_depth_holes.argtypes = [dp, dp, dbl, i32, i32, i32, dbl, dbl, i64, i32, dp, i32p, dp]
    if hasattr(L, "dmi_smooth_depths"):
        L.dmi_depth_smoothing_weights.argtypes = [dbl, dbl, ctypes.POINTER(i32), dp]
        L.dmi_smooth_depths.argtypes = [dp, dp, dbl, i32, i32, i32, dbl, dbl, dbl, dbl, i32, i32, dp, i32p, dp]
    if hasattr(L, "dmi_views_create"):
        rp = ctypes.POINTER(ViewsStepReportC)
        L.dmi_views_create.argtypes = [i32, i32, i32, ctypes.POINTER(vp)]
        L.dmi_views_destroy.argtypes = [vp]
        L.dmi_views_destroy.restype = None
        L.dmi_views_last_error.argtypes = [vp]
        L.dmi_views_last_error.restype = ctypes.c_char_p
        L.dmi_views_add.argtypes = [vp, dp, dp, dbl, dp, dp, i32]
        L.dmi_views_clear.argtypes = [vp]
        L.dmi_views_get_info.argtypes = [vp, ctypes.POINTER(ViewsInfoC)]
        L.dmi_sizeof_views_info.restype = ctypes.c_size_t
        L.dmi_views_set_piece_bytes.argtypes = [vp, ctypes.c_uint64]
        L.dmi_views_filter_speckles.argtypes = [vp, dbl, dbl, i64, i32p, rp]
        L.dmi_views_fill_holes.argtypes = [vp, dbl, dbl, i64, i32p, rp]
        L.dmi_views_smooth.argtypes = [vp, dbl, dbl, dbl, dbl, i32, i32p, rp]
        L.dmi_views_filter_consistency.argtypes = [vp, dbl, dbl, i32, i32p, rp]
        L.dmi_views_estimate_bounds.argtypes = [vp, dp, dbl, i32, dp, dp, ctypes.POINTER(ctypes.c_uint64), dp]
        L.dmi_views_download.argtypes = [vp, i32, i32, dp]
        L.dmi_add_views_from_set.argtypes = [vp, vp, i32, i32]
    if hasattr(L, "dmi_views_build_points"):
        u64 = ctypes.c_uint64
        L.dmi_views_build_points.argtypes = [vp, dbl, dbl, dbl, dbl, i32, i32, i32, ctypes.POINTER(u64), ctypes.POINTER(ViewsPointsReportC)]
        L.dmi_views_download_points.argtypes = [vp, u64, u64, dp, ctypes.POINTER(ctypes.c_float), i32p, i32p, i32p]
        L.dmi_views_get_points_pass_ms.argtypes = [vp, dp]
    if hasattr(L, "dmi_thin_point_cloud"):
        u64, fp, u32p = ctypes.c_uint64, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
        tp = ctypes.POINTER(PointsThinReportC)
        L.dmi_thin_point_cloud.argtypes = [dp, fp, i32p, i32p, i32p, u64, dbl, i32, i32, dp, fp, i32p, i32p, i32p, u32p,
                                           ctypes.POINTER(u64), tp]
        L.dmi_views_thin_points.argtypes = [vp, dbl, i32, ctypes.POINTER(u64), tp]
        L.dmi_views_download_point_members.argtypes = [vp, u64, u64, u32p]
        L.dmi_views_get_thin_pass_ms.argtypes = [vp, dp]
        L.dmi_views_set_thin_wave_cell_points.argtypes = [vp, i32]
    if hasattr(L, "dmi_count_point_neighbors"):
        u32p, rp = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(PointsRadiusReportC)
        L.dmi_count_point_neighbors.argtypes = [dp, u64, dbl, i32, i32, u32p, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(u64), rp]
        L.dmi_views_filter_points_radius.argtypes = [vp, dbl, i32, ctypes.POINTER(u64), rp]
        L.dmi_views_download_point_neighbors.argtypes = [vp, u64, u64, u32p]
        L.dmi_views_get_radius_pass_ms.argtypes = [vp, dp]
        L.dmi_views_set_radius_group_points.argtypes = [vp, i32]
    if hasattr(L, "dmi_fit_point_planes"):
        u32p, fp, pp = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(PointsPlanesReportC)
        L.dmi_fit_point_planes.argtypes = [dp, fp, u64, dbl, i32, i32, i32, dp, fp, fp, u32p, pp]
        L.dmi_views_fit_point_planes.argtypes = [vp, dbl, i32, i32, pp]
        L.dmi_views_download_point_plane_rms.argtypes = [vp, u64, u64, fp]
        L.dmi_views_get_plane_fit_pass_ms.argtypes = [vp, dp]
    L.dmi_multi_default_options.argtypes = [ctypes.POINTER(MultiOptionsC)]
    L.dmi_multi_default_options.restype = None
    L.dmi_multi_view_shard.argtypes = [i64, i32, i32, i64p, i64p]
    L.dmi_multi_z_slab.argtypes = [i32, i32, i32, i32p, i32p]
    L.dmi_multi_slab_ranges.argtypes = [i32, i32, i32p, i32p, i32]
    if hasattr(L, "dmi_multi_peer_chunk"):
        L.dmi_multi_peer_chunk.argtypes = [i64, i32, i32, i64p, i64p]
    L.dmi_multi_create.argtypes = [ctypes.POINTER(GridDescC), ctypes.POINTER(RayPotentialC), ctypes.POINTER(MultiOptionsC),
                                   i32p, i32, ctypes.POINTER(vp)]
    L.dmi_multi_get_unique_id.argtypes = [u8p]
    L.dmi_multi_create_rank.argtypes = [ctypes.POINTER(GridDescC), ctypes.POINTER(RayPotentialC), ctypes.POINTER(MultiOptionsC),
                                        i32, i32, i32, u8p, ctypes.POINTER(vp)]
    L.dmi_multi_destroy.argtypes = [vp]
    L.dmi_multi_destroy.restype = None
    L.dmi_multi_last_error.argtypes = [vp]
    L.dmi_multi_last_error.restype = ctypes.c_char_p
    L.dmi_multi_add_views.argtypes = [vp, dp, dp, dbl, dp, dp, i32, i32, i32]
    L.dmi_multi_add_views_f32.argtypes = [vp, ctypes.POINTER(ctypes.c_float), dp, dp, i32, i32, i32]
    L.dmi_multi_add_local_views.argtypes = [vp, i32, dp, dp, dbl, dp, dp, i32, i32, i32]
    L.dmi_multi_add_local_views_f32.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_float), dp, dp, i32, i32, i32]
    L.dmi_multi_clear_views.argtypes = [vp]
    L.dmi_multi_fuse.argtypes = [vp]
    L.dmi_multi_synchronize.argtypes = [vp]
    L.dmi_multi_download_grid_f32.argtypes = [vp, ctypes.POINTER(ctypes.c_float), i64p, i64p]
    L.dmi_multi_download_grid_f64.argtypes = [vp, dp, i64p, i64p]
    L.dmi_multi_get_info.argtypes = [vp, ctypes.POINTER(MultiInfoC)]
    L.dmi_multi_get_timings.argtypes = [vp, ctypes.POINTER(MultiTimingsC)]
    L.dmi_multi_local_context.argtypes = [vp, i32, ctypes.POINTER(vp)]
    from . import build as _b
    for name in ABI_SYMBOLS:
        if _b.LIB_OVERRIDE and not hasattr(L, name):
            continue  # an older build loaded side by side for an A/B (tools/gpu_exp.py); the shipped library has them all
        fn = getattr(L, name)
        if fn.restype is ctypes.c_int:
            fn.restype = ctypes.c_int
    _lib = L
    return L


def pinned_empty(shape, dtype) -> np.ndarray:
    """A numpy array over pinned host memory (dmi_alloc_pinned): hipMemcpyAsync from it is a DMA transfer that overlaps
    with kernels.  Never freed by this helper's user explicitly: the block lives until the process ends."""
    L = load()
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = ctypes.c_void_p()
    rc = L.dmi_alloc_pinned(n, ctypes.byref(p))
    if rc != DMI_OK:
        raise DmiError(rc, "dmi_alloc_pinned failed")
    buf = (ctypes.c_char * n).from_address(p.value)
    return np.frombuffer(buf, dtype=dtype).reshape(shape)


def pcie_probe(device: int = 0, n_bytes: int = 256 << 20) -> tuple[float, float]:
    """(host-to-device, device-to-host) GB/s of one pinned hipMemcpyAsync each way (dmi_pcie_probe)."""
    L = load()
    a, b = ctypes.c_double(), ctypes.c_double()
    rc = L.dmi_pcie_probe(int(device), int(n_bytes), ctypes.byref(a), ctypes.byref(b))
    if rc != DMI_OK:
        raise DmiError(rc, L.dmi_last_error(None).decode())
    return float(a.value), float(b.value)


def fp64_probe(device: int = 0, milliseconds: float = 20.0) -> float:
    """fp64 vector TFLOP/s the device sustains right now on independent v_fma_f64 chains (dmi_fp64_probe)."""
    L = load()
    a = ctypes.c_double()
    rc = L.dmi_fp64_probe(int(device), float(milliseconds), ctypes.byref(a))
    if rc != DMI_OK:
        raise DmiError(rc, L.dmi_last_error(None).decode())
    return float(a.value)


def device_count() -> int:
    return int(load().dmi_device_count())


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


class FusionContext:
    """One fusion = one context (dmi_create ... dmi_destroy)."""

    def __init__(self, grid: GridDesc, ray: RayPotential, *, device: int = 0, grid_dtype: str = "f64",
                 depth_storage: str = "auto", count_hits: bool = False, kernel_variant: int = 0,
                 stream: int | None = None, external_grid: int | None = None, z_first: int = 0):
        self._lib = load()
        self._h = ctypes.c_void_p()
        g = _grid_c(grid)
        r = RayPotentialC(float(ray.thickness), float(ray.rho), float(ray.eta), float(ray.delta))
        o = OptionsC()
        self._lib.dmi_default_options(ctypes.byref(o))
        o.device = device
        o.grid_dtype = {"f32": DMI_F32, "f64": DMI_F64}[grid_dtype]
        o.depth_storage = {"auto": DMI_DEPTH_AUTO, "f32": DMI_DEPTH_F32, "f64": DMI_DEPTH_F64}[depth_storage]
        o.count_hits = 1 if count_hits else 0
        o.kernel_variant = int(kernel_variant)
        o.z_first = int(z_first)
        o.stream = stream
        o.external_grid = external_grid
        self.grid = grid
        self.grid_dtype = grid_dtype
        self.n_voxels = grid.n_voxels
        self._mesh_counts = None  # (vertices, triangles, kept components) of the context's mesh; None: no extraction has succeeded yet
        rc = self._lib.dmi_create(ctypes.byref(g), ctypes.byref(r), ctypes.byref(o), ctypes.byref(self._h))
        if rc != DMI_OK:
            self._h = ctypes.c_void_p()
            raise DmiError(rc, self._lib.dmi_last_error(None).decode())

    # -- plumbing ------------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc != DMI_OK:
            raise DmiError(rc, self._lib.dmi_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.dmi_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- views ---------------------------------------------------------------------------------
    def add_views(self, views: Views, threshold: float | None = None):
        n, H, W = views.depth.shape
        K4 = np.ascontiguousarray(views.K4, dtype=np.float64).reshape(n, 16)
        RT4 = np.ascontiguousarray(views.RT4, dtype=np.float64).reshape(n, 16)
        if views.depth.dtype == np.float32:
            if views.best_cost is not None and threshold is not None:
                raise ValueError("f32 depth upload takes already-thresholded depths")
            d = np.ascontiguousarray(views.depth)
            self._check(self._lib.dmi_add_views_f32(self._h, d.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                    _dp(K4), _dp(RT4), n, W, H))
            return
        d = np.ascontiguousarray(views.depth, dtype=np.float64)
        bc = None
        if views.best_cost is not None and threshold is not None:
            bc = np.ascontiguousarray(views.best_cost, dtype=np.float64)
        self._check(self._lib.dmi_add_views(self._h, _dp(d), _dp(bc) if bc is not None else None,
                                            float(threshold) if threshold is not None else 0.0,
                                            _dp(K4), _dp(RT4), n, W, H))

    def add_views_from_set(self, view_set: "ViewSet", first: int | None = None, count: int | None = None):
        """Append views [first, first + count) of a resident ViewSet (all of them by default) as add_views would append their
        downloaded depths: the upload pass reads the set's planes on the device, nothing passes through the host, and the set
        stays as it is (dmi_add_views_from_set)."""
        first = 0 if first is None else int(first)
        count = view_set.info().n - first if count is None else int(count)
        self._check(self._lib.dmi_add_views_from_set(self._h, view_set._h, first, count))

    def clear_views(self):
        self._check(self._lib.dmi_clear_views(self._h))

    # -- grid ----------------------------------------------------------------------------------
    def reset_grid(self):
        self._check(self._lib.dmi_reset_grid(self._h))

    def upload_grid(self, grid: np.ndarray):
        g = np.ascontiguousarray(grid, dtype=np.float64).reshape(-1)
        if g.size != self.n_voxels:
            raise ValueError("grid size does not match the context")
        self._check(self._lib.dmi_upload_grid(self._h, _dp(g)))

    def fuse(self, first: int | None = None, count: int | None = None):
        if first is None:
            self._check(self._lib.dmi_fuse(self._h))
        else:
            self._check(self._lib.dmi_fuse_range(self._h, int(first), int(count)))

    def fuse_slab(self, z_first: int, z_count: int):
        """Fuse every resident view into cell layers [z_first, z_first + z_count) (multiples of 32 cells)."""
        self._check(self._lib.dmi_fuse_slab(self._h, int(z_first), int(z_count)))

    def synchronize(self):
        self._check(self._lib.dmi_synchronize(self._h))

    def fuse_download(self, first: int, count: int, dtype=np.float64, out: np.ndarray | None = None, n_slabs: int = 8) -> np.ndarray:
        """Fuse views [first, first + count) and return the grid as [nz, ny, nx]: with `dtype` the grid's own type the grid is
        fused in `n_slabs` z-slabs and every slab is copied to the host under the fusion of the next ones
        (dmi_fuse_range_download); bit for bit what fuse(first, count) + download_grid(dtype) return."""
        nx, ny, nz = (int(c) for c in self.grid.cell_dims)
        if out is None:
            out = np.empty(self.n_voxels, dtype=dtype)
        if out.dtype != np.dtype(dtype) or out.size != self.n_voxels or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous array of n_voxels elements of the requested dtype")
        if not hasattr(self._lib, "dmi_fuse_range_download"):  # an older prebuilt library: the same bits, nothing overlapped
            if count > 0:
                self.fuse(int(first), int(count))
            return self.download_grid(dtype, out)
        self._check(self._lib.dmi_fuse_range_download(self._h, int(first), int(count), ctypes.c_void_p(out.ctypes.data),
                                                      DMI_F64 if np.dtype(dtype) == np.float64 else DMI_F32, int(n_slabs)))
        return out.reshape(nz, ny, nx)

    def download_grid(self, dtype=np.float64, out: np.ndarray | None = None) -> np.ndarray:
        """The grid as [nz, ny, nx]; `out` (flat, contiguous, e.g. from pinned_empty) receives it when given."""
        nx, ny, nz = (int(c) for c in self.grid.cell_dims)
        if out is None:
            out = np.empty(self.n_voxels, dtype=dtype)
        if out.dtype != np.dtype(dtype) or out.size != self.n_voxels or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous array of n_voxels elements of the requested dtype")
        if np.dtype(dtype) == np.float64:
            self._check(self._lib.dmi_download_grid_f64(self._h, _dp(out)))
        else:
            self._check(self._lib.dmi_download_grid_f32(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
        return out.reshape(nz, ny, nx)

    def download_hits(self):
        nx, ny, nz = (int(c) for c in self.grid.cell_dims)
        vh = np.empty(self.n_voxels, dtype=np.uint32)
        mh = np.empty(self.info().n_views, dtype=np.uint64)
        self._check(self._lib.dmi_download_hits(self._h, vh.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                                mh.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return vh.reshape(nz, ny, nx), mh

    def grid_device_pointer(self) -> int:
        p = ctypes.c_void_p()
        self._check(self._lib.dmi_grid_device_pointer(self._h, ctypes.byref(p)))
        return int(p.value)

    def cell_to_point(self):
        """vtkCellDataToPointData of the grid on the device (asynchronous; Reconstruction/main.cxx:151-155)."""
        self._check(self._lib.dmi_cell_to_point(self._h))

    def download_point_data(self) -> np.ndarray:
        """The point-data form of the grid, [nz+1, ny+1, nx+1] f64."""
        nx, ny, nz = (int(c) for c in self.grid.cell_dims)
        out = np.empty((nz + 1) * (ny + 1) * (nx + 1), dtype=np.float64)
        self._check(self._lib.dmi_download_point_data_f64(self._h, _dp(out)))
        return out.reshape(nz + 1, ny + 1, nx + 1)

    def set_point_smoothing(self, sigma, truncate: float = 3.0) -> None:
        """A Gaussian over the point data from now on: every computation of the point data is followed by three separable
        passes with `sigma` lattice steps per axis (a scalar stands for all three; 0 skips an axis, all 0 switch it off),
        cut off at `truncate` sigmas, and download_point_data, iso_active_cells and the extractions read the smoothed field
        (dmi_set_point_smoothing).  A refused call keeps the old setting."""
        s = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (3,)))
        self._check(self._lib.dmi_set_point_smoothing(self._h, _dp(s), float(truncate)))

    def point_smoothing(self):
        """(sigma [3] f64, truncate) of the setting (dmi_get_point_smoothing); zeros and 3.0 in a new context."""
        s, t = np.zeros(3, dtype=np.float64), ctypes.c_double(0)
        self._check(self._lib.dmi_get_point_smoothing(self._h, _dp(s), ctypes.byref(t)))
        return s, float(t.value)

    def point_smoothing_kernel_ms(self) -> float:
        """hipEvent milliseconds of the smoothing kernels of the last computation of the point data; 0 while the setting is off
        (dmi_get_point_smoothing_kernel_ms)."""
        return self._get_ms("dmi_get_point_smoothing_kernel_ms")

    def iso_active_cells(self, iso: float, ids: bool = True):
        """(count, ids): the cells whose corner point values straddle `iso` (dmi_iso_active_cells); ids ascending int64, or
        None when ids=False."""
        n = ctypes.c_uint64(0)
        self._check(self._lib.dmi_iso_active_cells(self._h, float(iso), ctypes.byref(n), None, 0))
        if not ids:
            return int(n.value), None
        out = np.empty(int(n.value), dtype=np.int64)
        if n.value:
            self._check(self._lib.dmi_iso_active_cells(self._h, float(iso), ctypes.byref(n),
                                                       out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), out.size))
        return int(n.value), out

    def extract_isosurface(self, iso: float):
        """(vertices [n, 3] f64 world coordinates, triangles [m, 3] int64): marching cubes over the point data at `iso` on the
        device (dmi_extract_isosurface + dmi_download_isosurface; Reconstruction/main.cxx:166-182)."""
        nv, nt = ctypes.c_uint64(0), ctypes.c_uint64(0)
        # (a refused extraction -- a NaN iso -- leaves the mesh of the last successful one, and these counts with it; one that fails
        # later leaves no mesh on the C side, which then refuses the downloads itself)
        self._check(self._lib.dmi_extract_isosurface(self._h, float(iso), ctypes.byref(nv), ctypes.byref(nt)))
        verts = np.empty((max(int(nv.value), 1), 3), dtype=np.float64)    # never a null pointer, even for an empty mesh
        tris = np.empty((max(int(nt.value), 1), 3), dtype=np.int64)
        self._mesh_is(nv.value, nt.value)
        self._check(self._lib.dmi_download_isosurface(self._h, _dp(verts), tris.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return verts[:int(nv.value)], tris[:int(nt.value)]

    def extract_isosurface_with_normals(self, iso: float):
        """(vertices [n, 3] f64, triangles [m, 3] int64, normals [n, 3] f32): extract_isosurface's mesh, bit for bit, and one
        unit normal per vertex from the point data's gradient, in world coordinates (dmi_extract_isosurface_normals +
        dmi_download_isosurface + dmi_download_isosurface_normals)."""
        nv, nt = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self._lib.dmi_extract_isosurface_normals(self._h, float(iso), ctypes.byref(nv), ctypes.byref(nt)))   # (as above)
        verts = np.empty((max(int(nv.value), 1), 3), dtype=np.float64)    # never a null pointer, even for an empty mesh
        tris = np.empty((max(int(nt.value), 1), 3), dtype=np.int64)
        normals = np.empty((max(int(nv.value), 1), 3), dtype=np.float32)
        self._mesh_is(nv.value, nt.value)
        self._check(self._lib.dmi_download_isosurface(self._h, _dp(verts), tris.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        self._check(self._lib.dmi_download_isosurface_normals(self._h, normals.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
        return verts[:int(nv.value)], tris[:int(nt.value)], normals[:int(nv.value)]

    def filter_isosurface_components(self, mode: str = "min_triangles", min_triangles: int = 0):
        """(vertices, triangles, components found, components kept): label the connected components of the context's mesh -- the
        last extraction's, or the last filter's since -- and keep those of at least `min_triangles` triangles
        (mode="min_triangles") or the largest one (mode="largest"); the mesh is compacted on the device
        (dmi_filter_isosurface_components).  download_isosurface* return the filtered mesh afterwards."""
        m = {"min_triangles": DMI_COMPONENTS_MIN_TRIANGLES, "largest": DMI_COMPONENTS_LARGEST}[mode]
        out = [ctypes.c_uint64(0) for _ in range(4)]
        self._check(self._lib.dmi_filter_isosurface_components(self._h, m, int(min_triangles), *[ctypes.byref(x) for x in out]))
        self._mesh_is(out[0].value, out[1].value, regions=out[3].value)
        return tuple(int(x.value) for x in out)

    def _get_ms(self, symbol: str) -> float:
        a = ctypes.c_double(0)
        self._check(getattr(self._lib, symbol)(self._h, ctypes.byref(a)))
        return float(a.value)

    def _get_pass_ms(self, symbol: str, names) -> dict:
        a = (ctypes.c_double * len(names))()
        self._check(getattr(self._lib, symbol)(self._h, a))
        return dict(zip(names, (float(x) for x in a)))

    def _get_u64(self, symbol: str) -> int:
        a = ctypes.c_uint64(0)
        self._check(getattr(self._lib, symbol)(self._h, ctypes.byref(a)))
        return int(a.value)

    def _mesh_is(self, nv, nt, regions=0):
        """The sizes of the C side's mesh after a call that changed it (the downloads size their arrays by them): an extraction's, a
        decimation's, a fill's and a trim's counts with no regions, the component filter's with the components it kept."""
        self._mesh_counts = (int(nv), int(nt), int(regions))

    def _current_mesh_counts(self):
        c = self._mesh_counts      # a refused filter changes neither the C side's mesh nor these
        if c is None:
            raise DmiError(1, "no mesh: extract_isosurface has not succeeded")
        return c

    def download_isosurface(self):
        """(vertices [n, 3] f64, triangles [m, 3] int64) of the context's current mesh: the last extraction's, or the last
        filter_isosurface_components' since (dmi_download_isosurface)."""
        nv, nt, _ = self._current_mesh_counts()
        verts = np.empty((max(nv, 1), 3), dtype=np.float64)    # never a null pointer, even for an empty mesh
        tris = np.empty((max(nt, 1), 3), dtype=np.int64)
        self._check(self._lib.dmi_download_isosurface(self._h, _dp(verts), tris.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return verts[:nv], tris[:nt]

    def download_isosurface_normals(self):
        """normals [n, 3] f32 of the context's current mesh after filter_isosurface_components (the extraction had them)."""
        nv, _, _ = self._current_mesh_counts()
        normals = np.empty((max(nv, 1), 3), dtype=np.float32)
        self._check(self._lib.dmi_download_isosurface_normals(self._h, normals.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
        return normals[:nv]

    def download_isosurface_regions(self):
        """(RegionId [n] int64: each vertex's component, RegionSize [k] int64: each kept component's triangles) of the last
        filter_isosurface_components; components are numbered by ascending smallest vertex id (dmi_download_isosurface_regions)."""
        nv, _, nk = self._current_mesh_counts()
        rid = np.empty(max(nv, 1), dtype=np.int64)
        rsz = np.empty(max(nk, 1), dtype=np.int64)
        i64p = ctypes.POINTER(ctypes.c_int64)
        self._check(self._lib.dmi_download_isosurface_regions(self._h, rid.ctypes.data_as(i64p), rsz.ctypes.data_as(i64p)))
        return rid[:nv], rsz[:nk]

    def isosurface_filter_kernel_ms(self) -> float:
        """hipEvent milliseconds of the kernels of the last filter_isosurface_components (dmi_get_isosurface_filter_kernel_ms)."""
        return self._get_ms("dmi_get_isosurface_filter_kernel_ms")

    def isosurface_filter_cas_retries(self) -> int:
        """Compare-and-swaps of the last filter's hooking pass that lost a race (dmi_get_isosurface_filter_cas_retries)."""
        return self._get_u64("dmi_get_isosurface_filter_cas_retries")

    def isosurface_filter_pass_ms(self) -> dict:
        """The same pass by pass (dmi_get_isosurface_filter_pass_ms)."""
        return self._get_pass_ms("dmi_get_isosurface_filter_pass_ms", ("labels", "sizes", "scans", "compaction"))

    def smooth_isosurface(self, iterations: int, lam: float = 0.5, mu: float = -0.53) -> None:
        """Taubin lambda|mu smoothing of the context's mesh on the device, `iterations` times a step with `lam` and (mu != 0) one
        with `mu`; boundary vertices stay; normals, if the mesh has them, become the smoothed mesh's geometric ones
        (dmi_smooth_isosurface).  download_isosurface* return the smoothed mesh afterwards."""
        self._check(self._lib.dmi_smooth_isosurface(self._h, int(iterations), float(lam), float(mu)))

    def isosurface_smooth_kernel_ms(self) -> float:
        """hipEvent milliseconds of the kernels of the last smooth_isosurface (dmi_get_isosurface_smooth_kernel_ms)."""
        return self._get_ms("dmi_get_isosurface_smooth_kernel_ms")

    def isosurface_smooth_pass_ms(self) -> dict:
        """The same pass by pass (dmi_get_isosurface_smooth_pass_ms)."""
        return self._get_pass_ms("dmi_get_isosurface_smooth_pass_ms", ("adjacency", "steps", "normals"))

    def decimate_isosurface(self, cell_size: float, placement: str = "mean"):
        """(vertices, triangles) left after vertex clustering of the context's mesh on the device with cubic cells of `cell_size`
        world units: every cluster becomes the mean of its members, collapsed and duplicate triangles and unreferenced vertices
        go; normals, if the mesh has them, become the decimated mesh's geometric ones; the regions of an earlier filter are
        dropped (dmi_decimate_isosurface).  download_isosurface* return the decimated mesh afterwards.
        placement="quadric" puts every cluster's vertex where the planes of its triangles meet instead (creases and corners stay;
        the triangles are the same; dmi_decimate_isosurface_placed); any other string is a ValueError."""
        if placement not in DECIMATE_PLACEMENTS:
            raise ValueError(f"decimate_isosurface: placement {placement!r} is not one of {sorted(DECIMATE_PLACEMENTS)}")
        nv, nt = ctypes.c_uint64(0), ctypes.c_uint64(0)
        if placement == "mean":
            self._check(self._lib.dmi_decimate_isosurface(self._h, float(cell_size), ctypes.byref(nv), ctypes.byref(nt)))
        else:
            self._check(self._lib.dmi_decimate_isosurface_placed(self._h, float(cell_size), DECIMATE_PLACEMENTS[placement],
                                                                 ctypes.byref(nv), ctypes.byref(nt)))
        self._mesh_is(nv.value, nt.value)
        return int(nv.value), int(nt.value)

    def isosurface_decimate_kernel_ms(self) -> float:
        """hipEvent milliseconds of the kernels of the last decimate_isosurface (dmi_get_isosurface_decimate_kernel_ms)."""
        return self._get_ms("dmi_get_isosurface_decimate_kernel_ms")

    def isosurface_decimate_pass_ms(self) -> dict:
        """The same pass by pass (dmi_get_isosurface_decimate_pass_ms)."""
        return self._get_pass_ms("dmi_get_isosurface_decimate_pass_ms", ("clustering", "representatives", "triangles", "normals"))

    def fill_isosurface_holes(self, max_edges: int):
        """(vertices, triangles, holes filled, boundary edges left) after the small holes of the context's mesh are closed on the
        device: every boundary loop of 3 .. `max_edges` edges whose vertices each have one boundary edge in and one out gets one
        triangle (3 edges) or a new vertex at the mean of its rim and a fan round it; the old vertices and triangles stay in
        place, the new ones follow them; normals, if the mesh has them, stay and the new vertices get geometric ones; the regions,
        support counts and colours of earlier calls are dropped when something was filled (dmi_fill_isosurface_holes; DESIGN.md
        8f).  download_isosurface* return the filled mesh afterwards."""
        out = [ctypes.c_uint64(0) for _ in range(4)]
        self._check(self._lib.dmi_fill_isosurface_holes(self._h, int(max_edges), *[ctypes.byref(x) for x in out]))
        if out[2].value:   # something was filled
            self._mesh_is(out[0].value, out[1].value)
        return tuple(int(x.value) for x in out)

    def isosurface_holes_kernel_ms(self) -> float:
        """hipEvent milliseconds of the kernels of the last fill_isosurface_holes (dmi_get_isosurface_holes_kernel_ms)."""
        return self._get_ms("dmi_get_isosurface_holes_kernel_ms")

    def isosurface_holes_pass_ms(self) -> dict:
        """The same pass by pass (dmi_get_isosurface_holes_pass_ms)."""
        return self._get_pass_ms("dmi_get_isosurface_holes_pass_ms", ("boundary", "loops", "fill"))

    def filter_isosurface_support(self, min_views: int, tolerance: float, facing: bool = True):
        """(vertices, triangles) left after the trim of the context's mesh by view support on the device: every vertex is given the
        number of resident views that saw it -- in front of the camera, inside the image, within `tolerance` of the depth the
        fusion kept at its pixel and, with `facing`, with its normal towards the camera -- and only the triangles whose three
        vertices have at least `min_views` such views stay, with the vertices they name.  min_views 0: the counts only
        (dmi_filter_isosurface_support).  download_isosurface* return the trimmed mesh afterwards."""
        nv, nt = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self._lib.dmi_filter_isosurface_support(self._h, int(min_views), float(tolerance), 1 if facing else 0,
                                                            ctypes.byref(nv), ctypes.byref(nt)))
        old = self._mesh_counts
        if old is None or (int(nv.value), int(nt.value)) != old[:2]:   # something went: the regions of an earlier filter too
            self._mesh_is(nv.value, nt.value)
        return int(nv.value), int(nt.value)

    def download_isosurface_support(self):
        """support [n] int32: the supporting views of every vertex of the mesh as the last filter_isosurface_support left it
        (dmi_download_isosurface_support)."""
        nv, _, _ = self._current_mesh_counts()
        support = np.zeros(max(nv, 1), dtype=np.int32)    # never a null pointer, even for an empty mesh
        self._check(self._lib.dmi_download_isosurface_support(self._h, support.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return support[:nv]

    def isosurface_support_kernel_ms(self) -> float:
        """hipEvent milliseconds of the kernels of the last filter_isosurface_support (dmi_get_isosurface_support_kernel_ms)."""
        return self._get_ms("dmi_get_isosurface_support_kernel_ms")

    def isosurface_support_pass_ms(self) -> dict:
        """The same pass by pass (dmi_get_isosurface_support_pass_ms)."""
        return self._get_pass_ms("dmi_get_isosurface_support_pass_ms", ("counts", "scans", "compaction"))

    def color_isosurface(self, color_ctx: "ColorContext", fused_depth_tolerance: float | None = None) -> int:
        """Colour the context's mesh where it is, with the views resident in `color_ctx`; returns the number of vertices.  The
        three arrays stay on the device until download_isosurface_colors.  fused_depth_tolerance None: what
        color_ctx.process(<the downloaded vertices>) returns, bit for bit.  A number: the visibility test with the depths this
        context fused (thresholded by the best cost), view m of `color_ctx` being view m of this context
        (dmi_color_process_isosurface).  Any later change of the mesh drops the colours."""
        nv = ctypes.c_uint64(0)
        fused = fused_depth_tolerance is not None
        self._check(self._lib.dmi_color_process_isosurface(color_ctx._h, self._h, 1 if fused else 0,
                                                           float(fused_depth_tolerance) if fused else 0.0, ctypes.byref(nv)))
        return int(nv.value)

    def download_isosurface_colors(self):
        """(mean [n, 3] u8, median [n, 3] u8, count [n] i32) of the last color_isosurface (dmi_download_isosurface_colors)."""
        nv, _, _ = self._current_mesh_counts()
        mean = np.zeros((max(nv, 1), 3), dtype=np.uint8)    # never a null pointer: null means "not wanted"
        median = np.zeros((max(nv, 1), 3), dtype=np.uint8)
        count = np.zeros(max(nv, 1), dtype=np.int32)
        u8 = ctypes.POINTER(ctypes.c_uint8)
        self._check(self._lib.dmi_download_isosurface_colors(self._h, mean.ctypes.data_as(u8), median.ctypes.data_as(u8),
                                                             count.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return mean[:nv], median[:nv], count[:nv]

    def render_isosurface_depths(self, color_ctx: "ColorContext") -> None:
        """Render the context's mesh, where it is, into the depth planes of every view resident in `color_ctx`: bit for bit what
        color_ctx.render_depths(*download_isosurface()) leaves (dmi_color_render_isosurface_depths; DESIGN.md 8b'')."""
        self._check(self._lib.dmi_color_render_isosurface_depths(color_ctx._h, self._h))

    def isosurface_color_kernel_ms(self) -> float:
        """hipEvent milliseconds of the kernels of the last color_isosurface (dmi_get_isosurface_color_kernel_ms)."""
        return self._get_ms("dmi_get_isosurface_color_kernel_ms")

    def isosurface_kernel_ms(self) -> float:
        """hipEvent milliseconds of the kernels of the last extract_isosurface or extract_isosurface_with_normals
        (dmi_get_isosurface_kernel_ms)."""
        return self._get_ms("dmi_get_isosurface_kernel_ms")

    def brick_class_histogram(self) -> dict:
        """(brick, view) pairs of the last fuse by proven class (diagnostic)."""
        h = (ctypes.c_uint64 * 4)()
        self._check(self._lib.dmi_get_brick_class_histogram(self._h, h))
        return {"mixed": int(h[0]), "free": int(h[1]), "behind": int(h[2]), "skip": int(h[3])}

    def mixed_reason_histogram(self) -> dict:
        """Why the mixed (brick, view) pairs of the last fuse could not be proven uniform (diagnostic)."""
        h = (ctypes.c_uint64 * 8)()
        self._check(self._lib.dmi_get_mixed_reason_histogram(self._h, h))
        names = ["unspecified", "degenerate", "camera_plane", "image_border", "nan_depth", "sentinel_and_depth", "near_surface",
                 "free_or_no_depth"]
        return {n: int(h[i]) for i, n in enumerate(names)}

    def window_pair_count(self) -> int:
        """How many "free_or_no_depth" pairs of the last fuse were served from a window of validity bits (diagnostic)."""
        n = ctypes.c_uint64(0)
        if not hasattr(self._lib, "dmi_get_window_pair_count"):
            return 0
        self._check(self._lib.dmi_get_window_pair_count(self._h, ctypes.byref(n)))
        return int(n.value)

    def upload_kernel_ms(self) -> tuple:
        """(last, total) hipEvent milliseconds of the upload pass's kernels (dmi_get_upload_kernel_ms)."""
        if not hasattr(self._lib, "dmi_get_upload_kernel_ms"):
            return (0.0, 0.0)
        a, b = ctypes.c_double(0), ctypes.c_double(0)
        self._check(self._lib.dmi_get_upload_kernel_ms(self._h, ctypes.byref(a), ctypes.byref(b)))
        return (float(a.value), float(b.value))

    def timings(self) -> TimingsC:
        t = TimingsC()
        self._check(self._lib.dmi_get_timings(self._h, ctypes.byref(t)))
        return t

    def info(self) -> InfoC:
        i = InfoC()
        self._check(self._lib.dmi_get_info(self._h, ctypes.byref(i)))
        return i

    def view_paths(self) -> dict:
        """How many resident views take which path (dmi_get_view_paths)."""
        names = ("general_kernel", "tiled_general_k", "tiled_fp64_selection", "tiled_tier1", "tiled_tier1_per_lane_margin", "with_window_record")
        if not hasattr(self._lib, "dmi_get_view_paths"):
            return {}
        a = (ctypes.c_uint64 * 6)()
        self._check(self._lib.dmi_get_view_paths(self._h, a))
        return {k: int(v) for k, v in zip(names, a)}


def _grid_c(grid: GridDesc) -> GridDescC:
    g = GridDescC()
    for i in range(3):
        g.cell_dims[i] = int(grid.cell_dims[i])
        g.origin[i] = float(grid.origin[i])
        g.spacing[i] = float(grid.spacing[i])
    gm = np.ascontiguousarray(grid.grid_matrix, dtype=np.float64).reshape(16)
    for i in range(16):
        g.grid_matrix[i] = gm[i]
    return g


def multi_view_shard(n: int, rank: int, world: int) -> tuple[int, int]:
    """[lo, hi) of n items for `rank` of `world` (dmi_multi_view_shard; needs no GPU)."""
    a, b = ctypes.c_int64(), ctypes.c_int64()
    if load().dmi_multi_view_shard(int(n), int(rank), int(world), ctypes.byref(a), ctypes.byref(b)) != DMI_OK:
        raise ValueError("rank/world out of range")
    return int(a.value), int(a.value + b.value)


def multi_z_slab(nz: int, rank: int, world: int) -> tuple[int, int]:
    """Cell layers [z0, z1) of `rank` under DMI_PARTITION_Z_SLABS (dmi_multi_z_slab; needs no GPU)."""
    a, b = ctypes.c_int32(), ctypes.c_int32()
    if load().dmi_multi_z_slab(int(nz), int(rank), int(world), ctypes.byref(a), ctypes.byref(b)) != DMI_OK:
        raise ValueError("rank/world out of range")
    return int(a.value), int(a.value + b.value)


def multi_peer_chunk(n: int, world: int, c: int) -> tuple[int, int]:
    """[first, first + count) of an n-element slab that rank c of a peer-copy exchange sums (dmi_multi_peer_chunk)."""
    a, b = ctypes.c_int64(), ctypes.c_int64()
    rc = load().dmi_multi_peer_chunk(int(n), int(world), int(c), ctypes.byref(a), ctypes.byref(b))
    if rc != DMI_OK:
        raise DmiError(rc, "dmi_multi_peer_chunk: invalid argument")
    return int(a.value), int(b.value)


def multi_slab_ranges(nz: int, n_slabs: int) -> list[tuple[int, int]]:
    """(z_first, z_count) of the z-slabs of the overlapped exchange (dmi_multi_slab_ranges; needs no GPU)."""
    a, b = (ctypes.c_int32 * 64)(), (ctypes.c_int32 * 64)()
    n = load().dmi_multi_slab_ranges(int(nz), int(n_slabs), a, b, 64)
    return [(int(a[i]), int(b[i])) for i in range(n)]


def multi_unique_id() -> bytes:
    """The 128-byte id rank 0 creates and the launcher hands to every rank (dmi_multi_get_unique_id)."""
    L = load()
    buf = (ctypes.c_uint8 * DMI_UNIQUE_ID_BYTES)()
    rc = L.dmi_multi_get_unique_id(buf)
    if rc != DMI_OK:
        raise DmiError(rc, L.dmi_multi_last_error(None).decode())
    return bytes(buf)


class MultiContext:
    """One fusion over several GPUs (dmi_multi_create / dmi_multi_create_rank ... dmi_multi_destroy).

    devices=[...]                      all ranks in this process
    rank=, world=, unique_id=, device= one rank per process (unique_id from multi_unique_id() on rank 0)"""

    def __init__(self, grid: GridDesc, ray: RayPotential, *, devices=None, rank: int | None = None, world: int | None = None,
                 unique_id: bytes | None = None, device: int = 0, grid_dtype: str = "f32", depth_storage: str = "auto",
                 kernel_variant: int = 0, partition: str = "views", exchange: str = "all_reduce", n_slabs: int = 0):
        self._lib = load()
        self._h = ctypes.c_void_p()
        o = MultiOptionsC()
        self._lib.dmi_multi_default_options(ctypes.byref(o))
        o.grid_dtype = {"f32": DMI_F32, "f64": DMI_F64}[grid_dtype]
        o.depth_storage = {"auto": DMI_DEPTH_AUTO, "f32": DMI_DEPTH_F32, "f64": DMI_DEPTH_F64}[depth_storage]
        o.kernel_variant = int(kernel_variant)
        o.partition = {"views": DMI_PARTITION_VIEWS, "z_slabs": DMI_PARTITION_Z_SLABS}[partition]
        o.exchange = {"all_reduce": DMI_EXCHANGE_ALL_REDUCE, "reduce_scatter": DMI_EXCHANGE_REDUCE_SCATTER,
                      "peer_copy": DMI_EXCHANGE_PEER_COPY}[exchange]
        o.n_slabs = int(n_slabs)
        g = _grid_c(grid)
        r = RayPotentialC(float(ray.thickness), float(ray.rho), float(ray.eta), float(ray.delta))
        self.grid = grid
        self.grid_dtype = grid_dtype
        self.n_voxels = grid.n_voxels
        if devices is not None:
            d = (ctypes.c_int32 * len(devices))(*[int(x) for x in devices])
            rc = self._lib.dmi_multi_create(ctypes.byref(g), ctypes.byref(r), ctypes.byref(o), d, len(devices), ctypes.byref(self._h))
        else:
            if rank is None or world is None:
                raise ValueError("MultiContext needs devices=[...] or rank= and world=")
            idbuf = None
            if unique_id is not None:
                if len(unique_id) != DMI_UNIQUE_ID_BYTES:
                    raise ValueError("unique_id must be 128 bytes")
                idbuf = (ctypes.c_uint8 * DMI_UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
            rc = self._lib.dmi_multi_create_rank(ctypes.byref(g), ctypes.byref(r), ctypes.byref(o), int(device), int(rank),
                                                 int(world), idbuf, ctypes.byref(self._h))
        if rc != DMI_OK:
            self._h = ctypes.c_void_p()
            raise DmiError(rc, self._lib.dmi_multi_last_error(None).decode())

    def _check(self, rc: int):
        if rc != DMI_OK:
            raise DmiError(rc, self._lib.dmi_multi_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.dmi_multi_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_views(self, views: Views, threshold: float | None = None, local_index: int | None = None):
        """local_index None: the SAME batch on every rank; each rank takes its share (views partition) or all of it
        (z-slabs).  local_index i: views of local rank i alone (the caller has partitioned, dmi_multi_add_local_views)."""
        n, H, W = views.depth.shape
        K4 = np.ascontiguousarray(views.K4, dtype=np.float64).reshape(n, 16)
        RT4 = np.ascontiguousarray(views.RT4, dtype=np.float64).reshape(n, 16)
        L = self._lib
        if views.depth.dtype == np.float32:
            d = np.ascontiguousarray(views.depth)
            dptr = d.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
            if local_index is None:
                self._check(L.dmi_multi_add_views_f32(self._h, dptr, _dp(K4), _dp(RT4), n, W, H))
            else:
                self._check(L.dmi_multi_add_local_views_f32(self._h, int(local_index), dptr, _dp(K4), _dp(RT4), n, W, H))
            return
        d = np.ascontiguousarray(views.depth, dtype=np.float64)
        bc = None
        if views.best_cost is not None and threshold is not None:
            bc = np.ascontiguousarray(views.best_cost, dtype=np.float64)
        thr = float(threshold) if threshold is not None else 0.0
        if local_index is None:
            self._check(L.dmi_multi_add_views(self._h, _dp(d), _dp(bc) if bc is not None else None, thr, _dp(K4), _dp(RT4), n, W, H))
        else:
            self._check(L.dmi_multi_add_local_views(self._h, int(local_index), _dp(d), _dp(bc) if bc is not None else None, thr,
                                                    _dp(K4), _dp(RT4), n, W, H))

    def clear_views(self):
        self._check(self._lib.dmi_multi_clear_views(self._h))

    def fuse(self):
        self._check(self._lib.dmi_multi_fuse(self._h))

    def synchronize(self):
        self._check(self._lib.dmi_multi_synchronize(self._h))

    def download_grid(self, dtype=np.float32, out: np.ndarray | None = None):
        """(grid as [nz, ny, nx], (first, count)): the element range of the flat grid this process's ranks own."""
        nx, ny, nz = (int(c) for c in self.grid.cell_dims)
        if out is None:
            out = np.zeros(self.n_voxels, dtype=dtype)
        a, b = ctypes.c_int64(), ctypes.c_int64()
        if np.dtype(dtype) == np.float64:
            self._check(self._lib.dmi_multi_download_grid_f64(self._h, _dp(out), ctypes.byref(a), ctypes.byref(b)))
        else:
            self._check(self._lib.dmi_multi_download_grid_f32(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                              ctypes.byref(a), ctypes.byref(b)))
        return out.reshape(nz, ny, nx), (int(a.value), int(b.value))

    def info(self) -> MultiInfoC:
        i = MultiInfoC()
        self._check(self._lib.dmi_multi_get_info(self._h, ctypes.byref(i)))
        return i

    def timings(self) -> MultiTimingsC:
        t = MultiTimingsC()
        self._check(self._lib.dmi_multi_get_timings(self._h, ctypes.byref(t)))
        return t

    def local_timings(self, local_index: int = 0) -> TimingsC:
        """dmi_timings of one local rank's single-GPU context."""
        h = ctypes.c_void_p()
        self._check(self._lib.dmi_multi_local_context(self._h, int(local_index), ctypes.byref(h)))
        t = TimingsC()
        if h:
            rc = self._lib.dmi_get_timings(h, ctypes.byref(t))
            if rc != DMI_OK:
                raise DmiError(rc, self._lib.dmi_last_error(h).decode())
        return t

    def local_context_grid(self, local_index: int, dtype=np.float32) -> np.ndarray:
        """The grid as local rank `local_index` holds it (after an all-reduce exchange every rank holds the sums)."""
        h = ctypes.c_void_p()
        self._check(self._lib.dmi_multi_local_context(self._h, int(local_index), ctypes.byref(h)))
        nx, ny, nz = (int(c) for c in self.grid.cell_dims)
        out = np.zeros(self.n_voxels, dtype=dtype)
        if np.dtype(dtype) == np.float64:
            rc = self._lib.dmi_download_grid_f64(h, _dp(out))
        else:
            rc = self._lib.dmi_download_grid_f32(h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        if rc != DMI_OK:
            raise DmiError(rc, self._lib.dmi_last_error(h).decode())
        return out.reshape(nz, ny, nx)

    def local_info(self, local_index: int = 0) -> InfoC:
        h = ctypes.c_void_p()
        self._check(self._lib.dmi_multi_local_context(self._h, int(local_index), ctypes.byref(h)))
        i = InfoC()
        if h:
            self._lib.dmi_get_info(h, ctypes.byref(i))
        return i


def color_mesh(points, colors, K4, RT4, device: int = 0):
    """MeshColoration::ProcessColoration on the GPU (include/dmi.h: dmi_color_mesh).
    points [nv,3] f64; colors [n,H,W,3] u8 in vtk row order; returns (mean u8[nv,3], median u8[nv,3], count i32[nv])."""
    L = load()
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    col = np.ascontiguousarray(colors, dtype=np.uint8)
    n, H, W, _ = col.shape
    k = np.ascontiguousarray(K4, dtype=np.float64).reshape(n, 16)
    rt = np.ascontiguousarray(RT4, dtype=np.float64).reshape(n, 16)
    nv = pts.shape[0]
    mean = np.zeros((nv, 3), dtype=np.uint8)
    median = np.zeros((nv, 3), dtype=np.uint8)
    count = np.zeros(nv, dtype=np.int32)
    u8 = ctypes.POINTER(ctypes.c_uint8)
    rc = L.dmi_color_mesh(_dp(pts), nv, col.ctypes.data_as(u8), _dp(k), _dp(rt), n, W, H, device, mean.ctypes.data_as(u8),
                          median.ctypes.data_as(u8), count.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    if rc != DMI_OK:
        raise DmiError(rc, L.dmi_color_last_error().decode())
    return mean, median, count


def filter_depth_consistency(views: Views, *, min_views: int, abs_tolerance: float = 0.0, rel_tolerance: float = 0.0,
                             threshold: float | None = None, device: int = 0, out: np.ndarray | None = None):
    """Depth maps filtered by cross-view consistency (include/dmi.h: dmi_filter_depth_consistency): a depth is kept only where at
    least min_views other views hold a depth within abs_tolerance + rel_tolerance * z of the same world point's camera z.
    threshold applies views.best_cost first (best cost > threshold => -1).  Returns (Views with the filtered depths, the same cameras
    and best_cost None; counts int32 [n, H, W]; the kernels' hipEvent time in ms).  out: where the filtered depths go; it may be
    views.depth itself (f64, C-contiguous), which is then filtered in place."""
    L = load()
    d = np.ascontiguousarray(views.depth, dtype=np.float64)
    if d.ndim != 3:
        raise ValueError(f"views.depth must be [n, H, W], got {d.shape}")
    n, H, W = d.shape
    k = np.ascontiguousarray(views.K4, dtype=np.float64).reshape(-1)
    rt = np.ascontiguousarray(views.RT4, dtype=np.float64).reshape(-1)
    if k.size != 16 * n or rt.size != 16 * n:
        raise ValueError("views.K4 and views.RT4 must be [n, 4, 4]")
    bc = None
    if threshold is not None and views.best_cost is not None:
        bc = np.ascontiguousarray(views.best_cost, dtype=np.float64)
        if bc.shape != d.shape:
            raise ValueError("views.best_cost must have the shape of views.depth")
    if out is None:
        out = np.empty_like(d)
    elif out.dtype != np.float64 or out.shape != d.shape or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous f64 array of the depths' shape")
    counts = np.zeros(d.shape, dtype=np.int32)
    ms = ctypes.c_double(0.0)
    rc = L.dmi_filter_depth_consistency(_dp(d), None if bc is None else _dp(bc), 0.0 if threshold is None else float(threshold), _dp(k),
                                        _dp(rt), n, W, H, float(abs_tolerance), float(rel_tolerance), int(min_views), int(device),
                                        _dp(out), counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(ms))
    if rc != DMI_OK:
        raise DmiError(rc, L.dmi_last_error(None).decode())
    return Views(out, views.K4, views.RT4, None), counts, float(ms.value)


def filter_depth_speckles(views: Views, *, min_pixels: int, abs_tolerance: float = 0.0, rel_tolerance: float = 0.0,
                          threshold: float | None = None, device: int = 0, out: np.ndarray | None = None):
    """Depth maps without their small segments (include/dmi.h: dmi_filter_depth_speckles): two 4-neighbours of a view are linked
    where their depths differ by at most abs_tolerance + rel_tolerance * the smaller one, and a depth is kept only where its
    connected segment has at least min_pixels pixels.  threshold applies views.best_cost first (best cost > threshold => -1).
    The cameras are not read.  Returns (Views with the filtered depths, the same cameras and best_cost None; sizes int32 [n, H, W];
    the kernels' hipEvent time in ms).  out: where the filtered depths go; it may be views.depth itself (f64, C-contiguous), which is
    then filtered in place."""
    L = load()
    d = np.ascontiguousarray(views.depth, dtype=np.float64)
    if d.ndim != 3:
        raise ValueError(f"views.depth must be [n, H, W], got {d.shape}")
    n, H, W = d.shape
    bc = None
    if threshold is not None and views.best_cost is not None:
        bc = np.ascontiguousarray(views.best_cost, dtype=np.float64)
        if bc.shape != d.shape:
            raise ValueError("views.best_cost must have the shape of views.depth")
    if out is None:
        out = np.empty_like(d)
    elif out.dtype != np.float64 or out.shape != d.shape or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous f64 array of the depths' shape")
    sizes = np.zeros(d.shape, dtype=np.int32)
    ms = ctypes.c_double(0.0)
    rc = L.dmi_filter_depth_speckles(_dp(d), None if bc is None else _dp(bc), 0.0 if threshold is None else float(threshold), n, W, H,
                                     float(abs_tolerance), float(rel_tolerance), int(min_pixels), int(device), _dp(out),
                                     sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(ms))
    if rc != DMI_OK:
        raise DmiError(rc, L.dmi_last_error(None).decode())
    return Views(out, views.K4, views.RT4, None), sizes, float(ms.value)


def fill_depth_holes(views: Views, *, max_pixels: int, abs_tolerance: float = 0.0, rel_tolerance: float = 0.0,
                     threshold: float | None = None, device: int = 0, out: np.ndarray | None = None):
    """Depth maps with their small holes filled (include/dmi.h: dmi_fill_depth_holes): a hole is a 4-connected component of the
    pixels without a depth; one of at most max_pixels pixels that does not touch the image's border and whose rim depths lo..hi
    satisfy hi - lo <= abs_tolerance + rel_tolerance * lo gets, at every pixel, a depth interpolated between the nearest valid
    pixels of its row and of its column.  threshold applies views.best_cost first (best cost > threshold => -1).  The cameras are
    not read.  Returns (Views with the filled depths, the same cameras and best_cost None; sizes int32 [n, H, W]: every pixel's hole
    size, 0 at a valid pixel; the kernels' hipEvent time in ms).  out: where the filled depths go; it may be views.depth itself
    (f64, C-contiguous), which is then filled in place."""
    L = load()
    d = np.ascontiguousarray(views.depth, dtype=np.float64)
    if d.ndim != 3:
        raise ValueError(f"views.depth must be [n, H, W], got {d.shape}")
    n, H, W = d.shape
    bc = None
    if threshold is not None and views.best_cost is not None:
        bc = np.ascontiguousarray(views.best_cost, dtype=np.float64)
        if bc.shape != d.shape:
            raise ValueError("views.best_cost must have the shape of views.depth")
    if out is None:
        out = np.empty_like(d)
    elif out.dtype != np.float64 or out.shape != d.shape or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous f64 array of the depths' shape")
    sizes = np.zeros(d.shape, dtype=np.int32)
    ms = ctypes.c_double(0.0)
    rc = L.dmi_fill_depth_holes(_dp(d), None if bc is None else _dp(bc), 0.0 if threshold is None else float(threshold), n, W, H,
                                float(abs_tolerance), float(rel_tolerance), int(max_pixels), int(device), _dp(out),
                                sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(ms))
    if rc != DMI_OK:
        raise DmiError(rc, L.dmi_last_error(None).decode())
    return Views(out, views.K4, views.RT4, None), sizes, float(ms.value)


def depth_smoothing_weights(sigma: float, truncate: float = 2.0) -> np.ndarray:
    """s[0..r], the spatial weights of one axis of the depth smoothing with r = ceil(truncate * sigma): s[0] = 1, not normalised, as
    the library computes them (dmi_depth_smoothing_weights; no GPU needed).  DmiError with code 1 for parameters outside the
    definition."""
    L = load()
    r, s = ctypes.c_int32(0), np.zeros(9, dtype=np.float64)
    code = L.dmi_depth_smoothing_weights(float(sigma), float(truncate), ctypes.byref(r), _dp(s))
    if code != 0:
        raise DmiError(code, (L.dmi_last_error(None) or b"").decode())
    return s[:int(r.value) + 1].copy()


def smooth_depths(views: Views, *, sigma: float, truncate: float = 2.0, abs_tolerance: float = 0.0, rel_tolerance: float = 0.0,
                  iterations: int = 1, threshold: float | None = None, device: int = 0, out: np.ndarray | None = None):
    """Depth maps smoothed with their edges preserved (include/dmi.h: dmi_smooth_depths): every valid depth c moves to the weighted
    mean of the valid depths q within r = ceil(truncate * sigma) pixels with (q - c)^2 < tau^2, tau = abs_tolerance +
    rel_tolerance * c, the weight a spatial Gaussian times Tukey's biweight of q - c; `iterations` passes, each on the output of
    the one before.  threshold applies views.best_cost first (best cost > threshold => -1).  The cameras are not read.  Returns
    (Views with the smoothed depths, the same cameras and best_cost None; counts int32 [n, H, W]: the taps taken at every pixel in
    the last pass, 0 at a pixel without a depth; the kernels' hipEvent time in ms).  out: where the smoothed depths go; it may be
    views.depth itself (f64, C-contiguous), which is then smoothed in place."""
    L = load()
    d = np.ascontiguousarray(views.depth, dtype=np.float64)
    if d.ndim != 3:
        raise ValueError(f"views.depth must be [n, H, W], got {d.shape}")
    n, H, W = d.shape
    bc = None
    if threshold is not None and views.best_cost is not None:
        bc = np.ascontiguousarray(views.best_cost, dtype=np.float64)
        if bc.shape != d.shape:
            raise ValueError("views.best_cost must have the shape of views.depth")
    if out is None:
        out = np.empty_like(d)
    elif out.dtype != np.float64 or out.shape != d.shape or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous f64 array of the depths' shape")
    counts = np.zeros(d.shape, dtype=np.int32)
    ms = ctypes.c_double(0.0)
    rc = L.dmi_smooth_depths(_dp(d), None if bc is None else _dp(bc), 0.0 if threshold is None else float(threshold), n, W, H,
                             float(sigma), float(truncate), float(abs_tolerance), float(rel_tolerance), int(iterations), int(device),
                             _dp(out), counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(ms))
    if rc != DMI_OK:
        raise DmiError(rc, L.dmi_last_error(None).decode())
    return Views(out, views.K4, views.RT4, None), counts, float(ms.value)


def estimate_scene_bounds(views: Views, *, trim_fraction: float = 0.0, pixel_step: int = 1, axes=None, threshold: float | None = None,
                          device: int = 0):
    """The bounds of the scene the depth maps see (include/dmi.h: dmi_estimate_scene_bounds): per axis the element of rank k and
    of rank N-1-k of the back-projected valid pixels' coordinates, k = min(int(trim_fraction * N), (N - 1) // 2), over every
    pixel_step-th pixel of every pixel_step-th row.  axes: 3 x 3, the rows the coordinates are measured along (None: the world's).
    threshold applies views.best_cost first (best cost > threshold => not valid).  Returns (lo [3] f64, hi [3] f64, the number of
    points N, the kernels' hipEvent time in ms); N == 0 gives NaN bounds."""
    L = load()
    d = np.ascontiguousarray(views.depth, dtype=np.float64)
    if d.ndim != 3:
        raise ValueError(f"views.depth must be [n, H, W], got {d.shape}")
    n, H, W = d.shape
    k = np.ascontiguousarray(views.K4, dtype=np.float64).reshape(-1)
    rt = np.ascontiguousarray(views.RT4, dtype=np.float64).reshape(-1)
    if k.size != 16 * n or rt.size != 16 * n:
        raise ValueError("views.K4 and views.RT4 must be [n, 4, 4]")
    bc = None
    if threshold is not None and views.best_cost is not None:
        bc = np.ascontiguousarray(views.best_cost, dtype=np.float64)
        if bc.shape != d.shape:
            raise ValueError("views.best_cost must have the shape of views.depth")
    a = None
    if axes is not None:
        a = np.ascontiguousarray(axes, dtype=np.float64).reshape(-1)
        if a.size != 9:
            raise ValueError("axes must be 3 x 3")
    lo, hi = np.zeros(3, dtype=np.float64), np.zeros(3, dtype=np.float64)
    count, ms = ctypes.c_uint64(0), ctypes.c_double(0.0)
    rc = L.dmi_estimate_scene_bounds(_dp(d), None if bc is None else _dp(bc), 0.0 if threshold is None else float(threshold), _dp(k),
                                     _dp(rt), n, W, H, None if a is None else _dp(a), float(trim_fraction), int(pixel_step),
                                     int(device), _dp(lo), _dp(hi), ctypes.byref(count), ctypes.byref(ms))
    if rc != DMI_OK:
        raise DmiError(rc, L.dmi_last_error(None).decode())
    return lo, hi, int(count.value), float(ms.value)


def thin_point_cloud(xyz, normal=None, view=None, pixel=None, count=None, *, cell_size: float, min_points: int = 1, device: int = 0,
                     in_place: bool = False, return_members: bool = True):
    """A point cloud thinned and merged on a voxel grid (include/dmi.h: dmi_thin_point_cloud): one point per occupied cell of
    size cell_size that has at least min_points members, at their mean, with a merged normal, the first member's view and pixel
    and the largest count.  xyz [P, 3] f64; normal [P, 3] f32, view, pixel, count [P] int32, each optional (absent: zeros).
    Returns (arrays, report): arrays has xyz, normal, view, pixel, count and -- with return_members -- members (uint32), in cell
    order; report has points_in, cells, cells_kept, multi_view_cells, largest_cell, with_normal, kernel_ms.  in_place: the
    arrays given (C-contiguous, of the dtypes above) receive the result themselves and the returned arrays are views of them."""
    L = load()
    kinds = dict(xyz=(np.float64, 3), normal=(np.float32, 3), view=(np.int32, 1), pixel=(np.int32, 1), count=(np.int32, 1))
    given = dict(xyz=xyz, normal=normal, view=view, pixel=pixel, count=count)
    if xyz is None:
        raise ValueError("xyz is required")
    inputs = {}
    for name, a in given.items():
        dtype, width = kinds[name]
        if a is None:
            inputs[name] = None
            continue
        b = np.ascontiguousarray(a, dtype=dtype)
        if in_place and b is not a:
            raise ValueError(f"in_place needs a C-contiguous {np.dtype(dtype).name} array for {name}")
        inputs[name] = b
    p = inputs["xyz"].size // 3
    for name, b in inputs.items():
        if b is not None and b.size != p * kinds[name][1]:
            raise ValueError(f"{name} must hold {kinds[name][1]} values per point")
    out = {name: (inputs[name].reshape(-1) if in_place and inputs[name] is not None else np.empty(p * width, dtype=dtype))
           for name, (dtype, width) in kinds.items()}
    members = np.empty(p, dtype=np.uint32) if return_members else None
    i32p, fp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)

    def ptr(a, kind):
        return None if a is None else a.ctypes.data_as(kind)

    n_out, r = ctypes.c_uint64(0), PointsThinReportC()
    rc = L.dmi_thin_point_cloud(ptr(inputs["xyz"], ctypes.POINTER(ctypes.c_double)), ptr(inputs["normal"], fp), ptr(inputs["view"], i32p),
                                ptr(inputs["pixel"], i32p), ptr(inputs["count"], i32p), p, float(cell_size), int(min_points), int(device),
                                ptr(out["xyz"], ctypes.POINTER(ctypes.c_double)), ptr(out["normal"], fp), ptr(out["view"], i32p),
                                ptr(out["pixel"], i32p), ptr(out["count"], i32p), ptr(members, ctypes.POINTER(ctypes.c_uint32)),
                                ctypes.byref(n_out), ctypes.byref(r))
    if rc != DMI_OK:
        raise DmiError(rc, L.dmi_last_error(None).decode())
    q = int(n_out.value)
    arrays = {name: (out[name][:q * width].reshape(q, 3) if width == 3 else out[name][:q]) for name, (_, width) in kinds.items()}
    if return_members:
        arrays["members"] = members[:q]
    return arrays, {name: getattr(r, name) for name, _ in PointsThinReportC._fields_}


def count_point_neighbors(xyz, *, radius: float, min_neighbors: int = 1, device: int = 0):
    """Every point's number of other points within `radius`, and which points have at least min_neighbors of them (include/dmi.h:
    dmi_count_point_neighbors).  xyz [P, 3] f64.  Returns (neighbors uint32 [P], keep bool [P], report): report has points_in,
    points_kept, isolated, max_neighbors, neighbor_sum, distance_tests, kernel_ms.  xyz[keep] is the filtered cloud."""
    L = load()
    a = np.ascontiguousarray(xyz, dtype=np.float64)
    if a.size % 3:
        raise ValueError("xyz must hold 3 values per point")
    p = a.size // 3
    neighbors, keep = np.empty(p, dtype=np.uint32), np.empty(p, dtype=np.uint8)
    n_kept, r = ctypes.c_uint64(0), PointsRadiusReportC()
    rc = L.dmi_count_point_neighbors(_dp(a), p, float(radius), int(min_neighbors), int(device),
                                     neighbors.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                     keep.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(n_kept), ctypes.byref(r))
    if rc != DMI_OK:
        raise DmiError(rc, L.dmi_last_error(None).decode())
    return neighbors, keep.astype(bool), {name: getattr(r, name) for name, _ in PointsRadiusReportC._fields_}


def fit_point_planes(xyz, normal=None, *, radius: float, min_neighbors: int = 5, move: bool = True, normals: bool = True,
                     device: int = 0):
    """A plane fitted to the points within `radius` of every point that has at least min_neighbors of them; the point moved onto it
    (move) and its normal replaced by the plane's, on the side of the old one (normals) (include/dmi.h: dmi_fit_point_planes).
    xyz [P, 3] f64, normal [P, 3] f32 or None.  Returns (arrays, report): arrays has xyz, normal, plane_rms f32 [P] (-1: no fit) and
    neighbors uint32 [P]; an array whose flag is not set is the input's (zeros for absent normals).  report has points_in, fitted,
    unsupported, crowded, max_neighbors, neighbor_sum, distance_tests, max_shift, kernel_ms."""
    L = load()
    a = np.ascontiguousarray(xyz, dtype=np.float64)
    if a.size % 3:
        raise ValueError("xyz must hold 3 values per point")
    p = a.size // 3
    old = None if normal is None else np.ascontiguousarray(normal, dtype=np.float32)
    if old is not None and old.size != 3 * p:
        raise ValueError("normal must hold 3 values per point")
    flags = (PLANE_FIT_MOVE if move else 0) | (PLANE_FIT_NORMALS if normals else 0)
    fp = ctypes.POINTER(ctypes.c_float)
    out_xyz = a.reshape(p, 3).copy()
    out_normal = np.zeros((p, 3), dtype=np.float32) if old is None else old.reshape(p, 3).copy()
    rms, neighbors = np.empty(p, dtype=np.float32), np.empty(p, dtype=np.uint32)
    r = PointsPlanesReportC()
    rc = L.dmi_fit_point_planes(_dp(a), None if old is None else old.ctypes.data_as(fp), p, float(radius), int(min_neighbors), flags,
                                int(device), _dp(out_xyz) if move else None, out_normal.ctypes.data_as(fp) if normals else None,
                                rms.ctypes.data_as(fp), neighbors.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(r))
    if rc != DMI_OK:
        raise DmiError(rc, L.dmi_last_error(None).decode())
    return (dict(xyz=out_xyz, normal=out_normal, plane_rms=rms, neighbors=neighbors),
            {name: getattr(r, name) for name, _ in PointsPlanesReportC._fields_})


class ViewSet:
    """Depth maps resident on the device from the first filter to the fusion (dmi_views_create ... dmi_views_destroy;
    include/dmi.h states the definition).  add() uploads once; every step replaces the set's depths by exactly what the
    context-free function of the same name returns for them, and returns its report -- computed on the device -- as a dict;
    FusionContext.add_views_from_set hands the depths over without a host copy."""

    def __init__(self, W: int, H: int, device: int = 0):
        self._lib = load()
        self._h = ctypes.c_void_p()
        self.W, self.H = int(W), int(H)
        rc = self._lib.dmi_views_create(int(device), self.W, self.H, ctypes.byref(self._h))
        if rc != DMI_OK:
            self._h = ctypes.c_void_p()
            raise DmiError(rc, self._lib.dmi_views_last_error(None).decode())

    def _check(self, rc):
        if rc != DMI_OK:
            raise DmiError(rc, self._lib.dmi_views_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.dmi_views_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, views: Views, threshold: float | None = None):
        """Append views (depth [n, H, W] f64 in vtk row order, K4 / RT4 [n, 4, 4]).  threshold applies views.best_cost (best cost >
        threshold => -1), here and once: the costs are not kept."""
        d = np.ascontiguousarray(views.depth, dtype=np.float64)
        if d.ndim != 3 or d.shape[1:] != (self.H, self.W):
            raise ValueError(f"views.depth must be [n, {self.H}, {self.W}], got {d.shape}")
        n = d.shape[0]
        k = np.ascontiguousarray(views.K4, dtype=np.float64).reshape(-1)
        rt = np.ascontiguousarray(views.RT4, dtype=np.float64).reshape(-1)
        if k.size != 16 * n or rt.size != 16 * n:
            raise ValueError("views.K4 and views.RT4 must be [n, 4, 4]")
        bc = None
        if threshold is not None and views.best_cost is not None:
            bc = np.ascontiguousarray(views.best_cost, dtype=np.float64)
            if bc.shape != d.shape:
                raise ValueError("views.best_cost must have the shape of views.depth")
        self._check(self._lib.dmi_views_add(self._h, _dp(d), None if bc is None else _dp(bc), 0.0 if threshold is None else float(threshold),
                                            _dp(k), _dp(rt), n))

    def clear(self):
        self._check(self._lib.dmi_views_clear(self._h))

    def set_piece_bytes(self, n_bytes: int):
        """Bound the f64 planes of the views a pass works on at a time (whole views, at least one).  No result depends on it."""
        self._check(self._lib.dmi_views_set_piece_bytes(self._h, int(n_bytes)))

    def info(self) -> ViewsInfoC:
        out = ViewsInfoC()
        self._check(self._lib.dmi_views_get_info(self._h, ctypes.byref(out)))
        return out

    def _step(self, call, args, return_aux):
        aux = np.zeros((self.info().n, self.H, self.W), dtype=np.int32) if return_aux else None
        r = ViewsStepReportC()
        self._check(call(self._h, *args, None if aux is None else aux.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(r)))
        report = {name: getattr(r, name) for name, _ in ViewsStepReportC._fields_}
        return (report, aux) if return_aux else report

    def filter_speckles(self, *, min_pixels: int, abs_tolerance: float = 0.0, rel_tolerance: float = 0.0, return_aux: bool = False):
        """filter_depth_speckles on the set's depths.  Returns the report, and the sizes int32 [n, H, W] with return_aux."""
        return self._step(self._lib.dmi_views_filter_speckles, (float(abs_tolerance), float(rel_tolerance), int(min_pixels)), return_aux)

    def fill_holes(self, *, max_pixels: int, abs_tolerance: float = 0.0, rel_tolerance: float = 0.0, return_aux: bool = False):
        """fill_depth_holes on the set's depths.  Returns the report, and the hole sizes int32 [n, H, W] with return_aux."""
        return self._step(self._lib.dmi_views_fill_holes, (float(abs_tolerance), float(rel_tolerance), int(max_pixels)), return_aux)

    def smooth(self, *, sigma: float, truncate: float = 2.0, abs_tolerance: float = 0.0, rel_tolerance: float = 0.0, iterations: int = 1,
               return_aux: bool = False):
        """smooth_depths on the set's depths.  Returns the report, and the last pass's tap counts int32 [n, H, W] with return_aux."""
        return self._step(self._lib.dmi_views_smooth, (float(sigma), float(truncate), float(abs_tolerance), float(rel_tolerance),
                                                       int(iterations)), return_aux)

    def filter_consistency(self, *, min_views: int, abs_tolerance: float = 0.0, rel_tolerance: float = 0.0, return_aux: bool = False):
        """filter_depth_consistency on the set's depths.  Returns the report, and the counts int32 [n, H, W] with return_aux."""
        return self._step(self._lib.dmi_views_filter_consistency, (float(abs_tolerance), float(rel_tolerance), int(min_views)), return_aux)

    def estimate_bounds(self, *, trim_fraction: float = 0.0, pixel_step: int = 1, axes=None):
        """estimate_scene_bounds on the set's depths: (lo [3] f64, hi [3] f64, the number of points, the kernels' time in ms)."""
        a = None
        if axes is not None:
            a = np.ascontiguousarray(axes, dtype=np.float64).reshape(-1)
            if a.size != 9:
                raise ValueError("axes must be 3 x 3")
        lo, hi = np.zeros(3, dtype=np.float64), np.zeros(3, dtype=np.float64)
        count, ms = ctypes.c_uint64(0), ctypes.c_double(0.0)
        self._check(self._lib.dmi_views_estimate_bounds(self._h, None if a is None else _dp(a), float(trim_fraction), int(pixel_step),
                                                        _dp(lo), _dp(hi), ctypes.byref(count), ctypes.byref(ms)))
        return lo, hi, int(count.value), float(ms.value)

    def download(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """The set's depths of views [first, first + count) (all from `first` on by default), [count, H, W] f64 in vtk row order."""
        count = self.info().n - int(first) if count is None else int(count)
        out = np.empty((max(count, 0), self.H, self.W), dtype=np.float64)
        self._check(self._lib.dmi_views_download(self._h, int(first), count, _dp(out)))
        return out

    def build_points(self, *, abs_tolerance: float, rel_tolerance: float, normal_abs_tolerance: float | None = None,
                     normal_rel_tolerance: float | None = None, min_views: int = 1, pixel_step: int = 1, dedupe: bool = True) -> dict:
        """The fused point cloud of the set's depths (include/dmi.h: dmi_views_build_points): the valid pixels, every pixel_step-th
        of every pixel_step-th row, that at least min_views other views agree with, and -- with dedupe -- that no lower view holds
        already, each with a normal from its own depth map.  The normal tolerances default to the agreement pair (None).  The points
        stay on the device (download_points) until the depths change.  Returns the report: valid, candidates, owned, points,
        with_normal, kernel_ms."""
        n_abs = abs_tolerance if normal_abs_tolerance is None else normal_abs_tolerance
        n_rel = rel_tolerance if normal_rel_tolerance is None else normal_rel_tolerance
        count, r = ctypes.c_uint64(0), ViewsPointsReportC()
        self._check(self._lib.dmi_views_build_points(self._h, float(abs_tolerance), float(rel_tolerance), float(n_abs), float(n_rel),
                                                     int(min_views), int(pixel_step), int(dedupe), ctypes.byref(count), ctypes.byref(r)))
        self._n_points = int(count.value)
        return {name: getattr(r, name) for name, _ in ViewsPointsReportC._fields_}

    def points_pass_ms(self) -> dict:
        """The last build_points' kernel time by pass (ms): flip, count, flags, scan (the block counts with it), scatter."""
        out = np.zeros(5, dtype=np.float64)
        self._check(self._lib.dmi_views_get_points_pass_ms(self._h, _dp(out)))
        return dict(zip(("flip", "count", "flags", "scan", "scatter"), out.tolist()))

    def download_points(self, first: int = 0, count: int | None = None) -> dict:
        """The points [first, first + count) of the last build_points (all from `first` on by default): xyz f64 [count, 3], normal
        f32 [count, 3] (zero where a point has none), view, pixel (py * W + px in image coordinates) and count (the views that
        agree) int32 [count], in ascending (view, py, px)."""
        first = int(first)
        if count is None:  # (what the last build reported; whether those points still stand is the library's to say)
            count = max(getattr(self, "_n_points", 0) - first, 0)
        count = int(count)
        if first < 0 or count < 0:
            raise ValueError("first and count must not be negative")
        arrays = dict(xyz=np.empty((count, 3), dtype=np.float64), normal=np.empty((count, 3), dtype=np.float32),
                      view=np.empty(count, dtype=np.int32), pixel=np.empty(count, dtype=np.int32), count=np.empty(count, dtype=np.int32))
        i32p = ctypes.POINTER(ctypes.c_int32)
        self._check(self._lib.dmi_views_download_points(
            self._h, first, count, _dp(arrays["xyz"]), arrays["normal"].ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
            arrays["view"].ctypes.data_as(i32p), arrays["pixel"].ctypes.data_as(i32p), arrays["count"].ctypes.data_as(i32p)))
        return arrays

    def thin_points(self, cell_size: float, min_points: int = 1) -> dict:
        """The set's cloud replaced by its thinned one (include/dmi.h: dmi_views_thin_points): one point per occupied cell of size
        cell_size with at least min_points members, at their mean.  On a cloud built with dedupe=False the mean averages what the
        views saw of one surface element.  Once per build.  Returns the report: points_in, cells, cells_kept, multi_view_cells,
        largest_cell, with_normal, kernel_ms; download_points serves the thinned cloud, download_point_members its cell sizes."""
        count, r = ctypes.c_uint64(0), PointsThinReportC()
        self._check(self._lib.dmi_views_thin_points(self._h, float(cell_size), int(min_points), ctypes.byref(count), ctypes.byref(r)))
        self._n_points = int(count.value)
        return {name: getattr(r, name) for name, _ in PointsThinReportC._fields_}

    def download_point_members(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """How many input points each of the points [first, first + count) was merged from, uint32 (1 on a cloud not thinned)."""
        first = int(first)
        if count is None:
            count = max(getattr(self, "_n_points", 0) - first, 0)
        count = int(count)
        if first < 0 or count < 0:
            raise ValueError("first and count must not be negative")
        out = np.empty(count, dtype=np.uint32)
        self._check(self._lib.dmi_views_download_point_members(self._h, first, count, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
        return out

    def thin_pass_ms(self) -> dict:
        """The last thin_points' kernel time by pass (ms): bounds, keys, sort, ranks (with their scans), representatives."""
        out = np.zeros(5, dtype=np.float64)
        self._check(self._lib.dmi_views_get_thin_pass_ms(self._h, _dp(out)))
        return dict(zip(("bounds", "keys", "sort", "ranks", "representatives"), out.tolist()))

    def set_thin_wave_cell_points(self, k: int):
        """Cells of more than k members are summed by a wave of their own.  No result depends on it."""
        self._check(self._lib.dmi_views_set_thin_wave_cell_points(self._h, int(k)))

    def filter_points_radius(self, radius: float, min_neighbors: int = 1) -> dict:
        """The set's cloud, built or thinned, replaced by its points that have at least min_neighbors other points within `radius`
        (include/dmi.h: dmi_views_filter_points_radius), in their order, every array carried as it is.  min_neighbors=0 drops
        nothing and only counts.  Returns the report: points_in, points_kept, isolated, max_neighbors, neighbor_sum,
        distance_tests, kernel_ms; download_point_neighbors serves the counts of the kept points."""
        count, r = ctypes.c_uint64(0), PointsRadiusReportC()
        self._check(self._lib.dmi_views_filter_points_radius(self._h, float(radius), int(min_neighbors), ctypes.byref(count),
                                                             ctypes.byref(r)))
        self._n_points = int(count.value)
        return {name: getattr(r, name) for name, _ in PointsRadiusReportC._fields_}

    def download_point_neighbors(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """How many neighbours each of the points [first, first + count) had in the cloud the last filter_points_radius found, uint32."""
        first = int(first)
        if count is None:
            count = max(getattr(self, "_n_points", 0) - first, 0)
        count = int(count)
        if first < 0 or count < 0:
            raise ValueError("first and count must not be negative")
        out = np.empty(count, dtype=np.uint32)
        self._check(self._lib.dmi_views_download_point_neighbors(self._h, first, count, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
        return out

    def radius_pass_ms(self) -> dict:
        """The last filter_points_radius' kernel time by pass (ms): bounds, keys, sort, ranks, permute, count, compaction."""
        out = np.zeros(7, dtype=np.float64)
        self._check(self._lib.dmi_views_get_radius_pass_ms(self._h, _dp(out)))
        return dict(zip(("bounds", "keys", "sort", "ranks", "permute", "count", "compaction"), out.tolist()))

    def set_radius_group_points(self, k: int):
        """A wave of the neighbour count takes at most k points of one grid row as its queries (1..64).  No result depends on it."""
        self._check(self._lib.dmi_views_set_radius_group_points(self._h, int(k)))

    def fit_point_planes(self, radius: float, min_neighbors: int = 5, *, move: bool = True, normals: bool = True) -> dict:
        """The set's cloud -- built, thinned or filtered -- with every point that has at least min_neighbors others within `radius`
        moved onto the plane fitted to them (move) and carrying that plane's normal (normals) (include/dmi.h:
        dmi_views_fit_point_planes).  Order, layout and every other array stay.  Returns the report: points_in, fitted, unsupported,
        crowded, max_neighbors, neighbor_sum, distance_tests, max_shift, kernel_ms; download_point_plane_rms serves the residuals."""
        r = PointsPlanesReportC()
        flags = (PLANE_FIT_MOVE if move else 0) | (PLANE_FIT_NORMALS if normals else 0)
        self._check(self._lib.dmi_views_fit_point_planes(self._h, float(radius), int(min_neighbors), flags, ctypes.byref(r)))
        return {name: getattr(r, name) for name, _ in PointsPlanesReportC._fields_}

    def download_point_plane_rms(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """The RMS distance of each of the points' [first, first + count) balls from their planes, f32; -1 where none was fitted."""
        first = int(first)
        if count is None:
            count = max(getattr(self, "_n_points", 0) - first, 0)
        count = int(count)
        if first < 0 or count < 0:
            raise ValueError("first and count must not be negative")
        out = np.empty(count, dtype=np.float32)
        self._check(self._lib.dmi_views_download_point_plane_rms(self._h, first, count, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
        return out

    def plane_fit_pass_ms(self) -> dict:
        """The last fit_point_planes' kernel time by pass (ms): bounds, keys, sort, ranks, permute, fit."""
        out = np.zeros(6, dtype=np.float64)
        self._check(self._lib.dmi_views_get_plane_fit_pass_ms(self._h, _dp(out)))
        return dict(zip(("bounds", "keys", "sort", "ranks", "permute", "fit"), out.tolist()))


class ColorContext:
    """MeshColoration with resident views (dmi_color_create ... dmi_color_destroy)."""

    def __init__(self, device: int = 0):
        self._lib = load()
        self._h = ctypes.c_void_p()
        self._n_views, self._W, self._H = 0, 0, 0
        rc = self._lib.dmi_color_create(device, ctypes.byref(self._h))
        if rc != DMI_OK:
            self._h = ctypes.c_void_p()
            raise DmiError(rc, self._lib.dmi_color_last_error().decode())

    def _check(self, rc):
        if rc != DMI_OK:
            raise DmiError(rc, self._lib.dmi_color_last_error().decode())

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.dmi_color_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_views(self, colors, K4, RT4, depths=None):
        """Append views: colors [n, H, W, 3] u8 in vtk row order, K4 / RT4 [n, 4, 4].  depths [n, H, W] f64 (the "Depths"
        arrays, vtk row order): kept resident for the depth test (set_depth_test); views added without them cannot take it."""
        col = np.ascontiguousarray(colors, dtype=np.uint8)
        n, H, W, _ = col.shape
        k = np.ascontiguousarray(K4, dtype=np.float64).reshape(n, 16)
        rt = np.ascontiguousarray(RT4, dtype=np.float64).reshape(n, 16)
        u8 = ctypes.POINTER(ctypes.c_uint8)
        if depths is None:
            self._check(self._lib.dmi_color_add_views(self._h, col.ctypes.data_as(u8), _dp(k), _dp(rt), n, W, H))
            self._n_views, self._W, self._H = self._n_views + n, W, H
            return
        d = np.ascontiguousarray(depths, dtype=np.float64)
        if d.shape != (n, H, W):
            raise ValueError(f"depths {d.shape} do not match the colour planes ({n}, {H}, {W})")
        self._check(self._lib.dmi_color_add_views_with_depth(self._h, col.ctypes.data_as(u8), _dp(d), _dp(k), _dp(rt), n, W, H))
        self._n_views, self._W, self._H = self._n_views + n, W, H

    def set_depth_test(self, enable: bool, tolerance: float = 0.0):
        """The visibility test (include/dmi.h, dmi_color_set_depth_test): a pair counts only if the vertex is in front of the
        camera and its camera z is within `tolerance` of the view's depth at the pixel (> 0).  Off: the reference's colouring."""
        self._check(self._lib.dmi_color_set_depth_test(self._h, 1 if enable else 0, float(tolerance)))

    def clear_views(self):
        self._check(self._lib.dmi_color_clear_views(self._h))
        self._n_views, self._W, self._H = 0, 0, 0

    def process(self, points, out=None):
        """(mean [n, 3] u8, median [n, 3] u8, count [n] i32) of the vertices `points` [n, 3] f64.  out: the three arrays to fill
        (e.g. over pinned memory, pinned_empty -- with `points` pinned too the copies are DMA transfers that overlap the kernels of
        the neighbouring chunks); else fresh ones."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        nv = pts.shape[0]
        if out is None:
            mean = np.zeros((nv, 3), dtype=np.uint8)
            median = np.zeros((nv, 3), dtype=np.uint8)
            count = np.zeros(nv, dtype=np.int32)
        else:
            mean, median, count = out
            if (mean.shape, median.shape, count.shape) != ((nv, 3), (nv, 3), (nv,)) or mean.dtype != np.uint8 or median.dtype != np.uint8 \
                    or count.dtype != np.int32 or not (mean.flags.c_contiguous and median.flags.c_contiguous and count.flags.c_contiguous):
                raise ValueError("out = (mean [n, 3] u8, median [n, 3] u8, count [n] i32), contiguous")
        u8 = ctypes.POINTER(ctypes.c_uint8)
        self._check(self._lib.dmi_color_process(self._h, _dp(pts), nv, mean.ctypes.data_as(u8), median.ctypes.data_as(u8),
                                                count.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return mean, median, count

    def render_depths(self, points, triangles):
        """Render the triangle mesh (points [n, 3] f64, triangles [t, 3] ids) into the depth plane of every resident view: the
        z-buffer the visibility test then compares against (dmi_color_render_depths; DESIGN.md 8b'').  Views added without
        depths get a plane, uploaded planes are replaced."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        tri = np.ascontiguousarray(triangles, dtype=np.int64).reshape(-1, 3)
        self._check(self._lib.dmi_color_render_depths(self._h, _dp(pts), pts.shape[0], tri.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                      tri.shape[0]))

    def download_depths(self, first: int = 0, count: int | None = None):
        """The depth planes of views [first, first + count) as [count, H, W] f64 in vtk row order -- what add_views(depths=...)
        takes --, -1 where nothing was rendered (dmi_color_download_depths).  count None: all views from `first` on."""
        n, W, H = self._n_views, self._W, self._H  # (kept by add_views / clear_views: the C ABI has no query for them)
        if count is None:
            count = max(n - int(first), 0)
        out = np.zeros((max(int(count), 1), H, W), dtype=np.float64)
        self._check(self._lib.dmi_color_download_depths(self._h, int(first), int(count), _dp(out)))
        return out[:int(count)]

    def render_kernel_ms(self) -> float:
        """hipEvent milliseconds of the kernels of the last render_depths / render_isosurface_depths."""
        v = ctypes.c_double(0)
        self._check(self._lib.dmi_color_get_render_kernel_ms(self._h, ctypes.byref(v)))
        return float(v.value)

    def render_pass_ms(self) -> dict:
        """The same pass by pass: the fill, the small passes, the large passes (dmi_color_get_render_pass_ms)."""
        a = (ctypes.c_double * 3)()
        self._check(self._lib.dmi_color_get_render_pass_ms(self._h, a))
        return dict(zip(("init", "small", "large"), (float(x) for x in a)))

    def render_queued_pairs(self) -> int:
        """(triangle, view) pairs the last rendering's large passes took (dmi_color_get_render_queued_pairs)."""
        v = ctypes.c_uint64(0)
        self._check(self._lib.dmi_color_get_render_queued_pairs(self._h, ctypes.byref(v)))
        return int(v.value)

    def set_render_queue_capacity(self, n: int):
        """Entries the rasteriser's queue of large (triangle, view) pairs starts with (it grows on demand; same result)."""
        self._check(self._lib.dmi_color_set_render_queue_capacity(self._h, int(n)))

    def set_scratch_budget(self, n_bytes: int):
        """Bound the device scratch of one vertex chunk (more, smaller chunks; same result)."""
        self._check(self._lib.dmi_color_set_scratch_budget(self._h, int(n_bytes)))

    def set_vertex_reorder(self, enable: bool):
        """Work through each chunk's vertices along a Z-order curve (same results, better gathers for unordered vertices)."""
        self._check(self._lib.dmi_color_set_vertex_reorder(self._h, 1 if enable else 0))

    def kernel_ms(self) -> float:
        v = ctypes.c_double(0)
        self._check(self._lib.dmi_color_get_kernel_ms(self._h, ctypes.byref(v)))
        return float(v.value)


def fuse_once(grid: GridDesc, ray: RayPotential, views: Views, *, threshold: float | None = None,
              init_grid: np.ndarray | None = None, count_hits: bool = True, **ctx_kwargs):
    """create -> (upload grid) -> add views -> fuse -> download.  Returns (grid, voxel_hits, map_hits)."""
    with FusionContext(grid, ray, count_hits=count_hits, **ctx_kwargs) as ctx:
        if init_grid is not None:
            ctx.upload_grid(init_grid)
        ctx.add_views(views, threshold)
        ctx.fuse()
        out = ctx.download_grid(np.float64)
        vh, mh = ctx.download_hits() if count_hits else (None, None)
    return out, vh, mh


# ---- host-side mirror of the reference's operator interface (include/dmi_host.h) -----------------------
HOST_ABI_SYMBOLS = [
    "dmi_filter_new", "dmi_filter_delete", "dmi_filter_set_ray_potential_thickness", "dmi_filter_set_ray_potential_rho",
    "dmi_filter_set_ray_potential_eta", "dmi_filter_set_ray_potential_delta", "dmi_filter_set_threshold_best_cost",
    "dmi_filter_set_file_path_krtd", "dmi_filter_set_file_path_vti", "dmi_filter_set_grid_matrix",
    "dmi_filter_set_input_data", "dmi_filter_add_view", "dmi_filter_clear_views", "dmi_filter_set_device",
    "dmi_filter_set_kernel_variant", "dmi_filter_set_devices", "dmi_filter_set_partition", "dmi_filter_set_host_chunk_bytes", "dmi_filter_set_fill_on_calling_thread", "dmi_filter_update", "dmi_filter_get_execution_time",
    "dmi_filter_get_fuse_kernel_ms", "dmi_filter_get_number_of_cells", "dmi_filter_get_output",
    "dmi_filter_last_error", "dmi_read_krtd_file", "dmi_extract_all_file_path", "dmi_k3_to_k4",
    "dmi_apply_depth_threshold", "dmi_read_depth_map", "dmi_read_depth_map_color", "dmi_mesh_coloration_from_lists",
    "dmi_cli_read_arguments", "dmi_cli_main", "dmi_write_polydata", "dmi_write_polydata_with_normals",
    "dmi_write_polydata_with_arrays", "dmi_write_polydata_with_colors",
    "dmi_mesh_coloration_from_lists_with_depth", "dmi_mesh_coloration_from_lists_with_mesh_depth", "dmi_read_polydata", "dmi_polydata_free", "dmi_polydata_counts",
    "dmi_polydata_array", "dmi_polydata_designations", "dmi_color_cli_read_arguments", "dmi_color_cli_main",
]

_host_bound = False


def load_host() -> ctypes.CDLL:
    """Bind the dmi_host.h entry points of the same shared library."""
    global _host_bound
    L = load()
    if _host_bound:
        return L
    vp, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    dp = ctypes.POINTER(ctypes.c_double)
    ip = ctypes.POINTER(ctypes.c_int32)
    L.dmi_filter_new.restype = vp
    L.dmi_filter_new.argtypes = []
    L.dmi_filter_delete.restype = None
    L.dmi_filter_delete.argtypes = [vp]
    for name in ("thickness", "rho", "eta", "delta"):
        fn = getattr(L, f"dmi_filter_set_ray_potential_{name}")
        fn.restype, fn.argtypes = None, [vp, dbl]
    L.dmi_filter_set_threshold_best_cost.restype, L.dmi_filter_set_threshold_best_cost.argtypes = None, [vp, dbl]
    L.dmi_filter_set_file_path_krtd.restype, L.dmi_filter_set_file_path_krtd.argtypes = None, [vp, ctypes.c_char_p]
    L.dmi_filter_set_file_path_vti.restype, L.dmi_filter_set_file_path_vti.argtypes = None, [vp, ctypes.c_char_p]
    L.dmi_filter_set_grid_matrix.restype, L.dmi_filter_set_grid_matrix.argtypes = None, [vp, dp]
    L.dmi_filter_set_input_data.restype, L.dmi_filter_set_input_data.argtypes = None, [vp, ip, dp, dp]
    L.dmi_filter_add_view.restype, L.dmi_filter_add_view.argtypes = ctypes.c_int, [vp, dp, dp, i32, i32, dp, dp]
    L.dmi_filter_clear_views.restype, L.dmi_filter_clear_views.argtypes = None, [vp]
    L.dmi_filter_set_device.restype, L.dmi_filter_set_device.argtypes = None, [vp, i32]
    L.dmi_filter_set_kernel_variant.restype, L.dmi_filter_set_kernel_variant.argtypes = None, [vp, i32]
    L.dmi_filter_set_devices.restype, L.dmi_filter_set_devices.argtypes = None, [vp, ip, i32]
    L.dmi_filter_set_partition.restype, L.dmi_filter_set_partition.argtypes = None, [vp, i32]
    L.dmi_filter_set_host_chunk_bytes.restype, L.dmi_filter_set_host_chunk_bytes.argtypes = None, [vp, ctypes.c_uint64]
    L.dmi_filter_set_fill_on_calling_thread.restype, L.dmi_filter_set_fill_on_calling_thread.argtypes = None, [vp, i32]
    L.dmi_filter_update.restype, L.dmi_filter_update.argtypes = ctypes.c_int, [vp]
    L.dmi_filter_get_execution_time.restype, L.dmi_filter_get_execution_time.argtypes = dbl, [vp]
    L.dmi_filter_get_fuse_kernel_ms.restype, L.dmi_filter_get_fuse_kernel_ms.argtypes = dbl, [vp]
    L.dmi_filter_get_number_of_cells.restype, L.dmi_filter_get_number_of_cells.argtypes = i64, [vp]
    L.dmi_filter_get_output.restype, L.dmi_filter_get_output.argtypes = i64, [vp, dp]
    L.dmi_filter_last_error.restype, L.dmi_filter_last_error.argtypes = ctypes.c_char_p, [vp]
    L.dmi_read_krtd_file.restype, L.dmi_read_krtd_file.argtypes = ctypes.c_int, [ctypes.c_char_p, dp, dp]
    L.dmi_extract_all_file_path.restype = ctypes.c_int
    L.dmi_extract_all_file_path.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
    L.dmi_k3_to_k4.restype, L.dmi_k3_to_k4.argtypes = None, [dp, dp]
    L.dmi_apply_depth_threshold.restype, L.dmi_apply_depth_threshold.argtypes = i64, [dp, dp, i64, dbl]
    L.dmi_read_depth_map.restype, L.dmi_read_depth_map.argtypes = ctypes.c_int, [ctypes.c_char_p, ip, dp, dp, ip]
    L.dmi_read_depth_map_color.restype = ctypes.c_int
    L.dmi_read_depth_map_color.argtypes = [ctypes.c_char_p, ip, ctypes.POINTER(ctypes.c_uint8), ip]
    L.dmi_mesh_coloration_from_lists.restype = ctypes.c_int
    L.dmi_mesh_coloration_from_lists.argtypes = [dp, i64, ctypes.c_char_p, ctypes.c_char_p, i32, ctypes.POINTER(ctypes.c_uint8),
                                                 ctypes.POINTER(ctypes.c_uint8), ip, ctypes.c_char_p, ctypes.c_size_t]
    L.dmi_mesh_coloration_from_lists_with_depth.restype = ctypes.c_int
    L.dmi_mesh_coloration_from_lists_with_depth.argtypes = [dp, i64, ctypes.c_char_p, ctypes.c_char_p, i32, ctypes.c_double,
                                                            ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8),
                                                            ctypes.POINTER(ctypes.c_int32), ctypes.c_char_p, ctypes.c_size_t]
    L.dmi_mesh_coloration_from_lists_with_mesh_depth.restype = ctypes.c_int
    L.dmi_mesh_coloration_from_lists_with_mesh_depth.argtypes = [dp, i64, ctypes.POINTER(ctypes.c_int64), i64, ctypes.c_char_p, ctypes.c_char_p,
                                                                 i32, ctypes.c_double, ctypes.POINTER(ctypes.c_uint8),
                                                                 ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int32), dp,
                                                                 ctypes.c_char_p, ctypes.c_size_t]
    L.dmi_read_polydata.restype = ctypes.c_void_p
    L.dmi_read_polydata.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
    L.dmi_polydata_free.restype = None
    L.dmi_polydata_free.argtypes = [ctypes.c_void_p]
    L.dmi_polydata_counts.restype = ctypes.c_int
    L.dmi_polydata_counts.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]
    L.dmi_polydata_array.restype = ctypes.c_int
    L.dmi_polydata_array.argtypes = [ctypes.c_void_p, i32, i32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_char_p),
                                     ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_void_p)]
    L.dmi_polydata_designations.restype = ctypes.c_char_p
    L.dmi_polydata_designations.argtypes = [ctypes.c_void_p, i32]
    L.dmi_write_polydata.restype = ctypes.c_int
    L.dmi_write_polydata.argtypes = [ctypes.c_char_p, dp, i64, ctypes.POINTER(ctypes.c_int64), i64]
    L.dmi_write_polydata_with_normals.restype = ctypes.c_int
    L.dmi_write_polydata_with_normals.argtypes = [ctypes.c_char_p, dp, i64, ctypes.POINTER(ctypes.c_int64), i64,
                                                  ctypes.POINTER(ctypes.c_float), ctypes.c_double]
    L.dmi_write_polydata_with_arrays.restype = ctypes.c_int
    L.dmi_write_polydata_with_arrays.argtypes = [ctypes.c_char_p, dp, i64, ctypes.POINTER(ctypes.c_int64), i64,
                                                 ctypes.POINTER(ctypes.c_float), ctypes.c_double, ctypes.POINTER(ctypes.c_int64)]
    L.dmi_write_polydata_with_colors.restype = ctypes.c_int
    L.dmi_write_polydata_with_colors.argtypes = L.dmi_write_polydata_with_arrays.argtypes + [
        ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int32)]
    _host_bound = True
    return L


class ReconstructionFilter:
    """The reference's vtkCudaReconstructionFilter (filt.h:48-120) through the host mirror: same setter
    names, Update() returns RequestData's 1 / 0, the output is the "reconstruction_scalar" cell array."""

    def __init__(self):
        self._lib = load_host()
        self._h = self._lib.dmi_filter_new()
        if not self._h:
            raise MemoryError("dmi_filter_new failed")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dmi_filter_delete(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def SetRayPotentialThickness(self, v): self._lib.dmi_filter_set_ray_potential_thickness(self._h, float(v))
    def SetRayPotentialRho(self, v): self._lib.dmi_filter_set_ray_potential_rho(self._h, float(v))
    def SetRayPotentialEta(self, v): self._lib.dmi_filter_set_ray_potential_eta(self._h, float(v))
    def SetRayPotentialDelta(self, v): self._lib.dmi_filter_set_ray_potential_delta(self._h, float(v))
    def SetThresholdBestCost(self, v): self._lib.dmi_filter_set_threshold_best_cost(self._h, float(v))

    def SetFilePathKRTD(self, path):
        self._lib.dmi_filter_set_file_path_krtd(self._h, None if path is None else os.fsencode(path))

    def SetFilePathVTI(self, path):
        self._lib.dmi_filter_set_file_path_vti(self._h, None if path is None else os.fsencode(path))

    def SetGridMatrix(self, m):
        if m is None:
            self._lib.dmi_filter_set_grid_matrix(self._h, None)
            return
        a = np.ascontiguousarray(m, dtype=np.float64).reshape(16)
        self._lib.dmi_filter_set_grid_matrix(self._h, _dp(a))

    def SetInputData(self, point_dims, origin, spacing):
        d = (ctypes.c_int32 * 3)(*[int(x) for x in point_dims])
        o = np.ascontiguousarray(origin, dtype=np.float64)
        s = np.ascontiguousarray(spacing, dtype=np.float64)
        self._point_dims = tuple(int(x) for x in point_dims)
        self._lib.dmi_filter_set_input_data(self._h, d, _dp(o), _dp(s))

    def AddView(self, depths, K3, RT4, best_cost=None):
        d = np.ascontiguousarray(depths, dtype=np.float64)
        H, W = d.shape
        bc = None if best_cost is None else np.ascontiguousarray(best_cost, dtype=np.float64)
        k = np.ascontiguousarray(K3, dtype=np.float64).reshape(9)
        rt = np.ascontiguousarray(RT4, dtype=np.float64).reshape(16)
        if not self._lib.dmi_filter_add_view(self._h, _dp(d), _dp(bc) if bc is not None else None, W, H, _dp(k), _dp(rt)):
            raise ValueError("dmi_filter_add_view rejected the view")

    def ClearViews(self): self._lib.dmi_filter_clear_views(self._h)
    def SetDevice(self, d): self._lib.dmi_filter_set_device(self._h, int(d))
    def SetKernelVariant(self, v): self._lib.dmi_filter_set_kernel_variant(self._h, int(v))

    def SetDevices(self, devices):
        d = (ctypes.c_int32 * len(devices))(*[int(x) for x in devices])
        self._lib.dmi_filter_set_devices(self._h, d, len(devices))

    def SetPartition(self, partition: str):
        self._lib.dmi_filter_set_partition(self._h, {"views": DMI_PARTITION_VIEWS, "z_slabs": DMI_PARTITION_Z_SLABS}[partition])

    def SetHostChunkBytes(self, n): self._lib.dmi_filter_set_host_chunk_bytes(self._h, int(n))
    def SetFillOnCallingThread(self, yes): self._lib.dmi_filter_set_fill_on_calling_thread(self._h, 1 if yes else 0)
    def Update(self) -> int: return int(self._lib.dmi_filter_update(self._h))
    def GetExecutionTime(self) -> float: return float(self._lib.dmi_filter_get_execution_time(self._h))
    def GetFuseKernelMs(self) -> float: return float(self._lib.dmi_filter_get_fuse_kernel_ms(self._h))
    def GetNumberOfCells(self) -> int: return int(self._lib.dmi_filter_get_number_of_cells(self._h))
    def LastError(self) -> str: return self._lib.dmi_filter_last_error(self._h).decode()

    def GetOutputScalars(self) -> np.ndarray:
        """The "reconstruction_scalar" cell array as [nz, ny, nx] (x fastest, filt.cxx:129-135)."""
        n = self.GetNumberOfCells()
        out = np.zeros(n, dtype=np.float64)
        got = self._lib.dmi_filter_get_output(self._h, _dp(out))
        if got != n:
            return out[:got]
        px, py, pz = self._point_dims
        return out.reshape(pz - 1, py - 1, px - 1)


class CliOptionsC(ctypes.Structure):
    _fields_ = [("grid_dims", ctypes.c_int32 * 3), ("grid_spacing", ctypes.c_double * 3), ("grid_origin", ctypes.c_double * 3),
                ("grid_end", ctypes.c_double * 3), ("grid_matrix", ctypes.c_double * 16), ("ray_thick", ctypes.c_double),
                ("ray_rho", ctypes.c_double), ("ray_eta", ctypes.c_double), ("ray_delta", ctypes.c_double),
                ("thresh_best_cost", ctypes.c_double), ("contour", ctypes.c_double), ("verbose", ctypes.c_int32),
                ("summary", ctypes.c_int32), ("force_cubic_voxel", ctypes.c_int32), ("extract_mesh", ctypes.c_int32),
                ("mesh_normals", ctypes.c_int32), ("mesh_largest_component", ctypes.c_int32), ("mesh_region_ids", ctypes.c_int32),
                ("mesh_min_component_triangles", ctypes.c_int64), ("mesh_smooth_iterations", ctypes.c_int64),
                ("mesh_smooth_lambda", ctypes.c_double), ("mesh_smooth_mu", ctypes.c_double),
                ("mesh_decimate_cell_size", ctypes.c_double), ("mesh_coloration", ctypes.c_int32),
                ("mesh_coloration_fused", ctypes.c_int32), ("mesh_coloration_depth_tolerance", ctypes.c_double),
                ("mesh_coloration_depth_from_mesh", ctypes.c_int32), ("mesh_decimate_quadric", ctypes.c_int32),
                ("depth_consistency_min_views", ctypes.c_int64), ("depth_consistency_tolerance", ctypes.c_double),
                ("depth_consistency_rel_tolerance", ctypes.c_double),
                ("grid_auto_bounds", ctypes.c_int32), ("grid_auto_bounds_trim", ctypes.c_double),
                ("grid_auto_bounds_margin", ctypes.c_double), ("grid_auto_bounds_pixel_step", ctypes.c_int64),
                ("mesh_fill_holes", ctypes.c_int64),
                ("contour_smooth_sigma", ctypes.c_double * 3), ("contour_smooth_truncate", ctypes.c_double),
                ("depth_speckle_min_pixels", ctypes.c_int64), ("depth_speckle_tolerance", ctypes.c_double),
                ("depth_speckle_rel_tolerance", ctypes.c_double),
                ("depth_fill_holes_max_pixels", ctypes.c_int64), ("depth_fill_holes_tolerance", ctypes.c_double),
                ("depth_fill_holes_rel_tolerance", ctypes.c_double),
                ("depth_smooth_sigma", ctypes.c_double), ("depth_smooth_truncate", ctypes.c_double),
                ("depth_smooth_tolerance", ctypes.c_double), ("depth_smooth_rel_tolerance", ctypes.c_double),
                ("depth_smooth_iterations", ctypes.c_int64), ("depth_staged_filters", ctypes.c_int32),
                ("point_cloud_cell_size", ctypes.c_double), ("point_cloud_min_cell_points", ctypes.c_int64),
                ("point_cloud_outlier_radius", ctypes.c_double), ("point_cloud_min_neighbors", ctypes.c_int64),
                ("point_cloud_plane_fit_radius", ctypes.c_double), ("point_cloud_plane_fit_min_neighbors", ctypes.c_int64),
                ("point_cloud_plane_fit_iterations", ctypes.c_int64), ("point_cloud_plane_fit_keep_positions", ctypes.c_int32),
                ("point_cloud_plane_fit_keep_normals", ctypes.c_int32)]


def cli_read_arguments(args):
    """ReadArguments of the `Reconstruction` tool (Reconstruction/main.cxx:216-343) on ["prog", "--flag", ...]:
    (options or None, the text the tool would print)."""
    L = load_host()
    L.dmi_cli_read_arguments.restype = ctypes.c_int
    L.dmi_cli_read_arguments.argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(CliOptionsC),
                                         ctypes.c_char_p, ctypes.c_size_t]
    argv = (ctypes.c_char_p * len(args))(*[os.fsencode(a) for a in args])
    out = CliOptionsC()
    err = ctypes.create_string_buffer(1 << 15)
    ok = L.dmi_cli_read_arguments(len(args), argv, ctypes.byref(out), err, len(err))
    return (out if ok else None), err.value.decode()


def write_polydata(path, points, triangles):
    """dmi_write_polydata: points [n, 3] f64 and triangles [m, 3] int64 as a VTK XML PolyData (.vtp) file; no GPU needed."""
    L = load_host()
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, dtype=np.int64).reshape(-1, 3)
    ok = L.dmi_write_polydata(os.fsencode(path), _dp(p), p.shape[0], t.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), t.shape[0])
    if not ok:
        raise OSError(f"dmi_write_polydata failed: {path}")


def write_polydata_with_normals(path, points, triangles, normals, contour):
    """dmi_write_polydata_with_normals: write_polydata's file plus the point arrays Normals ([n, 3] f32) and
    reconstruction_scalar (f64, `contour` at every point); no GPU needed."""
    L = load_host()
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, dtype=np.int64).reshape(-1, 3)
    n = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    if n.shape != p.shape:
        raise ValueError(f"normals {n.shape} do not match points {p.shape}")
    ok = L.dmi_write_polydata_with_normals(os.fsencode(path), _dp(p), p.shape[0], t.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                           t.shape[0], n.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), float(contour))
    if not ok:
        raise OSError(f"dmi_write_polydata_with_normals failed: {path}")


def write_polydata_with_arrays(path, points, triangles, normals=None, contour=0.0, region_ids=None, colors=None):
    """dmi_write_polydata_with_arrays: write_polydata's file (normals None) or write_polydata_with_normals' plus the point array
    RegionId ([n] int64) when region_ids is given; with colors = (mean [n, 3] u8, median [n, 3] u8, count [n] i32) the arrays
    MeanColoration, MedianColoration and NbProjectedDepthMap behind those (dmi_write_polydata_with_colors); no GPU needed."""
    L = load_host()
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, dtype=np.int64).reshape(-1, 3)
    n = r = None
    if normals is not None:
        n = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        if n.shape != p.shape:
            raise ValueError(f"normals {n.shape} do not match points {p.shape}")
        n = np.concatenate([n.reshape(-1), np.zeros(1, np.float32)])     # never a null pointer, even for an empty mesh
    if region_ids is not None:
        r = np.ascontiguousarray(region_ids, dtype=np.int64).reshape(-1)
        if r.shape[0] != p.shape[0]:
            raise ValueError(f"region ids {r.shape} do not match points {p.shape}")
        r = np.concatenate([r, np.zeros(1, np.int64)])
    args = [os.fsencode(path), _dp(p), p.shape[0], t.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
            t.shape[0], None if n is None else n.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
            float(contour), None if r is None else r.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))]
    if colors is not None:
        mean = np.concatenate([np.ascontiguousarray(colors[0], dtype=np.uint8).reshape(-1, 3), np.zeros((1, 3), np.uint8)])
        median = np.concatenate([np.ascontiguousarray(colors[1], dtype=np.uint8).reshape(-1, 3), np.zeros((1, 3), np.uint8)])
        count = np.concatenate([np.ascontiguousarray(colors[2], dtype=np.int32).reshape(-1), np.zeros(1, np.int32)])
        if not (mean.shape[0] == median.shape[0] == count.shape[0] == p.shape[0] + 1):
            raise ValueError("colors do not match points")
        u8 = ctypes.POINTER(ctypes.c_uint8)
        ok = L.dmi_write_polydata_with_colors(*args, mean.ctypes.data_as(u8), median.ctypes.data_as(u8),
                                              count.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    else:
        ok = L.dmi_write_polydata_with_arrays(*args)
    if not ok:
        raise OSError(f"dmi_write_polydata_with_arrays failed: {path}")


def cli_binary() -> str:
    """Path of the dmi_reconstruction executable next to the library (linked now if the build has not done so: it needs
    hipcc, which a box that only runs a prebuilt library may lack -- loading the library never depends on it)."""
    from . import build as _build
    # always through build_cli(): it returns at once when the executable's digest names the library's sources, and relinks one
    # left over from older sources (an older ABI's main against this library) -- only without hipcc is an existing file taken as is
    try:
        _build.build_cli()
    except Exception:
        if not os.path.exists(_build.CLI_PATH):
            raise
    return _build.CLI_PATH


def read_krtd_file(path):
    L = load_host()
    K = np.zeros(9)
    RT = np.zeros(16)
    ok = L.dmi_read_krtd_file(os.fsencode(path), _dp(K), _dp(RT))
    return bool(ok), K.reshape(3, 3), RT.reshape(4, 4)


def extract_all_file_path(list_path):
    L = load_host()
    buf = ctypes.create_string_buffer(1 << 16)
    n = L.dmi_extract_all_file_path(os.fsencode(list_path), buf, len(buf))
    paths = buf.value.decode().split("\n") if n else []
    return paths


def k3_to_k4(K3):
    L = load_host()
    k = np.ascontiguousarray(K3, dtype=np.float64).reshape(9)
    out = np.zeros(16)
    L.dmi_k3_to_k4(_dp(k), _dp(out))
    return out.reshape(4, 4)


def apply_depth_threshold(depths, best_cost, threshold):
    L = load_host()
    d = np.ascontiguousarray(depths, dtype=np.float64).copy()
    b = np.ascontiguousarray(best_cost, dtype=np.float64)
    changed = L.dmi_apply_depth_threshold(_dp(d.reshape(-1)), _dp(b.reshape(-1)), d.size, float(threshold))
    return d, int(changed)


def read_depth_map(path):
    L = load_host()
    dims = (ctypes.c_int32 * 3)()
    has = ctypes.c_int32(0)
    if not L.dmi_read_depth_map(os.fsencode(path), dims, None, None, ctypes.byref(has)):
        return None
    n = dims[0] * dims[1] * dims[2]
    d = np.zeros(n)
    bc = np.zeros(n)
    L.dmi_read_depth_map(os.fsencode(path), dims, _dp(d), _dp(bc), ctypes.byref(has))
    shape = (dims[1], dims[0])
    return d.reshape(shape), (bc.reshape(shape) if has.value else None)


def read_depth_map_color(path):
    """The "Color" array of a depth-map .vti as [H, W, 3] u8 (vtk row order), or None when the file has none."""
    L = load_host()
    dims = (ctypes.c_int32 * 3)()
    has = ctypes.c_int32(0)
    if not L.dmi_read_depth_map_color(os.fsencode(path), dims, None, ctypes.byref(has)) or not has.value:
        return None
    c = np.zeros(dims[0] * dims[1] * dims[2] * 3, dtype=np.uint8)
    L.dmi_read_depth_map_color(os.fsencode(path), dims, c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(has))
    return c.reshape(dims[1], dims[0], 3)


def mesh_coloration_from_lists(points, vti_list, krtd_list, device: int = 0, depth_tolerance: float | None = None, triangles=None):
    """MeshColoration(mesh, vtiList, krtdList).ProcessColoration() through the host mirror (reads the .vti/.krtd files).
    depth_tolerance: with the depth test of dmi_color_set_depth_test (MeshColoration::SetDepthTolerance).  triangles [t, 3] ids
    (needs depth_tolerance): the test compares against the mesh's own rendered depth and the files need no "Depths" arrays
    (dmi_mesh_coloration_from_lists_with_mesh_depth)."""
    L = load_host()
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    nv = pts.shape[0]
    mean = np.zeros((nv, 3), dtype=np.uint8)
    median = np.zeros((nv, 3), dtype=np.uint8)
    count = np.zeros(nv, dtype=np.int32)
    err = ctypes.create_string_buffer(512)
    u8 = ctypes.POINTER(ctypes.c_uint8)
    outs = (mean.ctypes.data_as(u8), median.ctypes.data_as(u8), count.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), err, len(err))
    if triangles is not None:
        if depth_tolerance is None:
            raise ValueError("triangles (the mesh's own depth) need a depth_tolerance")
        tri = np.ascontiguousarray(triangles, dtype=np.int64).reshape(-1, 3)
        ok = L.dmi_mesh_coloration_from_lists_with_mesh_depth(_dp(pts), nv, tri.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), tri.shape[0],
                                                              os.fsencode(vti_list), os.fsencode(krtd_list), device, float(depth_tolerance),
                                                              outs[0], outs[1], outs[2], None, err, len(err))
    elif depth_tolerance is None:
        ok = L.dmi_mesh_coloration_from_lists(_dp(pts), nv, os.fsencode(vti_list), os.fsencode(krtd_list), device, *outs)
    else:
        ok = L.dmi_mesh_coloration_from_lists_with_depth(_dp(pts), nv, os.fsencode(vti_list), os.fsencode(krtd_list), device,
                                                         float(depth_tolerance), *outs)
    if not ok:
        raise RuntimeError(err.value.decode())
    return mean, median, count


# ---- the `Coloration` tool: .vtp in, coloured .vtp out (include/dmi_host.h) ----------------------------------------------------
_VTK_DTYPES = {"Int8": np.int8, "UInt8": np.uint8, "Int16": np.int16, "UInt16": np.uint16, "Int32": np.int32, "UInt32": np.uint32,
               "Int64": np.int64, "UInt64": np.uint64, "Float32": np.float32, "Float64": np.float64}


class PolyDataFile(NamedTuple):
    """What dmi_read_polydata reads from a .vtp: arrays in their stored types; a data array of one component is [n], else
    [n, components]; designations are (key, value) pairs of <PointData ...> / <CellData ...>."""
    points: np.ndarray
    connectivity: np.ndarray
    offsets: np.ndarray
    point_data: dict
    cell_data: dict
    point_designations: list
    cell_designations: list


def read_polydata(path) -> PolyDataFile:
    """VTK XML PolyData without VTK (csrc/host/vtp_reader.h); no GPU needed.  Raises ValueError with the reader's reason."""
    L = load_host()
    err = ctypes.create_string_buffer(4096)
    h = L.dmi_read_polydata(os.fsencode(path), err, len(err))
    if not h:
        raise ValueError(err.value.decode())
    try:
        counts = (ctypes.c_int64 * 5)()
        L.dmi_polydata_counts(h, counts)

        def array(kind, index):
            name, tname, comps, n, data = ctypes.c_char_p(), ctypes.c_char_p(), ctypes.c_int32(), ctypes.c_int64(), ctypes.c_void_p()
            if not L.dmi_polydata_array(h, kind, index, ctypes.byref(name), ctypes.byref(tname), ctypes.byref(comps), ctypes.byref(n),
                                        ctypes.byref(data)):
                raise ValueError(f"{path}: no array {kind}/{index}")
            dt = np.dtype(_VTK_DTYPES[tname.value.decode()])
            nbytes = n.value * comps.value * dt.itemsize
            a = np.frombuffer(ctypes.string_at(data.value, nbytes) if nbytes else b"", dtype=dt).copy()
            return name.value.decode(), (a.reshape(-1, comps.value) if comps.value != 1 else a)

        def designations(cell):
            text = L.dmi_polydata_designations(h, cell).decode()
            return [tuple(line.split("=", 1)) for line in text.splitlines() if line]

        return PolyDataFile(array(0, 0)[1], array(1, 0)[1], array(2, 0)[1],
                            dict(array(3, i) for i in range(counts[3])), dict(array(4, i) for i in range(counts[4])),
                            designations(0), designations(1))
    finally:
        L.dmi_polydata_free(h)


class ColorCliOptionsC(ctypes.Structure):
    _fields_ = [("input", ctypes.c_char * 4096), ("output", ctypes.c_char * 4096), ("krtd", ctypes.c_char * 4096),
                ("vti", ctypes.c_char * 4096), ("verbose", ctypes.c_int32), ("device", ctypes.c_int32), ("depth_test", ctypes.c_int32),
                ("depth_tolerance", ctypes.c_double), ("depth_from_mesh", ctypes.c_int32)]


def color_cli_read_arguments(args):
    """ReadArguments of the `Coloration` tool (Coloration/main.cxx:105-135) on ["prog", "--flag", ...]:
    (options or None, the text the tool would print)."""
    L = load_host()
    L.dmi_color_cli_read_arguments.restype = ctypes.c_int
    L.dmi_color_cli_read_arguments.argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ColorCliOptionsC),
                                               ctypes.c_char_p, ctypes.c_size_t]
    argv = (ctypes.c_char_p * len(args))(*[os.fsencode(a) for a in args])
    out = ColorCliOptionsC()
    err = ctypes.create_string_buffer(1 << 15)
    ok = L.dmi_color_cli_read_arguments(len(args), argv, ctypes.byref(out), err, len(err))
    return (out if ok else None), err.value.decode()


def coloration_cli_binary() -> str:
    """Path of the dmi_coloration executable next to the library (linked now if the build has not done so; see cli_binary)."""
    from . import build as _build
    try:
        _build.build_color_cli()
    except Exception:
        if not os.path.exists(_build.COLOR_CLI_PATH):
            raise
    return _build.COLOR_CLI_PATH
