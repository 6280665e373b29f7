"""--pointCloudPlaneFitRadius and its companions at the command line's argument reader (recon_cli.cpp through
dmi_cli_read_arguments): what they need, what they refuse, what --help says, and that the options struct of
include/dmi_host.h and its Python binding carry them; the refusals of dmi_fit_point_planes that need no device; the exported
symbols.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from cudadepthmapintegration_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["prog", "--gridOrigin", "-1", "-1", "-1", "--gridEnd", "1", "1", "1", "--dataFolder", "data", "--outputGridFilename", "out.vts",
        "--outputMeshFilename", "mesh.vtp", "--rayThick", "0.1", "--gridDims", "10"]
CLOUD = ["--outputPointCloudFilename", "cloud.vtp", "--pointCloudTolerance", "0.02"]
FIT = ["--pointCloudPlaneFitRadius", "0.25"]
SYMBOLS = ("dmi_fit_point_planes", "dmi_views_fit_point_planes", "dmi_views_download_point_plane_rms", "dmi_views_get_plane_fit_pass_ms")


def test_the_options_reach_the_host_struct():
    o, text = capi.cli_read_arguments(BASE + CLOUD)
    assert o is not None and o.point_cloud_plane_fit_radius == 0.0 and o.point_cloud_plane_fit_min_neighbors == 5, text
    assert o.point_cloud_plane_fit_iterations == 1 and not o.point_cloud_plane_fit_keep_positions and not o.point_cloud_plane_fit_keep_normals
    o, text = capi.cli_read_arguments(BASE + CLOUD + FIT)
    assert o is not None and o.point_cloud_plane_fit_radius == 0.25 and o.point_cloud_plane_fit_min_neighbors == 5, text
    o, text = capi.cli_read_arguments(BASE + CLOUD + FIT + ["--pointCloudPlaneFitMinNeighbors", "2", "--pointCloudPlaneFitIterations", "3",
                                                            "--pointCloudPlaneFitKeepNormals", "--pointCloudOutlierRadius", "1e-3",
                                                            "--pointCloudMinNeighbors", "0"])
    assert o is not None and o.point_cloud_plane_fit_min_neighbors == 2 and o.point_cloud_plane_fit_iterations == 3, text
    assert o.point_cloud_plane_fit_keep_normals == 1 and o.point_cloud_plane_fit_keep_positions == 0
    assert o.point_cloud_outlier_radius == 1e-3 and o.point_cloud_min_neighbors == 0   # the fields in front of the new ones stand where they stood
    assert capi.cli_read_arguments(BASE + CLOUD + FIT + ["--pointCloudPlaneFitKeepPositions"])[0].point_cloud_plane_fit_keep_positions == 1


def test_the_flags_refusals_say_why():
    o, text = capi.cli_read_arguments(BASE + FIT)
    assert o is None and text.startswith("Error : --pointCloudPlaneFitRadius needs --outputPointCloudFilename"), text
    for flag in (["--pointCloudPlaneFitMinNeighbors", "3"], ["--pointCloudPlaneFitIterations", "2"], ["--pointCloudPlaneFitKeepPositions"],
                 ["--pointCloudPlaneFitKeepNormals"]):
        o, text = capi.cli_read_arguments(BASE + CLOUD + flag)
        assert o is None and text.startswith(f"Error : {flag[0]} needs --pointCloudPlaneFitRadius"), text
    o, text = capi.cli_read_arguments(BASE + CLOUD + FIT + ["--pointCloudPlaneFitKeepPositions", "--pointCloudPlaneFitKeepNormals"])
    assert o is None and "nothing to do" in text.split("\n")[0], text
    for value in ("0", "-1", "nan", "inf", "x", "1e-200", "1e200"):
        o, text = capi.cli_read_arguments(BASE + CLOUD + ["--pointCloudPlaneFitRadius", value])
        assert o is None and "--pointCloudPlaneFitRadius" in text.split("\n")[0], (value, text[:200])
    for value in ("1", "0", "-2", "1.5", str(2 ** 31)):
        o, text = capi.cli_read_arguments(BASE + CLOUD + FIT + ["--pointCloudPlaneFitMinNeighbors", value])
        assert o is None and "--pointCloudPlaneFitMinNeighbors" in text.split("\n")[0], (value, text[:200])
    for value in ("0", "-1", "101", "2.5"):
        o, text = capi.cli_read_arguments(BASE + CLOUD + FIT + ["--pointCloudPlaneFitIterations", value])
        assert o is None and "--pointCloudPlaneFitIterations" in text.split("\n")[0], (value, text[:200])


def test_help_names_the_flags_and_the_array():
    o, text = capi.cli_read_arguments(BASE + ["--help"])
    text = " ".join(text.split())
    for flag in ("--pointCloudPlaneFitRadius", "--pointCloudPlaneFitMinNeighbors", "--pointCloudPlaneFitIterations",
                 "--pointCloudPlaneFitKeepPositions", "--pointCloudPlaneFitKeepNormals", "PlaneRms"):
        assert flag in text, flag
    assert o is None and "behind --pointCloudOutlierRadius and before --pointCloudCellSize" in text


def test_the_library_exports_the_new_symbols_and_the_binding_follows_the_header():
    lib = ctypes.CDLL(capi.load()._name)
    for name in SYMBOLS:
        assert name in capi.ABI_SYMBOLS and hasattr(lib, name), name
    assert lib.dmi_abi_version() == 5
    header = open(os.path.join(ROOT, "include", "dmi.h")).read()
    body = re.search(r"typedef struct dmi_points_planes_report \{(.*?)\}", header, re.S).group(1)
    assert re.findall(r"\b([a-z_0-9]+)\s*[,;]", body) == [name for name, _ in capi.PointsPlanesReportC._fields_]
    assert re.search(r"#define DMI_PLANE_FIT_MOVE (\d+)", header).group(1) == str(capi.PLANE_FIT_MOVE)
    assert re.search(r"#define DMI_PLANE_FIT_NORMALS (\d+)", header).group(1) == str(capi.PLANE_FIT_NORMALS)


def test_the_refusals_that_need_no_device():
    """Every argument check comes before the device is touched; P = 0 succeeds without one."""
    xyz = np.zeros((4, 3))
    for radius in (float("nan"), float("inf"), 0.0, -1.0, 1e-200, 1e200):
        with pytest.raises(capi.DmiError) as e:
            capi.fit_point_planes(xyz, radius=radius)
        assert e.value.code == 1 and "radius" in str(e.value) and "dmi_fit_point_planes" in str(e.value)
    for min_neighbors in (1, 0, -1):
        with pytest.raises(capi.DmiError) as e:
            capi.fit_point_planes(xyz, radius=1.0, min_neighbors=min_neighbors)
        assert e.value.code == 1 and "min_neighbors" in str(e.value)
    with pytest.raises(capi.DmiError) as e:
        capi.fit_point_planes(xyz, radius=1.0, move=False, normals=False)
    assert e.value.code == 1 and "flags" in str(e.value)
    L = capi.load()
    assert L.dmi_fit_point_planes(None, None, 4, 1.0, 5, 4, 0, None, None, None, None, None) == 1 and b"flags" in L.dmi_last_error(None)
    assert L.dmi_fit_point_planes(None, None, 4, 1.0, 5, 3, 0, None, None, None, None, None) == 1 and b"xyz is null" in L.dmi_last_error(None)
    assert L.dmi_fit_point_planes(xyz.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, 4, 1.0, 5, 1, 0, None, None, None, None, None) == 1
    assert b"out_xyz" in L.dmi_last_error(None)
    assert L.dmi_fit_point_planes(xyz.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, 4, 1.0, 5, 2, 0, None, None, None, None, None) == 1
    assert b"out_normal" in L.dmi_last_error(None)
    arrays, report = capi.fit_point_planes(np.zeros((0, 3)), radius=1.0)
    assert len(arrays["plane_rms"]) == 0 and len(arrays["neighbors"]) == 0 and report["points_in"] == 0 and report["fitted"] == 0
    assert L.dmi_views_fit_point_planes(None, 1.0, 5, 3, None) == 1 and L.dmi_views_download_point_plane_rms(None, 0, 0, None) == 1
