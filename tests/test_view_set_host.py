"""The resident view set without a GPU: csrc/view_set_rules.h in a stand-alone program (tests/cpp/
view_set_rules_host.cpp) built with AddressSanitizer + UBSan and run -- nothing is loaded into Python --, the build's file lists,
and the argument checks of dmi_views_create that come before the device is asked for."""
import ctypes
import os
import shutil
import subprocess

import pytest

from cudadepthmapintegration_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudadepthmapintegration_amd", "csrc")


def test_partition_bytes_and_report_rules(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "view_set_rules_host")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "view_set_rules_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failed"), (r.stdout[-3000:], r.stderr[-3000:])


def test_the_build_knows_the_new_files():
    from cudadepthmapintegration_amd import build

    assert {"view_set_kernels.hip", "dmi_capi_viewset.hip"} <= set(build._sources())
    headers = {os.path.relpath(h, CSRC) for h in build._headers()}
    assert {"dmi_view_set.h", "view_set_kernels.h", "view_set_rules.h"} <= headers
    rules = open(os.path.join(CSRC, "view_set_rules.h")).read()
    assert "hip/" not in rules and "__device__" not in rules and "__global__" not in rules
    # one implementation per filter: the set's file launches no filter pass itself
    viewset = open(os.path.join(CSRC, "dmi_capi_viewset.hip")).read()
    for launch in ("launch_speckle_local", "launch_holes_local", "launch_depth_smooth", "launch_consistency_count", "launch_bounds_count"):
        assert launch not in viewset
    for body, home in (("run_speckle_piece", "dmi_capi_speckle.hip"), ("run_holes_piece", "dmi_capi_holes.hip"),
                       ("run_smooth_piece", "dmi_capi_smooth.hip"), ("run_consistency_count", "dmi_capi_consistency.hip"),
                       ("run_bounds_select", "dmi_capi_bounds.hip")):
        assert body in viewset and open(os.path.join(CSRC, home)).read().count(body) >= 2   # defined and called there


def test_create_checks_its_arguments_before_it_asks_for_a_device():
    lib = capi.load()
    assert lib.dmi_sizeof_views_info() == ctypes.sizeof(capi.ViewsInfoC)
    assert lib.dmi_views_create(0, 64, 64, None) == 1 and b"out is null" in lib.dmi_views_last_error(None)
    for W, H, name in ((0, 64, b"W"), (32769, 64, b"W"), (64, 0, b"H"), (64, 32769, b"H"), (-3, 64, b"W")):
        handle = ctypes.c_void_p(7)
        assert lib.dmi_views_create(0, W, H, ctypes.byref(handle)) == 1
        assert lib.dmi_views_last_error(None).startswith(b"dmi_views_create: " + name + b" must lie in [1, 32768]") and not handle.value
    with pytest.raises(capi.DmiError) as e:
        capi.ViewSet(0, 70)
    assert e.value.code == 1
    if capi.device_count() == 0:   # legal sizes reach the device question, and only then
        with pytest.raises(capi.DmiError) as e:
            capi.ViewSet(150, 70)
        assert e.value.code == 2 and "no HIP device" in str(e.value)
    # a null set is refused by every entry point, and destroying one is a no-op
    lib.dmi_views_destroy(None)
    r = capi.ViewsStepReportC()
    assert lib.dmi_views_filter_speckles(None, 0.0, 0.0, 1, None, ctypes.byref(r)) == 1
    assert lib.dmi_views_download(None, 0, 1, None) == 1 and lib.dmi_views_clear(None) == 1
    assert lib.dmi_views_get_info(None, None) == 1 and lib.dmi_views_set_piece_bytes(None, 1) == 1
    assert b"the set is null" in lib.dmi_views_last_error(None)


def test_cli_takes_the_staged_flag_with_one_of_the_five_and_refuses_it_alone():
    base = ["prog", "--gridOrigin", "-2.29", "-2.24", "-2.2", "--gridEnd", "1.19", "1.67", "1.22", "--dataFolder", "data",
            "--outputGridFilename", "out.vts", "--outputMeshFilename", "mesh.vtp", "--rayThick", "0.1", "--gridDims", "10"]
    o, text = capi.cli_read_arguments(base)
    assert o is not None and o.depth_staged_filters == 0, text
    for with_flag in (["--depthSpeckleMinPixels", "5"], ["--depthFillHolesMaxPixels", "4"], ["--depthSmoothSigma", "1"],
                      ["--depthConsistencyMinViews", "1"]):
        o, text = capi.cli_read_arguments(base + with_flag)
        assert o is not None and o.depth_staged_filters == 0, text
        o, text = capi.cli_read_arguments(base + with_flag + ["--depthStagedFilters"])
        assert o is not None and o.depth_staged_filters == 1, text
    auto = [a for a in base if a not in ("--gridOrigin", "-2.29", "-2.24", "-2.2", "--gridEnd", "1.19", "1.67", "1.22")]
    o, text = capi.cli_read_arguments(auto + ["--gridAutoBounds", "--depthStagedFilters"])
    assert o is not None and o.depth_staged_filters == 1 and o.grid_auto_bounds == 1, text
    o, text = capi.cli_read_arguments(base + ["--depthStagedFilters"])
    assert o is None and text.startswith("Error : --depthStagedFilters needs --depthSpeckleMinPixels"), text
    o, text = capi.cli_read_arguments(base + ["--depthStagedFilters", "--depthSpeckleTolerance", "1"])   # a dependent flag does not do
    assert o is None and text.startswith("Error : "), text
    o, text = capi.cli_read_arguments(base + ["--help"])
    assert o is None and "--depthStagedFilters" in text and "not in the reference" in text.split("--depthStagedFilters")[1].split("--gridAutoBounds ")[0]
