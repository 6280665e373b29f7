"""The host-side rules of the radius neighbour count (csrc/depth_points_radius_rules.h), checked on the CPU: a
stand-alone program (tests/cpp/depth_points_radius_rules_host.cpp) built with AddressSanitizer + UBSan and run; nothing is loaded into
Python.  The cell-size rule at the 2^21 edge, the clamped row ranges against a plain walk, the completeness of the 27-cell search on
adversarial pairs; and that the build, the header and the binding know the new entry points."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudadepthmapintegration_amd", "csrc")
SYMBOLS = ("dmi_count_point_neighbors", "dmi_views_filter_points_radius", "dmi_views_download_point_neighbors",
           "dmi_views_get_radius_pass_ms", "dmi_views_set_radius_group_points")


def test_depth_points_radius_rules_at_their_boundaries(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "depth_points_radius_rules_host")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "cpp", "depth_points_radius_rules_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failed"), (r.stdout[-3000:], r.stderr[-3000:])


def test_the_build_knows_the_new_files():
    from cudadepthmapintegration_amd import build

    assert {"depth_points_radius.hip", "dmi_capi_points_radius.hip"} <= set(build._sources())
    assert {"depth_points_radius.h", "depth_points_radius_rules.h"} <= {os.path.relpath(h, CSRC) for h in build._headers()}


def test_the_library_exports_the_new_symbols_and_the_binding_follows_the_header():
    import ctypes

    from cudadepthmapintegration_amd import capi

    lib = ctypes.CDLL(capi.load()._name)
    for name in SYMBOLS:
        assert name in capi.ABI_SYMBOLS and hasattr(lib, name), name
    assert lib.dmi_abi_version() == 5
    header = open(os.path.join(ROOT, "include", "dmi.h")).read()
    body = re.search(r"typedef struct dmi_points_radius_report \{(.*?)\}", header, re.S).group(1)
    assert re.findall(r"\b([a-z_0-9]+)\s*[,;]", body) == [name for name, _ in capi.PointsRadiusReportC._fields_]
    rules = open(os.path.join(CSRC, "depth_points_radius_rules.h")).read()
    default = int(re.search(r"kDefaultGroupPoints = (\d+);", rules).group(1))
    assert f"uses the default, {default}." in header


def test_the_refusals_that_need_no_device():
    """Every argument check comes before the device is touched; P = 0 succeeds without one."""
    import numpy as np

    from cudadepthmapintegration_amd import capi

    xyz = np.zeros((4, 3))
    for radius in (float("nan"), float("inf"), 0.0, -1.0, 1e-200, 1e200):
        with pytest.raises(capi.DmiError) as e:
            capi.count_point_neighbors(xyz, radius=radius)
        assert e.value.code == 1 and "radius" in str(e.value) and "dmi_count_point_neighbors" in str(e.value)
    with pytest.raises(capi.DmiError) as e:
        capi.count_point_neighbors(xyz, radius=1.0, min_neighbors=-1)
    assert e.value.code == 1 and "min_neighbors" in str(e.value)
    neighbors, keep, report = capi.count_point_neighbors(np.zeros((0, 3)), radius=1.0)
    assert len(neighbors) == 0 and len(keep) == 0 and report["points_in"] == 0 and report["points_kept"] == 0
    L = capi.load()
    assert L.dmi_count_point_neighbors(None, 4, 1.0, 1, 0, None, None, None, None) == 1 and b"n_kept" in L.dmi_last_error(None)
