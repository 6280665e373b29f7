"""csrc/depth_holes_rules.h on the CPU: a stand-alone program (tests/cpp/depth_holes_rules_host.cpp), built with
AddressSanitizer + UBSan and run; nothing is loaded into Python.  A row's links between hole pixels and the nearest valid column on
either side of a lane against naive loops at every lane, the record word, the walk limit."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudadepthmapintegration_amd", "csrc")


def test_hole_run_and_nearest_valid_rules(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "depth_holes_rules_host")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "depth_holes_rules_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failed"), (r.stdout[-3000:], r.stderr[-3000:])


def test_the_build_knows_the_new_files():
    from cudadepthmapintegration_amd import build

    assert {"depth_holes.hip", "dmi_capi_holes.hip", "depth_speckle.hip"} <= set(build._sources())
    headers = {os.path.relpath(h, CSRC) for h in build._headers()}
    assert {"depth_holes.h", "depth_holes_rules.h", "depth_speckle_rules.h", "union_find_device.h"} <= headers
    # the union-find and the tile rules are shared, not copied
    text = open(os.path.join(CSRC, "depth_holes.hip")).read()
    assert '#include "union_find_device.h"' in text and "uint32_t find_root(" not in text
    rules = open(os.path.join(CSRC, "depth_holes_rules.h")).read()
    assert '#include "depth_speckle_rules.h"' in rules and "inline int run_start(" not in rules
