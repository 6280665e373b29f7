"""csrc/depth_speckle_rules.h on the CPU: a stand-alone program (tests/cpp/depth_speckle_rules_host.cpp), built
with AddressSanitizer + UBSan and run; nothing is loaded into Python.  The run arithmetic of a row's 64 link bits against naive
loops at every lane, the lanes that hook, the tile counts and the border pairs for W, H in {1, 63, 64, 65, 32768}."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudadepthmapintegration_amd", "csrc")


def test_run_and_tile_rules(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "depth_speckle_rules_host")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "depth_speckle_rules_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failed"), (r.stdout[-3000:], r.stderr[-3000:])


def test_the_build_knows_the_new_files():
    from cudadepthmapintegration_amd import build

    assert {"depth_speckle.hip", "dmi_capi_speckle.hip", "isosurface_components.hip"} <= set(build._sources())
    headers = {os.path.relpath(h, CSRC) for h in build._headers()}
    assert {"depth_speckle.h", "depth_speckle_rules.h", "union_find_device.h"} <= headers
    # one union-find, shared: neither kernel file keeps a copy of its own
    for name in ("isosurface_components.hip", "depth_speckle.hip"):
        text = open(os.path.join(CSRC, name)).read()
        assert '#include "union_find_device.h"' in text and "uint32_t find_root(" not in text, name
