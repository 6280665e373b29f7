"""csrc/depth_smooth_rules.h on the CPU: a stand-alone program (tests/cpp/depth_smooth_rules_host.cpp), built with
AddressSanitizer + UBSan and run; nothing is loaded into Python.  The radius rule at its edges, the weights within an ulp of exp,
the refusals that write nothing."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudadepthmapintegration_amd", "csrc")


def test_radius_rule_weights_and_refusals(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "depth_smooth_rules_host")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "depth_smooth_rules_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failed"), (r.stdout[-3000:], r.stderr[-3000:])


def test_the_build_knows_the_new_files():
    from cudadepthmapintegration_amd import build

    assert {"depth_smooth.hip", "dmi_capi_smooth.hip"} <= set(build._sources())
    headers = {os.path.relpath(h, CSRC) for h in build._headers()}
    assert {"depth_smooth.h", "depth_smooth_rules.h", "depth_speckle_rules.h"} <= headers
    # the rules header is plain C++ (the command line's parser includes it), and the tile geometry is shared, not copied
    rules = open(os.path.join(CSRC, "depth_smooth_rules.h")).read()
    assert "hip/" not in rules and "__device__" not in rules
    kernel = open(os.path.join(CSRC, "depth_smooth.hip")).read()
    assert '#include "depth_speckle_rules.h"' in kernel and "kTileWidth = 64" not in kernel
    assert '#include "../depth_smooth_rules.h"' in open(os.path.join(CSRC, "host", "recon_cli.cpp")).read()
