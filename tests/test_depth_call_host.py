"""The scaffold of the context-free depth-map calls (csrc/dmi_depth_call.h) on the CPU: tests/cpp/depth_call_host.cpp, a stand-alone
program built with AddressSanitizer + UBSan against the host stand-in of the HIP runtime (tests/cpp/support_host/) and run; nothing
is loaded into Python.  What a call holds is released exactly once with the allocator failing at every hipMalloc in turn, a refused
opening creates nothing, the staging rule at its edges and against the expression it replaced, the shared checks at their bounds,
the staged upload in pieces of 3 and 2 views."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudadepthmapintegration_amd", "csrc")


def test_the_scaffold_releases_everything_once_and_stages_by_the_rule(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "depth_call_host")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "tests", "cpp", "support_host"), "-I" + CSRC,
                           os.path.join(ROOT, "tests", "cpp", "depth_call_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failed"), (r.stdout[-3000:], r.stderr[-3000:])


def test_the_build_knows_the_header():
    from cudadepthmapintegration_amd import build

    assert "dmi_depth_call.h" in {os.path.relpath(h, CSRC) for h in build._headers()}
