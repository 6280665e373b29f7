"""What the mesh stages share (csrc/dmi_mesh_stage.h) on the CPU: tests/cpp/mesh_stage_host.cpp, a stand-alone program built with
AddressSanitizer + UBSan against the host stand-in of the HIP runtime (tests/cpp/support_host/) and run; nothing is loaded into
Python.  A stage's events are created all or none with the creation failing at every event in turn and destroyed exactly once,
the times read from them, every size refusal on both sides of its bound with the text it had before, the commit of a stage's result
for every row of the drop table with and without normals, the scratch carving against the expressions it replaced."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudadepthmapintegration_amd", "csrc")


def test_events_times_refusals_commits_and_carving(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "mesh_stage_host")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "tests", "cpp", "support_host"), "-I" + CSRC,
                           os.path.join(ROOT, "tests", "cpp", "mesh_stage_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failed"), (r.stdout[-3000:], r.stderr[-3000:])


def test_the_build_knows_the_header_and_the_header_stands_alone():
    from cudadepthmapintegration_amd import build

    assert "dmi_mesh_stage.h" in {os.path.relpath(h, CSRC) for h in build._headers()}
    # a host program can only compile it while it keeps away from the context's header (fusion_kernels.h is device code)
    with open(os.path.join(CSRC, "dmi_mesh_stage.h")) as fh:
        includes = [line.split()[1].strip('"<>') for line in fh if line.startswith("#include")]
    assert set(includes) == {"../../include/dmi.h", "dmi_buffer.h", "array", "string", "utility"}, includes
