"""The host-side rules of dmi_views_build_points (csrc/depth_points_rules.h), checked on the CPU: a stand-alone
program (tests/cpp/depth_points_rules_host.cpp) built with AddressSanitizer + UBSan and run; nothing is loaded into Python.  The
choice of tangent over all sixteen patterns of usable neighbours; the compaction's blocks at sizes around the block size, a whole
count / scan / rank against a plain walk; the byte offsets of the point arrays above 2^32 bytes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudadepthmapintegration_amd", "csrc")


def test_depth_points_rules_at_their_boundaries(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "depth_points_rules_host")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "depth_points_rules_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failed"), (r.stdout[-3000:], r.stderr[-3000:])


def test_the_build_knows_the_new_files():
    """The source digest sees a header only through build._headers(), and the library a source only through build._sources()."""
    from cudadepthmapintegration_amd import build

    assert "depth_points.hip" in set(build._sources())
    assert {"depth_points.h", "depth_points_rules.h"} <= {os.path.relpath(h, CSRC) for h in build._headers()}


def test_the_new_kernels_use_no_scratch_memory(tmp_path):
    """depth_points.hip compiled to gfx950 assembly with the build's flags: the five kernels are there and none spills."""
    import re

    from cudadepthmapintegration_amd import build

    out = str(tmp_path / "depth_points.s")
    subprocess.check_call([build.hipcc_path()] + build.COMMON_FLAGS + build.HIP_FLAGS +
                          ["--cuda-device-only", "-S", os.path.join(CSRC, "depth_points.hip"), "-o", out])
    sizes = {m.group(1): int(m.group(2)) for m in re.finditer(
        r"\.amdhsa_kernel (\S+)\b.*?\.amdhsa_private_segment_fixed_size (\d+)", open(out).read(), re.S)}
    for kernel in ("points_flags_kernel", "points_block_counts_kernel", "points_scan_kernel", "points_scatter_kernel",
                   "points_sum_normals_kernel"):
        assert [v for k, v in sizes.items() if kernel in k] == [0], (kernel, sizes)
