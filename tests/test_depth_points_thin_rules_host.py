"""The host-side rules of the voxel-grid thinning (csrc/depth_points_thin_rules.h), checked on the CPU: a stand-alone
program (tests/cpp/depth_points_thin_rules_host.cpp) built with AddressSanitizer + UBSan and run; nothing is loaded into Python.
The bin limit at its edge, the keys and their bits, the output arrays' offsets against the build's layout, the wave pass's queue
against the worst cell sizes, and a whole numbering on the host against a plain walk."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudadepthmapintegration_amd", "csrc")
KERNELS = ("thin_bounds_kernel", "thin_keys_kernel", "thin_heads_kernel", "thin_starts_kernel", "thin_kept_kernel", "thin_permute_kernel",
           "thin_lane_cells_kernel", "thin_wave_cells_kernel")


def test_depth_points_thin_rules_at_their_boundaries(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "depth_points_thin_rules_host")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "depth_points_thin_rules_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failed"), (r.stdout[-3000:], r.stderr[-3000:])


def test_the_build_knows_the_new_files():
    """The source digest sees a header only through build._headers(), and the library a source only through build._sources()."""
    from cudadepthmapintegration_amd import build

    assert {"depth_points_thin.hip", "dmi_capi_points_thin.hip"} <= set(build._sources())
    assert {"depth_points_thin.h", "depth_points_thin_rules.h"} <= {os.path.relpath(h, CSRC) for h in build._headers()}


def test_the_python_binding_follows_the_header():
    """The report's fields in the order of include/dmi.h, and the default threshold the header's text names."""
    from cudadepthmapintegration_amd import capi

    header = open(os.path.join(ROOT, "include", "dmi.h")).read()
    body = re.search(r"typedef struct dmi_points_thin_report \{(.*?)\}", header, re.S).group(1)
    names = re.findall(r"\b([a-z_]+)\s*[,;]", body)
    assert names == [name for name, _ in capi.PointsThinReportC._fields_]
    rules = open(os.path.join(CSRC, "depth_points_thin_rules.h")).read()
    default = int(re.search(r"kDefaultWaveCellPoints = (\d+);", rules).group(1))
    assert f"uses the default, {default}." in header


def test_the_new_kernels_use_no_scratch_memory_and_no_float_atomics(tmp_path):
    """depth_points_thin.hip compiled to gfx950 assembly with the build's flags: the eight kernels are there, none spills, and no
    floating point atomic stands anywhere in the file."""
    from cudadepthmapintegration_amd import build

    out = str(tmp_path / "depth_points_thin.s")
    subprocess.check_call([build.hipcc_path()] + build.COMMON_FLAGS + build.HIP_FLAGS +
                          ["--cuda-device-only", "-S", os.path.join(CSRC, "depth_points_thin.hip"), "-o", out])
    text = open(out).read()
    sizes = {m.group(1): int(m.group(2)) for m in re.finditer(
        r"\.amdhsa_kernel (\S+)\b.*?\.amdhsa_private_segment_fixed_size (\d+)", text, re.S)}
    for kernel in KERNELS:
        assert [v for k, v in sizes.items() if kernel in k] == [0], (kernel, sizes)
    assert not re.search(r"atomic_(add|min|max|pk_add)_(f|bf)\w*", text)
