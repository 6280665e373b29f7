"""The host-side rules of dmi_estimate_scene_bounds (csrc/scene_bounds_rules.h), checked on the CPU: a stand-alone
program (tests/cpp/scene_bounds_rules_host.cpp) built with AddressSanitizer + UBSan and run; nothing is loaded into Python.  The key
and its inverse at the sign boundary; k where trim * N is an exact integer, just below one, at N = 1, N = 2 and at trim 0.5; the bin
scan with the rank on a bin's first and last element and empty bins around it; a whole digit-by-digit select against std::sort."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudadepthmapintegration_amd", "csrc")


def _build_and_run(tmp_path, name, includes):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / name)
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] +
                          ["-I" + i for i in includes] + [os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failed"), (r.stdout[-3000:], r.stderr[-3000:])


def test_scene_bounds_rules_at_their_boundaries(tmp_path):
    _build_and_run(tmp_path, "scene_bounds_rules_host", [CSRC])


def test_the_build_knows_the_new_files():
    """The source digest sees a header only through build._headers(), and the library a source only through build._sources()."""
    from cudadepthmapintegration_amd import build

    assert {"scene_bounds.hip", "dmi_capi_bounds.hip"} <= set(build._sources())
    headers = {os.path.relpath(h, CSRC) for h in build._headers()}
    assert {"scene_bounds.h", "scene_bounds_rules.h", "depth_consistency.h"} <= headers


def test_the_new_kernels_use_no_scratch_memory(tmp_path):
    """scene_bounds.hip compiled to gfx950 assembly with the build's flags: the count and the select kernel are there (whatever else a tuning build adds) and neither spills."""
    import re

    from cudadepthmapintegration_amd import build

    out = str(tmp_path / "scene_bounds.s")
    subprocess.check_call([build.hipcc_path()] + build.COMMON_FLAGS + build.HIP_FLAGS +
                          ["--cuda-device-only", "-S", os.path.join(CSRC, "scene_bounds.hip"), "-o", out])
    text = open(out).read()
    sizes = {m.group(1): int(m.group(2)) for m in re.finditer(
        r"\.amdhsa_kernel (\S+)\b.*?\.amdhsa_private_segment_fixed_size (\d+)", text, re.S)}
    ours = {k: v for k, v in sizes.items() if "bounds_count_kernel" in k or "bounds_select_kernel" in k}
    assert any("bounds_count_kernel" in k for k in ours) and any("bounds_select_kernel" in k for k in ours), sizes
    assert set(ours.values()) == {0}, ours
