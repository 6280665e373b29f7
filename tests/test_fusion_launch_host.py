"""What a fusion launch decides and how its buffers grow, checked on the CPU: two stand-alone programs (tests/cpp/), each built
with AddressSanitizer + UBSan and run; nothing is loaded into Python.

  fusion_launch_rules_host  csrc/fusion_launch_rules.h -- hole traits, default tile shape, classes on or off, class pitch, windows,
                            the zero-free rule and the cost order -- at every threshold's boundary; the expected values restate the
                            expressions fuse_run carried before the rules had a header of their own.  The record tables' rule
                            (capacity, bytes read, bytes allocated) at n = 1, 31, 32, 33, 63, 64, 65, 129, 130, 131, and a replay of
                            "fuse at a views, then at b >= a" for all 1 <= a <= b <= 140: what is held covers what is read -- the
                            WinRec beyond the last view, which the window column prefetches, included.
  buffer_growth_host        csrc/dmi_buffer.h against host stand-ins for hipMalloc / hipFree / hipStreamSynchronize
                            (tests/cpp/support_host/) whose allocator fails on the N-th call, for every N over a four-buffer unit
                            growth and a single one: no buffer keeps an old capacity, the byte count is the sum of the capacities,
                            the call succeeds when repeated; AddressSanitizer reports a buffer freed twice or never."""
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


def test_launch_rules_at_their_boundaries(tmp_path):
    _build_and_run(tmp_path, "fusion_launch_rules_host", [CSRC])


def test_buffer_growth_survives_a_failing_allocator(tmp_path):
    _build_and_run(tmp_path, "buffer_growth_host", [os.path.join(ROOT, "tests", "cpp", "support_host"), CSRC])


def test_the_build_knows_the_new_files():
    """The source digest and the accumulator audit see a header only through build._headers()."""
    from cudadepthmapintegration_amd import build

    assert "dmi_capi_fuse.hip" in build._sources()
    headers = {os.path.relpath(h, CSRC) for h in build._headers()}
    assert {"dmi_buffer.h", "fusion_launch_rules.h", "dmi_context.h", "fusion_kernels.h"} <= headers
