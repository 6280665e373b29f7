"""The window-pair table's index (csrc/fusion_launch_rules.h: win_pair_index), checked on the CPU by a stand-alone program
(tests/cpp/winpair_index_host.cpp) built with AddressSanitizer + UBSan and run; nothing is loaded into Python.

Over brick counts 1, 63, 64, 135 and 4097 and pitches 64 and 128 the index is a bijection onto [0, bricks * pitch), a brick's 32
views of a block are consecutive entries, and block b of brick k starts at (b * bricks + k) * 32 -- what window_origin_kernel
(a run of 64 bricks x 512 bytes per workgroup) and fuse_tile_kernel (512 bytes per brick and block) rely on."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudadepthmapintegration_amd", "csrc")


def test_win_pair_index_is_a_block_major_bijection(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "winpair_index_host")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "winpair_index_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failed"), (r.stdout[-3000:], r.stderr[-3000:])
