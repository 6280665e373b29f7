"""The buffers of the loads that bring a brick's window pairs into LDS (csrc/fusion_launch_rules.h: win_pair_fill,
win_pair_piece_stride; used by fuse_tile_kernel), checked on the CPU by a stand-alone program (tests/cpp/winpair_fill_host.cpp)
built with AddressSanitizer + UBSan and run; nothing is loaded into Python.

With the hardware's range check modelled (a lane whose 16 bytes end beyond the buffer's range gets zeros): over 1, 63 and 135
bricks and pitches 64 .. 512, for every brick and every group of 256 views up to two groups beyond the table, no lane reads a
byte outside the table, view v's entry lands at (v & 255) * 16 of the area for every view below the pitch, and zeros beyond it;
at the largest table that gets windows (2^22 - 1 bricks) the offsets still fit 32 bits and the range saturates."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudadepthmapintegration_amd", "csrc")


def test_win_pair_fill_reads_the_right_entries_and_nothing_outside_the_table(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "winpair_fill_host")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "winpair_fill_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failed"), (r.stdout[-3000:], r.stderr[-3000:])
