"""The per-view records of the fusion kernels (csrc/view_records.h: make_view_records), pinned on the CPU to recorded bytes by a
stand-alone program (tests/cpp/view_records_host.cpp) built with g++, AddressSanitizer + UBSan and run; nothing is loaded into
Python.

tests/golden/view_records.bin holds fifteen cases, 1200 bytes each behind a 16-byte head: name, ViewFrame (grid, z_first, W, H),
rt, k, then the TileMapRec, WinRec and FootRec bytes, k_mode, finite and tile_ok.  The expected bytes were recorded from commit
1aed04c -- the last one whose dmi_capi.hip formed the records itself (make_tile_rec, make_centred_rows and the tail of
add_views_impl, on a default-constructed dmi_context) -- by a host-only harness compiled with
`hipcc --cuda-host-only -x hip -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math`, not from the header under test.  hipcc's
clang recorded them and g++ -O1 replays them, so the test also pins that the arithmetic has no compiler-dependent step.

The cases (cell_dims (33, 17, 40), origin (-1, -0.5, -1.25), spacing 1/16, identity grid matrix, z_first 0, 320 x 240,
rt = [1 0 0 .1; 0 1 0 -.2; 0 0 1 4], K = [300 0 160 0; 0 300 120 0; 0 0 1 0] unless said otherwise) and what each reaches:
outside (K_PINHOLE, t1_ok 1, windows), skew (K[1] = 0.5: K_PINHOLE_SKEW), generalK (a general third row and fourth column:
K_GENERAL, errz > 0, e_abs = inf), rotated (a rotated grid matrix: cz_err > 0), inside (rt[11] = 0.3: t1_ok 2, t1_b > 0),
rot_inside, behind (c.z < 0: t1_ok 2), geo (translations of 5e6 that cancel: corner-based zabs), far_offset (offsets of 1e9 and
f = 1e5: tile_ok 0), big_image (4096 x 4096: the fp32 index is not exact, t1_ok 0), zslab (z_first 32), one_pixel (1 x 1),
odd_image (641 x 479, a rotated camera), huge_k (K[0] = 1e61: not finite), nan_rt (rt[11] = NaN: compared by its decisions only,
a propagated NaN's payload being the compiler's choice).  The program fails if the set stops reaching t1_ok 0, 1 and 2, a finite
and an infinite e_abs, tile_ok 0 and 1, all three KModes, or an aligned and a rotated grid.  Without the fixture it checks
view_path over the product of its inputs against a written-out table, and grid_axis_aligned for each off-diagonal entry."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudadepthmapintegration_amd", "csrc")


def test_view_records_match_the_recorded_bytes(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "view_records_host")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "view_records_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "view_records.bin")], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failed"), (r.stdout[-3000:], r.stderr[-3000:])


def test_the_build_knows_the_header_and_the_views_file():
    """The source digest sees a header only through build._headers(); the library gets a file only through build._sources()."""
    from cudadepthmapintegration_amd import build

    assert "dmi_capi_views.hip" in build._sources()
    assert "view_records.h" in {os.path.relpath(h, CSRC) for h in build._headers()}
