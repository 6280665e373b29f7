"""The host-side rules of the plane fit (csrc/depth_points_planes_rules.h), checked on the CPU: a stand-alone program
(tests/cpp/depth_points_planes_rules_host.cpp) built with AddressSanitizer + UBSan and run; nothing is loaded into Python.  The
lattice at powers of two, |q| <= 2^15, the fit on degenerate matrices, the crowded rule from moments; and the fit's outputs for a
fixed list of moments, compared bit for bit with the numpy restatement: the header and numpy agree without a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import depth_points_planes_np as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudadepthmapintegration_amd", "csrc")


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("planes_rules") / "depth_points_planes_rules_host")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "cpp", "depth_points_planes_rules_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failed"), (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_depth_points_planes_rules_at_their_boundaries(program_output):
    assert "FAILED" not in program_output


def test_the_header_and_the_restatement_fit_the_same_planes_to_the_bit(program_output):
    lines = program_output.split("FITS\n")[1].strip().split("\n")[:-1]
    rows = np.array([[float.fromhex(x) for x in line.split()] for line in lines])
    assert rows.shape == (10, 21)
    m, S, T, old = rows[:, 0].astype(np.int64), rows[:, 1:4].astype(np.int64), rows[:, 4:10].astype(np.int64), rows[:, 10:13]
    assert m.max() == F.MAX_MEMBERS
    inv_s = np.float64(2.0 ** -18)
    t, n, rms = F.results_from_moments(m, S, T, inv_s, old)
    _, _, lam = F.fit_from_moments(m, S, T)
    want = np.column_stack([n, lam, t, rms.astype(np.float64), 1.25 + t * n[:, 0], -3.5 + t * n[:, 2]])
    assert np.isfinite(want).all()
    assert want.view(np.uint64).tolist() == rows[:, 13:].copy().view(np.uint64).tolist()


def test_the_build_knows_the_new_files():
    from cudadepthmapintegration_amd import build

    assert {"depth_points_planes.hip", "dmi_capi_points_planes.hip"} <= set(build._sources())
    assert {"depth_points_planes.h", "depth_points_planes_rules.h", "depth_points_search_device.h"} <= {os.path.relpath(h, CSRC) for h in build._headers()}
