"""The kernels of csrc/isosurface_support.hip, compiled as plain C++ against host stand-ins for the HIP names they use
(tests/cpp/support_host/) into a stand-alone program and run under AddressSanitizer + UBSan on the CPU: counts, trimmed mesh and
compacted counts against isosurface_support_np, bit for bit, and no access past a buffer -- every buffer of the program has its exact
size.  This covers indexing, the view groups with their atomic adds and the compaction; the device's own arithmetic, its scalar loads
and the visibility between workgroups are the GPU tests' (test_isosurface_support.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import isosurface_normals_np as N
import isosurface_support_np as S
import test_isosurface_support as T
from oracle import oracle_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = tmp_path_factory.mktemp("support_host") / "support_host_harness"
    csrc = os.path.join(ROOT, "cudadepthmapintegration_amd", "csrc")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-Wno-attributes", "-I" + os.path.join(ROOT, "tests", "cpp", "support_host"), "-I" + csrc, "-x", "c++",
           os.path.join(ROOT, "tests", "cpp", "support_host_harness.cpp"), "-o", str(out)]
    subprocess.check_call(cmd)
    return str(out)


def _run(harness, d, v, t, n, views, depths, f64, facing, min_views, tol):
    os.makedirs(d, exist_ok=True)
    n_views, H, W = depths.shape
    for name, a, dt in (("vertices", v, np.float64), ("triangles", t, np.int64), ("normals", n, np.float32), ("K4", views.K4, np.float64),
                        ("RT4", views.RT4, np.float64), ("depth_top_row_first", depths[:, ::-1, :], np.float64)):
        np.ascontiguousarray(a, dtype=dt).tofile(os.path.join(d, name + ".bin"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([harness, d, str(n_views), str(W), str(H), str(int(f64)), str(int(facing)), str(min_views), repr(float(tol))],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    stored = depths if f64 else depths.astype(np.float32).astype(np.float64)
    want = S.support(v, n, stored, views.K4, views.RT4, tol, facing)
    got = np.fromfile(os.path.join(d, "support.out"), np.int32)
    assert np.array_equal(got, want), int((got != want).sum())
    if min_views > 0:
        wv, wt, wn = S.filter_mesh(v, t, n, want, min_views)
        kept = np.zeros(len(v), dtype=bool)
        kept[t[(want[t] >= min_views).all(axis=1)].reshape(-1)] = True
        assert r.stdout.strip() == f"kept {len(wv)} {len(wt)}", r.stdout
        assert np.fromfile(os.path.join(d, "vertices.out"), np.float64).tobytes() == wv.tobytes()
        assert np.fromfile(os.path.join(d, "normals.out"), np.float32).tobytes() == wn.tobytes()
        assert np.array_equal(np.fromfile(os.path.join(d, "triangles.out"), np.int64).reshape(-1, 3), wt)
        assert np.array_equal(np.fromfile(os.path.join(d, "support_compacted.out"), np.int32), want[kept])
    return want


@pytest.mark.parametrize("iso", [0.0, 1.0])
def test_kernels_on_the_host_are_the_restatement(harness, tmp_path, iso):
    _, _, views, thresholded = T._scene()
    v, t, n = T._cpu_mesh(iso)
    for facing in (True, False):
        for f64 in (False, True):
            for min_views in (0, 1, 2, 7):
                want = _run(harness, str(tmp_path / f"{int(facing)}{int(f64)}{min_views}"), v, t, n, views, thresholded, f64, facing,
                            min_views, T.TOLERANCE)
    assert (want > 0).any() and (want == 0).any()


def test_kernels_on_the_host_with_seventy_views(harness, tmp_path):
    """Nine view groups over gridDim.y, the partial counts added atomically; then the filter reads those counts."""
    grid, ray, views, thresholded = T._many_views_scene()
    cells, _, _ = oracle_np.fuse(grid.cell_dims, grid.origin, grid.spacing, grid.grid_matrix, ray.thickness, ray.rho, ray.eta, ray.delta,
                                 thresholded, views.K4, views.RT4)
    v, t, n = N.extract_with_normals(oracle_np.cell_to_point_np(cells), T.MANY_ISO, grid.origin, grid.spacing, np.asarray(grid.grid_matrix))
    for facing in (True, False):
        want = _run(harness, str(tmp_path / f"many{int(facing)}"), v, t, n, views, thresholded, False, facing, 1, T.TOLERANCE)
        assert want.max() > 1 and (want == 0).any()
