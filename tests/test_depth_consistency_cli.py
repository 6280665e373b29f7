"""dmi_reconstruction --depthConsistencyMinViews end to end: a 24^3 grid and 6 views of 48 x 36 with injected outliers,
written as .vti / .krtd files.  With N = 0 the written volumes are those of a run without the flag, byte for byte; with N = 2 the
volume is the fusion of filter_depth_consistency's output, bit for bit, and the summary carries the counts; with --extractMesh
--meshColoration the Color planes still reach the colour sink."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import depth_consistency_np as C
from cudadepthmapintegration_amd import capi, scene

pytestmark = pytest.mark.gpu
N_VIEWS, W, H = 6, 48, 36
THRESHOLD = 0.9
REL_TOLERANCE = 0.01


@functools.lru_cache(maxsize=None)
def _scene():
    grid = scene.default_grid(24)
    ray = scene.default_ray_potential(grid)
    v = scene.make_views(N_VIEWS, W, H, seed=6, with_best_cost=True)
    rng = np.random.default_rng(3)
    sel = (v.depth > 0) & (rng.random(v.depth.shape) < 0.05)
    depth = np.where(sel, v.depth * np.where(rng.random(v.depth.shape) < 0.5, 0.8, 1.25), v.depth)
    views = scene.Views(depth, v.K4, v.RT4, v.best_cost)
    for a in (views.depth, views.K4, views.RT4, views.best_cost):
        a.setflags(write=False)
    return grid, ray, views


def _reconstruct(tmp_path, lv, lk, name, extra):
    grid, ray, _ = _scene()
    end = [grid.origin[a] + (grid.cell_dims[a] + 1) * grid.spacing[a] for a in range(3)]
    work = tmp_path / name                     # meta_image_volume.mha goes to the working directory
    work.mkdir()
    args = [capi.cli_binary(), "--dataFolder", os.path.dirname(lv), "--depthMapFile", os.path.basename(lv), "--KRTFile", os.path.basename(lk),
            "--gridDims"] + [str(c + 1) for c in grid.cell_dims] + ["--gridOrigin"] + [repr(float(x)) for x in grid.origin] + \
           ["--gridEnd"] + [repr(float(x)) for x in end] + \
           ["--rayThick", repr(ray.thickness), "--rayRho", repr(ray.rho), "--rayEta", repr(ray.eta), "--rayDelta", repr(ray.delta),
            "--threshBestCost", repr(THRESHOLD), "--outputGridFilename", str(work / "volume.vts"),
            "--outputMeshFilename", str(work / "mesh.vtp")] + extra
    r = subprocess.run(args, cwd=str(work), capture_output=True, text=True, timeout=300)
    r.args_used = args
    return r, work


def _vts_cells(path):
    raw = open(path, "rb").read()
    head, _, tail = raw.partition(b'<AppendedData encoding="raw">\n   _')
    ext = [int(v) for v in head.decode().split('WholeExtent="')[1].split('"')[0].split()]
    n_cells = ext[1] * ext[3] * ext[5]
    (nb,) = struct.unpack_from("<Q", tail, 0)
    assert nb == 8 * n_cells
    return np.frombuffer(tail, dtype=np.float64, count=n_cells, offset=8)


def test_cli_filters_the_depth_maps_before_the_fusion(tmp_path):
    grid, ray, views = _scene()
    data = tmp_path / "data"
    data.mkdir()
    lv, lk = scene.write_view_files(str(data), views, scene.make_colors(N_VIEWS, W, H, seed=2))

    plain, plain_dir = _reconstruct(tmp_path, lv, lk, "plain", [])
    assert plain.returncode == 0, plain.stderr + plain.stdout
    zero, zero_dir = _reconstruct(tmp_path, lv, lk, "zero", ["--depthConsistencyMinViews", "0"])
    assert zero.returncode == 0, zero.stderr + zero.stdout
    for name in ("volume.vts", "meta_image_volume.mha"):
        assert open(zero_dir / name, "rb").read() == open(plain_dir / name, "rb").read(), name

    two, two_dir = _reconstruct(tmp_path, lv, lk, "two", ["--depthConsistencyMinViews", "2", "--depthConsistencyRelTolerance",
                                                          repr(REL_TOLERANCE), "--summary", "--verbose"])
    assert two.returncode == 0, two.stderr + two.stdout
    filtered, counts, _ = capi.filter_depth_consistency(views, min_views=2, rel_tolerance=REL_TOLERANCE, threshold=THRESHOLD)
    o, _ = capi.cli_read_arguments(two.args_used)   # the grid as the tool derives it from --gridEnd
    tool_grid = scene.GridDesc(tuple(int(d) - 1 for d in o.grid_dims), tuple(o.grid_origin), tuple(o.grid_spacing),
                               np.array(o.grid_matrix).reshape(4, 4))
    want, _, _ = capi.fuse_once(tool_grid, ray, filtered, count_hits=False)
    cells = _vts_cells(str(two_dir / "volume.vts"))
    assert cells.tobytes() == np.ascontiguousarray(want).tobytes()
    assert cells.tobytes() != _vts_cells(str(plain_dir / "volume.vts")).tobytes()
    valid = int(C.valid_pixels(C.thresholded(views.depth, views.best_cost, THRESHOLD)).sum())
    kept = int((filtered.depth > 0).sum())
    assert 0 < kept < valid
    summary = open(data / "summary.txt").read()
    assert "depth consistency\n" in summary and f"minimum agreeing views  2\n" in summary and f"views  {N_VIEWS}\n" in summary
    assert f"pixels with a depth  {valid}\n" in summary and f"pixels kept  {kept}\n" in summary and "GPU kernels  " in summary
    line = [x for x in two.stdout.splitlines() if x.startswith("depth consistency:")]
    assert len(line) == 1 and f"{valid} pixels with a depth, {kept} kept" in line[0] and "ms of GPU kernels" in line[0], two.stdout

    mesh, mesh_dir = _reconstruct(tmp_path, lv, lk, "mesh", ["--depthConsistencyMinViews", "2", "--depthConsistencyRelTolerance",
                                                            repr(REL_TOLERANCE), "--contour", "0.0", "--extractMesh", "--meshColoration"])
    assert mesh.returncode == 0, mesh.stderr + mesh.stdout
    colored = capi.read_polydata(str(mesh_dir / "mesh.vtp"))
    assert list(colored.point_data) == ["MeanColoration", "MedianColoration", "NbProjectedDepthMap"]
    assert len(colored.points) > 0 and np.asarray(colored.point_data["NbProjectedDepthMap"]).max() > 0
    assert _vts_cells(str(mesh_dir / "volume.vts")).tobytes() == cells.tobytes()

    refused, _ = _reconstruct(tmp_path, lv, lk, "refused", ["--depthConsistencyTolerance", "0.1"])
    assert refused.returncode != 0 and "--depthConsistencyTolerance needs --depthConsistencyMinViews" in refused.stderr
