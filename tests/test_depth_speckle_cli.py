"""dmi_reconstruction --depthSpeckleMinPixels end to end: a 24^3 grid and 6 views of 48 x 36 with injected outliers,
written as .vti / .krtd files.  With N = 0 the written volumes are those of a run without the flag, byte for byte; with N = 20 the
volume is the fusion of the restatement's filtered views, bit for bit, and the summary carries the counts; together with
--depthConsistencyMinViews the speckle filter runs first; with --extractMesh a mesh is written from the filtered fusion."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import depth_consistency_np as C
import depth_speckle_np as S
from cudadepthmapintegration_amd import capi, scene

pytestmark = pytest.mark.gpu
N_VIEWS, W, H = 6, 48, 36
THRESHOLD = 0.9
REL_TOLERANCE = 0.05          # (images this small need it: at 0.01 the slanted surface falls apart)
MIN_PIXELS = 20


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


def _fused(args_used, ray, views):
    o, _ = capi.cli_read_arguments(args_used)   # the grid as the tool derives it from --gridEnd
    tool_grid = scene.GridDesc(tuple(int(d) - 1 for d in o.grid_dims), tuple(o.grid_origin), tuple(o.grid_spacing),
                               np.array(o.grid_matrix).reshape(4, 4))
    want, _, _ = capi.fuse_once(tool_grid, ray, views, count_hits=False)
    return np.ascontiguousarray(want).tobytes()


def test_cli_removes_the_speckles_before_the_fusion(tmp_path):
    grid, ray, views = _scene()
    data = tmp_path / "data"
    data.mkdir()
    lv, lk = scene.write_view_files(str(data), views, scene.make_colors(N_VIEWS, W, H, seed=2))
    speckle = ["--depthSpeckleMinPixels", str(MIN_PIXELS), "--depthSpeckleRelTolerance", repr(REL_TOLERANCE)]

    plain, plain_dir = _reconstruct(tmp_path, lv, lk, "plain", [])
    assert plain.returncode == 0, plain.stderr + plain.stdout
    zero, zero_dir = _reconstruct(tmp_path, lv, lk, "zero", ["--depthSpeckleMinPixels", "0"])
    assert zero.returncode == 0, zero.stderr + zero.stdout
    for name in ("volume.vts", "meta_image_volume.mha"):
        assert open(zero_dir / name, "rb").read() == open(plain_dir / name, "rb").read(), name

    # N = 20 against the fusion of the restatement's filtered views
    D = S.thresholded(views.depth, views.best_cost, THRESHOLD)
    want_depth, want_size = S.filter_depth_speckles(D, MIN_PIXELS, 0.0, REL_TOLERANCE)
    valid, kept = int(S.valid_pixels(D).sum()), int((want_depth > 0).sum())
    assert 0 < kept < valid
    roots = [np.unique(S.segment_labels(D[m], 0.0, REL_TOLERANCE)) for m in range(N_VIEWS)]
    segments = sum(int((r >= 0).sum()) for r in roots)
    kept_segments = sum(int((want_size[m].reshape(-1)[r[r >= 0]] >= MIN_PIXELS).sum()) for m, r in enumerate(roots))
    assert 0 < kept_segments < segments
    twenty, twenty_dir = _reconstruct(tmp_path, lv, lk, "twenty", speckle + ["--summary", "--verbose"])
    assert twenty.returncode == 0, twenty.stderr + twenty.stdout
    cells = _vts_cells(str(twenty_dir / "volume.vts"))
    assert cells.tobytes() == _fused(twenty.args_used, ray, scene.Views(want_depth, views.K4, views.RT4))
    assert cells.tobytes() != _vts_cells(str(plain_dir / "volume.vts")).tobytes()
    summary = open(data / "summary.txt").read()
    assert "depth speckles\n" in summary and f"minimum segment pixels  {MIN_PIXELS}\n" in summary and f"views  {N_VIEWS}\n" in summary
    assert f"pixels with a depth  {valid}\n" in summary and f"pixels kept  {kept}\n" in summary and "GPU kernels  " in summary
    assert f"segments  {segments}\n" in summary and f"segments kept  {kept_segments}\n" in summary
    assert "depth consistency" not in summary
    line = [x for x in twenty.stdout.splitlines() if x.startswith("depth speckles:")]
    assert len(line) == 1 and f"{valid} pixels with a depth, {kept} kept" in line[0] and "ms of GPU kernels" in line[0], twenty.stdout
    assert f"{segments} segments, {kept_segments} kept" in line[0]

    # with the consistency filter: speckles first, then the consistency of what is left
    both, both_dir = _reconstruct(tmp_path, lv, lk, "both", speckle + ["--depthConsistencyMinViews", "2", "--depthConsistencyRelTolerance",
                                                                        "0.01", "--summary"])
    assert both.returncode == 0, both.stderr + both.stdout
    then_consistent, _ = C.filter_depth_consistency(want_depth, views.K4, views.RT4, 2, 0.0, 0.01)
    other_order, _ = S.filter_depth_speckles(C.filter_depth_consistency(D, views.K4, views.RT4, 2, 0.0, 0.01)[0], MIN_PIXELS, 0.0, REL_TOLERANCE)
    assert then_consistent.tobytes() != other_order.tobytes()          # (the scene tells the two orders apart)
    both_cells = _vts_cells(str(both_dir / "volume.vts"))
    assert both_cells.tobytes() == _fused(both.args_used, ray, scene.Views(then_consistent, views.K4, views.RT4))
    summary = open(data / "summary.txt").read()
    assert summary.index("depth speckles\n") < summary.index("depth consistency\n")
    assert f"pixels with a depth  {kept}\n" in summary.split("depth consistency\n")[1]      # the consistency filter saw the kept ones
    assert f"pixels kept  {int((then_consistent > 0).sum())}\n" in summary.split("depth consistency\n")[1]

    mesh, mesh_dir = _reconstruct(tmp_path, lv, lk, "mesh", speckle + ["--contour", "0.0", "--extractMesh", "--meshColoration"])
    assert mesh.returncode == 0, mesh.stderr + mesh.stdout
    colored = capi.read_polydata(str(mesh_dir / "mesh.vtp"))
    assert list(colored.point_data) == ["MeanColoration", "MedianColoration", "NbProjectedDepthMap"]
    assert len(colored.points) > 0 and np.asarray(colored.point_data["NbProjectedDepthMap"]).max() > 0
    assert _vts_cells(str(mesh_dir / "volume.vts")).tobytes() == cells.tobytes()

    refused, _ = _reconstruct(tmp_path, lv, lk, "refused", ["--depthSpeckleTolerance", "0.1"])
    assert refused.returncode != 0 and "--depthSpeckleTolerance needs --depthSpeckleMinPixels" in refused.stderr
