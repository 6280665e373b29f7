"""dmi_reconstruction --depthFillHolesMaxPixels.  Without a GPU: the three flags, their defaults, the "needs" errors
and the help text.  On the GPU, end to end: a 24^3 grid and 6 views of 48 x 36 with injected outliers and knocked-out pixels,
written as .vti / .krtd files and run with the speckle, the fill and the consistency flags together: the summary's counts are the
restatement's, and the written volume is the fusion of the depths the three restatements give in the order speckle, fill,
consistency -- and of no other order."""
import functools
import os

import numpy as np
import pytest

import depth_consistency_np as C
import depth_holes_np as F
import depth_speckle_np as S
from test_depth_speckle_cli import _fused, _reconstruct, _vts_cells
from cudadepthmapintegration_amd import capi, scene

N_VIEWS, W, H = 6, 48, 36
THRESHOLD = 0.9
REL_TOLERANCE = 0.05          # (images this small need it, as in test_depth_speckle_cli.py)
MIN_PIXELS, MAX_PIXELS = 20, 12
MIN_VIEWS, CONSISTENCY_REL = 1, 0.05   # (what lets several hundred depths of so small a scene through the consistency filter)

BASE = ["prog", "--gridOrigin", "-2.29", "-2.24", "-2.2", "--gridEnd", "1.19", "1.67", "1.22", "--dataFolder", "data",
        "--outputGridFilename", "out.vts", "--outputMeshFilename", "mesh.vtp", "--rayThick", "0.1", "--gridDims", "10"]


def test_cli_reads_the_three_flags():
    o, text = capi.cli_read_arguments(BASE)
    assert o is not None and o.depth_fill_holes_max_pixels == -1, text
    assert (o.depth_fill_holes_tolerance, o.depth_fill_holes_rel_tolerance) == (0.0, 0.01)
    o, text = capi.cli_read_arguments(BASE + ["--depthFillHolesMaxPixels", "16"])
    assert o is not None and o.depth_fill_holes_max_pixels == 16 and o.depth_speckle_min_pixels == -1, text
    assert (o.depth_fill_holes_tolerance, o.depth_fill_holes_rel_tolerance) == (0.0, 0.01)
    o, text = capi.cli_read_arguments(BASE + ["--depthFillHolesMaxPixels", "0", "--depthFillHolesTolerance", "0.25",
                                              "--depthFillHolesRelTolerance", "0", "--depthSpeckleMinPixels", "5",
                                              "--depthConsistencyMinViews", "2"])
    assert o is not None and o.depth_fill_holes_max_pixels == 0 and o.depth_speckle_min_pixels == 5, text
    assert o.depth_consistency_min_views == 2 and (o.depth_fill_holes_tolerance, o.depth_fill_holes_rel_tolerance) == (0.25, 0.0)
    assert (o.depth_speckle_tolerance, o.depth_speckle_rel_tolerance) == (0.0, 0.01)         # the neighbours' fields stay where they were


def test_cli_refuses_dependent_and_out_of_range_forms():
    for flag in ("--depthFillHolesTolerance", "--depthFillHolesRelTolerance"):
        o, text = capi.cli_read_arguments(BASE + [flag, "0.1"])
        assert o is None and text.startswith(f"Error : {flag} needs --depthFillHolesMaxPixels"), text
        o, text = capi.cli_read_arguments(BASE + ["--depthSpeckleMinPixels", "3", flag, "0.1"])      # the other filter's flag does not do
        assert o is None and text.startswith(f"Error : {flag} needs --depthFillHolesMaxPixels"), text
        for value in ("-1", "nan", "inf", "-inf", "x", ""):
            o, text = capi.cli_read_arguments(BASE + ["--depthFillHolesMaxPixels", "1", flag, value])
            assert o is None and text.startswith(f"Bad value for {flag}"), (value, text)
    for value in ("-1", "1.5", "x", ""):
        o, text = capi.cli_read_arguments(BASE + ["--depthFillHolesMaxPixels", value])
        assert o is None and text.startswith("Bad value for --depthFillHolesMaxPixels"), (value, text)


def test_help_shows_the_three_flags():
    o, text = capi.cli_read_arguments(BASE + ["--help"])
    assert o is None
    for flag in ("--depthFillHolesMaxPixels v", "--depthFillHolesTolerance v", "--depthFillHolesRelTolerance v"):
        assert flag in text and "not in the reference" in text.split(flag)[1].split("--help")[0], flag
    first = text.split("--depthFillHolesMaxPixels v")[1].split("--depthFillHolesTolerance v")[0]
    assert "--depthSpeckleMinPixels" in first and "--depthConsistencyMinViews" in first      # the order is part of the help


@functools.lru_cache(maxsize=None)
def _scene():
    grid = scene.default_grid(24)
    ray = scene.default_ray_potential(grid)
    v = scene.make_views(N_VIEWS, W, H, seed=6, with_best_cost=True)
    rng = np.random.default_rng(3)
    sel = (v.depth > 0) & (rng.random(v.depth.shape) < 0.05)
    depth = np.where(sel, v.depth * np.where(rng.random(v.depth.shape) < 0.5, 0.8, 1.25), v.depth)
    depth[rng.random(depth.shape) < 0.04] = -1.0            # scattered single-pixel holes
    depth[:, 10:13, 20:23] = -1.0                           # a hole of 9
    depth[:, 20:25, 30:35] = -1.0                           # one of 25: too large
    views = scene.Views(depth, v.K4, v.RT4, v.best_cost)
    for a in (views.depth, views.K4, views.RT4, views.best_cost):
        a.setflags(write=False)
    return grid, ray, views


@pytest.mark.gpu
def test_cli_fills_between_the_speckle_and_the_consistency_filter(tmp_path):
    grid, ray, views = _scene()
    data = tmp_path / "data"
    data.mkdir()
    lv, lk = scene.write_view_files(str(data), views, scene.make_colors(N_VIEWS, W, H, seed=2))
    speckle = ["--depthSpeckleMinPixels", str(MIN_PIXELS), "--depthSpeckleRelTolerance", repr(REL_TOLERANCE)]
    fill = ["--depthFillHolesMaxPixels", str(MAX_PIXELS), "--depthFillHolesRelTolerance", repr(REL_TOLERANCE)]
    consistency = ["--depthConsistencyMinViews", str(MIN_VIEWS), "--depthConsistencyRelTolerance", repr(CONSISTENCY_REL)]

    # the three restatements in the tool's order, and in the two orders that move the fill
    D = S.thresholded(views.depth, views.best_cost, THRESHOLD)
    speckled, _ = S.filter_depth_speckles(D, MIN_PIXELS, 0.0, REL_TOLERANCE)
    filled, sizes = F.fill_depth_holes(speckled, MAX_PIXELS, 0.0, REL_TOLERANCE)
    holes, filled_holes, filled_pixels = F.hole_counts(speckled, filled, sizes)
    assert 0 < filled_holes < holes and filled_pixels > filled_holes
    assert filled_pixels == int((~S.valid_pixels(speckled) & (filled != -1.0)).sum())
    want, _ = C.filter_depth_consistency(filled, views.K4, views.RT4, MIN_VIEWS, 0.0, CONSISTENCY_REL)
    fill_first = C.filter_depth_consistency(S.filter_depth_speckles(F.fill_depth_holes(D, MAX_PIXELS, 0.0, REL_TOLERANCE)[0], MIN_PIXELS, 0.0,
                                                                    REL_TOLERANCE)[0], views.K4, views.RT4, MIN_VIEWS, 0.0, CONSISTENCY_REL)[0]
    fill_last = F.fill_depth_holes(C.filter_depth_consistency(speckled, views.K4, views.RT4, MIN_VIEWS, 0.0, CONSISTENCY_REL)[0], MAX_PIXELS, 0.0, REL_TOLERANCE)[0]
    assert want.tobytes() != fill_first.tobytes() and want.tobytes() != fill_last.tobytes()      # (the scene tells the orders apart)

    run, run_dir = _reconstruct(tmp_path, lv, lk, "all", speckle + fill + consistency + ["--summary", "--verbose"])
    assert run.returncode == 0, run.stderr + run.stdout
    cells = _vts_cells(str(run_dir / "volume.vts"))
    assert cells.tobytes() == _fused(run.args_used, ray, scene.Views(want, views.K4, views.RT4))
    for other in (fill_first, fill_last):
        assert cells.tobytes() != _fused(run.args_used, ray, scene.Views(other, views.K4, views.RT4))
    summary = open(data / "summary.txt").read()
    assert summary.index("depth speckles\n") < summary.index("depth holes\n") < summary.index("depth consistency\n")
    block = summary.split("depth holes\n")[1].split("depth consistency\n")[0]
    assert f"maximum hole pixels  {MAX_PIXELS}\n" in block and f"views  {N_VIEWS}\n" in block and "GPU kernels  " in block
    assert f"holes  {holes}\n" in block and f"holes filled  {filled_holes}\n" in block and f"pixels filled  {filled_pixels}\n" in block
    assert f"pixels with a depth  {int((filled > 0).sum())}\n" in summary.split("depth consistency\n")[1]    # the consistency filter saw the filled ones
    line = [x for x in run.stdout.splitlines() if x.startswith("depth holes:")]
    assert len(line) == 1 and f"{holes} holes, {filled_holes} filled; {filled_pixels} pixels filled" in line[0], run.stdout
    assert "ms of GPU kernels" in line[0]

    # the fill alone, against the restatement handed to the fusion directly; N = 0 changes nothing
    alone, alone_dir = _reconstruct(tmp_path, lv, lk, "alone", fill)
    assert alone.returncode == 0, alone.stderr + alone.stdout
    only_filled, _ = F.fill_depth_holes(D, MAX_PIXELS, 0.0, REL_TOLERANCE)
    assert _vts_cells(str(alone_dir / "volume.vts")).tobytes() == _fused(alone.args_used, ray, scene.Views(only_filled, views.K4, views.RT4))
    plain, plain_dir = _reconstruct(tmp_path, lv, lk, "plain", [])
    zero, zero_dir = _reconstruct(tmp_path, lv, lk, "zero", ["--depthFillHolesMaxPixels", "0"])
    assert plain.returncode == 0 and zero.returncode == 0, zero.stderr + zero.stdout
    for name in ("volume.vts", "meta_image_volume.mha"):
        assert open(zero_dir / name, "rb").read() == open(plain_dir / name, "rb").read(), name
    assert _vts_cells(str(alone_dir / "volume.vts")).tobytes() != _vts_cells(str(plain_dir / "volume.vts")).tobytes()

    refused, _ = _reconstruct(tmp_path, lv, lk, "refused", ["--depthFillHolesTolerance", "0.1"])
    assert refused.returncode != 0 and "--depthFillHolesTolerance needs --depthFillHolesMaxPixels" in refused.stderr
