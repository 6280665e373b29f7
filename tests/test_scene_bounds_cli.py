"""dmi_reconstruction --gridAutoBounds.  On the CPU: what ReadArguments accepts and refuses, and that the explicit
path's parsed options are what they were.  On the GPU, end to end on 6 views of 48 x 36 with planted outliers, written as .vti /
.krtd files: the run with --gridAutoBounds equals the run with the --gridOrigin / --gridEnd it printed, byte for byte in the .vts and
the .vtp; the box is capi.estimate_scene_bounds plus the margin, recomputed here; with --depthConsistencyMinViews it is the box of
the filtered depths."""
import functools
import os
import subprocess

import numpy as np
import pytest

from cudadepthmapintegration_amd import capi, scene

N_VIEWS, W, H = 6, 48, 36
THRESHOLD = 0.9
REL_TOLERANCE = 0.01
EXPLICIT = ["Reconstruction", "--gridOrigin", "-2.29", "-2.24", "-2.2", "--gridEnd", "1.19", "1.67", "1.22", "--dataFolder", "data",
            "--outputGridFilename", "out.vts", "--outputMeshFilename", "mesh.vtp", "--rayThick", "0.1", "--gridDims", "10"]
AUTO = ["Reconstruction", "--gridAutoBounds", "--dataFolder", "data", "--outputGridFilename", "out.vts", "--outputMeshFilename", "mesh.vtp",
        "--rayThick", "0.1"]


def test_auto_bounds_is_accepted_without_origin_and_end():
    o, text = capi.cli_read_arguments(AUTO + ["--gridDims", "24"])
    assert o is not None, text
    assert o.grid_auto_bounds == 1 and o.grid_auto_bounds_trim == 0.005 and o.grid_auto_bounds_margin == 0.05
    assert o.grid_auto_bounds_pixel_step == 1 and list(o.grid_dims) == [24, 24, 24]
    assert list(o.grid_origin) == [0.0] * 3 and list(o.grid_end) == [0.0] * 3 and list(o.grid_spacing) == [0.0] * 3
    o, text = capi.cli_read_arguments(AUTO + ["--gridSpacing", "0.1", "0.2", "0.3", "--gridAutoBoundsTrim", "0.5", "--gridAutoBoundsMargin",
                                              "0", "--gridAutoBoundsPixelStep", "4", "--gridVecX", "0", "2", "0", "--gridVecY", "-1", "0", "0"])
    assert o is not None, text
    assert o.grid_auto_bounds_trim == 0.5 and o.grid_auto_bounds_margin == 0.0 and o.grid_auto_bounds_pixel_step == 4
    assert list(o.grid_spacing) == [0.1, 0.2, 0.3] and list(o.grid_dims) == [0, 0, 0]
    o, text = capi.cli_read_arguments(AUTO + ["--help"])
    assert o is None and all(f in text for f in ("--gridAutoBounds", "--gridAutoBoundsTrim", "--gridAutoBoundsMargin", "--gridAutoBoundsPixelStep"))


@pytest.mark.parametrize("extra,said", [
    (["--gridDims", "24", "--gridEnd", "1", "1", "1"], "--gridOrigin and --gridEnd must not be given"),
    (["--gridDims", "24", "--gridOrigin", "0", "0", "0"], "--gridOrigin and --gridEnd must not be given"),
    ([], "one of --gridDims / --gridSpacing is required"),
    (["--gridDims", "24", "--gridAutoBoundsMargin", "-0.1"], "Bad value for --gridAutoBoundsMargin"),
    (["--gridDims", "24", "--gridAutoBoundsTrim", "0.51"], "Bad value for --gridAutoBoundsTrim"),
    (["--gridDims", "24", "--gridAutoBoundsTrim", "-0.1"], "Bad value for --gridAutoBoundsTrim"),
    (["--gridDims", "24", "--gridAutoBoundsTrim", "nan"], "Bad value for --gridAutoBoundsTrim"),
    (["--gridDims", "24", "--gridAutoBoundsPixelStep", "0"], "Bad value for --gridAutoBoundsPixelStep"),
    (["--gridDims", "24", "--gridAutoBoundsPixelStep", "1.5"], "Bad value for --gridAutoBoundsPixelStep"),
])
def test_auto_bounds_refusals(extra, said):
    o, text = capi.cli_read_arguments(AUTO + extra)
    assert o is None and said in text, text


@pytest.mark.parametrize("flag,value", [("--gridAutoBoundsTrim", "0.01"), ("--gridAutoBoundsMargin", "0.1"), ("--gridAutoBoundsPixelStep", "2")])
def test_the_sub_flags_need_auto_bounds(flag, value):
    o, text = capi.cli_read_arguments(EXPLICIT + [flag, value])
    assert o is None and f"{flag} needs --gridAutoBounds" in text, text


def test_the_explicit_path_parses_as_before():
    o, text = capi.cli_read_arguments(EXPLICIT)
    assert o is not None, text
    origin, end = [-2.29, -2.24, -2.2], [1.19, 1.67, 1.22]
    assert list(o.grid_origin) == origin and list(o.grid_end) == end and list(o.grid_dims) == [10, 10, 10]
    assert list(o.grid_spacing) == [(e - s) / 10.0 for s, e in zip(origin, end)]
    assert o.grid_auto_bounds == 0 and o.grid_auto_bounds_trim == 0.005 and o.grid_auto_bounds_margin == 0.05
    o, text = capi.cli_read_arguments(EXPLICIT[:-2] + ["--gridSpacing", "0.5", "0.25", "0.125", "--forceCubicVoxel"])
    assert o is not None, text
    assert list(o.grid_dims) == [int((e - s) / h) for s, e, h in zip(origin, end, (0.5, 0.25, 0.125))] and list(o.grid_spacing) == [0.125] * 3
    for missing in ("--gridOrigin", "--gridEnd"):
        at = EXPLICIT.index(missing)
        o, text = capi.cli_read_arguments(EXPLICIT[:at] + EXPLICIT[at + 4:])
        assert o is None and "--gridOrigin, --gridEnd and the three axes take three values each" in text


@functools.lru_cache(maxsize=None)
def _scene():
    v = scene.make_views(N_VIEWS, W, H, seed=6, with_best_cost=True)
    rng = np.random.default_rng(3)
    sel = (v.depth > 0) & (rng.random(v.depth.shape) < 0.05)
    depth = np.where(sel, v.depth * np.where(rng.random(v.depth.shape) < 0.5, 0.8, 1.25), v.depth)
    views = scene.Views(depth, v.K4, v.RT4, v.best_cost)
    for a in (views.depth, views.K4, views.RT4, views.best_cost):
        a.setflags(write=False)
    return views


def _reconstruct(tmp_path, lv, lk, name, extra):
    ray = scene.default_ray_potential(scene.default_grid(24))
    work = tmp_path / name                     # meta_image_volume.mha goes to the working directory
    work.mkdir()
    args = [capi.cli_binary(), "--dataFolder", os.path.dirname(lv), "--depthMapFile", os.path.basename(lv), "--KRTFile", os.path.basename(lk),
            "--gridDims", "24", "--rayThick", repr(ray.thickness), "--rayRho", repr(ray.rho), "--rayEta", repr(ray.eta), "--rayDelta",
            repr(ray.delta), "--threshBestCost", repr(THRESHOLD), "--outputGridFilename", str(work / "volume.vts"), "--outputMeshFilename",
            str(work / "mesh.vtp"), "--contour", "0.0", "--extractMesh", "--verbose"] + extra
    r = subprocess.run(args, cwd=str(work), capture_output=True, text=True, timeout=300)
    return r, work


def _printed_box(stdout):
    line = [x for x in stdout.splitlines() if x.startswith("grid bounds:")]
    assert len(line) == 1, stdout
    words = line[0].split()
    at, end = words.index("--gridOrigin"), words.index("--gridEnd")
    return line[0], words[at + 1:at + 4], [w.rstrip(";") for w in words[end + 1:end + 4]]


def _with_margin(lo, hi, margin):
    pad = margin * (hi - lo)
    return lo - pad, hi + pad


@pytest.mark.gpu
def test_cli_takes_the_box_from_the_depth_maps(tmp_path):
    views = _scene()
    data = tmp_path / "data"
    data.mkdir()
    lv, lk = scene.write_view_files(str(data), views)

    auto, auto_dir = _reconstruct(tmp_path, lv, lk, "auto", ["--gridAutoBounds", "--summary"])
    assert auto.returncode == 0, auto.stderr + auto.stdout
    line, origin, end = _printed_box(auto.stdout)
    lo, hi, n_points, _ = capi.estimate_scene_bounds(views, trim_fraction=0.005, threshold=THRESHOLD)
    want_origin, want_end = _with_margin(lo, hi, 0.05)
    assert np.array([float(x) for x in origin]).tobytes() == want_origin.tobytes(), (origin, want_origin)
    assert np.array([float(x) for x in end]).tobytes() == want_end.tobytes(), (end, want_end)
    assert f"; {n_points} points of {N_VIEWS} views;" in line and "ms of GPU kernels" in line
    summary = open(data / "summary.txt").read()
    assert "grid bounds from the depth maps\n" in summary and f"points  {n_points}\n" in summary and "GPU kernels  " in summary
    assert "--gridOrigin  " + " ".join(origin) + "\n" in summary and "--gridEnd  " + " ".join(end) + "\n" in summary

    explicit, explicit_dir = _reconstruct(tmp_path, lv, lk, "explicit", ["--gridOrigin"] + origin + ["--gridEnd"] + end)
    assert explicit.returncode == 0, explicit.stderr + explicit.stdout
    assert "grid bounds:" not in explicit.stdout
    for name in ("volume.vts", "mesh.vtp", "meta_image_volume.mha"):
        a, b = open(auto_dir / name, "rb").read(), open(explicit_dir / name, "rb").read()
        assert len(a) > 1000 and a == b, name
    assert len(capi.read_polydata(str(auto_dir / "mesh.vtp")).points) > 0

    # other parameters reach the call; a box of the filtered depths when a filter is asked for
    other, _ = _reconstruct(tmp_path, lv, lk, "other", ["--gridAutoBounds", "--gridAutoBoundsTrim", "0.02", "--gridAutoBoundsMargin", "0.25",
                                                       "--gridAutoBoundsPixelStep", "3"])
    assert other.returncode == 0, other.stderr + other.stdout
    _, origin3, end3 = _printed_box(other.stdout)
    lo3, hi3, _, _ = capi.estimate_scene_bounds(views, trim_fraction=0.02, pixel_step=3, threshold=THRESHOLD)
    want3 = _with_margin(lo3, hi3, 0.25)
    assert np.array([float(x) for x in origin3]).tobytes() == want3[0].tobytes() and np.array([float(x) for x in end3]).tobytes() == want3[1].tobytes()

    both, _ = _reconstruct(tmp_path, lv, lk, "both", ["--gridAutoBounds", "--depthConsistencyMinViews", "2", "--depthConsistencyRelTolerance",
                                                     repr(REL_TOLERANCE)])
    assert both.returncode == 0, both.stderr + both.stdout
    _, origin_f, end_f = _printed_box(both.stdout)
    filtered, _, _ = capi.filter_depth_consistency(views, min_views=2, rel_tolerance=REL_TOLERANCE, threshold=THRESHOLD)
    lo_f, hi_f, n_f, _ = capi.estimate_scene_bounds(filtered, trim_fraction=0.005)
    want_f = _with_margin(lo_f, hi_f, 0.05)
    assert np.array([float(x) for x in origin_f]).tobytes() == want_f[0].tobytes() and np.array([float(x) for x in end_f]).tobytes() == want_f[1].tobytes()
    assert 0 < n_f < n_points and (origin_f, end_f) != (origin, end)
    assert both.stdout.index("depth consistency:") < both.stdout.index("grid bounds:")

    refused, _ = _reconstruct(tmp_path, lv, lk, "refused", ["--gridAutoBounds", "--gridEnd", "1", "1", "1"])
    assert refused.returncode != 0 and "--gridOrigin and --gridEnd must not be given" in refused.stderr


@pytest.mark.gpu
def test_cli_refuses_depth_maps_without_a_depth(tmp_path):
    views = _scene()
    data = tmp_path / "data"
    data.mkdir()
    lv, lk = scene.write_view_files(str(data), scene.Views(np.full(views.depth.shape, -1.0), views.K4, views.RT4))
    r, _ = _reconstruct(tmp_path, lv, lk, "empty", ["--gridAutoBounds"])
    assert r.returncode != 0 and "--gridAutoBounds: no pixel of the depth maps holds a depth" in r.stderr + r.stdout
