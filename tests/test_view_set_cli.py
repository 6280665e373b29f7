"""dmi_reconstruction on the resident view set, end to end on the GPU: view_set_cases.py's 5 views of 150 x 70 written
as .vti / .krtd files (vti_writer.py, raw appended f64) and run with all five depth-map options -- speckle filter, hole fill,
smoothing, consistency filter, --gridAutoBounds -- once as it is, on the resident set, and once with --depthStagedFilters: the
.vts, the .mha and the .vtp are the same bytes, the progress lines and summary.txt are the same apart from their times, and with
--meshColoration the coloured mesh is the same too."""
import os
import re
import subprocess

import numpy as np
import pytest

from view_set_cases import BOUNDS, CONSISTENCY, H, HOLES, N, SMOOTH, SPECKLES, W, view_set_scene
from vti_writer import write_vti
from cudadepthmapintegration_amd import capi, scene

pytestmark = pytest.mark.gpu

FIVE = ["--depthSpeckleMinPixels", str(SPECKLES["min_pixels"]), "--depthSpeckleTolerance", repr(SPECKLES["abs_tolerance"]),
        "--depthSpeckleRelTolerance", repr(SPECKLES["rel_tolerance"]),
        "--depthFillHolesMaxPixels", str(HOLES["max_pixels"]), "--depthFillHolesTolerance", repr(HOLES["abs_tolerance"]),
        "--depthFillHolesRelTolerance", repr(HOLES["rel_tolerance"]),
        "--depthSmoothSigma", repr(SMOOTH["sigma"]), "--depthSmoothTruncate", repr(SMOOTH["truncate"]),
        "--depthSmoothTolerance", repr(SMOOTH["abs_tolerance"]), "--depthSmoothRelTolerance", repr(SMOOTH["rel_tolerance"]),
        "--depthSmoothIterations", str(SMOOTH["iterations"]),
        "--depthConsistencyMinViews", str(CONSISTENCY["min_views"]), "--depthConsistencyTolerance", repr(CONSISTENCY["abs_tolerance"]),
        "--depthConsistencyRelTolerance", repr(CONSISTENCY["rel_tolerance"]),
        "--gridAutoBounds", "--gridAutoBoundsTrim", repr(BOUNDS["trim_fraction"])]
TIME = re.compile(r"[-+0-9.eE]+ (ms|s)\b")   # "3.2 ms of GPU kernels", "GPU kernels  3.2 ms", "execution time : 0.2 s", "total  0.3 s"


def _write_views(folder):
    views, threshold = view_set_scene()
    colors = scene.make_colors(N, W, H, seed=4)
    vti, krtd = [], []
    for m in range(N):
        v, k = f"frame_{m:04d}.vti", f"frame_{m:04d}.krtd"
        write_vti(os.path.join(folder, v), {"Depths": views.depth[m], "Best Cost Values": views.best_cost[m], "Color": colors[m]}, W, H,
                  mode="appended-raw")
        scene.write_krtd(os.path.join(folder, k), views.K4[m][:3, :3], views.RT4[m])
        vti.append(v)
        krtd.append(k)
    for name, files in (("vtiList.txt", vti), ("krtdList.txt", krtd)):
        with open(os.path.join(folder, name), "w") as fh:
            fh.write("".join(f"{i} {p}\n" for i, p in enumerate(files)))
    return threshold


def _run(tmp_path, data, threshold, name, extra):
    grid = scene.default_grid(24)
    ray = scene.default_ray_potential(grid)
    work = tmp_path / name                     # meta_image_volume.mha goes to the working directory
    work.mkdir()
    args = [capi.cli_binary(), "--dataFolder", str(data), "--depthMapFile", "vtiList.txt", "--KRTFile", "krtdList.txt", "--gridDims", "25",
            "--rayThick", repr(ray.thickness), "--rayRho", repr(ray.rho), "--rayEta", repr(ray.eta), "--rayDelta", repr(ray.delta),
            "--threshBestCost", repr(threshold), "--outputGridFilename", str(work / "volume.vts"),
            "--outputMeshFilename", str(work / "mesh.vtp"), "--contour", "0.0", "--extractMesh", "--summary", "--verbose"] + FIVE + extra
    r = subprocess.run(args, cwd=str(work), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    files = {f: open(work / f, "rb").read() for f in ("volume.vts", "meta_image_volume.mha", "mesh.vtp")}
    summary = open(data / "summary.txt").read()
    return files, r.stdout, summary


def _without_times(text, work_names):
    for name in work_names:   # (the two runs write into folders of their own, and the command line is echoed)
        text = text.replace(name, "RUN")
    return [TIME.sub(r"T \1", line) for line in text.replace(" --depthStagedFilters", "").splitlines()]


@pytest.mark.parametrize("coloured", [False, True])
def test_the_resident_set_and_the_staged_filters_write_the_same_files(tmp_path, coloured):
    data = tmp_path / "data"
    data.mkdir()
    threshold = _write_views(str(data))
    extra = ["--meshColoration"] if coloured else []
    resident = _run(tmp_path, data, threshold, "resident", extra)
    staged = _run(tmp_path, data, threshold, "staged", extra + ["--depthStagedFilters"])
    for name in resident[0]:
        assert resident[0][name] == staged[0][name], name
        assert len(resident[0][name]) > 1000, name
    if coloured:
        assert b"MeanColoration" in resident[0]["mesh.vtp"]
    names = ("resident", "staged")
    assert _without_times(resident[1], names) == _without_times(staged[1], names)
    assert _without_times(resident[2], names) == _without_times(staged[2], names)
    # every step has run and said so, on both paths; nothing fell back
    for word in ("depth speckles:", "depth holes:", "depth smoothing:", "depth consistency:", "grid bounds:"):
        assert sum(line.startswith(word) for line in resident[1].splitlines()) == 1, word
    assert "staged filters are used" not in resident[1] + staged[1]
    for head in ("depth speckles\n", "depth holes\n", "depth smoothing\n", "depth consistency\n"):
        assert head in resident[2], head
