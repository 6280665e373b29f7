"""dmi_reconstruction --depthSmoothSigma.  Without a GPU: the five flags, their defaults, the "needs" errors, the
radius check at parse time and the help text.  On the GPU, end to end: a `noisy` scene of 4 views of 64 x 48 written as .vti / .krtd
files and run with the flag fuses to the .mha, byte for byte, that a run without the flag writes from capi.smooth_depths's output,
and the report's counts are out_count's."""
import numpy as np
import pytest

import depth_smooth_np as S
from test_depth_speckle_cli import THRESHOLD, _reconstruct
from cudadepthmapintegration_amd import capi, scene

N_VIEWS, W, H = 4, 64, 48
FLAGS = ("--depthSmoothSigma", "--depthSmoothTruncate", "--depthSmoothTolerance", "--depthSmoothRelTolerance", "--depthSmoothIterations")

BASE = ["prog", "--gridOrigin", "-2.29", "-2.24", "-2.2", "--gridEnd", "1.19", "1.67", "1.22", "--dataFolder", "data",
        "--outputGridFilename", "out.vts", "--outputMeshFilename", "mesh.vtp", "--rayThick", "0.1", "--gridDims", "10"]


def _fields(o):
    return (o.depth_smooth_sigma, o.depth_smooth_truncate, o.depth_smooth_tolerance, o.depth_smooth_rel_tolerance, o.depth_smooth_iterations)


def test_cli_reads_the_five_flags():
    o, text = capi.cli_read_arguments(BASE)
    assert o is not None and _fields(o) == (-1.0, 2.0, 0.0, 0.01, 1), text
    o, text = capi.cli_read_arguments(BASE + ["--depthSmoothSigma", "1.5"])
    assert o is not None and _fields(o) == (1.5, 2.0, 0.0, 0.01, 1) and o.depth_fill_holes_max_pixels == -1, text
    o, text = capi.cli_read_arguments(BASE + ["--depthSmoothSigma", "0"])          # radius 0: legal, the identity
    assert o is not None and _fields(o) == (0.0, 2.0, 0.0, 0.01, 1), text
    o, text = capi.cli_read_arguments(BASE + ["--depthSmoothSigma", "2", "--depthSmoothTruncate", "4", "--depthSmoothTolerance", "0.25",
                                              "--depthSmoothRelTolerance", "0", "--depthSmoothIterations", "16",
                                              "--depthFillHolesMaxPixels", "7", "--depthSpeckleMinPixels", "5"])
    assert o is not None and _fields(o) == (2.0, 4.0, 0.25, 0.0, 16), text
    assert o.depth_fill_holes_max_pixels == 7 and o.depth_speckle_min_pixels == 5                # the neighbours' fields stay where they were
    assert (o.depth_fill_holes_tolerance, o.depth_fill_holes_rel_tolerance) == (0.0, 0.01)


def test_cli_refuses_dependent_and_out_of_range_forms():
    for flag in FLAGS[1:]:
        o, text = capi.cli_read_arguments(BASE + [flag, "1"])
        assert o is None and text.startswith(f"Error : {flag} needs --depthSmoothSigma"), text
        o, text = capi.cli_read_arguments(BASE + ["--depthFillHolesMaxPixels", "3", flag, "1"])     # the other step's flag does not do
        assert o is None and text.startswith(f"Error : {flag} needs --depthSmoothSigma"), text
    bad = {"--depthSmoothSigma": ("-1", "nan", "inf", "x", ""), "--depthSmoothTruncate": ("0", "-1", "4.5", "nan", "inf", "x", ""),
           "--depthSmoothTolerance": ("-1", "nan", "inf", "-inf", "x", ""), "--depthSmoothRelTolerance": ("-1", "nan", "inf", "x", ""),
           "--depthSmoothIterations": ("0", "17", "-1", "1.5", "x", "")}
    for flag, values in bad.items():
        for value in values:
            args = ["--depthSmoothSigma", "1"] if flag != "--depthSmoothSigma" else []
            o, text = capi.cli_read_arguments(BASE + args + [flag, value])
            assert o is None and text.startswith(f"Bad value for {flag}"), (flag, value, text)


def test_cli_checks_the_radius_with_the_librarys_rule():
    for sigma, truncate, ok in (("4", "2", True), ("4.01", "2", False), ("2", "4", True), ("2.01", "4", False), ("8", "1", True),
                                ("9", "1", False), ("4.5", None, False), ("4", None, True)):
        args = ["--depthSmoothSigma", sigma] + ([] if truncate is None else ["--depthSmoothTruncate", truncate])
        o, text = capi.cli_read_arguments(BASE + args)
        if ok:
            assert o is not None and o.depth_smooth_sigma == float(sigma), text
            assert len(capi.depth_smoothing_weights(float(sigma), 2.0 if truncate is None else float(truncate))) == 9
        else:
            assert o is None and text.startswith("Bad value for --depthSmoothSigma: the radius ceil(truncate * sigma) must not exceed 8"), text


def test_help_shows_the_five_flags():
    o, text = capi.cli_read_arguments(BASE + ["--help"])
    assert o is None
    for flag in FLAGS:
        assert flag + " v" in text and "not in the reference" in text.split(flag + " v")[1].split("--help")[0], flag
    first = text.split("--depthSmoothSigma v")[1].split("--depthSmoothTruncate v")[0]
    assert "--depthFillHolesMaxPixels" in first and "--depthConsistencyMinViews" in first      # the order is part of the help
    assert text.index("--depthFillHolesRelTolerance v") < text.index("--depthSmoothSigma v") < text.index("\n  --gridAutoBounds\n")


@pytest.mark.gpu
def test_cli_smooths_before_the_fusion(tmp_path):
    spacing = float(scene.default_grid(24).spacing[0])
    views, threshold = scene.make_scene_views("noisy", N_VIEWS, W, H, seed=2, holes=2, noise_sigma=spacing)
    assert threshold == THRESHOLD                                # (what _reconstruct passes as --threshBestCost)
    tolerance = 3 * spacing
    data = tmp_path / "data"
    data.mkdir()
    lv, lk = scene.write_view_files(str(data), views, scene.make_colors(N_VIEWS, W, H, seed=2))
    flags = ["--depthSmoothSigma", "1", "--depthSmoothTolerance", repr(tolerance), "--depthSmoothRelTolerance", "0",
             "--depthSmoothIterations", "2"]
    run, run_dir = _reconstruct(tmp_path, lv, lk, "smoothed", flags + ["--summary", "--verbose"])
    assert run.returncode == 0, run.stderr + run.stdout

    smoothed, counts, _ = capi.smooth_depths(views, sigma=1.0, abs_tolerance=tolerance, rel_tolerance=0.0, iterations=2, threshold=threshold)
    D = S.thresholded(views.depth, views.best_cost, threshold)
    valid = S.valid_pixels(D)
    assert np.array_equal(smoothed.depth != -1.0, valid)
    changed = int((smoothed.depth[valid] != D[valid]).sum())
    assert 0.5 * valid.sum() < changed <= valid.sum()
    handed = tmp_path / "handed"
    handed.mkdir()
    lv2, lk2 = scene.write_view_files(str(handed), scene.Views(smoothed.depth, views.K4, views.RT4, views.best_cost),
                                      scene.make_colors(N_VIEWS, W, H, seed=2))
    want, want_dir = _reconstruct(tmp_path, lv2, lk2, "handed_run", [])
    plain, plain_dir = _reconstruct(tmp_path, lv, lk, "plain", [])
    assert want.returncode == 0 and plain.returncode == 0, want.stderr + plain.stderr
    mha = lambda d: open(d / "meta_image_volume.mha", "rb").read()
    assert mha(run_dir) == mha(want_dir) and mha(run_dir) != mha(plain_dir)

    line = [x for x in run.stdout.splitlines() if x.startswith("depth smoothing:")]
    assert len(line) == 1 and "ms of GPU kernels" in line[0], run.stdout
    assert f"{N_VIEWS} views, {int(valid.sum())} pixels with a depth, {changed} changed; " in line[0], line[0]
    taps = float(line[0].split("changed; ")[1].split(" taps per pixel")[0])
    assert taps == pytest.approx(counts.sum() / valid.sum(), rel=1e-5) and int((counts > 0).sum()) == int(valid.sum())
    summary = open(data / "summary.txt").read()
    block = summary.split("depth smoothing\n")[1]
    assert "sigma  1 pixels\n" in block and "iterations  2\n" in block and f"views  {N_VIEWS}\n" in block
    assert f"pixels with a depth  {int(valid.sum())}\n" in block and f"pixels changed  {changed}\n" in block and "GPU kernels  " in block

    refused, _ = _reconstruct(tmp_path, lv, lk, "refused", ["--depthSmoothTolerance", "0.1"])
    assert refused.returncode != 0 and "--depthSmoothTolerance needs --depthSmoothSigma" in refused.stderr
