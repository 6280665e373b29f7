"""The `Coloration` command line (Coloration/main.cxx -> csrc/host/color_cli.cpp, dmi_coloration): flags and checks through the
C binding, the binary's help and error exits (no GPU); the tool end to end after dmi_reconstruction on a GPU box."""
import os
import subprocess

import numpy as np
import pytest

from cudadepthmapintegration_amd import capi, scene
from coloration_depth_np import color_mesh_depth_np

REQUIRED = ["Coloration", "--input", "mesh.vtp", "--output", "out.vtp", "--krtd", "kList.txt", "--vti", "vtiList.txt"]


def test_required_flags_of_the_reference():
    o, text = capi.color_cli_read_arguments(REQUIRED)
    assert o is not None, text
    assert (o.input, o.output, o.krtd, o.vti) == (b"mesh.vtp", b"out.vtp", b"kList.txt", b"vtiList.txt")
    assert (o.verbose, o.device, o.depth_test) == (0, 0, 0)
    for i in range(1, len(REQUIRED), 2):                       # cmain:126-132: each of the four is required
        o, text = capi.color_cli_read_arguments(REQUIRED[:i] + REQUIRED[i + 2:])
        assert o is None and "Missing arguments..." in text and "--input" in text, text
    o, _ = capi.color_cli_read_arguments(REQUIRED + ["--verbose", "--device", "3", "--depthTolerance", "0.05"])
    assert (o.verbose, o.device, o.depth_test, o.depth_tolerance) == (1, 3, 1, 0.05)
    o, _ = capi.color_cli_read_arguments(REQUIRED + ["--depthTolerance", "0"])
    assert o.depth_test == 1 and o.depth_tolerance == 0.0


@pytest.mark.parametrize("extra,needle", [
    (["--help"], "--depthTolerance"),
    (["--depthTolerance", "nan"], "finite number >= 0"),
    (["--depthTolerance", "-0.5"], "finite number >= 0"),
    (["--depthTolerance", "inf"], "finite number >= 0"),
    (["--depthTolerance", "abc"], "Bad value for --depthTolerance"),
    (["--depthTolerance"], "needs a value"),
    (["--device", "x"], "Bad value for --device"),
    (["--nonsense"], "Unknown argument"),
])
def test_rejected_command_lines(extra, needle):
    o, text = capi.color_cli_read_arguments(REQUIRED + extra)
    assert o is None and needle in text, text


def test_binary_is_built_and_prints_help():
    exe = capi.coloration_cli_binary()
    assert os.path.exists(exe), exe
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--input" in r.stderr and "--vti" in r.stderr and "--depthTolerance" in r.stderr
    assert "not in the reference" in r.stderr and "exits with status 1" in r.stderr


def test_failures_exit_non_zero_with_the_error(tmp_path):
    """Where the reference returns EXIT_SUCCESS and writes nothing (cmain:82-99), this tool says why and returns 1."""
    exe = capi.coloration_cli_binary()
    capi.write_polydata(str(tmp_path / "mesh.vtp"), np.zeros((3, 3)), np.array([[0, 1, 2]]))
    r = subprocess.run([exe, "--input", str(tmp_path / "none.vtp"), "--output", str(tmp_path / "o.vtp"), "--krtd", "k", "--vti", "v"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "cannot open" in r.stderr and not os.path.exists(tmp_path / "o.vtp")
    r = subprocess.run([exe, "--input", str(tmp_path / "mesh.vtp"), "--output", str(tmp_path / "o.vtp"), "--krtd",
                        str(tmp_path / "k.txt"), "--vti", str(tmp_path / "v.txt"), "--verbose"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Error during coloration process..." in r.stdout and "dmi_coloration:" in r.stderr
    assert "** Read input..." in r.stdout and not os.path.exists(tmp_path / "o.vtp")


def test_empty_mesh_is_written_back_without_a_device(tmp_path):
    """No vertex: nothing reaches the GPU, and the writer still carries the input's arrays and adds the three (empty) ones."""
    views = scene.make_views(2, 12, 10, seed=3)
    lv, lk = scene.write_view_files(str(tmp_path), views, scene.make_colors(2, 12, 10, seed=4))
    capi.write_polydata_with_normals(str(tmp_path / "mesh.vtp"), np.zeros((0, 3)), np.zeros((0, 3), np.int64),
                                     np.zeros((0, 3), np.float32), 1.0)
    r = subprocess.run([capi.coloration_cli_binary(), "--input", str(tmp_path / "mesh.vtp"), "--output", str(tmp_path / "o.vtp"),
                        "--krtd", lk, "--vti", lv, "--verbose"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert "** Write output image" in r.stdout
    o = capi.read_polydata(str(tmp_path / "o.vtp"))
    assert list(o.point_data) == ["Normals", "reconstruction_scalar", "MeanColoration", "MedianColoration", "NbProjectedDepthMap"]
    assert o.point_data["MeanColoration"].dtype == np.uint8 and o.point_data["NbProjectedDepthMap"].dtype == np.int32
    assert o.point_designations == [("Normals", "Normals"), ("Scalars", "reconstruction_scalar")]


def _reconstruct(tmp_path, views, colors):
    """dmi_reconstruction --extractMesh --meshNormals on a data folder whose .vti files carry Color arrays: (mesh.vtp, lists)."""
    grid = scene.default_grid((24, 20, 16), rotated=True)
    rp = scene.default_ray_potential(grid)
    data = tmp_path / "data"
    data.mkdir()
    lv, lk = scene.write_view_files(str(data), views, colors)
    gm = np.asarray(grid.grid_matrix).reshape(4, 4)
    end = [grid.origin[a] + (grid.cell_dims[a] + 1) * grid.spacing[a] for a in range(3)]
    args = [capi.cli_binary(), "--dataFolder", str(data), "--depthMapFile", os.path.basename(lv), "--KRTFile", os.path.basename(lk),
            "--gridDims"] + [str(c + 1) for c in grid.cell_dims] + ["--gridOrigin"] + [repr(float(v)) for v in grid.origin] + \
           ["--gridEnd"] + [repr(float(v)) for v in end] + ["--gridVecX"] + [repr(float(v)) for v in gm[0, :3]] + \
           ["--gridVecY"] + [repr(float(v)) for v in gm[1, :3]] + ["--gridVecZ"] + [repr(float(v)) for v in gm[2, :3]] + \
           ["--rayThick", repr(rp.thickness), "--rayRho", repr(rp.rho), "--rayEta", repr(rp.eta), "--rayDelta", repr(rp.delta),
            "--threshBestCost", "0.7", "--contour", "0.25", "--outputGridFilename", str(tmp_path / "volume.vts"),
            "--outputMeshFilename", str(tmp_path / "mesh.vtp"), "--extractMesh", "--meshNormals"]
    r = subprocess.run(args, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    return str(tmp_path / "mesh.vtp"), lv, lk


@pytest.mark.gpu
def test_gpu_reconstruction_then_coloration_end_to_end(tmp_path):
    """mesh.vtp of dmi_reconstruction --extractMesh --meshNormals, coloured by dmi_coloration: the three arrays are the oracle's
    over the mesh's points, points / polys / Normals / reconstruction_scalar are carried through bit for bit; with
    --depthTolerance the arrays are the restatement's (depths as the .vti files hold them)."""
    from oracle import oracle
    views = scene.make_views(5, 48, 36, seed=4, dense=True, with_best_cost=True)
    colors = scene.make_colors(5, 48, 36, seed=5)
    mesh, lv, lk = _reconstruct(tmp_path, views, colors)
    m = capi.read_polydata(mesh)
    assert len(m.points) > 100
    exe = capi.coloration_cli_binary()
    out = str(tmp_path / "colored.vtp")
    r = subprocess.run([exe, "--input", mesh, "--output", out, "--krtd", lk, "--vti", lv, "--verbose"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "** Read input..." in r.stdout and "** Write output image" in r.stdout
    c = capi.read_polydata(out)
    assert c.points.tobytes() == m.points.tobytes() and np.array_equal(c.connectivity, m.connectivity)
    assert np.array_equal(c.offsets, m.offsets) and c.connectivity.dtype == m.connectivity.dtype
    for k in ("Normals", "reconstruction_scalar"):
        assert c.point_data[k].tobytes() == m.point_data[k].tobytes(), k
    assert c.point_designations == m.point_designations
    want = oracle.color_mesh(m.points, colors, views.K4, views.RT4)
    for name, w in zip(("MeanColoration", "MedianColoration", "NbProjectedDepthMap"), want):
        assert np.array_equal(c.point_data[name], w), name
    assert want[2].max() >= 3
    # the same with the visibility test: the restatement's arrays over the depths of the .vti files
    r = subprocess.run([exe, "--input", mesh, "--output", out, "--krtd", lk, "--vti", lv, "--depthTolerance", "0.05"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    c2 = capi.read_polydata(out)
    depths = np.stack([capi.read_depth_map(os.path.join(os.path.dirname(lv), f"frame_{i:04d}.vti"))[0] for i in range(views.n)])
    want2 = color_mesh_depth_np(m.points, colors, depths, views.K4, views.RT4, 0.05)
    for name, w in zip(("MeanColoration", "MedianColoration", "NbProjectedDepthMap"), want2):
        assert np.array_equal(c2.point_data[name], w), name
    assert c2.points.tobytes() == m.points.tobytes() and c2.point_data["Normals"].tobytes() == m.point_data["Normals"].tobytes()
    assert want2[2].sum() < want[2].sum() and want2[2].max() >= 1     # the test rejects some pairs and keeps others
    # colouring an already coloured mesh replaces its three arrays where they stand (vtkFieldData::AddArray)
    r = subprocess.run([exe, "--input", out, "--output", str(tmp_path / "again.vtp"), "--krtd", lk, "--vti", lv],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    a = capi.read_polydata(str(tmp_path / "again.vtp"))
    assert list(a.point_data) == list(c2.point_data)
    for name, w in zip(("MeanColoration", "MedianColoration", "NbProjectedDepthMap"), want):
        assert np.array_equal(a.point_data[name], w), name
