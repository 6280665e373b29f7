"""dmi_coloration --depthFromMesh and dmi_reconstruction --meshColorationDepthFromMesh (DESIGN.md 8b''): flag parsing and
refusals, the host fan-triangulation and the new option parsing under sanitizers in a stand-alone program, and on the GPU both
tools end to end against the numpy restatements (tests/mesh_depth_np.py feeding tests/coloration_depth_np.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import coloration_depth_np as CD
import mesh_depth_np as MD
from cudadepthmapintegration_amd import capi, scene
from vtp_writer import write_vtp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cudadepthmapintegration_amd", "csrc", "host")
COLOR_ARRAYS = ("MeanColoration", "MedianColoration", "NbProjectedDepthMap")
RECON = ["Reconstruction", "--gridOrigin", "-2.29", "-2.24", "-2.2", "--gridEnd", "1.19", "1.67", "1.22", "--dataFolder", "data",
         "--outputGridFilename", "out.vts", "--outputMeshFilename", "mesh.vtp", "--rayThick", "0.1", "--gridDims", "10"]
COLOR = ["Coloration", "--input", "a.vtp", "--output", "b.vtp", "--krtd", "k.txt", "--vti", "v.txt"]


def test_depth_from_mesh_flags_of_both_tools():
    o, text = capi.color_cli_read_arguments(COLOR + ["--depthTolerance", "0.1", "--depthFromMesh"])
    assert o is not None and (o.depth_test, o.depth_tolerance, o.depth_from_mesh) == (1, 0.1, 1), text
    o, text = capi.color_cli_read_arguments(COLOR + ["--depthTolerance", "0.1"])
    assert o is not None and (o.depth_test, o.depth_from_mesh) == (1, 0), text
    o, text = capi.color_cli_read_arguments(COLOR + ["--depthFromMesh"])
    assert o is None and text.split("\n")[0].startswith("Error : --depthFromMesh needs --depthTolerance"), text
    o, text = capi.color_cli_read_arguments(COLOR + ["--help"])
    assert o is None and "--depthFromMesh\n" in text and "not in the reference" in text.split("--depthFromMesh\n")[1]
    full = ["--extractMesh", "--meshColoration", "--meshColorationDepthTolerance", "0.1", "--meshColorationDepthFromMesh"]
    o, text = capi.cli_read_arguments(RECON + full)
    assert o is not None and (o.mesh_coloration, o.mesh_coloration_fused, o.mesh_coloration_depth_from_mesh) == (1, 1, 1), text
    o, text = capi.cli_read_arguments(RECON + full[:-1])
    assert o is not None and (o.mesh_coloration_fused, o.mesh_coloration_depth_from_mesh) == (1, 0), text
    for without in ("--meshColoration", "--meshColorationDepthTolerance"):
        args = list(full)
        i = args.index(without)
        del args[i:i + (2 if without.endswith("Tolerance") else 1)]
        o, text = capi.cli_read_arguments(RECON + args)
        assert o is None and text.split("\n")[0].startswith("Error : --meshColorationDepth"), (without, text)
    o, text = capi.cli_read_arguments(RECON + ["--extractMesh", "--meshColorationDepthFromMesh"])
    assert o is None and text.split("\n")[0].startswith("Error : --meshColorationDepthFromMesh needs --meshColoration and --meshColorationDepthTolerance"), text
    o, text = capi.cli_read_arguments(RECON + ["--help"])
    assert o is None and "--meshColorationDepthFromMesh\n" in text
    r = subprocess.run([capi.coloration_cli_binary()] + COLOR[1:] + ["--depthFromMesh"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--depthFromMesh needs --depthTolerance" in r.stderr
    r = subprocess.run([capi.cli_binary()] + RECON[1:] + ["--extractMesh", "--meshColoration", "--meshColorationDepthFromMesh"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--meshColorationDepthFromMesh needs" in r.stderr


SANITIZER_MAIN = r"""
#include <cstdio>
#include <sstream>
#include <vector>
#include "color_cli.h"
#include "fan_triangulate.h"
#include "recon_cli.h"
using namespace dmi::host;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED: %s\n", #x); ++fails; } } while (0)
int main() {
  // a triangle, a quad, a pentagon, a degenerate two-corner polygon, an empty one
  const std::vector<int64_t> conn = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13};
  const std::vector<int64_t> offs = {3, 7, 12, 14, 14};
  const std::vector<int64_t> t = FanTriangulate(conn.data(), (int64_t)conn.size(), offs.data(), (int64_t)offs.size());
  const std::vector<int64_t> want = {0, 1, 2, 3, 4, 5, 3, 5, 6, 7, 8, 9, 7, 9, 10, 7, 10, 11};
  CHECK(t == want);
  CHECK(FanTriangulate(nullptr, 0, nullptr, 0).empty());
  const std::vector<int64_t> overrun = {3, 99};  // a second polygon past the connectivity: skipped, nothing read beyond it
  CHECK(FanTriangulate(conn.data(), 5, overrun.data(), 2).size() == 3);
  const char *ok[] = {"c", "--input", "a", "--output", "b", "--krtd", "k", "--vti", "v", "--depthTolerance", "0.5", "--depthFromMesh"};
  color_cli::Options o;
  std::ostringstream err;
  CHECK(color_cli::ReadArguments(12, ok, &o, err) && o.depthFromMesh && o.depthTest && o.depthTolerance == 0.5);
  const char *bad[] = {"c", "--input", "a", "--output", "b", "--krtd", "k", "--vti", "v", "--depthFromMesh"};
  color_cli::Options o2;
  std::ostringstream err2;
  CHECK(!color_cli::ReadArguments(10, bad, &o2, err2) && err2.str().rfind("Error : --depthFromMesh needs --depthTolerance", 0) == 0);
  const char *cut[] = {"c", "--depthFromMesh", "--depthTolerance"};  // a value flag at the end of the line
  color_cli::Options o3;
  std::ostringstream err3;
  CHECK(!color_cli::ReadArguments(3, cut, &o3, err3));
  // the Reconstruction tool's parser: the new flag with its two companions, without either, and cut short
  const char *base[] = {"r", "--gridOrigin", "-2", "-2", "-2", "--gridEnd", "1", "1", "1", "--dataFolder", "d", "--outputGridFilename", "o.vts",
                        "--outputMeshFilename", "m.vtp", "--rayThick", "0.1", "--gridDims", "10", "--extractMesh"};
  auto parse = [&](std::vector<const char *> extra, cli::Options *out, std::string *text) {
    std::vector<const char *> argv(base, base + sizeof(base) / sizeof(base[0]));
    argv.insert(argv.end(), extra.begin(), extra.end());
    std::ostringstream e;
    const bool ok = cli::ReadArguments((int)argv.size(), argv.data(), out, e);
    *text = e.str();
    return ok;
  };
  std::string text;
  cli::Options r1, r2, r3, r4;
  CHECK(parse({"--meshColoration", "--meshColorationDepthTolerance", "0.25", "--meshColorationDepthFromMesh"}, &r1, &text) &&
        r1.meshColorationDepthFromMesh && r1.meshColoration && r1.meshColorationDepthToleranceGiven && r1.meshColorationDepthTolerance == 0.25);
  CHECK(!parse({"--meshColoration", "--meshColorationDepthFromMesh"}, &r2, &text) &&
        text.rfind("Error : --meshColorationDepthFromMesh needs --meshColoration and --meshColorationDepthTolerance", 0) == 0);
  CHECK(!parse({"--meshColorationDepthFromMesh"}, &r3, &text) && text.rfind("Error : --meshColorationDepthFromMesh needs", 0) == 0);
  CHECK(!parse({"--meshColoration", "--meshColorationDepthFromMesh", "--meshColorationDepthTolerance"}, &r4, &text));
  std::printf(fails ? "%d FAILED\n" : "ALL OK\n", fails);
  return fails ? 1 : 0;
}
"""


def test_fan_triangulation_and_option_parsing_under_sanitizers(tmp_path):
    """Host code only, in a program of its own: the fan triangulation (a header) and the argument parsers of both tools, compiled
    with -fsanitize=address,undefined.  The parsers' translation units also hold the tools' Run, whose callees live in the
    library: sections nobody reaches are dropped at the link, so none of them is needed."""
    cxx = shutil.which("clang++") or shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not (shutil.which(cxx) or os.path.exists(cxx)):
        pytest.skip("no host C++ compiler")
    main = tmp_path / "main.cpp"
    main.write_text(SANITIZER_MAIN)
    exe = str(tmp_path / "host_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffunction-sections", "-fdata-sections",
           "-I" + HOST, str(main), os.path.join(HOST, "color_cli.cpp"), os.path.join(HOST, "recon_cli.cpp"), "-Wl,--gc-sections", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr


def _write_color_only_views(directory, views, colors):
    """The scene's views as .vti files that hold a Color array and NOTHING else, with their .krtd files and the two lists."""
    from vti_writer import write_vti
    n, h, w = views.depth.shape
    vti, krtd = [], []
    for m in range(n):
        vti.append(os.path.join(directory, f"color_{m:04d}.vti"))
        krtd.append(os.path.join(directory, f"color_{m:04d}.krtd"))
        write_vti(vti[-1], {"Color": colors[m]}, w, h, mode="appended-raw")
        scene.write_krtd(krtd[-1], views.K4[m][:3, :3], views.RT4[m])
    lv, lk = os.path.join(directory, "colorVtiList.txt"), os.path.join(directory, "colorKrtdList.txt")
    open(lv, "w").write("".join(f"{i} {os.path.basename(f)}\n" for i, f in enumerate(vti)))
    open(lk, "w").write("".join(f"{i} {os.path.basename(f)}\n" for i, f in enumerate(krtd)))
    return lv, lk


def test_files_without_depths_are_images_only_for_the_rendered_depth(tmp_path):
    """No GPU: a .vti with a Color array alone is refused as before by everything that wants its Depths ("view 0 has no image"),
    and is an image for the colouring that renders its own depth -- which then gets as far as the device."""
    _, _, views, colors = _scene()
    lv, lk = _write_color_only_views(str(tmp_path), views, colors)
    pts = np.array([[0.0, 0.0, 0.6], [0.1, 0.0, 0.6], [0.0, 0.1, 0.6]])
    for tolerance in (None, 0.1):
        with pytest.raises(RuntimeError) as e:
            capi.mesh_coloration_from_lists(pts, lv, lk, depth_tolerance=tolerance)
        assert "has no image" in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        capi.mesh_coloration_from_lists(pts, lv, lk, triangles=[[0, 1, 2]])
    if capi.device_count() > 0:
        mean, median, count = capi.mesh_coloration_from_lists(pts, lv, lk, depth_tolerance=0.1, triangles=[[0, 1, 2]])
        assert count.shape == (3,)
    else:
        with pytest.raises(RuntimeError) as e:
            capi.mesh_coloration_from_lists(pts, lv, lk, depth_tolerance=0.1, triangles=[[0, 1, 2]])
        assert "has no image" not in str(e.value) and "Depths" not in str(e.value), str(e.value)


# ---- GPU: both tools end to end --------------------------------------------------------------------------------------------------
SW, SH, S_VIEWS = 80, 60, 4
TOLERANCE = 2.0 / 32


def _scene():
    grid = scene.default_grid(32)
    ray = scene.default_ray_potential(grid)
    views = scene.make_views(S_VIEWS, SW, SH, seed=3, with_best_cost=True)
    colors = scene.make_colors(S_VIEWS, SW, SH, seed=5)
    return grid, ray, views, colors


def _reconstruct(tmp_path, lv, lk, name, extra):
    grid, ray, _, _ = _scene()
    end = [grid.origin[a] + (grid.cell_dims[a] + 1) * grid.spacing[a] for a in range(3)]
    args = [capi.cli_binary(), "--dataFolder", os.path.dirname(lv), "--depthMapFile", os.path.basename(lv), "--KRTFile", os.path.basename(lk),
            "--gridDims"] + [str(c + 1) for c in grid.cell_dims] + ["--gridOrigin"] + [repr(float(v)) for v in grid.origin] + \
           ["--gridEnd"] + [repr(float(v)) for v in end] + \
           ["--rayThick", repr(ray.thickness), "--rayRho", repr(ray.rho), "--rayEta", repr(ray.eta), "--rayDelta", repr(ray.delta),
            "--threshBestCost", "1e9", "--contour", "0.0", "--outputGridFilename", str(tmp_path / (name + ".vts")),
            "--outputMeshFilename", str(tmp_path / (name + ".vtp")), "--extractMesh"] + extra
    return subprocess.run(args, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)


def _colorize(tmp_path, mesh, out, lv, lk, extra=()):
    r = subprocess.run([capi.coloration_cli_binary(), "--input", str(tmp_path / mesh), "--output", str(tmp_path / out), "--krtd", lk, "--vti", lv]
                       + list(extra), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    return capi.read_polydata(str(tmp_path / out))


def _triangles_of(mesh):
    off = np.asarray(mesh.offsets, dtype=np.int64)
    assert (np.diff(np.concatenate([[0], off])) == 3).all()
    return np.asarray(mesh.connectivity, dtype=np.int64).reshape(-1, 3)


def _restatement(points, triangles):
    _, _, views, colors = _scene()
    planes = MD.to_vtk_depths(MD.render_depths_np(points, triangles, views.K4, views.RT4, SW, SH))
    return CD.color_mesh_depth_np(points, colors, planes, views.K4, views.RT4, TOLERANCE)


@pytest.mark.gpu
def test_both_tools_with_the_meshs_own_depth_are_the_restatement(tmp_path):
    _, _, views, colors = _scene()
    data = tmp_path / "data"
    data.mkdir()
    lv, lk = scene.write_view_files(str(data), views, colors)
    tol = ["--meshColoration", "--meshColorationDepthTolerance", repr(TOLERANCE)]
    r = _reconstruct(tmp_path, lv, lk, "fused", tol + ["--summary"])
    assert r.returncode == 0, r.stderr + r.stdout
    fused_bytes = open(tmp_path / "fused.vtp", "rb").read()
    r = _reconstruct(tmp_path, lv, lk, "rendered", tol + ["--meshColorationDepthFromMesh", "--summary"])
    assert r.returncode == 0, r.stderr + r.stdout
    line = [x for x in r.stdout.splitlines() if x.startswith("mesh coloration:")]
    assert len(line) == 1 and "against the mesh's own rendered depth" in line[0] and "to render" in line[0], r.stdout
    assert "against the mesh's own rendered depth" in open(os.path.join(os.path.dirname(lv), "summary.txt")).read()
    fused, rendered = capi.read_polydata(str(tmp_path / "fused.vtp")), capi.read_polydata(str(tmp_path / "rendered.vtp"))
    assert rendered.points.tobytes() == fused.points.tobytes() and np.array_equal(rendered.connectivity, fused.connectivity)
    want = _restatement(rendered.points, _triangles_of(rendered))
    for k, w in zip(COLOR_ARRAYS, want):
        got = np.ascontiguousarray(rendered.point_data[k]).reshape(w.shape)
        assert got.dtype == w.dtype and got.tobytes() == w.tobytes(), k
    assert (want[2] > 0).any()
    # dmi_coloration --depthFromMesh on the same mesh: the same three arrays; without the flag its output is what it was
    by_tool = _colorize(tmp_path, "fused.vtp", "by_tool.vtp", lv, lk, ["--depthTolerance", repr(TOLERANCE), "--depthFromMesh"])
    for k in COLOR_ARRAYS:
        assert np.ascontiguousarray(by_tool.point_data[k]).tobytes() == np.ascontiguousarray(rendered.point_data[k]).tobytes(), k
    assert np.array_equal(by_tool.connectivity, fused.connectivity) and np.array_equal(by_tool.offsets, fused.offsets)
    # without the new flags: byte for byte the files of the flags that existed before
    r = _reconstruct(tmp_path, lv, lk, "fused_again", tol)
    assert r.returncode == 0 and open(tmp_path / "fused_again.vtp", "rb").read() == fused_bytes
    plain = _colorize(tmp_path, "fused.vtp", "plain_tool.vtp", lv, lk, ["--depthTolerance", repr(TOLERANCE)])
    views_depth = CD.color_mesh_depth_np(plain.points, colors, views.depth, views.K4, views.RT4, TOLERANCE)
    for k, w in zip(COLOR_ARRAYS, views_depth):
        assert np.ascontiguousarray(plain.point_data[k]).reshape(w.shape).tobytes() == w.tobytes(), k


@pytest.mark.gpu
def test_coloration_tool_fan_triangulates_polygons_for_the_rendering_only(tmp_path):
    """A quad and a pentagon in front of one camera: rendered as their fans, written as they came."""
    _, _, views, colors = _scene()
    data = tmp_path / "data"
    data.mkdir()
    lv, lk = scene.write_view_files(str(data), views, colors)
    pts = np.array([[-0.4, -0.4, 0.1], [0.4, -0.4, 0.1], [0.4, 0.4, 0.1], [-0.4, 0.4, 0.1],
                    [-0.2, -0.2, -0.3], [0.2, -0.2, -0.3], [0.3, 0.1, -0.3], [0.0, 0.3, -0.3], [-0.3, 0.1, -0.3]])
    conn, offs = np.arange(9, dtype=np.int64), np.array([4, 9], dtype=np.int64)
    write_vtp(str(tmp_path / "polys.vtp"), pts, conn, offs)
    out = _colorize(tmp_path, "polys.vtp", "polys_out.vtp", lv, lk, ["--depthTolerance", repr(TOLERANCE), "--depthFromMesh"])
    assert np.array_equal(out.connectivity, conn) and np.array_equal(out.offsets, offs)
    fans = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7], [4, 7, 8]], dtype=np.int64)
    want = _restatement(pts, fans)
    for k, w in zip(COLOR_ARRAYS, want):
        assert np.ascontiguousarray(out.point_data[k]).reshape(w.shape).tobytes() == w.tobytes(), k
    assert (want[2] > 0).any() and (want[2] < S_VIEWS).any()


@pytest.mark.gpu
def test_depth_from_mesh_needs_no_depths_arrays(tmp_path):
    """The motivating case: a mesh from elsewhere and views that have colours only.  dmi_coloration --depthFromMesh and the host
    entry point give the restatement's arrays; without the flag the same files are refused."""
    _, _, views, colors = _scene()
    lv, lk = _write_color_only_views(str(tmp_path), views, colors)
    rng = np.random.default_rng(11)
    # a closed box around the origin, each face two triangles, and a few loose points on and off it
    c = 0.45 * np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], dtype=np.float64)
    pts = np.concatenate([c, rng.uniform(-0.6, 0.6, (40, 3))])
    tri = np.array([[0, 1, 2], [0, 2, 3], [4, 6, 5], [4, 7, 6], [0, 4, 5], [0, 5, 1], [1, 5, 6], [1, 6, 2], [2, 6, 7], [2, 7, 3], [3, 7, 4], [3, 4, 0]],
                   dtype=np.int64)
    write_vtp(str(tmp_path / "box.vtp"), pts, tri.ravel(), 3 * np.arange(1, len(tri) + 1, dtype=np.int64))
    want = _restatement(pts, tri)
    assert (want[2] > 0).any() and (want[2] < S_VIEWS).any()
    out = _colorize(tmp_path, "box.vtp", "box_out.vtp", lv, lk, ["--depthTolerance", repr(TOLERANCE), "--depthFromMesh"])
    for k, w in zip(COLOR_ARRAYS, want):
        assert np.ascontiguousarray(out.point_data[k]).reshape(w.shape).tobytes() == w.tobytes(), k
    got = capi.mesh_coloration_from_lists(pts, lv, lk, depth_tolerance=TOLERANCE, triangles=tri)
    for k, g, w in zip(COLOR_ARRAYS, got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), k
    for extra in ([], ["--depthTolerance", repr(TOLERANCE)]):
        r = subprocess.run([capi.coloration_cli_binary(), "--input", str(tmp_path / "box.vtp"), "--output", str(tmp_path / "no.vtp"), "--krtd", lk,
                            "--vti", lv] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and not os.path.exists(tmp_path / "no.vtp"), r.stdout + r.stderr
