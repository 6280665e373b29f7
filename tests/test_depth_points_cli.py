"""dmi_reconstruction --outputPointCloudFilename, end to end on the GPU, on the files of test_view_set_cli.py's
scene: the .vtp parses and holds what ViewSet.build_points + download_points give on the same chain of steps (positions and normals
by their bytes), Color is each point's pixel of the colours written, the .vts, the .mha and the mesh are the bytes of a run without
the flag, and the flag's refusals say why."""
import re
import subprocess

import numpy as np
import pytest

from test_view_set_cli import _run, _write_views
from view_set_cases import CHAIN, CONSISTENCY, H, N, W, view_set_scene
from cudadepthmapintegration_amd import capi, scene

pytestmark = pytest.mark.gpu
STEP_METHODS = {"speckles": "filter_speckles", "holes": "fill_holes", "smooth": "smooth", "consistency": "filter_consistency"}
NUMPY_TYPES = {"Float64": np.float64, "Float32": np.float32, "Int64": np.int64, "Int32": np.int32, "UInt8": np.uint8}


def _read_vtp(data):
    """{array name: values} of a VTK XML PolyData file with raw appended data and UInt64 headers, and the Piece's attributes."""
    start = data.index(b"<AppendedData")
    head = data[:start].decode()
    assert 'byte_order="LittleEndian"' in head and 'header_type="UInt64"' in head and b'encoding="raw"' in data[start:start + 40]
    base = data.index(b"_", start) + 1
    piece = dict(re.findall(r'(NumberOf\w+)="(\d+)"', re.search(r"<Piece [^>]*>", head).group(0)))
    arrays = {}
    for tag in re.findall(r"<DataArray [^>]*/>", head):
        a = dict(re.findall(r'(\w+)="([^"]*)"', tag))
        assert a["format"] == "appended"
        at = base + int(a["offset"])
        n_bytes = int(np.frombuffer(data[at:at + 8], dtype="<u8")[0])
        values = np.frombuffer(data[at + 8:at + 8 + n_bytes], dtype=NUMPY_TYPES[a["type"]])
        arrays[a["Name"]] = values.reshape(-1, int(a["NumberOfComponents"])) if "NumberOfComponents" in a else values
    assert data[base:].rstrip().endswith(b"</VTKFile>")
    return arrays, {k: int(v) for k, v in piece.items()}, head


def _points_of_the_chain(**params):
    views, threshold = view_set_scene()
    with capi.ViewSet(W, H) as s:
        s.add(views, threshold)
        for name, step in CHAIN:
            getattr(s, STEP_METHODS[name])(**step)
        report = s.build_points(abs_tolerance=CONSISTENCY["abs_tolerance"], rel_tolerance=CONSISTENCY["rel_tolerance"], **params)
        return s.download_points(), report


def _check_cloud(data, want, report, colors):
    arrays, piece, head = _read_vtp(data)
    n = report["points"]
    assert n > 0 and piece == dict(NumberOfPoints=n, NumberOfVerts=n, NumberOfLines=0, NumberOfStrips=0, NumberOfPolys=0)
    assert arrays["Points"].dtype == np.float64 and arrays["Points"].tobytes() == want["xyz"].tobytes()
    assert arrays["Normals"].dtype == np.float32 and arrays["Normals"].tobytes() == want["normal"].tobytes()
    assert arrays["ViewIndex"].dtype == np.int32 and np.array_equal(arrays["ViewIndex"], want["view"])
    assert arrays["NbAgreeingViews"].dtype == np.int32 and np.array_equal(arrays["NbAgreeingViews"], want["count"])
    assert np.array_equal(arrays["connectivity"], np.arange(n)) and np.array_equal(arrays["offsets"], np.arange(1, n + 1))
    assert '<PointData Normals="Normals">' in head and "<Verts>" in head
    if colors is None:
        assert "Color" not in arrays
    else:
        py, px = want["pixel"] // W, want["pixel"] % W
        assert arrays["Color"].dtype == np.uint8 and np.array_equal(arrays["Color"], colors[want["view"], H - 1 - py, px])
        assert len(np.unique(arrays["Color"], axis=0)) > 100


def test_the_point_cloud_is_the_view_sets_and_changes_no_other_file(tmp_path):
    data = tmp_path / "data"
    data.mkdir()
    threshold = _write_views(str(data))
    colors = scene.make_colors(N, W, H, seed=4)   # what _write_views wrote
    plain = _run(tmp_path, data, threshold, "plain", [])
    want, report = _points_of_the_chain()
    for name, extra, rgb in (("cloud", [], None), ("coloured", ["--pointCloudColors"], colors)):
        cloud = tmp_path / (name + ".vtp")
        files, out, summary = _run(tmp_path, data, threshold, name, ["--outputPointCloudFilename", str(cloud)] + extra)
        for other in files:
            assert files[other] == plain[0][other], (name, other)
        _check_cloud(cloud.read_bytes(), want, report, rgb)
        line = [text for text in out.splitlines() if text.startswith("point cloud:")]
        assert len(line) == 1
        for key in ("valid", "candidates", "owned", "points", "with_normal"):
            assert f" {report[key]} " in line[0], key
        assert "point cloud\n" in summary and f"\n  points  {report['points']}\n" in summary
        assert f"\n  points with a normal  {report['with_normal']}\n" in summary and "GPU kernels" in summary.split("point cloud\n")[1]
    # the options reach the build: every view keeps its points, every second pixel, looser normals, no agreement asked
    want, report = _points_of_the_chain(min_views=0, pixel_step=2, dedupe=False, normal_abs_tolerance=0.05, normal_rel_tolerance=0.0)
    cloud = tmp_path / "options.vtp"
    _run(tmp_path, data, threshold, "options",
         ["--outputPointCloudFilename", str(cloud), "--pointCloudMinViews", "0", "--pointCloudPixelStep", "2", "--pointCloudKeepDuplicates",
          "--pointCloudNormalTolerance", "0.05", "--pointCloudNormalRelTolerance", "0"])
    assert report["owned"] == 0
    _check_cloud(cloud.read_bytes(), want, report, None)


def _refused(tmp_path, args):
    r = subprocess.run([capi.cli_binary()] + args, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    return r.stdout + r.stderr


def test_the_flags_refusals_say_why(tmp_path):
    data = tmp_path / "data"
    data.mkdir()
    threshold = _write_views(str(data))
    base = ["--dataFolder", str(data), "--depthMapFile", "vtiList.txt", "--KRTFile", "krtdList.txt", "--gridDims", "25", "--gridOrigin",
            "-1", "-1", "-1", "--gridEnd", "1", "1", "1", "--threshBestCost", repr(threshold), "--outputGridFilename",
            str(tmp_path / "volume.vts"), "--outputMeshFilename", str(tmp_path / "mesh.vtp")]
    cloud = ["--outputPointCloudFilename", str(tmp_path / "cloud.vtp")]
    consistency = ["--depthConsistencyMinViews", "1", "--depthConsistencyTolerance", "0.02"]
    text = _refused(tmp_path, base + cloud + consistency + ["--depthStagedFilters"])
    assert "--outputPointCloudFilename" in text and "--depthStagedFilters" in text and "resident" in text
    text = _refused(tmp_path, base + cloud)
    assert "--pointCloudTolerance or --pointCloudRelTolerance" in text
    text = _refused(tmp_path, base + ["--pointCloudMinViews", "2"])
    assert "--pointCloudMinViews needs --outputPointCloudFilename" in text
    text = _refused(tmp_path, base + ["--outputPointCloudFilename", str(tmp_path / "cloud.ply"), "--pointCloudTolerance", "0.02"])
    assert ".vtp" in text
    assert not (tmp_path / "cloud.vtp").exists() and not (tmp_path / "volume.vts").exists()
