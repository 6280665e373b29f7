"""dmi_reconstruction --pointCloudCellSize, end to end on the GPU, on the files of test_view_set_cli.py's scene: with
--pointCloudKeepDuplicates the written .vtp holds the restatement of the thinning (depth_points_thin_np.py) applied to the restated
build (depth_points_np.py) on the restated chain of steps -- points and normals by their bytes, ViewIndex, NbAgreeingViews,
NbMergedPoints, and Color through each point's first member; without the flag the file is, byte for byte, the file the format has
always been (restated here from recon_cli.h's description).  The flags' refusals: test_depth_points_thin_host.py, without a GPU."""
import struct

import numpy as np
import pytest

import depth_points_np as P
import depth_points_thin_np as T
import test_depth_points_cli as cli
from test_depth_points import AGREEMENT, _chain_depth
from test_view_set_cli import _run, _write_views
from view_set_cases import H, N, W, view_set_scene
from cudadepthmapintegration_amd import scene

pytestmark = pytest.mark.gpu
cli.NUMPY_TYPES.setdefault("UInt32", np.uint32)   # NbMergedPoints' type
CELL = 0.1


def _restated_build(dedupe):
    views, _ = view_set_scene()
    return P.build_points(_chain_depth(), views.K4, views.RT4, min_views=1, pixel_step=1, dedupe=dedupe, **AGREEMENT)


def _plain_file(cloud):
    """The .vtp of a cloud that is not thinned, as the tool has always written it."""
    n = len(cloud["view"])
    blocks = [cloud["xyz"].tobytes(), np.arange(n, dtype=np.int64).tobytes(), np.arange(1, n + 1, dtype=np.int64).tobytes(),
              cloud["normal"].tobytes(), cloud["view"].tobytes(), cloud["count"].tobytes()]
    offsets = np.concatenate([[0], np.cumsum([8 + len(b) for b in blocks])]).tolist()
    head = ('<?xml version="1.0"?>\n<VTKFile type="PolyData" version="1.0" byte_order="LittleEndian" header_type="UInt64">\n'
            f'  <PolyData>\n    <Piece NumberOfPoints="{n}" NumberOfVerts="{n}" NumberOfLines="0" NumberOfStrips="0" NumberOfPolys="0">\n'
            '      <PointData Normals="Normals">\n'
            f'        <DataArray type="Float32" Name="Normals" NumberOfComponents="3" format="appended" offset="{offsets[3]}"/>\n'
            f'        <DataArray type="Int32" Name="ViewIndex" format="appended" offset="{offsets[4]}"/>\n'
            f'        <DataArray type="Int32" Name="NbAgreeingViews" format="appended" offset="{offsets[5]}"/>\n'
            '      </PointData>\n      <Points>\n'
            '        <DataArray type="Float64" Name="Points" NumberOfComponents="3" format="appended" offset="0"/>\n'
            '      </Points>\n      <Verts>\n'
            f'        <DataArray type="Int64" Name="connectivity" format="appended" offset="{offsets[1]}"/>\n'
            f'        <DataArray type="Int64" Name="offsets" format="appended" offset="{offsets[2]}"/>\n'
            '      </Verts>\n    </Piece>\n  </PolyData>\n  <AppendedData encoding="raw">\n   _')
    body = b"".join(struct.pack("<Q", len(b)) + b for b in blocks)
    return head.encode() + body + b"\n  </AppendedData>\n</VTKFile>\n"


def test_the_thinned_cloud_is_the_restatements_and_the_plain_one_is_unchanged(tmp_path):
    data = tmp_path / "data"
    data.mkdir()
    threshold = _write_views(str(data))
    colors = scene.make_colors(N, W, H, seed=4)   # what _write_views wrote
    # without the new flag: the file the format has always been, with and without duplicates
    for name, extra, dedupe in (("plain", [], True), ("duplicates", ["--pointCloudKeepDuplicates"], False)):
        cloud = tmp_path / (name + ".vtp")
        _run(tmp_path, data, threshold, name, ["--outputPointCloudFilename", str(cloud)] + extra)
        built, _ = _restated_build(dedupe)
        assert cloud.read_bytes() == _plain_file(built), name
        assert b"NbMergedPoints" not in cloud.read_bytes()
    # with it: the restated thinning of the restated build
    built, _ = _restated_build(False)
    for name, min_points, extra in (("thinned", 1, []), ("dense", 3, ["--pointCloudMinCellPoints", "3", "--pointCloudColors"])):
        want, report = T.thin(*(built[k] for k in ("xyz", "normal", "view", "pixel", "count")), cell_size=CELL, min_points=min_points)
        assert report["multi_view_cells"] > 50 and report["largest_cell"] >= 3 and 0 < report["cells_kept"] < len(built["view"])
        cloud = tmp_path / (name + ".vtp")
        files, out, summary = _run(tmp_path, data, threshold, name, ["--outputPointCloudFilename", str(cloud), "--pointCloudKeepDuplicates",
                                                                     "--pointCloudCellSize", repr(CELL)] + extra)
        arrays, piece, head = cli._read_vtp(cloud.read_bytes())
        n = report["cells_kept"]
        assert piece == dict(NumberOfPoints=n, NumberOfVerts=n, NumberOfLines=0, NumberOfStrips=0, NumberOfPolys=0)
        assert arrays["Points"].dtype == np.float64 and arrays["Points"].tobytes() == want["xyz"].tobytes()
        assert arrays["Normals"].dtype == np.float32 and arrays["Normals"].tobytes() == want["normal"].tobytes()
        assert arrays["ViewIndex"].dtype == np.int32 and np.array_equal(arrays["ViewIndex"], want["view"])
        assert arrays["NbAgreeingViews"].dtype == np.int32 and np.array_equal(arrays["NbAgreeingViews"], want["count"])
        assert arrays["NbMergedPoints"].dtype == np.uint32 and np.array_equal(arrays["NbMergedPoints"], want["members"])
        assert np.array_equal(arrays["connectivity"], np.arange(n)) and np.array_equal(arrays["offsets"], np.arange(1, n + 1))
        if "--pointCloudColors" in extra:   # a real member's colour: through the first member's view and pixel
            py, px = want["pixel"] // W, want["pixel"] % W
            assert arrays["Color"].dtype == np.uint8 and np.array_equal(arrays["Color"], colors[want["view"], H - 1 - py, px])
        else:
            assert "Color" not in arrays
        line = [text for text in out.splitlines() if text.startswith("point cloud thinning:")]
        assert len(line) == 1
        for key in ("points_in", "cells", "cells_kept", "multi_view_cells", "largest_cell", "with_normal"):
            assert f" {report[key]} " in line[0], key
        assert f"point cloud thinning\n  cell size  {CELL}\n  minimum points per cell  {min_points}\n  occupied cells  {report['cells']}\n" in summary
        assert f"\n  cells kept  {report['cells_kept']}\n" in summary
