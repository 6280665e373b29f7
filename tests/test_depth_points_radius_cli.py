"""dmi_reconstruction --pointCloudOutlierRadius, end to end on the GPU, on the files of test_view_set_cli.py's scene:
the written .vtp holds the restatement of the filter (depth_points_radius_np.py) applied to the restated build (depth_points_np.py)
on the restated chain of steps, with NbNeighbors; with --pointCloudCellSize behind it the file is the restated thinning of the
filtered cloud, without NbNeighbors; without the flag the file is, byte for byte, the file the format has always been.  The flags'
refusals: test_depth_points_radius_host.py, without a GPU."""
import numpy as np
import pytest

import depth_points_radius_np as R
import depth_points_thin_np as T
import test_depth_points_cli as cli
from test_depth_points_thin_cli import _plain_file, _restated_build
from test_view_set_cli import _run, _write_views
from view_set_cases import H, N, W
from cudadepthmapintegration_amd import scene

pytestmark = pytest.mark.gpu
RADIUS, MIN_NEIGHBORS, CELL = 0.05, 3, 0.1
NAMES = ("xyz", "normal", "view", "pixel", "count")


def _check(arrays, piece, want, n):
    assert piece == dict(NumberOfPoints=n, NumberOfVerts=n, NumberOfLines=0, NumberOfStrips=0, NumberOfPolys=0)
    assert arrays["Points"].dtype == np.float64 and arrays["Points"].tobytes() == want["xyz"].tobytes()
    assert arrays["Normals"].dtype == np.float32 and arrays["Normals"].tobytes() == want["normal"].tobytes()
    assert arrays["ViewIndex"].dtype == np.int32 and np.array_equal(arrays["ViewIndex"], want["view"])
    assert arrays["NbAgreeingViews"].dtype == np.int32 and np.array_equal(arrays["NbAgreeingViews"], want["count"])
    assert np.array_equal(arrays["connectivity"], np.arange(n)) and np.array_equal(arrays["offsets"], np.arange(1, n + 1))


def test_the_filtered_cloud_is_the_restatements_and_the_plain_one_is_unchanged(tmp_path):
    data = tmp_path / "data"
    data.mkdir()
    threshold = _write_views(str(data))
    colors = scene.make_colors(N, W, H, seed=4)   # what _write_views wrote
    built, _ = _restated_build(False)
    # without the new flag: the file the format has always been
    cloud = tmp_path / "plain.vtp"
    _run(tmp_path, data, threshold, "plain", ["--outputPointCloudFilename", str(cloud), "--pointCloudKeepDuplicates"])
    assert cloud.read_bytes() == _plain_file(built) and b"NbNeighbors" not in cloud.read_bytes()
    # with it: the restated filter of the restated build, NbNeighbors behind NbAgreeingViews and before Color
    want, report = R.filter_radius({k: built[k] for k in NAMES}, RADIUS, MIN_NEIGHBORS)
    assert 0 < report["points_kept"] < report["points_in"] and report["isolated"] > 0
    cloud = tmp_path / "sifted.vtp"
    files, out, summary = _run(tmp_path, data, threshold, "sifted",
                               ["--outputPointCloudFilename", str(cloud), "--pointCloudKeepDuplicates", "--pointCloudOutlierRadius",
                                repr(RADIUS), "--pointCloudMinNeighbors", str(MIN_NEIGHBORS), "--pointCloudColors"])
    arrays, piece, head = cli._read_vtp(cloud.read_bytes())
    _check(arrays, piece, want, report["points_kept"])
    assert arrays["NbNeighbors"].dtype == np.uint32 and np.array_equal(arrays["NbNeighbors"], want["neighbors"])
    assert "NbMergedPoints" not in arrays and head.index("NbAgreeingViews") < head.index("NbNeighbors") < head.index('Name="Color"')
    py, px = want["pixel"] // W, want["pixel"] % W
    assert arrays["Color"].dtype == np.uint8 and np.array_equal(arrays["Color"], colors[want["view"], H - 1 - py, px])
    line = [text for text in out.splitlines() if text.startswith("point cloud outliers:")]
    assert len(line) == 1
    for key in R.REPORT_NAMES:
        assert f" {report[key]} " in line[0], key
    assert (f"point cloud outliers\n  radius  {RADIUS}\n  minimum neighbours  {MIN_NEIGHBORS}\n  points in  {report['points_in']}\n"
            f"  points kept  {report['points_kept']}\n") in summary
    # the default --pointCloudMinNeighbors is 1; the thinning behind the filter takes the filtered cloud: strays never become cells
    once, once_report = R.filter_radius({k: built[k] for k in NAMES}, RADIUS, 1)
    thinned, thin_report = T.thin(*(once[k] for k in NAMES), cell_size=CELL, min_points=1)
    assert thin_report["points_in"] == once_report["points_kept"] < once_report["points_in"]
    cloud = tmp_path / "both.vtp"
    files, out, summary = _run(tmp_path, data, threshold, "both",
                               ["--outputPointCloudFilename", str(cloud), "--pointCloudKeepDuplicates", "--pointCloudOutlierRadius",
                                repr(RADIUS), "--pointCloudCellSize", repr(CELL)])
    arrays, piece, head = cli._read_vtp(cloud.read_bytes())
    _check(arrays, piece, thinned, thin_report["cells_kept"])
    assert "NbNeighbors" not in arrays and np.array_equal(arrays["NbMergedPoints"], thinned["members"])
    assert out.index("point cloud outliers:") < out.index("point cloud thinning:")
