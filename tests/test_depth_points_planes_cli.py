"""dmi_reconstruction --pointCloudPlaneFitRadius, end to end on the GPU, on the files of test_view_set_cli.py's scene:
the written .vtp holds the restatement of the fit (depth_points_planes_np.py) applied to the restated build (depth_points_np.py)
on the restated chain of steps, with PlaneRms; behind --pointCloudOutlierRadius it fits the filtered cloud; with
--pointCloudCellSize behind it the file is the restated thinning of the fitted cloud, without PlaneRms; without the flag the file is,
byte for byte, the file the format has always been.  The flags' refusals: test_depth_points_planes_host.py, without a GPU."""
import numpy as np
import pytest

import depth_points_planes_np as F
import depth_points_radius_np as R
import depth_points_thin_np as T
import test_depth_points_cli as cli
from test_depth_points_radius_cli import _check
from test_depth_points_thin_cli import _plain_file, _restated_build
from test_view_set_cli import _run, _write_views
from view_set_cases import H, N, W
from cudadepthmapintegration_amd import scene

pytestmark = pytest.mark.gpu
RADIUS, MIN_NEIGHBORS, CELL, OUTLIER = 0.05, 4, 0.1, 0.05
NAMES = ("xyz", "normal", "view", "pixel", "count")


def _fit(cloud, flags=3, passes=1):
    out = dict(cloud)
    for _ in range(passes):
        fitted, report = F.fit_planes(out["xyz"], out["normal"], RADIUS, MIN_NEIGHBORS, flags)
        out.update(xyz=fitted["xyz"], normal=fitted["normal"], plane_rms=fitted["plane_rms"])
    return out, report


def test_the_fitted_cloud_is_the_restatements_and_the_plain_one_is_unchanged(tmp_path):
    data = tmp_path / "data"
    data.mkdir()
    threshold = _write_views(str(data))
    colors = scene.make_colors(N, W, H, seed=4)   # what _write_views wrote
    built, _ = _restated_build(False)
    built = {k: built[k] for k in NAMES}
    base = ["--pointCloudKeepDuplicates", "--pointCloudPlaneFitRadius", repr(RADIUS), "--pointCloudPlaneFitMinNeighbors", str(MIN_NEIGHBORS)]
    # without the new flags: the file the format has always been
    cloud = tmp_path / "plain.vtp"
    _run(tmp_path, data, threshold, "plain", ["--outputPointCloudFilename", str(cloud), "--pointCloudKeepDuplicates"])
    assert cloud.read_bytes() == _plain_file(built) and b"PlaneRms" not in cloud.read_bytes()
    # with them: the restated fit of the restated build, PlaneRms before Color
    want, report = _fit(built)
    assert 0 < report["fitted"] < report["points_in"]
    cloud = tmp_path / "fitted.vtp"
    files, out, summary = _run(tmp_path, data, threshold, "fitted", ["--outputPointCloudFilename", str(cloud), "--pointCloudColors"] + base)
    arrays, piece, head = cli._read_vtp(cloud.read_bytes())
    _check(arrays, piece, want, report["points_in"])
    assert arrays["PlaneRms"].dtype == np.float32 and arrays["PlaneRms"].tobytes() == want["plane_rms"].tobytes()
    assert "NbNeighbors" not in arrays and head.index("NbAgreeingViews") < head.index("PlaneRms") < head.index('Name="Color"')
    py, px = want["pixel"] // W, want["pixel"] % W
    assert np.array_equal(arrays["Color"], colors[want["view"], H - 1 - py, px])
    line = [text for text in out.splitlines() if text.startswith("point cloud plane fit:")]
    assert len(line) == 1
    for key in F.REPORT_NAMES:
        assert f" {report[key]} " in line[0], key
    assert (f"point cloud plane fit\n  radius  {RADIUS}\n  minimum neighbours  {MIN_NEIGHBORS}\n  passes  1\n  positions  moved\n"
            f"  normals  replaced\n  points in  {report['points_in']}\n  points fitted  {report['fitted']}\n") in summary
    # two passes, the positions kept: the second pass fits the first one's cloud
    want, report = _fit(built, flags=F.NORMALS, passes=2)
    cloud = tmp_path / "twice.vtp"
    _run(tmp_path, data, threshold, "twice", ["--outputPointCloudFilename", str(cloud), "--pointCloudPlaneFitIterations", "2",
                                              "--pointCloudPlaneFitKeepPositions"] + base)
    arrays, piece, head = cli._read_vtp(cloud.read_bytes())
    _check(arrays, piece, want, report["points_in"])
    assert arrays["Points"].tobytes() == built["xyz"].tobytes() and arrays["PlaneRms"].tobytes() == want["plane_rms"].tobytes()
    # behind the outlier filter, before the thinning
    sifted, sift_report = R.filter_radius(built, OUTLIER, 1)
    want, report = _fit({k: sifted[k] for k in NAMES})
    assert report["points_in"] == sift_report["points_kept"] < sift_report["points_in"]
    cloud = tmp_path / "sifted.vtp"
    files, out, summary = _run(tmp_path, data, threshold, "sifted",
                               ["--outputPointCloudFilename", str(cloud), "--pointCloudOutlierRadius", repr(OUTLIER)] + base)
    arrays, piece, head = cli._read_vtp(cloud.read_bytes())
    _check(arrays, piece, want, report["points_in"])
    assert np.array_equal(arrays["NbNeighbors"], sifted["neighbors"]) and arrays["PlaneRms"].tobytes() == want["plane_rms"].tobytes()
    assert head.index("NbNeighbors") < head.index("PlaneRms") and out.index("point cloud outliers:") < out.index("point cloud plane fit:")
    thinned, thin_report = T.thin(*(want[k] for k in NAMES), cell_size=CELL, min_points=1)
    cloud = tmp_path / "all.vtp"
    files, out, summary = _run(tmp_path, data, threshold, "all",
                               ["--outputPointCloudFilename", str(cloud), "--pointCloudOutlierRadius", repr(OUTLIER), "--pointCloudCellSize",
                                repr(CELL)] + base)
    arrays, piece, head = cli._read_vtp(cloud.read_bytes())
    _check(arrays, piece, thinned, thin_report["cells_kept"])
    assert "PlaneRms" not in arrays and "NbNeighbors" not in arrays and np.array_equal(arrays["NbMergedPoints"], thinned["members"])
    assert out.index("point cloud outliers:") < out.index("point cloud plane fit:") < out.index("point cloud thinning:")
