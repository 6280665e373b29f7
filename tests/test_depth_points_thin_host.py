"""--pointCloudCellSize and --pointCloudMinCellPoints at the command line's argument reader (recon_cli.cpp through
dmi_cli_read_arguments): what they need, what they refuse, what --help says, and that the options struct of
include/dmi_host.h and its Python binding carry them.  No GPU."""
from cudadepthmapintegration_amd import capi

BASE = ["prog", "--gridOrigin", "-1", "-1", "-1", "--gridEnd", "1", "1", "1", "--dataFolder", "data", "--outputGridFilename", "out.vts",
        "--outputMeshFilename", "mesh.vtp", "--rayThick", "0.1", "--gridDims", "10"]
CLOUD = ["--outputPointCloudFilename", "cloud.vtp", "--pointCloudTolerance", "0.02"]


def test_the_options_reach_the_host_struct():
    o, text = capi.cli_read_arguments(BASE + CLOUD)
    assert o is not None and o.point_cloud_cell_size == 0.0 and o.point_cloud_min_cell_points == 1, text
    o, text = capi.cli_read_arguments(BASE + CLOUD + ["--pointCloudCellSize", "0.25"])
    assert o is not None and o.point_cloud_cell_size == 0.25 and o.point_cloud_min_cell_points == 1, text
    o, text = capi.cli_read_arguments(BASE + CLOUD + ["--pointCloudKeepDuplicates", "--pointCloudCellSize", "1e-3", "--pointCloudMinCellPoints", "4"])
    assert o is not None and o.point_cloud_cell_size == 1e-3 and o.point_cloud_min_cell_points == 4, text
    assert o.depth_staged_filters == 0 and o.depth_smooth_iterations == 1   # the fields in front of the new ones stand where they stood


def test_the_flags_refusals_say_why():
    o, text = capi.cli_read_arguments(BASE + ["--pointCloudCellSize", "0.1"])
    assert o is None and text.startswith("Error : --pointCloudCellSize needs --outputPointCloudFilename"), text
    o, text = capi.cli_read_arguments(BASE + CLOUD + ["--pointCloudMinCellPoints", "2"])
    assert o is None and text.startswith("Error : --pointCloudMinCellPoints needs --pointCloudCellSize"), text
    for value in ("0", "-1", "nan", "inf", "x"):
        o, text = capi.cli_read_arguments(BASE + CLOUD + ["--pointCloudCellSize", value])
        assert o is None and "--pointCloudCellSize" in text.split("\n")[0], (value, text[:200])
    for value in ("0", "-2", "1.5", str(2 ** 31)):
        o, text = capi.cli_read_arguments(BASE + CLOUD + ["--pointCloudCellSize", "0.1", "--pointCloudMinCellPoints", value])
        assert o is None and "--pointCloudMinCellPoints" in text.split("\n")[0], (value, text[:200])


def test_help_says_what_averages_across_views():
    o, text = capi.cli_read_arguments(BASE + ["--help"])
    text = " ".join(text.split())
    assert o is None and "--pointCloudCellSize" in text and "--pointCloudMinCellPoints" in text and "NbMergedPoints" in text
    assert "Together with --pointCloudCellSize this is what averages across views" in text
