"""--pointCloudOutlierRadius and --pointCloudMinNeighbors at the command line's argument reader (recon_cli.cpp through
dmi_cli_read_arguments): what they need, what they refuse, what --help says, and that the options struct of
include/dmi_host.h and its Python binding carry them.  No GPU."""
from cudadepthmapintegration_amd import capi

BASE = ["prog", "--gridOrigin", "-1", "-1", "-1", "--gridEnd", "1", "1", "1", "--dataFolder", "data", "--outputGridFilename", "out.vts",
        "--outputMeshFilename", "mesh.vtp", "--rayThick", "0.1", "--gridDims", "10"]
CLOUD = ["--outputPointCloudFilename", "cloud.vtp", "--pointCloudTolerance", "0.02"]


def test_the_options_reach_the_host_struct():
    o, text = capi.cli_read_arguments(BASE + CLOUD)
    assert o is not None and o.point_cloud_outlier_radius == 0.0 and o.point_cloud_min_neighbors == 1, text
    o, text = capi.cli_read_arguments(BASE + CLOUD + ["--pointCloudOutlierRadius", "0.25"])
    assert o is not None and o.point_cloud_outlier_radius == 0.25 and o.point_cloud_min_neighbors == 1, text
    o, text = capi.cli_read_arguments(BASE + CLOUD + ["--pointCloudOutlierRadius", "1e-3", "--pointCloudMinNeighbors", "0", "--pointCloudCellSize",
                                                      "0.5", "--pointCloudMinCellPoints", "4"])
    assert o is not None and o.point_cloud_outlier_radius == 1e-3 and o.point_cloud_min_neighbors == 0, text
    assert o.point_cloud_cell_size == 0.5 and o.point_cloud_min_cell_points == 4   # the fields in front of the new ones stand where they stood


def test_the_flags_refusals_say_why():
    o, text = capi.cli_read_arguments(BASE + ["--pointCloudOutlierRadius", "0.1"])
    assert o is None and text.startswith("Error : --pointCloudOutlierRadius needs --outputPointCloudFilename"), text
    o, text = capi.cli_read_arguments(BASE + CLOUD + ["--pointCloudMinNeighbors", "2"])
    assert o is None and text.startswith("Error : --pointCloudMinNeighbors needs --pointCloudOutlierRadius"), text
    for value in ("0", "-1", "nan", "inf", "x", "1e-200", "1e200"):
        o, text = capi.cli_read_arguments(BASE + CLOUD + ["--pointCloudOutlierRadius", value])
        assert o is None and "--pointCloudOutlierRadius" in text.split("\n")[0], (value, text[:200])
    for value in ("-2", "1.5", str(2 ** 31)):
        o, text = capi.cli_read_arguments(BASE + CLOUD + ["--pointCloudOutlierRadius", "0.1", "--pointCloudMinNeighbors", value])
        assert o is None and "--pointCloudMinNeighbors" in text.split("\n")[0], (value, text[:200])


def test_help_names_the_flags_and_the_array():
    o, text = capi.cli_read_arguments(BASE + ["--help"])
    text = " ".join(text.split())
    assert o is None and "--pointCloudOutlierRadius" in text and "--pointCloudMinNeighbors" in text and "NbNeighbors" in text
    assert "before --pointCloudCellSize" in text
