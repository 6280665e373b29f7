"""bench.py's plain single-GPU run and --dump-outputs, on a workload of seconds: the result line holds the headline fields and
none of the measurements --full adds, --steps sets the timed steps, and the dumped grid is the one the path fuses from the same
views in this process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOAD = "64x4@320x240"   # 64^3 cells (fewer voxels than bench.DUMP_SAMPLES: the whole grid is dumped), 4 views


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_grid(tmp_path):
    out_dir = tmp_path / "dump"
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--workload", WORKLOAD, "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == d["unit"] == "Gvoxel-projections/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    for key in ("scenes", "roofline_valu", "ablation", "box_state", "cell_to_point", "end_to_end", "coloration", "cpu_baseline"):
        assert key not in d, key

    files = sorted(os.listdir(out_dir))
    assert files == ["grid_sample.npy", "grid_sample_index.npy", "grid_summary.npy"], files
    assert sum(os.path.getsize(out_dir / f) for f in files) <= 64 << 20
    sample = np.load(out_dir / "grid_sample.npy")
    index = np.load(out_dir / "grid_sample_index.npy")
    summary = np.load(out_dir / "grid_summary.npy")
    assert sample.dtype == np.float32 and index.dtype == summary.dtype == np.float64

    import bench
    from cudadepthmapintegration_amd import capi, scene

    cells, maps, w, h = bench.parse_workload(WORKLOAD)
    grid = scene.default_grid(cells)
    ray = scene.default_ray_potential(grid)
    with capi.FusionContext(grid, ray, grid_dtype="f32", depth_storage="auto") as ctx:
        bench.upload_scene(ctx, scene, "speckle", maps, w, h, float(max(grid.spacing)))
        ctx.fuse()
        want = ctx.download_grid(np.float32).reshape(-1).copy()
    assert np.array_equal(index, np.arange(want.size, dtype=np.float64))
    assert np.array_equal(sample.view(np.uint32), want.view(np.uint32)), "dumped grid differs from the path's fusion"
    assert summary[0] == want.size and summary[5] == np.count_nonzero(want) > 0
    assert summary[3] == want.min() and summary[4] == want.max()
