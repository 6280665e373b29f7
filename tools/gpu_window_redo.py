#!/usr/bin/env python3
"""How many wave-voxels does the window column send to its redo loop?  A tuning build (DMI_TUNING=1 python -m
cudadepthmapintegration_amd.build) counts, per launch, the window pairs executed and the redo iterations after their columns in
two 64-bit counters behind TileArgs::wg_times (one lane per wave adds at the end of a brick).  Prints one JSON line.

    DMI_DEBUG_WG_TIMES=1 DMI_LIB_OVERRIDE=cudadepthmapintegration_amd/csrc/libdmi_hip_tuning.so python tools/gpu_window_redo.py --scene speckle
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import parse_workload, upload_scene  # noqa: E402
from cudadepthmapintegration_amd import capi, scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg3")
    ap.add_argument("--scene", default="speckle")
    ap.add_argument("--variant", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the record to this JSON file")
    args = ap.parse_args()
    assert os.environ.get("DMI_DEBUG_WG_TIMES"), "set DMI_DEBUG_WG_TIMES=1 (and load the tuning build)"
    lib = capi.load()
    lib.dmi_debug_window_counts.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    cells, n_maps, W, H = parse_workload(args.workload)
    grid = scene.default_grid(cells)
    ray = scene.default_ray_potential(grid)
    with capi.FusionContext(grid, ray, grid_dtype="f32", kernel_variant=args.variant) as ctx:
        upload_scene(ctx, scene, args.scene, n_maps, W, H, float(max(grid.spacing)))
        ctx.reset_grid()
        ctx.fuse()
        ctx.synchronize()
        out = (ctypes.c_uint64 * 2)()
        rc = lib.dmi_debug_window_counts(ctx._h, out)
        assert rc == 0
        pairs_by_table = ctx.window_pair_count()
    pairs, redo = int(out[0]), int(out[1])
    rec = {"workload": args.workload, "scene": args.scene, "variant": args.variant, "library": os.environ.get("DMI_LIB_OVERRIDE"),
           "window_pairs_executed": pairs, "window_pairs_in_table": pairs_by_table, "redo_wave_voxels": redo,
           "redo_per_window_pair": redo / max(1, pairs)}
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
