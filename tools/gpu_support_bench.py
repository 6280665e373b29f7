"""Kernel time of the support pass (dmi_filter_isosurface_support) next to the coloration of the same mesh from the same views with
the fused depth test (dmi_color_process_isosurface), in one process: the bench's cfg-2 scene (256^3, 64 views of 640 x 480,
speckle, as bench.py builds it) fused, its iso-surface extracted with normals, then
  - the counts-only pass (min_views 0), dmi_get_isosurface_support_kernel_ms: median of --repeat after a warm-up;
  - the colouring with the fused test at the same tolerance, dmi_get_isosurface_color_kernel_ms, alternating with it;
  - one min_views = 1 trim after a fresh extraction, pass by pass (median of --repeat).
The support pass does strictly less per (vertex, view) pair than the colouring -- no colour gather, no scratch table, no median --
so its kernel time is expected below the colouring's.  Prints one JSON line.

    python tools/gpu_support_bench.py [--iso 0.0] [--tolerance-spacings 2] [--repeat 5] [--workload cfg2] [--no-facing]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cudadepthmapintegration_amd import capi, scene  # noqa: E402

WORKLOADS = {"cfg1": (64, 4, 320, 240), "cfg2": (256, 64, 640, 480)}  # bench.py's: cells per axis, views, W, H
SCENE_SEED = 1000                                                     # bench.py's


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iso", type=float, default=0.0)
    ap.add_argument("--tolerance-spacings", type=float, default=2.0, help="the depth tolerance in grid spacings")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--workload", default="cfg2", choices=list(WORKLOADS))
    ap.add_argument("--no-facing", action="store_true")
    a = ap.parse_args()
    cells, n, W, H = WORKLOADS[a.workload]
    grid = scene.default_grid(cells)
    ray = scene.default_ray_potential(grid)
    spacing = float(max(grid.spacing))
    tol = a.tolerance_spacings * spacing
    facing = not a.no_facing
    with capi.FusionContext(grid, ray) as ctx, capi.ColorContext() as colors:
        for c0 in range(0, n, 32):
            v, thr = scene.make_scene_views("speckle", n, W, H, seed=SCENE_SEED, view_range=(c0, min(n, c0 + 32)), noise_sigma=spacing)
            ctx.add_views(v, threshold=thr)
            colors.add_views(scene.make_colors(v.n, W, H, seed=2000 + c0), v.K4, v.RT4)
        ctx.fuse()
        ctx.synchronize()
        verts, tris, _ = ctx.extract_isosurface_with_normals(a.iso)
        nv, nt = len(verts), len(tris)
        del verts, tris
        support_ms, color_ms = [], []
        for r in range(a.repeat + 1):                   # round 0 is the warm-up: buffers sized, code loaded
            ctx.filter_isosurface_support(0, tol, facing)
            s = ctx.isosurface_support_kernel_ms()
            ctx.color_isosurface(colors, fused_depth_tolerance=tol)
            c = ctx.isosurface_color_kernel_ms()
            if r:
                support_ms.append(s)
                color_ms.append(c)
        counts = ctx.download_isosurface_support()
        histogram = [int(x) for x in np.bincount(counts, minlength=1)[:16]]
        trim_ms, trim_pass, left = [], [], (nv, nt)
        for r in range(a.repeat + 1):
            ctx.extract_isosurface_with_normals(a.iso)
            left = ctx.filter_isosurface_support(1, tol, facing)
            if r:
                trim_ms.append(ctx.isosurface_support_kernel_ms())
                trim_pass.append(ctx.isosurface_support_pass_ms())
    med = statistics.median
    out = {"workload": a.workload, "iso": a.iso, "views": n, "vertices": nv, "triangles": nt, "tolerance": tol, "facing": facing,
           "support_kernel_ms": support_ms, "support_kernel_ms_median": med(support_ms),
           "color_fused_kernel_ms": color_ms, "color_fused_kernel_ms_median": med(color_ms),
           "support_over_color": med(support_ms) / med(color_ms),
           "pairs_per_ns": nv * n / (med(support_ms) * 1e6),
           "support_histogram_first_16": histogram,
           "trim_min_views_1": {"vertices_left": left[0], "triangles_left": left[1], "kernel_ms": trim_ms, "kernel_ms_median": med(trim_ms),
                                "pass_ms_median": {k: med([p[k] for p in trim_pass]) for k in ("counts", "scans", "compaction")}}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
