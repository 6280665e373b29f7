"""Kernel time of dmi_extract_isosurface on the cfg-3 speckle scene (512^3, 256 views of 1280 x 720, as bench.py --full builds
it), next to the HBM floor of reading the point lattice.  Prints one JSON line.  With --normals it times
dmi_extract_isosurface_normals too, the two calls alternating in the same process (kernel_ms / normals_kernel_ms).

    python tools/gpu_isosurface_time.py [--iso 1.0] [--views 256] [--repeat 5] [--normals]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cudadepthmapintegration_amd import capi, scene  # noqa: E402

HBM_TBPS = 8.0        # MI355X peak
C2P_TBPS = 4.7        # what the cell -> point pass achieves (profiles/NOTEBOOK.md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iso", type=float, default=1.0)
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--normals", action="store_true", help="also time the call with normals, alternating with the plain one")
    a = ap.parse_args()
    grid = scene.default_grid(512)
    ray = scene.default_ray_potential(grid)
    spacing = float(max(grid.spacing))
    with capi.FusionContext(grid, ray) as ctx:
        for c0 in range(0, a.views, 32):
            v, thr = scene.make_scene_views("speckle", 256, 1280, 720, seed=1000, view_range=(c0, min(a.views, c0 + 32)),
                                            noise_sigma=spacing)
            ctx.add_views(v, threshold=thr)
        ctx.fuse()
        ctx.cell_to_point()
        nv, nt = 0, 0
        verts, tris = ctx.extract_isosurface(a.iso)      # warm-up: buffers sized, code loaded
        if a.normals:
            ctx.extract_isosurface_with_normals(a.iso)
        times, ntimes = [], []
        for _ in range(a.repeat):
            verts, tris = ctx.extract_isosurface(a.iso)
            times.append(ctx.isosurface_kernel_ms())
            if a.normals:
                ctx.extract_isosurface_with_normals(a.iso)
                ntimes.append(ctx.isosurface_kernel_ms())
        nv, nt = len(verts), len(tris)
    n_points = 513 ** 3
    lattice = n_points * 8
    out = {"iso": a.iso, "views": a.views, "vertices": nv, "triangles": nt, "kernel_ms": times, "kernel_ms_min": min(times),
           "lattice_bytes": lattice, "mesh_bytes": nv * 24 + nt * 24,
           "floor_ms_8tbps": lattice / HBM_TBPS / 1e9, "floor_ms_c2p_rate": lattice / C2P_TBPS / 1e9,
           "two_reads_floor_ms_8tbps": 2 * lattice / HBM_TBPS / 1e9}
    if a.normals:
        out.update({"normals_kernel_ms": ntimes, "normals_kernel_ms_min": min(ntimes), "normals_bytes": nv * 12,
                    "normals_over_plain_min": min(ntimes) / min(times)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
