"""Time of dmi_smooth_depths beside dmi_filter_depth_speckles on the same input, and what the smoothing does to the fusion.  Prints
one JSON line.  Meant to be run under a time limit of its own:

    timeout -k 10 600 python tools/gpu_depth_smooth_time.py --views 64 --width 640 --height 480 [--repeat 3]
                                                            [--sigma 1.5 4] [--truncate 2] [--iterations 1] [--rms] [--fusion 512]

The input is scene.make_scene_views("noisy"): 10 % of the pixels invalid by their best cost, depth noise of one voxel spacing of
the --grid grid (default 512, the headline's), discs without a depth.  Per --sigma value: the kernels' hipEvent time of the whole
call (best of --repeat after a warm-up call), the radius, the taps taken per valid pixel, the share of the valid pixels that
moved, and with --rms the RMS error against the noise-free scene before and after.  The tolerance is --tolerance-spacings voxel spacings
(default 3), the relative tolerance 0.  Beside them the speckle filter's time on the same input in the same process: the yardstick
of the depth-map stage.
--fusion N additionally fuses the views into an N^3 grid (scene.default_grid) before and after the smoothing with the first
--sigma value, in this one process and alternating: the fusion's kernel time (dmi_timings.last_fuse_kernel_ms, best of --repeat
after a warm-up each) and the iso-surface's vertex and triangle counts for the unsmoothed and for the smoothed views.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from cudadepthmapintegration_amd import capi, scene  # noqa: E402


def timed(fn, repeat):
    best, result = None, None
    for r in range(repeat + 1):                        # call 0 is the warm-up: code loaded, the host pages touched
        result = fn()
        ms = result[2]
        if r and (best is None or ms < best):
            best = ms
    return best, result


def fusion_ms(ctx, views, repeat):
    ctx.clear_views()
    ctx.add_views(views, None)
    best = None
    for r in range(repeat + 1):
        ctx.reset_grid()
        ctx.fuse()
        ms = float(ctx.timings().last_fuse_kernel_ms)
        if r and (best is None or ms < best):
            best = ms
    return best


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--views", type=int, default=64)
    p.add_argument("--width", type=int, default=640)
    p.add_argument("--height", type=int, default=480)
    p.add_argument("--grid", type=int, default=512)
    p.add_argument("--repeat", type=int, default=3)
    p.add_argument("--sigma", type=float, nargs="+", default=[1.5, 4.0])
    p.add_argument("--truncate", type=float, default=2.0)
    p.add_argument("--iterations", type=int, default=1)
    p.add_argument("--tolerance-spacings", type=float, default=3.0)
    p.add_argument("--speckle-min-pixels", type=int, default=50)
    p.add_argument("--speckle-rel-tolerance", type=float, default=0.01)
    p.add_argument("--rms", action="store_true")
    p.add_argument("--fusion", type=int, default=0)
    p.add_argument("--iso", type=float, default=1.0)
    a = p.parse_args()
    n, W, H = a.views, a.width, a.height
    spacing = float(scene.default_grid(a.grid).spacing[0])
    tolerance = a.tolerance_spacings * spacing
    rec = {"views": n, "width": W, "height": H, "scene": "noisy", "pixels": n * W * H, "noise_sigma": spacing, "abs_tolerance": tolerance,
           "rel_tolerance": 0.0, "truncate": a.truncate, "iterations": a.iterations}
    capi.load()
    print("making the scene ...", file=sys.stderr, flush=True)
    views, threshold = scene.make_scene_views("noisy", n, W, H, seed=1, noise_sigma=spacing)
    # thresholded once on the host: both filters and the fusion then take the same plain depths
    depth = np.ascontiguousarray(views.depth, dtype=np.float64)
    depth[np.asarray(views.best_cost) > threshold] = -1.0
    plain = scene.Views(depth, views.K4, views.RT4, None)
    valid = (depth > 0) & (depth < np.inf)
    rec["valid_share"] = float(valid.mean())
    rms = lambda d: None
    if a.rms:                                          # (the scene a second time, without its noise)
        truth = np.asarray(scene.make_scene_views("noisy", n, W, H, seed=1, noise_sigma=0.0)[0].depth, dtype=np.float64)[valid]
        rms = lambda d: float(np.sqrt(np.mean((d[valid] - truth) ** 2)))
    rec["rms_unsmoothed"] = rms(depth)

    print("speckle filter ...", file=sys.stderr, flush=True)
    ms, _ = timed(lambda: capi.filter_depth_speckles(plain, min_pixels=a.speckle_min_pixels, abs_tolerance=0.0,
                                                     rel_tolerance=a.speckle_rel_tolerance), a.repeat)
    rec["speckle_filter"] = {"min_pixels": a.speckle_min_pixels, "kernel_ms": ms}

    rec["smooth"] = []
    smoothed_views = None
    for sigma in a.sigma:
        radius = len(capi.depth_smoothing_weights(sigma, a.truncate)) - 1
        print(f"smooth, sigma {sigma} (radius {radius}) ...", file=sys.stderr, flush=True)
        ms, (out, counts, _) = timed(lambda: capi.smooth_depths(plain, sigma=sigma, truncate=a.truncate, abs_tolerance=tolerance,
                                                                 rel_tolerance=0.0, iterations=a.iterations), a.repeat)
        taps = float(counts.sum(dtype=np.int64) / max(1, valid.sum()))
        rec["smooth"].append({"sigma": sigma, "radius": radius, "kernel_ms": ms, "ratio_to_speckle_filter": ms / rec["speckle_filter"]["kernel_ms"],
                              "window_taps": (2 * radius + 1) ** 2, "taps_taken_per_valid_pixel": taps,
                              "ns_per_pixel_and_window_tap": 1e6 * ms / (n * W * H * (2 * radius + 1) ** 2 * a.iterations),
                              "moved_share_of_valid": float((out.depth[valid] != depth[valid]).mean()), "rms_smoothed": rms(out.depth),
                              "validity_unchanged": bool(np.array_equal(out.depth != -1.0, valid))})
        if smoothed_views is None:
            smoothed_views = out

    if a.fusion:
        print("fusion ...", file=sys.stderr, flush=True)
        grid = scene.default_grid(a.fusion)
        ray = scene.default_ray_potential(grid)
        with capi.FusionContext(grid, ray, count_hits=False) as ctx:
            before, after, mesh = [], [], {}
            for _ in range(2):                         # alternating: each side is timed in two separate rounds
                before.append(fusion_ms(ctx, plain, a.repeat))
                verts, tris = ctx.extract_isosurface(a.iso)
                mesh["unsmoothed"] = {"vertices": int(len(verts)), "triangles": int(len(tris))}
                after.append(fusion_ms(ctx, smoothed_views, a.repeat))
                verts, tris = ctx.extract_isosurface(a.iso)
                mesh["smoothed"] = {"vertices": int(len(verts)), "triangles": int(len(tris))}
        rec["fusion"] = {"grid": a.fusion, "sigma": a.sigma[0], "iso": a.iso, "kernel_ms_unsmoothed": min(before), "kernel_ms_smoothed": min(after),
                         "rounds_unsmoothed": before, "rounds_smoothed": after, "mesh": mesh}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
