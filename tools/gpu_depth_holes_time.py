"""Time of dmi_fill_depth_holes beside dmi_filter_depth_speckles on the same input, and what the fill does to the fusion.  Prints one
JSON line.  Meant to be run under a time limit of its own:

    timeout -k 10 600 python tools/gpu_depth_holes_time.py --views 64 --width 640 --height 480 --scene speckle [--repeat 3]
                                                           [--max-pixels 16 256] [--rel-tolerance 0.01] [--fusion 512]

--scene   speckle  scene.make_scene_views("speckle"): 10 % of the pixels invalid by their best cost, scattered
          blobs    scene.make_scene_views("blobs"): discs of 8-40 pixels radius without a depth
Per --max-pixels value: the kernels' hipEvent time of the whole call (best of --repeat after a warm-up call), the share of the
invalid pixels that were filled, and the holes.  Beside them the speckle filter's time on the same input in the same process: the
same labelling on the complement, so it is the yardstick.  In a tuning build of the library (DMI_TUNING=1 in the environment of
both the build and this tool) the time per pass is reported for both.
--fusion N additionally fuses the views into an N^3 grid (scene.default_grid) before and after the fill with the first
--max-pixels value, in this one process and alternating: the fusion's kernel time (dmi_timings.last_fuse_kernel_ms, best of
--repeat after a warm-up each) for the unfilled and for the filled views.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from cudadepthmapintegration_amd import capi, scene  # noqa: E402

HOLES_PASSES = ("local", "border", "merge", "output")
SPECKLE_PASSES = ("local", "border", "sizes", "output")


def timed(fn, tuning, getter, names, repeat):
    best, best_passes, result = None, None, None
    for r in range(repeat + 1):                        # call 0 is the warm-up: code loaded, the host pages touched
        result = fn()
        ms = result[2]
        if r and (best is None or ms < best):
            best = ms
            if tuning is not None:
                passes = (ctypes.c_double * 4)()
                getattr(tuning, getter)(passes)
                best_passes = dict(zip(names, (float(x) for x in passes)))
    return best, best_passes, result


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
    p.add_argument("--scene", choices=("speckle", "blobs"), default="speckle")
    p.add_argument("--repeat", type=int, default=3)
    p.add_argument("--max-pixels", type=int, nargs="+", default=[16, 256])
    p.add_argument("--abs-tolerance", type=float, default=0.0)
    p.add_argument("--rel-tolerance", type=float, default=0.01)
    p.add_argument("--speckle-min-pixels", type=int, default=50)
    p.add_argument("--fusion", type=int, default=0)
    a = p.parse_args()
    n, W, H = a.views, a.width, a.height
    rec = {"views": n, "width": W, "height": H, "scene": a.scene, "pixels": n * W * H, "abs_tolerance": a.abs_tolerance,
           "rel_tolerance": a.rel_tolerance, "tuning_build": bool(os.environ.get("DMI_TUNING"))}
    L = capi.load()
    tuning = ctypes.CDLL(L._name) if rec["tuning_build"] else None
    print("making the scene ...", file=sys.stderr, flush=True)
    views, threshold = scene.make_scene_views(a.scene, n, W, H, seed=1)
    # thresholded once on the host: both filters and the fusion then take the same plain depths
    depth = np.ascontiguousarray(views.depth, dtype=np.float64)
    if views.best_cost is not None and threshold is not None:
        depth[np.asarray(views.best_cost) > threshold] = -1.0
    plain = scene.Views(depth, views.K4, views.RT4, None)
    invalid = ~((depth > 0) & (depth < np.inf))
    rec["invalid_share"] = float(invalid.mean())

    print("speckle filter ...", file=sys.stderr, flush=True)
    ms, passes, _ = timed(lambda: capi.filter_depth_speckles(plain, min_pixels=a.speckle_min_pixels, abs_tolerance=a.abs_tolerance,
                                                             rel_tolerance=a.rel_tolerance),
                          tuning, "dmi_tuning_depth_speckle_pass_ms", SPECKLE_PASSES, a.repeat)
    rec["speckle_filter"] = {"min_pixels": a.speckle_min_pixels, "kernel_ms": ms, "pass_ms": passes}

    rec["fill"] = []
    filled_views = None
    for max_pixels in a.max_pixels:
        print(f"fill, max_pixels {max_pixels} ...", file=sys.stderr, flush=True)
        ms, passes, (out, sizes, _) = timed(lambda: capi.fill_depth_holes(plain, max_pixels=max_pixels, abs_tolerance=a.abs_tolerance,
                                                                          rel_tolerance=a.rel_tolerance),
                                            tuning, "dmi_tuning_depth_holes_pass_ms", HOLES_PASSES, a.repeat)
        filled = invalid & (out.depth != -1.0)
        counts = np.bincount(sizes[sizes > 0].ravel())
        holes = int(sum(c // s for s, c in enumerate(counts) if s))
        rec["fill"].append({"max_pixels": max_pixels, "kernel_ms": ms, "pass_ms": passes,
                            "ratio_to_speckle_filter": ms / rec["speckle_filter"]["kernel_ms"],
                            "filled_share_of_invalid": float(filled.sum() / max(1, invalid.sum())),
                            "invalid_share_after": float((invalid & ~filled).mean()), "holes": holes, "largest_hole": int(sizes.max())})
        if filled_views is None:
            filled_views = out

    if a.fusion:
        print("fusion ...", file=sys.stderr, flush=True)
        grid = scene.default_grid(a.fusion)
        ray = scene.default_ray_potential(grid)
        with capi.FusionContext(grid, ray, count_hits=False) as ctx:
            before, after = [], []
            for _ in range(2):                         # alternating: each side is timed in two separate rounds
                before.append(fusion_ms(ctx, plain, a.repeat))
                after.append(fusion_ms(ctx, filled_views, a.repeat))
        rec["fusion"] = {"grid": a.fusion, "max_pixels": a.max_pixels[0], "kernel_ms_unfilled": min(before), "kernel_ms_filled": min(after),
                         "rounds_unfilled": before, "rounds_filled": after}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
