"""Wall time of the depth-map chain through the context-free calls beside the same chain through a resident view set,
and of the hand-over to a fusion context beside dmi_add_views.  One process, prints one JSON line.  Meant to be run under a time
limit of its own:

    timeout -k 10 900 python tools/gpu_view_set_time.py --views 64 --width 640 --height 480 [--repeat 3]

The input is scene.make_scene_views("noisy"): 10 % of the pixels invalid by their best cost, scattered, depth noise of one voxel
spacing of the --grid grid (default 512, the headline's), discs without a depth; the host arrays are pinned.  The chain is speckle
filter -> hole fill -> smoothing -> consistency filter -> bounds estimate with the default tolerances of the stages' own timing
tools; the best costs go to the first step (the staged path) or to the add (the set).  Per path: the wall time of the whole chain
(a host clock round calls that synchronise; the median of --repeat after a warm-up), every step's kernel time as the call reports
it, and for the set the time of the report kernels with the bytes they read over it.  The two paths' depths are compared byte for
byte.  In a tuning build of the library (DMI_TUNING=1 in the environment of both the build and this tool) the record also holds
the yardstick of the bounds estimate: one plain read of the same planes.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from cudadepthmapintegration_amd import capi, scene  # noqa: E402

STEPS = ("speckles", "holes", "smooth", "consistency")


def pinned_copy(a):
    out = capi.pinned_empty(a.shape, a.dtype)
    out[...] = a
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--views", type=int, default=64)
    p.add_argument("--width", type=int, default=640)
    p.add_argument("--height", type=int, default=480)
    p.add_argument("--grid", type=int, default=512)
    p.add_argument("--repeat", type=int, default=3)
    p.add_argument("--fusion-grid", type=int, default=128)
    a = p.parse_args()
    n, W, H = a.views, a.width, a.height
    spacing = float(scene.default_grid(a.grid).spacing[0])
    params = {"speckles": dict(min_pixels=50, abs_tolerance=0.0, rel_tolerance=0.01),
              "holes": dict(max_pixels=16, abs_tolerance=0.0, rel_tolerance=0.01),
              "smooth": dict(sigma=1.5, truncate=2.0, abs_tolerance=3.0 * spacing, rel_tolerance=0.0, iterations=1),
              "consistency": dict(min_views=2, abs_tolerance=0.0, rel_tolerance=0.01)}
    bounds = dict(trim_fraction=0.005, pixel_step=1)
    pixels = n * W * H
    rec = {"views": n, "width": W, "height": H, "scene": "noisy", "pixels": pixels, "plane_bytes": pixels * 8, "params": params,
           "bounds": bounds, "repeat": a.repeat, "tuning_build": bool(os.environ.get("DMI_TUNING"))}
    lib = capi.load()
    print("making the scene ...", file=sys.stderr, flush=True)
    views, threshold = scene.make_scene_views("noisy", n, W, H, seed=1, noise_sigma=spacing)
    views = scene.Views(pinned_copy(np.ascontiguousarray(views.depth, dtype=np.float64)), views.K4, views.RT4,
                        pinned_copy(np.ascontiguousarray(views.best_cost, dtype=np.float64)))
    work = [capi.pinned_empty(views.depth.shape, np.float64) for _ in range(2)]
    calls = {"speckles": capi.filter_depth_speckles, "holes": capi.fill_depth_holes, "smooth": capi.smooth_depths,
             "consistency": capi.filter_depth_consistency}

    def staged_chain():
        ms, current = {}, views
        t0 = time.perf_counter()
        for k, name in enumerate(STEPS):
            extra = dict(threshold=threshold) if k == 0 else {}
            current, _, ms[name] = calls[name](current, out=work[k % 2], **params[name], **extra)
        ms["bounds"] = capi.estimate_scene_bounds(current, **bounds)[3]
        return 1e3 * (time.perf_counter() - t0), ms, current.depth

    def set_chain(s):
        ms, report_ms, reports = {}, {}, {}
        t0 = time.perf_counter()
        s.clear()
        s.add(views, threshold)
        added = time.perf_counter()
        for name in STEPS:
            method = {"speckles": s.filter_speckles, "holes": s.fill_holes, "smooth": s.smooth, "consistency": s.filter_consistency}[name]
            reports[name] = method(**params[name])
            ms[name] = reports[name].pop("kernel_ms")
            report_ms[name] = s.info().last_report_kernel_ms
        ms["bounds"] = s.estimate_bounds(**bounds)[3]
        done = time.perf_counter()
        return 1e3 * (done - t0), 1e3 * (added - t0), ms, report_ms, reports

    def median_of(samples):
        return {k: statistics.median(x[k] for x in samples) for k in samples[0]}

    print("the chain through the context-free calls ...", file=sys.stderr, flush=True)
    runs = [staged_chain() for _ in range(a.repeat + 1)][1:]          # run 0 is the warm-up: code loaded, the host pages touched
    staged_depth = runs[-1][2].copy()
    rec["staged"] = {"wall_ms": statistics.median(r[0] for r in runs), "kernel_ms": median_of([r[1] for r in runs])}
    if rec["tuning_build"]:
        tuning = ctypes.CDLL(lib._name)
        tuning.dmi_tuning_scene_bounds_plain_read_ms.restype = ctypes.c_double
        read_ms = float(tuning.dmi_tuning_scene_bounds_plain_read_ms())
        rec["plain_read"] = {"ms": read_ms, "GBps": pixels * 8 / read_ms / 1e6}

    print("the chain through the resident set ...", file=sys.stderr, flush=True)
    with capi.ViewSet(W, H) as s:
        runs = [set_chain(s) for _ in range(a.repeat + 1)][1:]
        report_ms = median_of([r[3] for r in runs])
        # what the report kernels read per pixel: the two planes; the label plane for the roots; the tap counts
        read_bytes = {"speckles": 20, "holes": 20, "smooth": 20, "consistency": 16}
        info = s.info()
        rec["set"] = {"wall_ms": statistics.median(r[0] for r in runs), "add_wall_ms": statistics.median(r[1] for r in runs),
                      "kernel_ms": median_of([r[2] for r in runs]), "report_kernel_ms": report_ms,
                      "report_GBps": {k: pixels * read_bytes[k] / report_ms[k] / 1e6 for k in report_ms}, "reports": runs[-1][4],
                      "device_bytes": int(info.device_bytes), "h2d_plane_bytes": int(info.h2d_plane_bytes),
                      "d2h_plane_bytes": int(info.d2h_plane_bytes)}
        rec["same_bytes"] = bool(s.download().tobytes() == staged_depth.tobytes())
        rec["wall_ratio_staged_over_set"] = rec["staged"]["wall_ms"] / rec["set"]["wall_ms"]

        print("the hand-over ...", file=sys.stderr, flush=True)
        grid = scene.default_grid(a.fusion_grid)
        host = scene.Views(pinned_copy(staged_depth), views.K4, views.RT4, None)
        with capi.FusionContext(grid, scene.default_ray_potential(grid)) as ctx:
            from_host, from_set = [], []
            for r in range(a.repeat + 1):                              # alternating; round 0 is the warm-up
                ctx.clear_views()
                t0 = time.perf_counter()
                ctx.add_views(host)
                t1 = time.perf_counter()
                ctx.clear_views()
                t2 = time.perf_counter()
                ctx.add_views_from_set(s)
                t3 = time.perf_counter()
                if r:
                    from_host.append(1e3 * (t1 - t0))
                    from_set.append(1e3 * (t3 - t2))
            rec["hand_over"] = {"add_views_pinned_wall_ms": statistics.median(from_host),
                                "add_views_from_set_wall_ms": statistics.median(from_set)}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
