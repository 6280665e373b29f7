"""Time of dmi_filter_depth_speckles, sizes and scene from the arguments.  Prints one JSON line: the kernels' hipEvent time of the
whole call (best of --repeat after a warm-up call), the achieved bytes per second over the algorithmic bytes (8 B of depth in, 8 B
out, 4 B of sizes when asked for, 8 B of costs when given), its ratio to the rate the fusion's own upload kernel reaches on its
bytes (3.7 TB/s), the whole call's wall time and the share of it that is not kernels.  Meant to be run under a time
limit of its own:

    timeout -k 10 600 python tools/gpu_depth_speckle_time.py --views 64 --width 640 --height 480 --scene dense [--repeat 3]
                                                             [--min-pixels 50] [--rel-tolerance 0.01] [--no-sizes] [--costs] [--check]

--scene  dense       the sphere scene, every pixel holds a depth (scene.make_views, dense)
         speckle     the same with 10 % of the pixels invalid, scattered: many tiny segments
         serpentine  a one-pixel-wide path through every second row of every view: the union-find's worst case
--check first runs a scene of --check-views views at a quarter of the width and height through the library and through the numpy
restatement (tests/depth_speckle_np.py) and records whether the two are identical.

In a tuning build of the library (DMI_TUNING=1 in the environment of both the build and this tool) the time per pass is reported
too, and --sweep times the variants the default build has decided between, alternating in this one process: tiles of 64 x 16,
64 x 32 and 64 x 64, and runs against per-pixel hooks in the local pass; the results of all variants must be identical.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from cudadepthmapintegration_amd import capi, scene  # noqa: E402

UPLOAD_KERNEL_BYTES_PER_SECOND = 3.7e12   # what upload_views_kernel reaches on its bytes
PASSES = ("local", "border", "sizes", "output")


def make_scene(a):
    n, W, H = a.views, a.width, a.height
    if a.scene == "serpentine":
        valid = np.zeros((H, W), dtype=bool)
        valid[0::2, :] = True
        for y in range(0, H - 2, 2):
            valid[y + 1, W - 1 if (y // 2) % 2 == 0 else 0] = True
        depth = np.broadcast_to(np.where(valid, 2.0, -1.0), (n, H, W)).copy()
        eye = np.tile(np.eye(4), (n, 1, 1))
        return scene.Views(depth, eye, eye, None)
    views = scene.make_views(n, W, H, seed=1, dense=True)
    if a.scene == "speckle":
        views.depth[np.random.default_rng(2).random(views.depth.shape) < 0.10] = -1.0
    return views


def call(L, depth, cost, a, out, sizes):
    dp = lambda x: None if x is None else x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    n, H, W = depth.shape
    ms = ctypes.c_double(0.0)
    rc = L.dmi_filter_depth_speckles(dp(depth), dp(cost), 0.5, n, W, H, a.abs_tolerance, a.rel_tolerance, a.min_pixels, 0, dp(out),
                                     None if sizes is None else sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(ms))
    if rc != 0:
        raise SystemExit("dmi_filter_depth_speckles: " + L.dmi_last_error(None).decode())
    return float(ms.value)


def timed(L, tuning, depth, cost, a, out, sizes):
    best_kernel, best_wall, best_passes = None, None, None
    for r in range(a.repeat + 1):                      # call 0 is the warm-up: code loaded, the host pages touched
        t0 = time.perf_counter()
        ms = call(L, depth, cost, a, out, sizes)
        wall = (time.perf_counter() - t0) * 1e3
        if r and (best_kernel is None or ms < best_kernel):
            best_kernel = ms
            if tuning is not None:
                passes = (ctypes.c_double * 4)()
                tuning.dmi_tuning_depth_speckle_pass_ms(passes)
                best_passes = dict(zip(PASSES, (float(x) for x in passes)))
        if r and (best_wall is None or wall < best_wall):
            best_wall = wall
    return best_kernel, best_wall, best_passes


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--views", type=int, default=64)
    p.add_argument("--width", type=int, default=640)
    p.add_argument("--height", type=int, default=480)
    p.add_argument("--scene", choices=("dense", "speckle", "serpentine"), default="dense")
    p.add_argument("--repeat", type=int, default=3)
    p.add_argument("--min-pixels", type=int, default=50)
    p.add_argument("--abs-tolerance", type=float, default=0.0)
    p.add_argument("--rel-tolerance", type=float, default=0.01)
    p.add_argument("--no-sizes", action="store_true")
    p.add_argument("--costs", action="store_true")
    p.add_argument("--check", action="store_true")
    p.add_argument("--check-views", type=int, default=4)
    p.add_argument("--sweep", action="store_true")
    a = p.parse_args()
    n, W, H = a.views, a.width, a.height
    bytes_per_pixel = 16 + (0 if a.no_sizes else 4) + (8 if a.costs else 0)
    rec = {"views": n, "width": W, "height": H, "scene": a.scene, "pixels": n * W * H, "min_pixels": a.min_pixels,
           "abs_tolerance": a.abs_tolerance, "rel_tolerance": a.rel_tolerance, "sizes": not a.no_sizes, "costs": a.costs,
           "algorithmic_bytes": n * W * H * bytes_per_pixel, "tuning_build": bool(os.environ.get("DMI_TUNING"))}
    L = capi.load()
    tuning = ctypes.CDLL(L._name) if rec["tuning_build"] else None
    if a.check:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import depth_speckle_np as S
        b = argparse.Namespace(**vars(a))
        b.views, b.width, b.height = a.check_views, max(W // 4, 8), max(H // 4, 8)
        small = make_scene(b).depth
        got, got_sizes = np.empty_like(small), np.zeros(small.shape, dtype=np.int32)
        call(L, small, None, a, got, got_sizes)
        want, want_sizes = S.filter_depth_speckles(small, a.min_pixels, a.abs_tolerance, a.rel_tolerance)
        rec["check_identical"] = bool(got.tobytes() == want.tobytes() and np.array_equal(got_sizes, want_sizes))
    depth = np.ascontiguousarray(make_scene(a).depth)
    cost = np.random.default_rng(3).random(depth.shape) * 0.5 if a.costs else None     # (none above the threshold of 0.5)
    out = np.empty_like(depth)
    sizes = None if a.no_sizes else np.zeros(depth.shape, dtype=np.int32)
    kernel_ms, wall_ms, passes = timed(L, tuning, depth, cost, a, out, sizes)
    rate = rec["algorithmic_bytes"] / (kernel_ms * 1e-3)
    rec.update({"kernel_ms": kernel_ms, "call_ms": wall_ms, "bytes_per_second": rate,
                "ratio_to_upload_kernel": rate / UPLOAD_KERNEL_BYTES_PER_SECOND, "transfer_share_of_call": 1.0 - kernel_ms / wall_ms,
                "kept_share": float((out > 0).mean()), "valid_share": float((depth > 0).mean())})
    if sizes is not None:
        rec["largest_segment"] = int(sizes.max())
    if passes is not None:
        rec["pass_ms"] = passes
    if a.sweep:
        if tuning is None:
            raise SystemExit("--sweep needs a tuning build: DMI_TUNING=1 in the environment of the build and of this tool")
        rec["sweep"], identical = {}, True
        other, other_sizes = np.empty_like(depth), None if sizes is None else np.zeros_like(sizes)
        for round_ in range(2):                        # the variants alternate: each is timed in two separate rounds
            for tile_height, runs in ((16, 1), (32, 1), (64, 1), (32, 0)):
                os.environ["DMI_DS_TILE_HEIGHT"], os.environ["DMI_DS_RUNS"] = str(tile_height), str(runs)
                k, _, ps = timed(L, tuning, depth, cost, a, other, other_sizes)
                key = f"tile64x{tile_height}_{'runs' if runs else 'pixels'}"
                if key not in rec["sweep"] or k < rec["sweep"][key]["kernel_ms"]:
                    rec["sweep"][key] = {"kernel_ms": k, "pass_ms": ps}
                identical = identical and other.tobytes() == out.tobytes() and (sizes is None or np.array_equal(other_sizes, sizes))
        del os.environ["DMI_DS_TILE_HEIGHT"], os.environ["DMI_DS_RUNS"]
        rec["sweep_results_identical"] = bool(identical)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
