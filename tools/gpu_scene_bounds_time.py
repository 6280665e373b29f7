"""Time of dmi_estimate_scene_bounds on the sphere scene (scene.make_views, dense: every pixel holds a depth), sizes from the
arguments.  Prints one JSON line per configuration: over --rounds rounds (after a warm-up call) the minimum and maximum of the
kernels' hipEvent time (the upload pass and the select passes) and of the whole call's wall time, the staging time beside it (the
call minus its kernels), the number of select passes and passes x the bytes of the taking-part pixels / kernel time as an effective
bandwidth.  Meant to be run under a time limit of its own:

    timeout -k 10 600 python tools/gpu_scene_bounds_time.py --views 64 --width 640 --height 480 [--rounds 5]
                                                             [--trim 0.005] [--pixel-step 1] [--compare] [--check]

--compare also times pixel_step 4 against 1 and trim 0 against the given trim.  --check first runs a scene of --check-views views
at a quarter of the size through the library and through the numpy restatement (tests/scene_bounds_np.py) and records whether the
two are identical.

In a tuning build of the library (DMI_TUNING=1 in the environment of both the build and this tool) the record also holds the select
passes alone and the yardstick: a plain read of the same resident planes by a one-line reduction kernel, timed in the same process,
and, at pixel step 1, the ratio of one select pass to it; --sweep then times the variants the default build has decided between:
the wave-aggregated LDS add switched off and with more rounds than the default's one, and a histogram per target even while an
axis's two prefixes are equal.
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

PASSES = 8  # csrc/scene_bounds_rules.h: kPasses, digits of 8 bits


def timed(views, rounds, trim, step, tuning=None):
    kernel, wall, select, read, result = [], [], [], [], None
    for r in range(rounds + 1):                        # call 0 is the warm-up: code loaded, the host pages touched
        t0 = time.perf_counter()
        lo, hi, n_points, ms = capi.estimate_scene_bounds(views, trim_fraction=trim, pixel_step=step)
        if r:
            wall.append((time.perf_counter() - t0) * 1e3)
            kernel.append(ms)
            if tuning is not None:
                select.append(tuning.dmi_tuning_scene_bounds_select_ms())
                read.append(tuning.dmi_tuning_scene_bounds_plain_read_ms())
        result = (lo.tolist(), hi.tolist(), n_points)
    plane_bytes = views.depth.size * 8
    n, H, W = views.depth.shape
    read_bytes = n * (-(-H // step)) * (-(-W // step)) * 8     # what a select pass reads: the taking-part pixels
    rec = {"trim": trim, "pixel_step": step, "n_points": result[2], "lo": result[0], "hi": result[1], "passes": PASSES,
           "kernel_ms": [min(kernel), max(kernel)], "call_ms": [min(wall), max(wall)],
           "staging_ms": [min(w - k for w, k in zip(wall, kernel)), max(w - k for w, k in zip(wall, kernel))],
           "pass_read_bytes": read_bytes,
           "effective_GBps": [PASSES * read_bytes / (max(kernel) * 1e-3) / 1e9, PASSES * read_bytes / (min(kernel) * 1e-3) / 1e9]}
    if tuning is not None:
        rec.update({"select_ms": [min(select), max(select)], "plain_read_ms": [min(read), max(read)],
                    "plain_read_GBps": [plane_bytes / (max(read) * 1e-3) / 1e9, plane_bytes / (min(read) * 1e-3) / 1e9]})
        if step == 1:                                  # the plain read visits every pixel: a yardstick for step 1 only
            rec["select_pass_over_plain_read"] = [min(select) / PASSES / max(read), max(select) / PASSES / min(read)]
    return rec


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--views", type=int, default=64)
    p.add_argument("--width", type=int, default=640)
    p.add_argument("--height", type=int, default=480)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--trim", type=float, default=0.005)
    p.add_argument("--pixel-step", type=int, default=1)
    p.add_argument("--compare", action="store_true")
    p.add_argument("--check", action="store_true")
    p.add_argument("--check-views", type=int, default=6)
    p.add_argument("--sweep", action="store_true")
    a = p.parse_args()
    n, W, H = a.views, a.width, a.height
    head = {"views": n, "width": W, "height": H, "plane_bytes": n * W * H * 8, "tuning_build": bool(os.environ.get("DMI_TUNING"))}
    tuning = None
    if head["tuning_build"]:
        tuning = ctypes.CDLL(capi.load()._name)
        tuning.dmi_tuning_scene_bounds_select_ms.restype = ctypes.c_double
        tuning.dmi_tuning_scene_bounds_plain_read_ms.restype = ctypes.c_double
    if a.check:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import scene_bounds_np as B
        small = scene.make_views(a.check_views, max(W // 4, 8), max(H // 4, 8), seed=1, dense=True)
        lo, hi, n_points, _ = capi.estimate_scene_bounds(small, trim_fraction=a.trim, pixel_step=a.pixel_step)
        want = B.estimate_scene_bounds(small.depth, small.K4, small.RT4, a.trim, a.pixel_step)
        head["check_identical"] = bool(lo.tobytes() == want[0].tobytes() and hi.tobytes() == want[1].tobytes() and n_points == want[2])
    views = scene.make_views(n, W, H, seed=1, dense=True)
    print(json.dumps(dict(head, **timed(views, a.rounds, a.trim, a.pixel_step, tuning))), flush=True)
    if a.compare:
        for trim, step in ((a.trim, 4), (0.0, a.pixel_step)):
            print(json.dumps(dict(head, **timed(views, a.rounds, trim, step, tuning))), flush=True)
    if a.sweep:
        if tuning is None:
            raise SystemExit("--sweep needs a tuning build: DMI_TUNING=1 in the environment of the build and of this tool")
        for name, env in (("aggregate_rounds_0", {"DMI_SB_AGGREGATE_ROUNDS": "0"}), ("aggregate_rounds_2", {"DMI_SB_AGGREGATE_ROUNDS": "2"}),
                          ("aggregate_rounds_4", {"DMI_SB_AGGREGATE_ROUNDS": "4"}), ("aggregate_rounds_64", {"DMI_SB_AGGREGATE_ROUNDS": "64"}),
                          ("histogram_per_target", {"DMI_SB_SHARE_HISTOGRAMS": "0"})):
            os.environ.update(env)
            print(json.dumps(dict(head, variant=name, **timed(views, a.rounds, a.trim, a.pixel_step, tuning))), flush=True)
            for k in env:
                del os.environ[k]


if __name__ == "__main__":
    main()
