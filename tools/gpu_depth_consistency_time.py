"""Time of dmi_filter_depth_consistency on the sphere scene (scene.make_views, dense: every pixel holds a depth), sizes from the
arguments.  Prints one JSON line: the kernels' hipEvent time (best of --repeat after a warm-up call), the (source pixel, target
view) pairs per second, the whole call's wall time and the share of it that is not kernels (staging up and down).  Meant to be
run under a time limit of its own:

    timeout -k 10 600 python tools/gpu_depth_consistency_time.py --views 64 --width 640 --height 480 [--repeat 3]
                                                                  [--min-views 2] [--rel-tolerance 0.01] [--check]

--check first runs a scene of --check-views views at a sixteenth of the size through the library and through the numpy restatement
(tests/depth_consistency_np.py) and records whether the two are identical.

In a tuning build of the library (DMI_TUNING=1 in the environment of both the build and this tool) --sweep also times the variants the
default build has decided between: the target views walked in groups of 16 and 64 per launch against all in one launch, and the
gather requested one view ahead against on demand; and it reports the share of pairs whose pixel the checked reciprocal left to the
exact division.
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


def timed(views, a, out):
    best_kernel, best_wall = None, None
    for r in range(a.repeat + 1):                      # call 0 is the warm-up: code loaded, the host pages touched
        t0 = time.perf_counter()
        _, counts, ms = capi.filter_depth_consistency(views, min_views=a.min_views, abs_tolerance=a.abs_tolerance,
                                                      rel_tolerance=a.rel_tolerance, out=out)
        wall = (time.perf_counter() - t0) * 1e3
        if r and (best_kernel is None or ms < best_kernel):
            best_kernel = ms
        if r and (best_wall is None or wall < best_wall):
            best_wall = wall
    return best_kernel, best_wall, counts


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--views", type=int, default=64)
    p.add_argument("--width", type=int, default=640)
    p.add_argument("--height", type=int, default=480)
    p.add_argument("--repeat", type=int, default=3)
    p.add_argument("--min-views", type=int, default=2)
    p.add_argument("--abs-tolerance", type=float, default=0.0)
    p.add_argument("--rel-tolerance", type=float, default=0.01)
    p.add_argument("--check", action="store_true")
    p.add_argument("--check-views", type=int, default=6)
    p.add_argument("--sweep", action="store_true")
    a = p.parse_args()
    n, W, H = a.views, a.width, a.height
    rec = {"views": n, "width": W, "height": H, "pairs": n * (n - 1) * W * H, "min_views": a.min_views,
           "abs_tolerance": a.abs_tolerance, "rel_tolerance": a.rel_tolerance, "tuning_build": bool(os.environ.get("DMI_TUNING"))}
    if a.check:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import depth_consistency_np as C
        small = scene.make_views(a.check_views, max(W // 4, 8), max(H // 4, 8), seed=1, dense=True)
        got, counts, _ = capi.filter_depth_consistency(small, min_views=a.min_views, abs_tolerance=a.abs_tolerance,
                                                       rel_tolerance=a.rel_tolerance)
        want, want_counts = C.filter_depth_consistency(small.depth, small.K4, small.RT4, a.min_views, a.abs_tolerance, a.rel_tolerance)
        rec["check_identical"] = bool(got.depth.tobytes() == want.tobytes() and np.array_equal(counts, want_counts))
    views = scene.make_views(n, W, H, seed=1, dense=True)
    out = np.empty_like(views.depth)
    kernel_ms, wall_ms, counts = timed(views, a, out)
    rec.update({"kernel_ms": kernel_ms, "call_ms": wall_ms, "pairs_per_second": rec["pairs"] / (kernel_ms * 1e-3),
                "transfer_share_of_call": 1.0 - kernel_ms / wall_ms, "kept_share": float((out > 0).mean()),
                "mean_count": float(counts.mean())})
    if a.sweep:
        if not rec["tuning_build"]:
            raise SystemExit("--sweep needs a tuning build: DMI_TUNING=1 in the environment of the build and of this tool")
        L = ctypes.CDLL(capi.load()._name)
        L.dmi_tuning_depth_consistency_undecided.restype = ctypes.c_ulonglong
        rec["undecided_share"] = L.dmi_tuning_depth_consistency_undecided() / rec["pairs"]
        rec["sweep"] = {}
        for group in (0, 16, 64):
            for ahead in (0, 1):
                os.environ["DMI_DC_VIEW_GROUP"], os.environ["DMI_DC_GATHER_AHEAD"] = str(group), str(ahead)
                k, _, c = timed(views, a, out)
                rec["sweep"][f"group{group}_ahead{ahead}"] = k
                rec["sweep_counts_identical"] = rec.get("sweep_counts_identical", True) and bool(np.array_equal(c, counts))
        del os.environ["DMI_DC_VIEW_GROUP"], os.environ["DMI_DC_GATHER_AHEAD"]
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
