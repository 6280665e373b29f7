"""Time and quality of dmi_views_filter_points_radius on the noisy scene (scene.make_scene_views: depth noise, best costs whose
threshold scatters holes), sizes from the arguments.  Prints one JSON line.  Per build (duplicates dropped and kept) and per radius
(the given multiples of the voxel spacing 2 / --cells of the bench grid that goes with the views): the report's counts, the kernel
time by pass (bounds, keys, sort, ranks, permute, count, compaction; the best call of --repeat, each on a fresh build), and two
yardsticks taken in the same run: the rocPRIM sort alone (the sort pass is nothing else) and the time a plain read of the input cloud
plus a write of the output takes at the rate DESIGN.md 8m measured for a plain read of the planes (--plain-tb-per-s).  For the count
kernel: distance_tests / neighbor_sum, and the floor distance_tests x --fp64-per-test / --fp64-lane-ops-per-s it is judged against.
With --sweep the count pass at every value of the knob in the list, duplicates kept.  With --quality a seeded --inject share of the
valid depths is replaced by uniform random depths within the scene's depth range, the cloud is built with min_views = 0 and
duplicates kept, and for every radius and --min-neighbors the share of the injected points removed and of the untouched points lost
is reported, beside the same for the thinning's min_points on cells of the same size (its cell membership taken on the host by the
thinning's own definition).  Meant to be run under a time limit of its own:

    timeout -k 10 900 python tools/gpu_depth_points_radius_time.py --views 64 --width 640 --height 480 --cells 256 --sweep --quality

--check first runs a small scene through the library and through the numpy restatements and records whether the two are identical.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from cudadepthmapintegration_amd import capi, scene  # noqa: E402


def cell_sizes(xyz, h):
    """For every point the members of its cell of size h, by the thinning's definition (bounds, floor((x - lo) / h))."""
    lo = xyz.min(axis=0)
    b = np.floor((xyz - lo) / h).astype(np.int64)
    n = b.max(axis=0) + 1
    keys = (b[:, 2] * n[1] + b[:, 1]) * n[0] + b[:, 0]
    _, inverse, counts = np.unique(keys, return_inverse=True, return_counts=True)
    return counts[inverse]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--views", type=int, default=64)
    p.add_argument("--width", type=int, default=640)
    p.add_argument("--height", type=int, default=480)
    p.add_argument("--cells", type=int, default=256, help="the bench grid's cells per axis: the voxel spacing is 2 / cells")
    p.add_argument("--radius-multiples", type=float, nargs="+", default=[2.0, 4.0])
    p.add_argument("--min-neighbors", type=int, nargs="+", default=[2, 8, 32])
    p.add_argument("--repeat", type=int, default=3)
    p.add_argument("--min-views", type=int, default=1)
    p.add_argument("--abs-tolerance", type=float, default=0.02)
    p.add_argument("--rel-tolerance", type=float, default=0.01)
    p.add_argument("--noise-sigma", type=float, default=0.002)
    p.add_argument("--plain-tb-per-s", type=float, default=6.04)
    p.add_argument("--fp64-per-test", type=float, default=9.0,
                   help="the count kernel's fp64 instructions per distance test, from its ISA: 3 v_add_f64 (the differences), "
                        "3 v_mul_f64, 2 v_add_f64, 1 v_cmp_ge_f64")
    p.add_argument("--fp64-lane-ops-per-s", type=float, default=256 * 64 * 2.4e9, help="256 CUs x 4 SIMDs x 16 lanes at 2.4 GHz")
    p.add_argument("--sweep", type=int, nargs="*", default=None, help="values of the knob (no value: 1 2 4 8 16 32 64)")
    p.add_argument("--quality", action="store_true")
    p.add_argument("--inject", type=float, default=0.01)
    p.add_argument("--check", action="store_true",
                   help="first compare a small scene (a few thousand points) with the numpy restatements; the comparison at "
                        "the sizes timed here, above 2^20 points, is tests/test_depth_points_scale.py")
    a = p.parse_args()
    n, W, H = a.views, a.width, a.height
    voxel = 2.0 / a.cells
    build = dict(abs_tolerance=a.abs_tolerance, rel_tolerance=a.rel_tolerance, min_views=a.min_views)
    rec = {"scene": "noisy", "views": n, "width": W, "height": H, "voxel": voxel, "noise_sigma": a.noise_sigma, **build,
           "plain_tb_per_s": a.plain_tb_per_s, "fp64_per_test": a.fp64_per_test, "fp64_lane_ops_per_s": a.fp64_lane_ops_per_s}
    if a.check:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import depth_points_np as P
        import depth_points_radius_np as R
        small, threshold = scene.make_scene_views("noisy", 5, max(W // 8, 8), max(H // 8, 8), seed=1, noise_sigma=a.noise_sigma, holes=1)
        with capi.ViewSet(small.depth.shape[2], small.depth.shape[1]) as s:
            s.add(small, threshold)
            s.build_points(dedupe=False, **build)
            report = s.filter_points_radius(8 * voxel, 4)
            got = dict(s.download_points(), neighbors=s.download_point_neighbors())
        cloud, _ = P.build_points(small.depth, small.K4, small.RT4, dedupe=False, best_cost=small.best_cost, threshold=threshold, **build)
        want, want_report = R.filter_radius(cloud, 8 * voxel, 4)
        rec["check_identical"] = bool(all(got[k].tobytes() == want[k].tobytes() for k in want) and
                                      all(int(report[k]) == want_report[k] for k in R.REPORT_NAMES))

    def measure(s, dedupe, radius, knob=None, min_neighbors=1):
        best = None
        for _ in range(a.repeat):
            s.build_points(dedupe=dedupe, **build)
            if knob is not None:
                s.set_radius_group_points(knob)
            report = s.filter_points_radius(radius, min_neighbors)
            if best is None or report["kernel_ms"] < best[0]["kernel_ms"]:
                best = (report, s.radius_pass_ms())
        return best

    def say(what):   # (stderr: the JSON line stays alone on stdout)
        print(what, file=sys.stderr, flush=True)

    say("rendering the views ...")
    views, threshold = scene.make_scene_views("noisy", n, W, H, seed=1, noise_sigma=a.noise_sigma)
    with capi.ViewSet(W, H) as s:
        s.add(views, threshold)
        say("timing ...")
        s.build_points(**build)
        s.filter_points_radius(voxel)   # the warm-up: code loaded, first allocations made
        for dedupe in (True, False):
            runs = {}
            for multiple in a.radius_multiples:
                report, passes = measure(s, dedupe, multiple * voxel)
                out = {k: int(v) for k, v in report.items() if k != "kernel_ms"}
                moved = 48 * out["points_in"] + 52 * out["points_kept"]
                plain_ms = moved / (a.plain_tb_per_s * 1e12) * 1e3
                floor_ms = out["distance_tests"] * a.fp64_per_test / a.fp64_lane_ops_per_s * 1e3
                out.update(radius=multiple * voxel, kernel_ms=report["kernel_ms"], pass_ms=passes, bytes_in_and_out=moved,
                           plain_read_write_ms=plain_ms, sort_alone_ms=passes["sort"],
                           count_over_sort=passes["count"] / passes["sort"] if passes["sort"] > 0 else None,
                           passes_over_plain={k: v / plain_ms for k, v in passes.items()},
                           tests_per_neighbor=out["distance_tests"] / out["neighbor_sum"] if out["neighbor_sum"] else None,
                           mean_neighbors=out["neighbor_sum"] / out["points_in"] if out["points_in"] else None,
                           count_fp64_floor_ms=floor_ms, count_fraction_of_floor=floor_ms / passes["count"] if passes["count"] > 0 else None,
                           scratch_bytes_per_point=56)
                runs[f"{multiple:g}_voxels"] = out
            rec["duplicates_dropped" if dedupe else "duplicates_kept"] = runs
        if a.sweep is not None:
            say("the knob's sweep ...")
            knobs = a.sweep or [1, 2, 4, 8, 16, 32, 64]
            sweep = {}
            for multiple in a.radius_multiples[:1]:
                sweep[f"{multiple:g}_voxels"] = {str(k): measure(s, False, multiple * voxel, k)[1]["count"] for k in knobs}
            s.set_radius_group_points(64)
            rec["count_ms_by_group_points"] = sweep
        rec["device_bytes_after"] = int(s.info().device_bytes)

    if a.quality:
        say("quality: injecting strays ...")
        rng = np.random.default_rng(7)
        depth = np.array(views.depth, dtype=np.float64, copy=True)
        valid = depth > 0
        if views.best_cost is not None and threshold is not None:
            valid &= np.asarray(views.best_cost) < threshold
        lo, hi = float(depth[valid].min()), float(depth[valid].max())
        injected = valid & (rng.random(depth.shape) < a.inject)
        depth[injected] = rng.uniform(lo, hi, int(injected.sum()))
        strayed = scene.Views(depth, views.K4, views.RT4, views.best_cost)
        quality = {"depth_range": [lo, hi], "valid": int(valid.sum()), "injected": int(injected.sum())}
        loose = dict(build, min_views=0)
        with capi.ViewSet(W, H) as s:
            s.add(strayed, threshold)
            s.build_points(dedupe=False, **loose)
            cloud = s.download_points()
            py, px = cloud["pixel"] // W, cloud["pixel"] % W
            stray = injected[cloud["view"], H - 1 - py, px]
            quality["points"] = int(len(stray))
            quality["stray_points"] = int(stray.sum())
            for multiple in a.radius_multiples:
                report = s.filter_points_radius(multiple * voxel, 0)   # the counts only: every threshold from one call
                neighbors = s.download_point_neighbors()
                members = cell_sizes(cloud["xyz"], multiple * voxel)
                row = {"radius": multiple * voxel, "kernel_ms": report["kernel_ms"], "max_neighbors": int(report["max_neighbors"])}
                for m in a.min_neighbors:
                    gone = neighbors < m
                    thin_gone = members < m + 1   # a cell of m + 1 members gives each of them m neighbours in the cell
                    row[f"min_neighbors_{m}"] = {
                        "strays_removed": float(gone[stray].mean()) if stray.any() else None,
                        "untouched_lost": float(gone[~stray].mean()),
                        "thinning_min_points": m + 1,
                        "thinning_strays_removed": float(thin_gone[stray].mean()) if stray.any() else None,
                        "thinning_untouched_lost": float(thin_gone[~stray].mean())}
                quality[f"{multiple:g}_voxels"] = row
                s.build_points(dedupe=False, **loose)
        rec["quality_strays"] = quality
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
