"""Time and quality of dmi_views_fit_point_planes on the noisy scene (scene.make_scene_views: depth noise, best costs whose threshold
scatters holes), sizes from the arguments, beside dmi_views_filter_points_radius of the same run.  Prints one JSON line.  Per build
(duplicates dropped and kept) and per radius (the given multiples of the voxel spacing 2 / --cells of the bench grid that goes with
the views): the report's counts, the kernel time by pass (bounds, keys, sort, ranks, permute, fit; the best call of --repeat, each
on a fresh build), the radius filter's count pass on the same cloud, and the fit kernel's issue floor: distance_tests x
--instructions-per-test / --lane-ops-per-s.  With --quality the points within 0.1 of the scene's sphere (radius 0.6): the RMS of
| |p| - 0.6 | and the mean angle between the normal and the radius, before and after the fit, and the same after a thinning at one
voxel behind each.  Meant to be run under a time limit of its own:

    timeout -k 10 900 python tools/gpu_depth_points_planes_time.py --views 64 --width 640 --height 480 --cells 256 --quality

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

SPHERE = 0.6


def quality_of(cloud):
    """RMS distance to the sphere and mean normal error (degrees) over the points within 0.1 of the sphere that have a normal."""
    xyz, normal = cloud["xyz"], cloud["normal"].astype(np.float64)
    r = np.linalg.norm(xyz, axis=1)
    near = np.abs(r - SPHERE) < 0.1
    has = near & (np.linalg.norm(normal, axis=1) > 0)
    cos = np.clip(np.abs((normal[has] * xyz[has]).sum(axis=1)) / r[has], 0.0, 1.0)
    return {"sphere_points": int(near.sum()), "rms_to_sphere": float(np.sqrt(np.mean((r[near] - SPHERE) ** 2))) if near.any() else None,
            "with_normal": int(has.sum()), "mean_normal_error_deg": float(np.degrees(np.arccos(cos)).mean()) if has.any() else None}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--views", type=int, default=64)
    p.add_argument("--width", type=int, default=640)
    p.add_argument("--height", type=int, default=480)
    p.add_argument("--cells", type=int, default=256, help="the bench grid's cells per axis: the voxel spacing is 2 / cells")
    p.add_argument("--radius-multiples", type=float, nargs="+", default=[2.0, 4.0])
    p.add_argument("--min-neighbors", type=int, default=5)
    p.add_argument("--repeat", type=int, default=3)
    p.add_argument("--min-views", type=int, default=1)
    p.add_argument("--abs-tolerance", type=float, default=0.02)
    p.add_argument("--rel-tolerance", type=float, default=0.01)
    p.add_argument("--noise-sigma", type=float, default=0.002)
    p.add_argument("--instructions-per-test", type=float, default=31.75,
                   help="the fit kernel's vector instructions per distance test, counted in its ISA (DESIGN.md 8q)")
    p.add_argument("--lane-ops-per-s", type=float, default=256 * 64 * 2.4e9, help="256 CUs x 4 SIMDs x 16 lanes at 2.4 GHz")
    p.add_argument("--quality", action="store_true")
    p.add_argument("--check", action="store_true", help="first compare a small scene with the numpy restatements")
    a = p.parse_args()
    n, W, H = a.views, a.width, a.height
    voxel = 2.0 / a.cells
    build = dict(abs_tolerance=a.abs_tolerance, rel_tolerance=a.rel_tolerance, min_views=a.min_views)
    rec = {"scene": "noisy", "views": n, "width": W, "height": H, "voxel": voxel, "noise_sigma": a.noise_sigma, **build,
           "min_neighbors": a.min_neighbors, "instructions_per_test": a.instructions_per_test, "lane_ops_per_s": a.lane_ops_per_s}
    if a.check:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import depth_points_np as P
        import depth_points_planes_np as F
        small, threshold = scene.make_scene_views("noisy", 5, max(W // 8, 8), max(H // 8, 8), seed=1, noise_sigma=a.noise_sigma, holes=1)
        with capi.ViewSet(small.depth.shape[2], small.depth.shape[1]) as s:
            s.add(small, threshold)
            s.build_points(dedupe=False, **build)
            report = s.fit_point_planes(8 * voxel, a.min_neighbors)
            got = dict(s.download_points(), plane_rms=s.download_point_plane_rms())
        cloud, _ = P.build_points(small.depth, small.K4, small.RT4, dedupe=False, best_cost=small.best_cost, threshold=threshold, **build)
        want, want_report = F.fit_planes(cloud["xyz"], cloud["normal"], 8 * voxel, a.min_neighbors, 3)
        rec["check_identical"] = bool(all(got[k].tobytes() == want[k].tobytes() for k in ("xyz", "normal", "plane_rms")) and
                                      all(int(report[k]) == want_report[k] for k in F.REPORT_NAMES))

    def say(what):   # (stderr: the JSON line stays alone on stdout)
        print(what, file=sys.stderr, flush=True)

    def measure(s, dedupe, radius):
        best = None
        for _ in range(a.repeat):
            s.build_points(dedupe=dedupe, **build)
            report = s.fit_point_planes(radius, a.min_neighbors)
            if best is None or report["kernel_ms"] < best[0]["kernel_ms"]:
                best = (report, s.plane_fit_pass_ms())
        count = None
        for _ in range(a.repeat):   # the count kernel on the same cloud: min_neighbors = 0 drops nothing
            s.build_points(dedupe=dedupe, **build)
            s.filter_points_radius(radius, 0)
            ms = s.radius_pass_ms()["count"]
            count = ms if count is None else min(count, ms)
        return best[0], best[1], count

    say("rendering the views ...")
    views, threshold = scene.make_scene_views("noisy", n, W, H, seed=1, noise_sigma=a.noise_sigma)
    with capi.ViewSet(W, H) as s:
        s.add(views, threshold)
        say("timing ...")
        s.build_points(**build)
        s.fit_point_planes(voxel, a.min_neighbors)   # the warm-up: code loaded, first allocations made
        for dedupe in (True, False):
            runs = {}
            for multiple in a.radius_multiples:
                report, passes, count_ms = measure(s, dedupe, multiple * voxel)
                out = {k: (float(v) if k in ("kernel_ms", "max_shift") else int(v)) for k, v in report.items()}
                floor_ms = out["distance_tests"] * a.instructions_per_test / a.lane_ops_per_s * 1e3
                out.update(radius=multiple * voxel, pass_ms=passes, count_kernel_ms=count_ms,
                           fit_over_count=passes["fit"] / count_ms if count_ms else None,
                           mean_neighbors=out["neighbor_sum"] / out["points_in"] if out["points_in"] else None,
                           tests_per_member=out["distance_tests"] / (out["neighbor_sum"] + out["points_in"]) if out["points_in"] else None,
                           fit_issue_floor_ms=floor_ms, fit_fraction_of_floor=floor_ms / passes["fit"] if passes["fit"] > 0 else None,
                           scratch_bytes_per_point=60)
                runs[f"{multiple:g}_voxels"] = out
            rec["duplicates_dropped" if dedupe else "duplicates_kept"] = runs
        rec["device_bytes_after"] = int(s.info().device_bytes)
        if a.quality:
            say("quality ...")
            quality = {}
            for multiple in a.radius_multiples:
                row = {}
                for fit in (False, True):
                    s.build_points(dedupe=False, **build)
                    if fit:
                        s.fit_point_planes(multiple * voxel, a.min_neighbors)
                    row["after" if fit else "before"] = quality_of(s.download_points())
                    s.thin_points(voxel)
                    row["after_then_thinned" if fit else "before_then_thinned"] = quality_of(s.download_points())
                quality[f"{multiple:g}_voxels"] = row
            rec["quality"] = quality
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
