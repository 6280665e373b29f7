"""Time and quality of dmi_views_thin_points on the noisy scene (scene.make_scene_views: depth noise, best costs whose threshold
scatters holes), sizes from the arguments.  Prints one JSON line.  Per build (duplicates dropped and kept) and per cell size (the
given multiples of the voxel spacing 2 / --cells of the bench grid that goes with the views): the report's counts, the kernel time by
pass (bounds, keys, sort, ranks, representatives; the best call of --repeat, each on a fresh build), and two yardsticks taken in
the same run: the rocPRIM sort alone (the sort pass is nothing else) and the time a plain read of the input cloud plus a write of the
output takes at the rate DESIGN.md 8m measured for a plain read of the planes (--plain-tb-per-s).  With --sweep the representatives
pass at every wave-pass threshold of the list, duplicates kept, at the first cell size.  With --quality the RMS distance of the
points on the scene's sphere (radius 0.6 about the origin; the points within --sphere-shell of it) to that sphere, before and after
the thinning with duplicates kept, beside the same for the noise-free twin (noise_sigma 0: the same holes, so what is left is
the pixel grid's own error).  Meant to be run under a time limit of its own:

    timeout -k 10 900 python tools/gpu_depth_points_thin_time.py --views 64 --width 640 --height 480 --cells 256 --sweep --quality

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

SPHERE_RADIUS = 0.6


def sphere_rms(xyz, shell, members=None):
    """(RMS of | |p| - 0.6 | over the points within `shell` of the sphere, their number); with `members` each point weighs as
    many as it was merged from."""
    r = np.sqrt(np.einsum("ij,ij->i", xyz, xyz))
    near = np.abs(r - SPHERE_RADIUS) < shell
    e = r[near] - SPHERE_RADIUS
    if not e.size:
        return None, 0
    w = np.ones(e.size) if members is None else members[near].astype(np.float64)
    return float(np.sqrt(np.sum(w * e * e) / np.sum(w))), int(e.size)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--views", type=int, default=64)
    p.add_argument("--width", type=int, default=640)
    p.add_argument("--height", type=int, default=480)
    p.add_argument("--cells", type=int, default=256, help="the bench grid's cells per axis: the voxel spacing is 2 / cells")
    p.add_argument("--cell-multiples", type=float, nargs="+", default=[1.0, 2.0])
    p.add_argument("--repeat", type=int, default=3)
    p.add_argument("--min-views", type=int, default=1)
    p.add_argument("--abs-tolerance", type=float, default=0.02)
    p.add_argument("--rel-tolerance", type=float, default=0.01)
    p.add_argument("--noise-sigma", type=float, default=0.002)
    p.add_argument("--plain-tb-per-s", type=float, default=6.04)
    p.add_argument("--sweep", type=int, nargs="*", default=None, help="wave-pass thresholds (no value: 1 2 4 ... 1024)")
    p.add_argument("--quality", action="store_true")
    p.add_argument("--sphere-shell", type=float, default=0.1)
    p.add_argument("--check", action="store_true",
                   help="first compare a small scene (a few thousand points) with the numpy restatements; the comparison at "
                        "the sizes timed here, above 2^20 points, is tests/test_depth_points_scale.py")
    a = p.parse_args()
    n, W, H = a.views, a.width, a.height
    voxel = 2.0 / a.cells
    build = dict(abs_tolerance=a.abs_tolerance, rel_tolerance=a.rel_tolerance, min_views=a.min_views)
    rec = {"scene": "noisy", "views": n, "width": W, "height": H, "voxel": voxel, "noise_sigma": a.noise_sigma, **build,
           "plain_tb_per_s": a.plain_tb_per_s}
    if a.check:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import depth_points_np as P
        import depth_points_thin_np as T
        small, threshold = scene.make_scene_views("noisy", 5, max(W // 8, 8), max(H // 8, 8), seed=1, noise_sigma=a.noise_sigma, holes=1)
        with capi.ViewSet(small.depth.shape[2], small.depth.shape[1]) as s:
            s.add(small, threshold)
            s.build_points(dedupe=False, **build)
            report = s.thin_points(8 * voxel, 2)
            got = dict(s.download_points(), members=s.download_point_members())
        cloud, _ = P.build_points(small.depth, small.K4, small.RT4, dedupe=False, best_cost=small.best_cost, threshold=threshold, **build)
        want, want_report = T.thin(*(cloud[k] for k in ("xyz", "normal", "view", "pixel", "count")), cell_size=8 * voxel, min_points=2)
        rec["check_identical"] = bool(all(got[k].tobytes() == want[k].tobytes() for k in want) and
                                      all(int(report[k]) == want_report[k] for k in T.REPORT_NAMES))

    def measure(s, dedupe, cell, knob=None):
        best = None
        for _ in range(a.repeat):
            s.build_points(dedupe=dedupe, **build)
            if knob is not None:
                s.set_thin_wave_cell_points(knob)
            report = s.thin_points(cell)
            if best is None or report["kernel_ms"] < best[0]["kernel_ms"]:
                best = (report, s.thin_pass_ms())
        return best

    def say(what):   # (stderr: the JSON line stays alone on stdout)
        print(what, file=sys.stderr, flush=True)

    say("rendering the views ...")
    views, threshold = scene.make_scene_views("noisy", n, W, H, seed=1, noise_sigma=a.noise_sigma)
    with capi.ViewSet(W, H) as s:
        s.add(views, threshold)
        del views
        say("timing ...")
        s.build_points(**build)
        s.thin_points(voxel)   # the warm-up: code loaded, first allocations made
        for dedupe in (True, False):
            runs = {}
            for multiple in a.cell_multiples:
                report, passes = measure(s, dedupe, multiple * voxel)
                out = {k: int(v) for k, v in report.items() if k != "kernel_ms"}
                moved = 48 * out["points_in"] + 52 * out["cells_kept"]
                plain_ms = moved / (a.plain_tb_per_s * 1e12) * 1e3
                out.update(cell_size=multiple * voxel, kernel_ms=report["kernel_ms"], pass_ms=passes, bytes_in_and_out=moved,
                           plain_read_write_ms=plain_ms, sort_alone_ms=passes["sort"],
                           representatives_over_sort=passes["representatives"] / passes["sort"] if passes["sort"] > 0 else None,
                           passes_over_plain={k: v / plain_ms for k, v in passes.items()})
                runs[f"{multiple:g}_voxels"] = out
            rec["duplicates_dropped" if dedupe else "duplicates_kept"] = runs
        if a.sweep is not None:
            say("the threshold sweep ...")
            thresholds = a.sweep or [1, 2, 4, 8, 16, 32, 64, 128, 256, 1024]
            sweep = {}
            for multiple in a.cell_multiples:
                sweep[f"{multiple:g}_voxels"] = {str(k): measure(s, False, multiple * voxel, k)[1]["representatives"] for k in thresholds}
            s.set_thin_wave_cell_points(32)
            rec["representatives_ms_by_wave_threshold"] = sweep
        rec["device_bytes_after"] = int(s.info().device_bytes)

    if a.quality:
        quality = {}
        for label, sigma in (("noisy", a.noise_sigma), ("noise_free", 0.0)):
            say(f"quality, {label}: rendering the views ...")
            views, threshold = scene.make_scene_views("noisy", n, W, H, seed=1, noise_sigma=sigma)
            with capi.ViewSet(W, H) as s:
                s.add(views, threshold)
                del views
                report = s.build_points(dedupe=False, **build)
                rms, used = sphere_rms(s.download_points()["xyz"], a.sphere_shell)
                row = {"before": {"points": int(report["points"]), "sphere_points": used, "rms": rms}}
                for multiple in a.cell_multiples:
                    s.build_points(dedupe=False, **build)
                    thinned = s.thin_points(multiple * voxel)
                    xyz, members = s.download_points()["xyz"], s.download_point_members()
                    after, used_after = sphere_rms(xyz, a.sphere_shell)
                    weighted, _ = sphere_rms(xyz, a.sphere_shell, members)
                    near = np.abs(np.sqrt(np.einsum("ij,ij->i", xyz, xyz)) - SPHERE_RADIUS) < a.sphere_shell
                    row[f"{multiple:g}_voxels"] = {"points": int(thinned["cells_kept"]), "sphere_points": used_after, "rms": after,
                                                   "ratio_to_before": after / rms if rms else None,
                                                   "rms_weighted_by_members": weighted,
                                                   "mean_members_on_sphere": float(members[near].mean()) if used_after else None,
                                                   "sphere_points_of_one_member": int((members[near] == 1).sum())}
                quality[label] = row
        rec["quality_duplicates_kept"] = quality
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
