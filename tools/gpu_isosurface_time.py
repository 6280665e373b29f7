"""Kernel time of dmi_extract_isosurface on the cfg-3 speckle scene (512^3, 256 views of 1280 x 720, as bench.py --full builds
it), next to the HBM floor of reading the point lattice.  Prints one JSON line.  With --normals it times
dmi_extract_isosurface_normals too, the two calls alternating in the same process (kernel_ms / normals_kernel_ms).  With
--components it times dmi_filter_isosurface_components beside the extraction (each filter follows a fresh extraction with
normals, the calls alternating): MIN(0), MIN at --min-triangles and LARGEST, pass by pass, with the mesh's component count and
size histogram, a floor derived from the bytes the filter must move, and the host alternative (download + the numpy restatement
of tests/isosurface_components_np.py, imported from there) for orientation.  With --smooth N it times dmi_smooth_isosurface
(N iterations) in the same alternating style, once on the raw mesh and once after MIN(--min-triangles): pass by pass, one step
against the bytes it must move, the scratch it needs, and the numpy restatement (tests/isosurface_smooth_np.py) on the raw
mesh for orientation.  With --decimate H (grid spacings; several may be given; a tiny H that the mesh's 2^21 bins refuse
becomes the smallest size it accepts: the weld) it times dmi_decimate_isosurface after a fresh extraction with normals, pass by
pass, with the counts before and after and the bytes each pass must move; --decimate-check compares with the numpy restatement
(tests/isosurface_decimate_np.py).  With --decimate-quadric every round also times dmi_decimate_isosurface_placed with the quadric
placement, after a fresh extraction of its own, in the same process and on the same mesh: the four passes of both placements
side by side, the quadric call's total over the mean's, and the scratch (record "quadric"; --decimate-check compares it with
tests/isosurface_decimate_quadric_np.py too).  With --color it times the coloration of the device mesh
(dmi_color_process_isosurface) against dmi_color_process, the fused depth test against the own-planes test, and both again after a
decimation (color_record).  With --render-depths it times the z-buffer rasteriser (dmi_color_render_isosurface_depths) on the
mesh, pass by pass, with the count of queued pairs, and the colouring with rendered planes next to the colouring with fused depths
(render_record).  With --holes N (several may be given) it times dmi_fill_isosurface_holes on the mesh the support trim
leaves, pass by pass (holes_record); --image W H sets the views' size (cfg 2: --grid 256 --views 64 --image 640 480).  --grid N runs the whole tool on an N^3 grid (a quick
run; the records in profiles/ are of the default 512).

    python tools/gpu_isosurface_time.py [--iso 1.0] [--views 256] [--repeat 5] [--normals] [--components [--min-triangles 100]]
                                         [--smooth 10 [--smooth-lambda 0.5] [--smooth-mu -0.53]]
                                         [--decimate 2 [--decimate 4 ...] [--decimate-check] [--decimate-quadric]]
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


def components_record(ctx, a):
    """The --components record of the context's grid at a.iso (a.repeat rounds after a warm-up round, a.min_triangles the mid
    threshold).  In every round each of the three filters follows a fresh extraction with normals, whose own kernel time is taken
    in the same breath: the ratios compare calls that alternate in one process."""
    import time

    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))   # the host alternative IS the tests' numpy restatement
    import isosurface_components_np as C
    rec = {"min_triangles_mid": a.min_triangles}
    cases = {"min0": ("min_triangles", 0), "mid": ("min_triangles", a.min_triangles), "largest": ("largest", 0)}
    for k in cases:
        rec[k] = {"kernel_ms": [], "pass_ms": [], "extraction_kernel_ms": [], "cas_retries": []}
    for r in range(a.repeat + 1):                       # round 0 is the warm-up: buffers sized, code loaded
        for k, (mode, n) in cases.items():
            ctx.extract_isosurface_with_normals(a.iso)
            ex = ctx.isosurface_kernel_ms()
            counts = ctx.filter_isosurface_components(mode, n)
            if r:
                rec[k]["extraction_kernel_ms"].append(ex)
                rec[k]["kernel_ms"].append(ctx.isosurface_filter_kernel_ms())
                rec[k]["pass_ms"].append(ctx.isosurface_filter_pass_ms())
                rec[k]["cas_retries"].append(ctx.isosurface_filter_cas_retries())
            rec[k]["counts"] = dict(zip(("vertices", "triangles", "components", "components_kept"), counts))
    # the size histogram, from the labels-only filter's RegionSize
    verts, tris, normals = ctx.extract_isosurface_with_normals(a.iso)
    nv, nt = len(verts), len(tris)
    ctx.filter_isosurface_components("min_triangles", 0)
    _, rsz = ctx.download_isosurface_regions()
    edges = [0, 1, 2, 4, 8, 16, 32, 64, 128, 256, 1024, 4096, 1 << 14, 1 << 16, 1 << 20, 1 << 62]
    hist = np.histogram(rsz, bins=edges)[0]
    rec["size_histogram"] = {f"[{lo},{hi})": int(c) for lo, hi, c in zip(edges[:-1], edges[1:], hist)}
    rec["largest_sizes"] = [int(x) for x in np.sort(rsz)[::-1][:5]]
    # The floor: triangles read twice and written once (3 x 24 B), positions and normals read and written once (2 x 36 B per
    # vertex), labels / sizes / maps written and read once each (16 B per vertex), RegionId written (8 B per vertex).
    rec["floor_bytes"] = nt * 72 + nv * (72 + 16 + 8)
    rec["floor_ms_c2p_rate"] = rec["floor_bytes"] / C2P_TBPS / 1e9
    for k in cases:
        rec[k]["kernel_ms_min"] = min(rec[k]["kernel_ms"])
        rec[k]["extraction_kernel_ms_min"] = min(rec[k]["extraction_kernel_ms"])
        rec[k]["over_extraction"] = rec[k]["kernel_ms_min"] / rec[k]["extraction_kernel_ms_min"]
        rec[k]["over_floor_c2p_rate"] = rec[k]["kernel_ms_min"] / rec["floor_ms_c2p_rate"]
    # the host alternative, for orientation: download the unfiltered mesh, label it with the numpy restatement
    ctx.extract_isosurface_with_normals(a.iso)
    ctx.filter_isosurface_components("min_triangles", 0)        # keeps everything: the download below is the whole mesh
    t0 = time.perf_counter()
    ctx.download_isosurface()
    ctx.download_isosurface_normals()
    t1 = time.perf_counter()
    want = C.filter_mesh(verts, tris, normals, C.LARGEST)
    t2 = time.perf_counter()
    rec["host_download_s"], rec["host_numpy_largest_s"] = t1 - t0, t2 - t1
    rec["host_matches_gpu"] = want["counts"] == tuple(rec["largest"]["counts"].values())
    return rec


def smooth_record(ctx, a):
    """The --smooth record of the context's grid at a.iso: a.smooth iterations with a.smooth_lambda / a.smooth_mu, a.repeat rounds
    after a warm-up round.  In every round each smoothing follows a fresh extraction with normals ("raw"), or that and the
    MIN(a.min_triangles) filter ("min"); the extraction's own kernel time is taken in the same breath."""
    import time

    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))   # the host alternative IS the tests' numpy restatement
    import isosurface_smooth_np as S
    steps = a.smooth * (2 if a.smooth_mu != 0 else 1)
    rec = {"iterations": a.smooth, "lambda": a.smooth_lambda, "mu": a.smooth_mu, "steps": steps, "min_triangles": a.min_triangles}
    for k in ("raw", "min"):
        rec[k] = {"kernel_ms": [], "pass_ms": [], "extraction_kernel_ms": []}
    for r in range(a.repeat + 1):                       # round 0 is the warm-up: buffers sized, code loaded
        for k in ("raw", "min"):
            ctx.extract_isosurface_with_normals(a.iso)
            ex = ctx.isosurface_kernel_ms()
            if k == "min":
                ctx.filter_isosurface_components("min_triangles", a.min_triangles)
            if r == 0:                                  # the mesh that is smoothed, for the counts and the host's run
                verts, tris = ctx.download_isosurface()
                normals = ctx.download_isosurface_normals()
                rec[k]["vertices"], rec[k]["triangles"] = len(verts), len(tris)
                if k == "raw":
                    raw = (verts, tris, normals)
                rec[k]["neighbour_entries"] = int(S.adjacency(len(verts), tris)[1].sum())
            ctx.smooth_isosurface(a.smooth, a.smooth_lambda, a.smooth_mu)
            if r:
                rec[k]["extraction_kernel_ms"].append(ex)
                rec[k]["kernel_ms"].append(ctx.isosurface_smooth_kernel_ms())
                rec[k]["pass_ms"].append(ctx.isosurface_smooth_pass_ms())
            if k == "raw" and r == a.repeat:
                got = (ctx.download_isosurface()[0], ctx.download_isosurface_normals())
    for k in ("raw", "min"):
        nv, nt, ne = rec[k]["vertices"], rec[k]["triangles"], rec[k]["neighbour_entries"]
        rec[k]["kernel_ms_min"] = min(rec[k]["kernel_ms"])
        rec[k]["extraction_kernel_ms_min"] = min(rec[k]["extraction_kernel_ms"])
        rec[k]["over_extraction"] = rec[k]["kernel_ms_min"] / rec[k]["extraction_kernel_ms_min"]
        for p in ("adjacency", "steps", "normals"):
            rec[k][p + "_ms_min"] = min(q[p] for q in rec[k]["pass_ms"])
        rec[k]["step_ms"] = rec[k]["steps_ms_min"] / steps
        # one step's floor: positions read and written once (2 x 24 B per vertex), the CSR read once (offsets and neighbour ids)
        rec[k]["step_floor_bytes"] = 48 * nv + 4 * (nv + 1) + 4 * ne
        rec[k]["step_floor_ms_c2p_rate"] = rec[k]["step_floor_bytes"] / C2P_TBPS / 1e9
        rec[k]["step_over_floor_c2p_rate"] = rec[k]["step_ms"] / rec[k]["step_floor_ms_c2p_rate"]
        # the scratch of the call, rocPRIM's own storage aside: two key arrays of 6 T, the fixed bits and three
        # u32 arrays per vertex, and the two step buffers (one of them is the component filter's second vertex buffer)
        rec[k]["scratch_bytes"] = 2 * max(6 * nt, 2) * 8 + (nv + 63) // 64 * 8 + 12 * (nv + 1) + 48 * nv
    t0 = time.perf_counter()
    want = S.smooth(raw[0], raw[1], a.smooth, a.smooth_lambda, a.smooth_mu, raw[2])
    rec["host_numpy_s"] = time.perf_counter() - t0
    rec["host_matches_gpu"] = want[0].tobytes() == got[0].tobytes() and want[1].tobytes() == got[1].tobytes()
    return rec


def decimate_record(ctx, a):
    """The --decimate record of the context's grid at a.iso: vertex clustering with cells of a.decimate grid spacings, a.repeat
    rounds after a warm-up round.  In every round the decimation follows a fresh extraction with normals whose own kernel time is
    taken in the same breath.  With a.decimate_check the numpy restatement runs on the raw mesh and is compared bit for bit.  With
    a.decimate_quadric the quadric placement follows in every round, on a fresh extraction of its own (rec["quadric"])."""
    import time

    sys.path.insert(0, os.path.join(ROOT, "tests"))   # the host alternative IS the tests' numpy restatement
    import isosurface_decimate_np as D
    h = a.decimate * float(min(scene.default_grid(a.grid).spacing))
    rec = {"cell_size_spacings": a.decimate, "cell_size": h, "kernel_ms": [], "pass_ms": [], "extraction_kernel_ms": []}
    for r in range(a.repeat + 1):                       # round 0 is the warm-up: buffers sized, code loaded
        raw = ctx.extract_isosurface_with_normals(a.iso)
        ex = ctx.isosurface_kernel_ms()
        if r == 0 and a.decimate < 1e-3:                # a weld: the smallest size this mesh accepts, if the one asked for is refused
            h = rec["cell_size"] = max(h, D.min_cell_size(raw[0]))
        rec["vertices"], rec["triangles"] = len(raw[0]), len(raw[1])
        rec["vertices_after"], rec["triangles_after"] = ctx.decimate_isosurface(h)
        if r:
            rec["extraction_kernel_ms"].append(ex)
            rec["kernel_ms"].append(ctx.isosurface_decimate_kernel_ms())
            rec["pass_ms"].append(ctx.isosurface_decimate_pass_ms())
        if a.decimate_check and r == a.repeat:          # (before the quadric placement replaces the mesh)
            got = ctx.download_isosurface() + (ctx.download_isosurface_normals(),)
        if a.decimate_quadric:
            if r == 0:
                quadric = rec["quadric"] = {"kernel_ms": [], "pass_ms": [], "device_bytes_before": int(ctx.info().device_bytes)}
            ctx.extract_isosurface_with_normals(a.iso)
            quadric["vertices_after"], quadric["triangles_after"] = ctx.decimate_isosurface(h, "quadric")
            if r:
                quadric["kernel_ms"].append(ctx.isosurface_decimate_kernel_ms())
                quadric["pass_ms"].append(ctx.isosurface_decimate_pass_ms())
            else:
                quadric["device_bytes_after"] = int(ctx.info().device_bytes)
    nv, nt, nv2, nt2 = rec["vertices"], rec["triangles"], rec["vertices_after"], rec["triangles_after"]
    rec["kernel_ms_min"] = min(rec["kernel_ms"])
    rec["extraction_kernel_ms_min"] = min(rec["extraction_kernel_ms"])
    rec["over_extraction"] = rec["kernel_ms_min"] / rec["extraction_kernel_ms_min"]
    for p in ("clustering", "representatives", "triangles", "normals"):
        rec[p + "_ms_min"] = min(q[p] for q in rec["pass_ms"])
    # what each pass must move at least: positions read twice (bounds, keys) and key, id and cluster written once; triangles read
    # twice (keys, compaction), key and value written once, survivors written; positions and ids read, representatives written;
    # output triangles and positions read, normals written
    floors = {"clustering": 2 * 24 * nv + 16 * nv, "triangles": 2 * 24 * nt + 16 * nt + 24 * nt2,
              "representatives": 28 * nv + 24 * nv2, "normals": 24 * nt2 + 24 * nv2 + 12 * nv2}
    rec["floor_bytes"] = floors
    rec["floor_ms_c2p_rate"] = {k: v / C2P_TBPS / 1e9 for k, v in floors.items()}
    # the scratch of the call, rocPRIM's own storage aside
    rec["scratch_bytes"] = 2 * max(nv, 2 * nt, 3 * nt) * 8 + 32 * (nv + 1) + 8 * (nt + 1)
    if a.decimate_quadric:
        quadric["kernel_ms_min"] = min(quadric["kernel_ms"])
        for p in ("clustering", "representatives", "triangles", "normals"):
            quadric[p + "_ms_min"] = min(q[p] for q in quadric["pass_ms"])
        quadric["over_mean"] = quadric["kernel_ms_min"] / rec["kernel_ms_min"]
        # its representative pass moves at least: triangles read for the corner keys, key and corner written and read; per corner
        # a triangle's ids and three positions gathered; positions and ids read for the mean, representatives written
        quadric["representatives_floor_bytes"] = 24 * nt + 2 * 8 * 3 * nt + 3 * nt * (24 + 72) + 28 * nv + 24 * nv2
        quadric["representatives_floor_ms_c2p_rate"] = quadric["representatives_floor_bytes"] / C2P_TBPS / 1e9
        # the corner pairs and their sort's other halves fill the key arrays that the normals' incidence sizes anyway (3 T u64 each)
        quadric["scratch_bytes"] = rec["scratch_bytes"]
        quadric["corner_pair_bytes"] = 4 * 3 * nt * 4
    if a.decimate_check:
        t0 = time.perf_counter()
        want = D.decimate(raw[0], raw[1], h, raw[2])
        rec["host_numpy_s"] = time.perf_counter() - t0
        rec["host_matches_gpu"] = all(w.tobytes() == g.tobytes() for w, g in zip(want, got))
        if a.decimate_quadric:
            import isosurface_decimate_quadric_np as Q
            got = ctx.download_isosurface() + (ctx.download_isosurface_normals(),)
            t0 = time.perf_counter()
            want = Q.decimate(raw[0], raw[1], h, raw[2])
            quadric["host_numpy_s"] = time.perf_counter() - t0
            quadric["host_matches_gpu"] = all(w.tobytes() == g.tobytes() for w, g in zip(want, got))
    return rec


def holes_record(ctx, a, spacing):
    """The --holes record: dmi_fill_isosurface_holes at every a.holes (max_edges) on the mesh of the context's grid at a.iso after the
    support trim (a.holes_min_views views within a.holes_tolerance grid spacings; 0 views: no trim), a.repeat rounds after a warm-up
    round, the values of max_edges alternating inside a round.  In every round the fill follows a fresh extraction with normals
    and a fresh trim.  With a.holes_check the numpy restatement runs on the trimmed mesh and is compared bit for bit."""
    import time

    sys.path.insert(0, os.path.join(ROOT, "tests"))   # the host alternative IS the tests' numpy restatement
    import isosurface_holes_np as H
    rec = {"min_views": a.holes_min_views, "tolerance": a.holes_tolerance * spacing, "runs": {}}
    for r in range(a.repeat + 1):                       # round 0 is the warm-up: buffers sized, code loaded
        for m in a.holes:
            run = rec["runs"].setdefault(str(m), {"max_edges": m, "kernel_ms": [], "pass_ms": []})
            ctx.extract_isosurface_with_normals(a.iso)
            if a.holes_min_views > 0:
                ctx.filter_isosurface_support(a.holes_min_views, a.holes_tolerance * spacing)
            if r == a.repeat and a.holes_check:
                raw = ctx.download_isosurface() + (ctx.download_isosurface_normals(),)
            run["vertices"], run["triangles"] = ctx._current_mesh_counts()[:2]
            run["vertices_after"], run["triangles_after"], run["filled"], run["boundary_edges_left"] = ctx.fill_isosurface_holes(m)
            if r:
                run["kernel_ms"].append(ctx.isosurface_holes_kernel_ms())
                run["pass_ms"].append(ctx.isosurface_holes_pass_ms())
            if r == a.repeat and a.holes_check:
                got = ctx.download_isosurface() + (ctx.download_isosurface_normals(),)
                t0 = time.perf_counter()
                want = H.fill(raw[0], raw[1], m, raw[2])
                run["host_numpy_s"] = time.perf_counter() - t0
                run["host_matches_gpu"] = all(want[k].tobytes() == g.tobytes() for k, g in zip(("vertices", "triangles", "normals"), got))
                sizes = want["loop_sizes"]
                run["boundary_edges"] = want["boundary_edges_left"] + sum(len(h) for h in want["filled"])
                run["loops"], run["longest_loop"] = len(sizes), max(sizes, default=0)
                run["longest_filled"] = max((len(h) for h in want["filled"]), default=0)
    for run in rec["runs"].values():
        run["kernel_ms_min"] = min(run["kernel_ms"])
        for p in ("boundary", "loops", "fill"):
            run[p + "_ms_min"] = min(q[p] for q in run["pass_ms"])
    return rec


def color_record(ctx, a, spacing):
    """The --color record: the mesh of the context's grid at a.iso coloured from the scene's first a.color_views views, the calls
    alternating in one process, a.repeat times each.  The mesh is extracted in a second context that holds those views (the fused
    test wants the same views on both sides) and a copy of the grid.  (i) dmi_color_process on the downloaded vertices against the
    in-place call: kernel and call wall time; (ii) the fused test against the own-planes test and the plain pass (the plain pass is (i)'s in-place call): kernel time, and
    the HBM the fused form does not allocate; (iii) the same after a decimation at a.color_decimate grid spacings."""
    import time

    import numpy as np
    n = a.color_views
    tol = 2.0 * spacing
    grid = scene.default_grid(a.grid)
    cells = ctx.download_grid()
    rec = {"views": n, "tolerance": tol, "meshes": []}
    with capi.FusionContext(grid, scene.default_ray_potential(grid)) as fc, capi.ColorContext() as plain, capi.ColorContext() as own:
        for c0 in range(0, n, 32):
            v, thr = scene.make_scene_views("speckle", 256, 1280, 720, seed=1000, view_range=(c0, min(n, c0 + 32)), noise_sigma=spacing)
            colors = scene.make_colors(v.n, 1280, 720, seed=2000 + c0)
            fc.add_views(v, threshold=thr)
            plain.add_views(colors, v.K4, v.RT4)
            own.add_views(colors, v.K4, v.RT4, depths=v.depth)
        own.set_depth_test(True, tol)
        rec["own_planes_bytes_not_allocated"] = n * ((1280 + 7) // 8) * ((720 + 3) // 4) * 32 * 8
        fc.upload_grid(cells)
        del cells
        verts, _ = fc.extract_isosurface(a.iso)
        for label in ("raw", "decimated"):
            if label == "decimated":
                fc.decimate_isosurface(a.color_decimate * float(min(grid.spacing)))
                verts, _ = fc.download_isosurface()
            m = {"mesh": label, "vertices": len(verts), "copy_bytes": len(verts) * 34, "copying": {"kernel_ms": [], "wall_ms": []},
                 "in_place": {"kernel_ms": [], "wall_ms": []}, "fused_kernel_ms": [], "own_planes_kernel_ms": []}
            if label == "decimated":
                m["cell_size_spacings"] = a.color_decimate
            for r in range(a.repeat + 1):                   # the first round warms up: buffers sized, code loaded
                t0 = time.perf_counter()
                want = plain.process(verts)
                t1 = time.perf_counter()
                k_copying = plain.kernel_ms()               # (the in-place call below overwrites it)
                fc.color_isosurface(plain)
                t2 = time.perf_counter()
                got = fc.download_isosurface_colors() if r == 0 else None
                k_in_place = fc.isosurface_color_kernel_ms()
                own.process(verts)
                k_own = own.kernel_ms()
                fc.color_isosurface(plain, fused_depth_tolerance=tol)
                k_fused = fc.isosurface_color_kernel_ms()
                if r == 0:
                    m["in_place_equals_copying"] = all(np.array_equal(x, y) for x, y in zip(got, want))
                    continue
                m["copying"]["kernel_ms"].append(k_copying)
                m["copying"]["wall_ms"].append(1e3 * (t1 - t0))
                m["in_place"]["kernel_ms"].append(k_in_place)
                m["in_place"]["wall_ms"].append(1e3 * (t2 - t1))
                m["own_planes_kernel_ms"].append(k_own)
                m["fused_kernel_ms"].append(k_fused)
            rec["meshes"].append(m)
    return rec


FP64_VECTOR_TFLOPS = 78.6   # MI355X peak fp64 vector rate (FMA = 2)


def render_record(ctx, a, spacing):
    """The --render-depths record: the mesh of the context's grid at a.iso rendered into the scene's first a.render_views views
    (dmi_color_render_isosurface_depths), a.repeat times after a warm-up call: the kernels' span, the fill, the small and the large
    passes, the queued (triangle, view) pairs; then, alternating, the colouring with the rendered planes (the colour context's own
    test) and with the fused depths, both in place at a tolerance of two voxels.  Floors: the projections on the fp64 vector rate
    (three vertices of 33 operations and two divisions each, counted at 30 operations a division), the fill at the HBM rate."""
    n = a.render_views
    tol = 2.0 * spacing
    grid = scene.default_grid(a.grid)
    cells = ctx.download_grid()
    rec = {"views": n, "tolerance": tol, "kernel_ms": [], "pass_ms": [], "queued_pairs": None, "color_rendered_kernel_ms": [],
           "color_fused_kernel_ms": [], "queue_capacity": a.render_queue}
    with capi.FusionContext(grid, scene.default_ray_potential(grid)) as fc, capi.ColorContext() as c:
        for c0 in range(0, n, 32):
            v, thr = scene.make_scene_views("speckle", 256, 1280, 720, seed=1000, view_range=(c0, min(n, c0 + 32)), noise_sigma=spacing)
            fc.add_views(v, threshold=thr)
            c.add_views(scene.make_colors(v.n, 1280, 720, seed=2000 + c0), v.K4, v.RT4)
        fc.upload_grid(cells)
        del cells
        verts, tris = fc.extract_isosurface(a.iso)
        rec["vertices"], rec["triangles"] = len(verts), len(tris)
        if a.render_queue:
            c.set_render_queue_capacity(a.render_queue)
        for r in range(a.repeat + 1):                       # the first round warms up: buffers sized, code loaded
            fc.render_isosurface_depths(c)
            k, p, q = c.render_kernel_ms(), c.render_pass_ms(), c.render_queued_pairs()
            c.set_depth_test(True, tol)
            fc.color_isosurface(c)
            k_rendered = fc.isosurface_color_kernel_ms()
            c.set_depth_test(False)
            fc.color_isosurface(c, fused_depth_tolerance=tol)
            k_fused = fc.isosurface_color_kernel_ms()
            if r == 0:
                continue
            rec["kernel_ms"].append(k)
            rec["pass_ms"].append(p)
            rec["queued_pairs"] = q
            rec["color_rendered_kernel_ms"].append(k_rendered)
            rec["color_fused_kernel_ms"].append(k_fused)
    rec["kernel_ms_min"] = min(rec["kernel_ms"])
    for p in ("init", "small", "large"):
        rec[p + "_ms_min"] = min(x[p] for x in rec["pass_ms"])
    rec["color_rendered_kernel_ms_min"] = min(rec["color_rendered_kernel_ms"])
    rec["color_fused_kernel_ms_min"] = min(rec["color_fused_kernel_ms"])
    pairs = rec["triangles"] * n
    rec["projections"] = pairs
    rec["projection_floor_ms_fp64_vector"] = pairs * 3 * (33 + 2 * 30) / (FP64_VECTOR_TFLOPS * 1e12) * 1e3
    rec["plane_bytes"] = n * ((1280 + 7) // 8) * ((720 + 3) // 4) * 32 * 8
    rec["init_floor_ms_8tbps"] = rec["plane_bytes"] / HBM_TBPS / 1e9
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iso", type=float, default=1.0)
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--normals", action="store_true", help="also time the call with normals, alternating with the plain one")
    ap.add_argument("--components", action="store_true", help="also time the connected-components filter after the extraction")
    ap.add_argument("--min-triangles", type=int, default=100, help="the mid threshold of --components")
    ap.add_argument("--smooth", type=int, default=0, help="also time the Taubin smoothing with this many iterations (0: not)")
    ap.add_argument("--smooth-lambda", type=float, default=0.5)
    ap.add_argument("--smooth-mu", type=float, default=-0.53)
    ap.add_argument("--decimate", type=float, action="append", default=[],
                    help="also time the vertex clustering with cells of this many grid spacings (may be given several times)")
    ap.add_argument("--decimate-check", action="store_true", help="... and compare each with the numpy restatement, bit for bit")
    ap.add_argument("--decimate-quadric", action="store_true",
                    help="... and time the quadric placement (dmi_decimate_isosurface_placed) next to each, in the same rounds")
    ap.add_argument("--color", action="store_true", help="also time the coloration of the device mesh against dmi_color_process")
    ap.add_argument("--color-views", type=int, default=64, help="... from the scene's first this many views")
    ap.add_argument("--color-decimate", type=float, default=2.0, help="... and again after a decimation at this many grid spacings")
    ap.add_argument("--render-depths", action="store_true", help="also time the rendering of the mesh's own depth planes and the colouring with them")
    ap.add_argument("--render-views", type=int, default=256, help="... into the scene's first this many views")
    ap.add_argument("--render-queue", type=int, default=0, help="... with this queue capacity (0: the default)")
    ap.add_argument("--holes", type=int, action="append", default=[],
                    help="also time the hole filler at this max_edges (may be given several times) on the mesh the support trim leaves")
    ap.add_argument("--holes-min-views", type=int, default=3, help="... the trim's views (0: no trim)")
    ap.add_argument("--holes-tolerance", type=float, default=2.0, help="... and its depth tolerance in grid spacings")
    ap.add_argument("--holes-check", action="store_true", help="... and compare each with the numpy restatement, bit for bit")
    ap.add_argument("--image", type=int, nargs=2, default=[1280, 720], help="the views' width and height (cfg 2: 640 480)")
    ap.add_argument("--grid", type=int, default=512, help="cells per axis (512: the cfg-3 grid)")
    a = ap.parse_args()
    grid = scene.default_grid(a.grid)
    ray = scene.default_ray_potential(grid)
    spacing = float(max(grid.spacing))
    with capi.FusionContext(grid, ray) as ctx:
        for c0 in range(0, a.views, 32):
            v, thr = scene.make_scene_views("speckle", 256, a.image[0], a.image[1], seed=1000, view_range=(c0, min(a.views, c0 + 32)),
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
        comp = components_record(ctx, a) if a.components else None
        smooth = smooth_record(ctx, a) if a.smooth > 0 else None
        decimate = []
        for h in a.decimate:
            decimate.append(decimate_record(ctx, argparse.Namespace(**{**vars(a), "decimate": h})))
        holes = holes_record(ctx, a, spacing) if a.holes else None
        color = color_record(ctx, a, spacing) if a.color else None
        render = render_record(ctx, a, spacing) if a.render_depths else None
    n_points = (a.grid + 1) ** 3
    lattice = n_points * 8
    out = {"iso": a.iso, "views": a.views, "vertices": nv, "triangles": nt, "kernel_ms": times, "kernel_ms_min": min(times),
           "lattice_bytes": lattice, "mesh_bytes": nv * 24 + nt * 24,
           "floor_ms_8tbps": lattice / HBM_TBPS / 1e9, "floor_ms_c2p_rate": lattice / C2P_TBPS / 1e9,
           "two_reads_floor_ms_8tbps": 2 * lattice / HBM_TBPS / 1e9}
    if a.normals:
        out.update({"normals_kernel_ms": ntimes, "normals_kernel_ms_min": min(ntimes), "normals_bytes": nv * 12,
                    "normals_over_plain_min": min(ntimes) / min(times)})
    if comp is not None:
        out["components"] = comp
    if smooth is not None:
        out["smooth"] = smooth
    if decimate:
        out["decimate"] = decimate
    if holes is not None:
        out["holes"] = holes
    if color is not None:
        out["color"] = color
    if render is not None:
        out["render_depths"] = render
    print(json.dumps(out))


if __name__ == "__main__":
    main()
