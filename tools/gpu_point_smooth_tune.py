#!/usr/bin/env python3
"""Times the point smoothing (dmi_set_point_smoothing) on a 512^3-cell f64 grid, sigma (1, 1, 1) and (2, 2, 2), truncate 3: the plain
form (three launches, one thread per point: DMI_PSMOOTH_PLAIN=1) against the tiled form (x and y fused through LDS, z columns) at the
tile heights a tuning build holds (DMI_PSMOOTH_BY, DMI_PSMOOTH_KZ), beside the cell -> point kernel of the same run and the floor of
two reads and two writes of the point data at the bandwidth that kernel reached.  Needs the tuning library: DMI_TUNING=1 at build time
and in the environment of this script.  Without it (the shipped library) only the shipped form is timed.  Prints one JSON record per
configuration; with a file name as its argument it writes them there as well."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cudadepthmapintegration_amd import build, capi, scene  # noqa: E402

N = int(os.environ.get("DMI_PSMOOTH_CELLS", "512"))
tuning = bool(os.environ.get("DMI_TUNING"))
grid = scene.default_grid((N, N, N))
ray = scene.default_ray_potential(grid)
# a caller-owned grid: the context recomputes the point data, and smooths it, on every call
g = torch.randn(N ** 3, dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
ctx = capi.FusionContext(grid, ray, grid_dtype="f64", external_grid=g.data_ptr())
point_bytes = 8 * (N + 1) ** 3
c2p_bytes = 8 * N ** 3 + point_bytes
digest = open(build.LIB_PATH + ".digest").read().strip() if os.path.exists(build.LIB_PATH + ".digest") else None
forms = [("plain", None, None), ("tiled", 16, 8), ("tiled", 16, 4), ("tiled", 16, 16), ("tiled", 16, 32), ("tiled", 8, 8), ("tiled", 32, 8)] if tuning \
    else [("tiled", 16, 8)]
res = []
for sigma in (1.0, 2.0):
    for form, by, kz in forms:
        os.environ["DMI_PSMOOTH_PLAIN"] = "1" if form == "plain" else "0"
        os.environ["DMI_PSMOOTH_BY"], os.environ["DMI_PSMOOTH_KZ"] = str(by or 16), str(kz or 8)
        ctx.set_point_smoothing(0.0)
        ctx.set_point_smoothing(sigma, 3.0)
        smooth, c2p = [], []
        for _ in range(11):
            ctx.cell_to_point()
            ctx.synchronize()
            smooth.append(ctx.point_smoothing_kernel_ms())
            c2p.append(ctx.timings().last_cell_to_point_ms)
        ms, c2p_ms = float(np.median(smooth[1:])), float(np.median(c2p[1:]))
        rate = c2p_bytes / c2p_ms / 1e6  # GB/s
        rec = {"cells": N, "sigma": sigma, "truncate": 3.0, "form": form, "by": by, "kz": kz, "smooth_ms": ms, "smooth_min_ms": float(min(smooth[1:])),
               "cell_to_point_ms": c2p_ms, "cell_to_point_GBps": rate, "floor_ms_two_reads_two_writes": 4 * point_bytes / rate / 1e6,
               "library": os.path.basename(build.LIB_PATH), "digest": digest}
        res.append(rec)
        print(json.dumps(rec), flush=True)
ctx.close()
if len(sys.argv) > 1:  # the records as one JSON file
    json.dump(res, open(sys.argv[1], "w"), indent=1)
