"""Kernel time of dmi_color_process with and without the depth test (dmi_color_set_depth_test) at bench.py's coloration probe
shape: 2 M vertices of the synthetic scene in mesh order (Z-order sorted) x 64 views of 1280 x 720 resident, the depth maps the
sphere's.  The plain and the depth-tested call alternate in one process on the same views; hipEvents around the projection and
median kernels.  Prints one JSON line.

    python tools/gpu_coloration_depth_time.py [--vertices 2000000] [--views 64] [--repeat 5] [--tol 0.01]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cudadepthmapintegration_amd import capi, scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vertices", type=int, default=2_000_000)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--tol", type=float, default=0.01)
    a = ap.parse_args()
    n, W, H = a.views, 1280, 720
    views = scene.make_views(n, 8, 8, seed=77)                      # bench.py's cameras
    K4 = views.K4.copy()
    K4[:, 0, 0] = K4[:, 1, 1] = 0.9 * W
    K4[:, 0, 2], K4[:, 1, 2] = W / 2.0, H / 2.0
    colors = np.empty((n, H, W, 3), dtype=np.uint8)
    colors[:] = (np.arange(H * W * 3, dtype=np.uint32) % 251).astype(np.uint8).reshape(1, H, W, 3)
    depths = np.stack([scene.render_sphere_depth(K4[m, :3, :3], views.RT4[m], W, H) for m in range(n)])
    pts = scene.make_mesh_points(a.vertices, seed=78)
    pts = np.ascontiguousarray(pts[scene.morton_order(pts)])
    plain, tested = [], []
    with capi.ColorContext() as c:
        c.add_views(colors, K4, views.RT4, depths=depths)
        c.process(pts)                                                # warm-up: buffers sized, code loaded
        c.set_depth_test(True, a.tol)
        c.process(pts)
        for _ in range(a.repeat):
            c.set_depth_test(False, a.tol)
            _, _, cnt_plain = c.process(pts)
            plain.append(c.kernel_ms())
            c.set_depth_test(True, a.tol)
            _, _, cnt = c.process(pts)
            tested.append(c.kernel_ms())
    print(json.dumps({"vertices": a.vertices, "views": n, "image": f"{W}x{H}", "order": "mesh (Z-order sorted)", "tol": a.tol,
                      "kernel_ms_plain": plain, "kernel_ms_depth": tested, "plain_min": min(plain), "depth_min": min(tested),
                      "depth_over_plain_min": min(tested) / min(plain),
                      "pairs_counted_plain": int(cnt_plain.sum(dtype=np.int64)), "pairs_counted_depth": int(cnt.sum(dtype=np.int64))}))


if __name__ == "__main__":
    main()
