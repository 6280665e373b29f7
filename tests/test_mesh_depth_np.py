"""tests/mesh_depth_np.py, the numpy restatement of the rendered depth planes (DESIGN.md 8b''), against exact rational arithmetic
on the same u, v, cz -- and the properties the definition promises: a fronto-parallel triangle renders its depth exactly, the
order of the triangles changes no bit.  No GPU."""
import os
import re
from fractions import Fraction

import numpy as np

import mesh_depth_np as md

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 40, 30

# Worst relative error of the restatement's planes against the exact rational evaluation, measured by this test on its 300
# triangles (it prints the figure): 2.880e-15 over 1194 covered pixels.  The bound is four times that.  (An earlier prototype
# measured 6.4e-16 on its own triangles; these include slivers with a depth range of 1 : 3 across a pixel, where the cancellation
# in the edge functions weighs more.)
MEASURED_WORST = 2.880e-15
BOUND = 4 * MEASURED_WORST


def camera():
    K = np.eye(4)
    K[0, 0] = K[1, 1] = 31.0
    K[0, 2], K[1, 2] = 19.3, 14.6
    RT = np.eye(4)
    RT[:3, 3] = (0.11, -0.07, 0.4)
    return K, RT


def random_triangles(rng, n=300):
    """Triangles of 0.7 to 60 pixels (log-uniform) anywhere over the image and a little beyond, camera z in [1, 3]."""
    K, RT = camera()
    size = np.exp(rng.uniform(np.log(0.7), np.log(60.0), n))
    centre = np.stack([rng.uniform(-5, W + 5, n), rng.uniform(-5, H + 5, n)], axis=1)
    px = centre[:, None, :] + (rng.uniform(-0.5, 0.5, (n, 3, 2)) * size[:, None, None])
    z = rng.uniform(1.0, 3.0, (n, 3))
    cam = np.stack([(px[..., 0] - K[0, 2]) / K[0, 0] * z, (px[..., 1] - K[1, 2]) / K[1, 1] * z, z], axis=-1)
    pts = (cam - RT[:3, 3]).reshape(-1, 3)
    tri = np.arange(3 * n, dtype=np.int64).reshape(n, 3)
    return pts, tri, K, RT


def exact_plane(pts, tri, K, RT):
    """Per pixel the exact minimum (a Fraction, or None) of d = s / q over the triangles that cover it exactly, evaluated in
    rational arithmetic on the f64 u, v, cz that the restatement's projection produced."""
    u, v, cz, ok = md.project(pts, K, RT)
    best = [[None] * W for _ in range(H)]
    for t in tri:
        if not ok[t].all():
            continue
        x0, x1, y0, y1 = (float(a[0]) for a in md.pixel_ranges(u[t][None], v[t][None], W, H))
        if not (x0 <= x1 and y0 <= y1):
            continue
        U, V, Z = ([Fraction(float(a)) for a in arr[t]] for arr in (u, v, cz))
        for y in range(int(y0), int(y1) + 1):
            for x in range(int(x0), int(x1) + 1):
                e0 = (U[2] - U[1]) * (y - V[1]) - (V[2] - V[1]) * (x - U[1])
                e1 = (U[0] - U[2]) * (y - V[2]) - (V[0] - V[2]) * (x - U[2])
                e2 = (U[1] - U[0]) * (y - V[0]) - (V[1] - V[0]) * (x - U[0])
                s = e0 + e1 + e2
                if s == 0 or not ((e0 >= 0 and e1 >= 0 and e2 >= 0) or (e0 <= 0 and e1 <= 0 and e2 <= 0)):
                    continue
                d = s / (e0 / Z[0] + e1 / Z[1] + e2 / Z[2])
                if d > 0 and (best[y][x] is None or d < best[y][x]):
                    best[y][x] = d
    return best


def test_restatement_is_within_four_times_its_measured_error_of_exact_rational_arithmetic():
    """Measured worst relative error: 2.880e-15 (printed below); asserted bound: 4 x that."""
    pts, tri, K, RT = random_triangles(np.random.default_rng(20260101))
    plane = md.render_view_np(pts, tri, K, RT, W, H)
    exact = exact_plane(pts, tri, K, RT)
    worst, covered = 0.0, 0
    for y in range(H):
        for x in range(W):
            if exact[y][x] is None:
                assert np.isinf(plane[y, x]), (x, y)
                continue
            assert np.isfinite(plane[y, x]), (x, y)
            covered += 1
            worst = max(worst, float(abs(Fraction(float(plane[y, x])) - exact[y][x]) / exact[y][x]))
    print(f"worst relative error against exact rational arithmetic: {worst:.3e} over {covered} covered pixels")
    assert covered > W * H // 2
    assert worst <= BOUND


def test_fronto_parallel_triangle_renders_its_depth_exactly():
    K, RT = camera()
    z = 1.7
    px = np.array([[3.2, 2.1], [35.7, 6.4], [12.9, 27.3]])
    cam = np.stack([(px[:, 0] - K[0, 2]) / K[0, 0] * z, (px[:, 1] - K[1, 2]) / K[1, 1] * z, np.full(3, z)], axis=-1)
    pts = cam - RT[:3, 3]
    pts[:, 2] = z - RT[2, 3]            # the same camera z for all three, whatever the rounding above did
    _, _, cz, _ = md.project(pts, K, RT)
    assert cz[0] == cz[1] == cz[2]
    plane = md.render_view_np(pts, [[0, 1, 2]], K, RT, W, H)
    hit = np.isfinite(plane)
    assert hit.sum() > 100
    # s carries two roundings, q = (e0/z + e1/z) + e2/z five (same-sign terms: no cancellation), the last division one: within
    # 8 u of z, u = 2^-53 -- and EXACT when every quotient is, which a power of two as the depth guarantees
    assert np.abs(plane[hit] / cz[0] - 1.0).max() <= 9 * 2.0 ** -53
    pts2 = pts.copy()
    pts2[:, 2] = 2.0 - RT[2, 3]
    _, _, cz2, _ = md.project(pts2, K, RT)
    assert (cz2 == 2.0).all()
    plane2 = md.render_view_np(pts2, [[0, 1, 2]], K, RT, W, H)
    assert (plane2[np.isfinite(plane2)] == 2.0).all() and np.isfinite(plane2).sum() > 100


def test_the_order_of_the_triangles_changes_no_bit():
    pts, tri, K, RT = random_triangles(np.random.default_rng(7), 120)
    a = md.render_view_np(pts, tri, K, RT, W, H)
    b = md.render_view_np(pts, tri[::-1], K, RT, W, H)
    c = md.render_view_np(pts, tri[:, ::-1], K, RT, W, H)   # the other winding covers the same pixels ...
    assert a.tobytes() == b.tobytes()
    assert (np.isfinite(a) == np.isfinite(c)).all()            # ... (its depths may differ in the last bits: other operand order)


def test_to_vtk_depths_flips_rows_and_marks_empty_pixels():
    p = np.full((1, 3, 2), np.inf)
    p[0, 0, 1] = 2.5
    out = md.to_vtk_depths(p)
    assert out.shape == (1, 3, 2) and out[0, 2, 1] == 2.5 and (np.delete(out.ravel(), 5) == -1.0).all()


NEW_SYMBOLS = ["dmi_color_render_depths", "dmi_color_render_isosurface_depths", "dmi_color_download_depths",
               "dmi_color_get_render_kernel_ms", "dmi_color_set_render_queue_capacity", "dmi_color_get_render_pass_ms",
               "dmi_color_get_render_queued_pairs"]


def test_header_and_binding_list_hold_the_new_symbols():
    from cudadepthmapintegration_amd import capi

    text = open(os.path.join(ROOT, "include", "dmi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in capi.ABI_SYMBOLS
    for method in ("render_depths", "download_depths", "render_kernel_ms", "set_render_queue_capacity", "render_pass_ms", "render_queued_pairs"):
        assert callable(getattr(capi.ColorContext, method))
    assert callable(capi.FusionContext.render_isosurface_depths)
    # the constants the tests aim at are the kernel's
    hdr = open(os.path.join(ROOT, "cudadepthmapintegration_amd", "csrc", "mesh_depth_render.h")).read()
    assert int(re.search(r"kRenderViewGroup = (\d+)", hdr).group(1)) == capi.RENDER_VIEW_GROUP
    assert int(re.search(r"kRenderLaneCap = (\d+)", hdr).group(1)) == capi.RENDER_LANE_CAP


def test_null_arguments_are_refused_without_a_gpu():
    import ctypes

    from cudadepthmapintegration_amd import capi

    L = capi.load()
    v = ctypes.c_double(0)
    assert L.dmi_color_render_depths(None, None, 0, None, 0) == 1
    assert b"dmi_color_render_depths" in L.dmi_color_last_error()
    assert L.dmi_color_download_depths(None, 0, 0, None) == 1
    assert L.dmi_color_get_render_kernel_ms(None, ctypes.byref(v)) == 1
    assert L.dmi_color_set_render_queue_capacity(None, 4) == 1
    assert L.dmi_color_get_render_pass_ms(None, (ctypes.c_double * 3)()) == 1
    assert L.dmi_color_get_render_queued_pairs(None, ctypes.byref(ctypes.c_uint64(0))) == 1
    assert L.dmi_color_render_isosurface_depths(None, None) == 1


def test_small_pass_uses_no_scratch_memory():
    """The small pass keeps a projected triangle in registers: its kernel descriptor asks for no private segment."""
    import shutil
    import subprocess
    import tempfile

    import pytest

    from cudadepthmapintegration_amd import build as b

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "r.s")
        r = subprocess.run([hipcc] + b.COMMON_FLAGS + b.HIP_FLAGS + ["--cuda-device-only", "-S", os.path.join(b.CSRC, "mesh_depth_render.hip"), "-o", out],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        text = open(out).read()
    sizes = {m.group(1): int(m.group(2)) for m in re.finditer(
        r"\.amdhsa_kernel (\S+)\b.*?\.amdhsa_private_segment_fixed_size (\d+)", text, re.S)}
    small = [k for k in sizes if "render_small_kernel" in k]
    assert small and all(sizes[k] == 0 for k in small), sizes
