"""dmi_set_point_smoothing: the library's weights, the CPU restatement (tests/point_smooth_np.py) on cases with exact
results, the CLI flags and the ABI on the CPU; on the GPU every bit of the smoothed point data against the restatement applied to
the GPU's own unsmoothed download with the library's weights, at the tile tails of the kernels, and its consumers and the CLI."""
import ctypes
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import isosurface_normals_np as RN
import isosurface_np as R
import point_smooth_np as PS
import vti_writer
from cudadepthmapintegration_amd import capi, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 1   # DMI_ERR_INVALID_ARGUMENT (include/dmi.h)
NEW_SYMBOLS = ["dmi_point_smoothing_weights", "dmi_set_point_smoothing", "dmi_get_point_smoothing", "dmi_get_point_smoothing_kernel_ms"]


def _weights3(sigma, truncate=3.0):
    """The library's weights for the three axes; sigma a scalar or (x, y, z)."""
    s = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (3,))
    return tuple(capi.point_smoothing_weights(float(v), truncate) for v in s)


# ---- the weights -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.5, 1.0, 2.5, 4.0])
@pytest.mark.parametrize("truncate", [1.0, 3.0, 4.0])
def test_weights_are_the_formula_normalised(sigma, truncate):
    k = capi.point_smoothing_weights(sigma, truncate)
    r = len(k) - 1
    assert r == int(np.ceil(truncate * sigma)) == PS.radius(sigma, truncate)
    assert (k > 0).all() and (np.diff(k) <= 0).all()
    want = PS.weights_np(sigma, truncate)
    assert (np.abs(k - want) <= 4 * np.spacing(want)).all(), (k - want) / np.spacing(want)
    total = Fraction(float(k[0])) + 2 * sum(Fraction(float(x)) for x in k[1:])          # exact
    assert abs(total - 1) <= Fraction(2 * r + 1, 2 ** 53), float(total - 1)


def test_weights_of_sigma_zero_and_refusals():
    k = capi.point_smoothing_weights(0.0, 3.0)
    assert k.tolist() == [1.0]
    assert capi.point_smoothing_weights(4.0, 4.0).shape == (17,)                         # radius 16, the cap
    nan, inf = float("nan"), float("inf")
    for sigma, truncate in ((-1.0, 3.0), (nan, 3.0), (inf, 3.0), (1.0, 0.0), (1.0, -1.0), (1.0, 4.5), (1.0, nan), (1.0, inf),
                            (4.3, 4.0), (4.25, 4.0), (16.5, 1.0)):
        with pytest.raises(capi.DmiError) as e:
            capi.point_smoothing_weights(sigma, truncate)
        assert e.value.code == INVALID_ARGUMENT and "dmi_point_smoothing_weights" in str(e.value), (sigma, truncate)
    L = capi.load()
    r, k = ctypes.c_int32(0), (ctypes.c_double * 17)()
    assert L.dmi_point_smoothing_weights(1.0, 3.0, None, k) == INVALID_ARGUMENT
    assert L.dmi_point_smoothing_weights(1.0, 3.0, ctypes.byref(r), None) == INVALID_ARGUMENT
    assert L.dmi_point_smoothing_weights(1.0, 3.0, ctypes.byref(r), k) == 0 and r.value == 3


# ---- the restatement on cases with exact results -----------------------------------------------------------------------------------
def _scalar_smooth(P, ks):
    """The definition once more, point by point in Python floats (IEEE f64, one rounded operation per line of arithmetic)."""
    P = np.array(P, dtype=np.float64)
    for axis, k in ((2, ks[0]), (1, ks[1]), (0, ks[2])):
        if len(k) == 1:
            continue
        src = np.moveaxis(P, axis, -1)
        out = np.empty_like(src)
        n = src.shape[-1]
        for idx in np.ndindex(src.shape[:-1]):
            line = [float(x) for x in src[idx]]
            for q in range(n):
                acc = float(k[0]) * line[q]
                for i in range(1, len(k)):
                    pair = line[max(q - i, 0)] + line[min(q + i, n - 1)]
                    term = float(k[i]) * pair
                    acc = acc + term
                out[idx + (q,)] = acc
        P = np.ascontiguousarray(np.moveaxis(out, -1, axis))
    return P


def test_interior_impulse_gives_the_products_of_the_weights():
    ks = _weights3((1.0, 0.8, 0.9))
    assert [len(k) - 1 for k in ks] == [3, 3, 3]
    P = np.zeros((15, 15, 15))
    P[7, 7, 7] = 1.0
    Q = PS.smooth(P, ks)
    want = np.zeros_like(P)
    for c in range(-3, 4):
        for b in range(-3, 4):
            for a in range(-3, 4):
                want[7 + c, 7 + b, 7 + a] = float(ks[2][abs(c)]) * (float(ks[1][abs(b)]) * float(ks[0][abs(a)]))
    assert PS.same_bits(Q, want) and np.count_nonzero(Q) == 7 ** 3


def test_corner_impulse_folds_the_clamped_taps_onto_the_border():
    k = capi.point_smoothing_weights(1.0, 3.0)
    k0, k1, k2, k3 = (float(x) for x in k)
    one = [1.0]
    # along x alone: the taps left of the border read the border's 1
    P = np.zeros((2, 2, 9))
    P[:, :, 0] = 1.0
    Q = PS.smooth(P, (k, one, one))
    line = [((k0 + k1) + k2) + k3, ((0.0 + k1) + k2) + k3, ((0.0 + 0.0) + k2) + k3, ((0.0 + 0.0) + 0.0) + k3, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert all(PS.same_bits(Q[z, y], np.array(line)) for z in range(2) for y in range(2))
    # the far border, mirrored
    assert PS.same_bits(PS.smooth(P[:, :, ::-1], (k, one, one)), Q[:, :, ::-1])
    # a corner of a lattice smaller than the radius, every tap clamped, all three axes: the point-by-point loop
    P = np.zeros((3, 4, 5))
    P[0, 0, 0] = 1.0
    P[2, 3, 4] = -2.5
    ks = _weights3((1.0, 1.0, 1.0))
    assert PS.same_bits(PS.smooth(P, ks), _scalar_smooth(P, ks))
    rng = np.random.default_rng(3)
    P = rng.normal(size=(4, 6, 7))
    ks = _weights3((1.5, 0.8, 0.5))
    assert [len(k) - 1 for k in ks] == [5, 3, 2] and PS.same_bits(PS.smooth(P, ks), _scalar_smooth(P, ks))


def test_skipped_axes_return_the_bits_of_the_input():
    P = np.random.default_rng(4).normal(size=(4, 5, 6))
    P[1, 2, 3] = -0.0
    P[0, 0, 0] = np.nan
    P[3, 4, 5] = -np.inf
    one = np.array([1.0])
    Q = PS.smooth(P, (one, one, one))
    assert Q.tobytes() == P.tobytes() and np.signbit(Q[1, 2, 3])
    # one axis on: a plane of -0.0 stays -0.0 along the skipped axes' neighbours ((-0.0) k + k (-0.0 + -0.0) = -0.0)
    Z = np.full((3, 3, 8), -0.0)
    k = capi.point_smoothing_weights(1.0, 3.0)
    assert np.signbit(PS.smooth(Z, (k, one, one))).all()
    # and a skipped axis in the middle leaves what the others make
    ks = (k, one, capi.point_smoothing_weights(0.5, 3.0))
    assert PS.same_bits(PS.smooth(P, ks), _scalar_smooth(P, ks))


def test_nan_spreads_to_its_clamped_box_and_a_constant_stays():
    ks = _weights3((1.0, 0.5, 0.4))
    rx, ry, rz = (len(k) - 1 for k in ks)
    assert (rx, ry, rz) == (3, 2, 2)
    P = np.random.default_rng(5).normal(size=(9, 10, 11))
    P[1, 8, 5] = np.nan
    Q = PS.smooth(P, ks)
    box = np.zeros(P.shape, dtype=bool)
    box[max(1 - rz, 0):1 + rz + 1, max(8 - ry, 0):8 + ry + 1, 5 - rx:5 + rx + 1] = True
    assert np.array_equal(np.isnan(Q), box) and box.sum() == 4 * 4 * 7
    for c in (1.0, 0.8 * 37, -3.0e-7):
        Q = PS.smooth(np.full((8, 9, 10), c), _weights3(1.0))
        assert (np.abs(Q - c) <= 3 * np.spacing(abs(c))).all(), np.abs(Q - c).max() / np.spacing(abs(c))


# ---- ABI and CLI flags ------------------------------------------------------------------------------------------------------------------
def test_abi_has_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "dmi.h")).read()
    lib = ctypes.CDLL(capi.load()._name)
    for name in NEW_SYMBOLS:
        assert name + "(" in header and name in capi.ABI_SYMBOLS and hasattr(lib, name), name
    assert lib.dmi_abi_version() == 5 and "#define DMI_ABI_VERSION 5 " in header
    for name in ("set_point_smoothing", "point_smoothing", "point_smoothing_kernel_ms"):
        assert callable(getattr(capi.FusionContext, name)), name
    L = capi.load()
    s = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    assert L.dmi_set_point_smoothing(None, s, 3.0) == INVALID_ARGUMENT
    assert "dmi_set_point_smoothing" in L.dmi_last_error(None).decode()
    assert L.dmi_get_point_smoothing(None, s, None) == INVALID_ARGUMENT
    assert L.dmi_get_point_smoothing_kernel_ms(None, None) == INVALID_ARGUMENT
    from cudadepthmapintegration_amd import build
    assert "point_smooth.hip" in build.SOURCES                     # in the digest: a change to the kernels rebuilds the library


BASE = ["Reconstruction", "--gridOrigin", "-2.29", "-2.24", "-2.2", "--gridEnd", "1.19", "1.67", "1.22", "--dataFolder", "data",
        "--outputGridFilename", "out.vts", "--outputMeshFilename", "mesh.vtp", "--rayThick", "0.1", "--gridDims", "10"]


def test_cli_contour_smoothing_flags():
    o, text = capi.cli_read_arguments(BASE + ["--extractMesh"])
    assert o is not None and list(o.contour_smooth_sigma) == [0.0, 0.0, 0.0] and o.contour_smooth_truncate == 3.0, text
    o, text = capi.cli_read_arguments(BASE + ["--extractMesh", "--contourSmoothSigma", "1.5"])
    assert o is not None and list(o.contour_smooth_sigma) == [1.5, 1.5, 1.5] and o.contour_smooth_truncate == 3.0, text
    o, text = capi.cli_read_arguments(BASE + ["--extractMesh", "--contourSmoothSigma", "1", "0", "2.5", "--contourSmoothTruncate", "4", "--meshFillHoles", "9"])
    assert o is not None and list(o.contour_smooth_sigma) == [1.0, 0.0, 2.5] and o.contour_smooth_truncate == 4.0, text
    assert (o.mesh_fill_holes, o.extract_mesh, o.grid_auto_bounds_pixel_step) == (9, 1, 1)      # every earlier field keeps its place
    o, text = capi.cli_read_arguments(BASE + ["--contourSmoothTruncate", "2", "--extractMesh", "--contourSmoothSigma", "5.4", "8", "0.1"])
    assert o is not None and list(o.contour_smooth_sigma) == [5.4, 8.0, 0.1], text          # radii 11, 16, 1
    for flag in (["--contourSmoothSigma", "1"], ["--contourSmoothSigma", "0"], ["--contourSmoothSigma", "1", "1", "1"], ["--contourSmoothTruncate", "2"]):
        o, text = capi.cli_read_arguments(BASE + flag)
        assert o is None and text.split("\n")[0].startswith("Error : " + flag[0] + " needs --extractMesh"), text
    bad = [["-1"], ["nan"], ["inf"], ["x"], [], ["1", "2"], ["1", "2", "3", "4"], ["1", "-0.5", "1"], ["1", "nan", "1"],
           ["5.4"], ["1", "1", "5.34"], ["17"]]                                                 # 3 * 5.4 = 16.2: radius 17
    for values in bad:
        o, text = capi.cli_read_arguments(BASE + ["--extractMesh", "--contourSmoothSigma"] + values)
        assert o is None and text.startswith("Bad value for --contourSmoothSigma"), (values, text)
    o, text = capi.cli_read_arguments(BASE + ["--extractMesh", "--contourSmoothSigma", "4.1", "--contourSmoothTruncate", "4"])
    assert o is None and text.startswith("Bad value for --contourSmoothSigma"), text            # radius 17 by the truncation
    for value in ("0", "-1", "4.5", "nan", "inf", "x"):
        o, text = capi.cli_read_arguments(BASE + ["--extractMesh", "--contourSmoothSigma", "1", "--contourSmoothTruncate", value])
        assert o is None and text.startswith("Bad value for --contourSmoothTruncate"), (value, text)
    o, text = capi.cli_read_arguments(BASE + ["--help"])
    assert o is None and "--contourSmoothSigma v [v ...]" in text and "--contourSmoothTruncate v" in text and "vtkImageGaussianSmooth" in text
    # the tool itself: the usual exit status
    r = subprocess.run([capi.cli_binary()] + BASE[1:] + ["--contourSmoothSigma", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--contourSmoothSigma needs --extractMesh" in r.stderr
    r = subprocess.run([capi.cli_binary()] + BASE[1:] + ["--extractMesh", "--contourSmoothSigma", "6"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "Bad value for --contourSmoothSigma" in r.stderr


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _context(cells, grid_dtype="f64", **kw):
    nz, ny, nx = cells.shape
    grid = scene.default_grid((nx, ny, nz))
    ctx = capi.FusionContext(grid, scene.default_ray_potential(grid), grid_dtype=grid_dtype, **kw)
    ctx.upload_grid(cells)
    return ctx


def _cells(dims, seed=0):
    nx, ny, nz = dims
    return np.random.default_rng(seed).normal(0.5, 1.0, size=(nz, ny, nx))


def _check(ctx, sigma, truncate):
    """Off, on, and every bit of the second download against the restatement of the first; returns both."""
    ctx.set_point_smoothing(0.0)
    P = ctx.download_point_data()
    assert ctx.point_smoothing_kernel_ms() == 0.0
    ctx.set_point_smoothing(sigma, truncate)
    Q = ctx.download_point_data()
    want = PS.smooth(P, _weights3(sigma, truncate))
    differ = ~((Q.view(np.uint64) == want.view(np.uint64)) | (np.isnan(Q) & np.isnan(want)))
    print(f"cells {ctx.grid.cell_dims} sigma {sigma} truncate {truncate}: {int(differ.sum())} of {Q.size} points differ, "
          f"kernels {ctx.point_smoothing_kernel_ms():.4f} ms")
    assert not differ.any(), np.argwhere(differ)[:8].tolist()
    s, t = ctx.point_smoothing()
    assert s.tolist() == np.broadcast_to(np.asarray(sigma, dtype=np.float64), (3,)).tolist() and t == truncate
    assert ctx.point_smoothing_kernel_ms() > 0.0
    return P, Q


# cell dims, sigma, truncate: everything clamped; two-point axes and x over three tiles; the tile tails on either side of the kernels'
# 64 x 16 tiles and 8-point columns (63, 64, 65 x 16, 17, 18 x 8, 9, 10 points) with three different radii; long z columns with
# the larger radius on z; skipped axes; radius 16, the cap, larger than the z axis
GPU_CASES = [((5, 4, 3), (1.0, 1.0, 1.0), 3.0), ((130, 1, 1), (2.0, 0.0, 0.0), 3.0),
             ((62, 15, 7), (1.5, 0.8, 0.5), 3.0), ((63, 16, 8), (1.5, 0.8, 0.5), 3.0), ((64, 17, 9), (1.5, 0.8, 0.5), 3.0),
             ((9, 5, 31), (0.5, 0.8, 1.5), 3.0), ((6, 3, 32), (0.5, 0.8, 1.5), 3.0), ((3, 2, 66), (0.0, 0.4, 1.5), 3.0),
             ((70, 33, 17), (0.0, 2.0, 0.0), 3.0), ((70, 33, 17), (0.0, 0.0, 2.0), 3.0), ((70, 33, 17), (2.0, 0.0, 0.0), 3.0),
             ((40, 20, 9), (4.0, 4.0, 4.0), 4.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("dims,sigma,truncate", GPU_CASES)
def test_gpu_smoothed_point_data_is_the_restatement_bit_for_bit(dims, sigma, truncate):
    with _context(_cells(dims, seed=sum(dims))) as ctx:
        P, Q = _check(ctx, sigma, truncate)
        assert not PS.same_bits(P, Q)


@pytest.mark.gpu
def test_gpu_f32_grid_and_special_values():
    cells = _cells((37, 18, 11), 6)
    with _context(cells, grid_dtype="f32") as ctx:
        P, _ = _check(ctx, (1.0, 0.7, 1.2), 3.0)
        assert PS.same_bits(P, np.asarray(_context_free_c2p(cells.astype(np.float32).astype(np.float64))))
    cells[4, 9, 20] = np.nan
    cells[0, 0, 0] = np.inf
    cells[10, 17, 36] = -np.inf
    cells[6:9, 3:7, 5:30] = -0.0
    with _context(cells) as ctx:
        P, Q = _check(ctx, (1.0, 0.7, 1.2), 3.0)
        assert np.isnan(Q).sum() > np.isnan(P).sum() > 0 and np.isposinf(Q).any() and np.isneginf(Q).any()
        assert (P == 0).any()               # (the cell -> point pass sums from +0.0: the block's interior is +0.0 in the point data)
        _check(ctx, (0.0, 0.0, 0.6), 2.0)


def _context_free_c2p(cells):
    """vtkCellDataToPointData by the oracle: what the unsmoothed download must be."""
    from oracle import oracle
    return oracle.cell_to_point(cells)


@pytest.mark.gpu
def test_gpu_setting_state_and_refusals():
    lib = capi.load()
    cells = _cells((21, 13, 10), 7)
    with _context(cells) as ctx:
        assert ctx.point_smoothing()[0].tolist() == [0.0, 0.0, 0.0] and ctx.point_smoothing()[1] == 3.0
        P, Q = _check(ctx, 1.0, 3.0)
        p = ctypes.c_void_p()
        assert lib.dmi_point_data_device_pointer(ctx._h, ctypes.byref(p)) == 0
        pointer = p.value
        # the same values again: nothing is recomputed; bad arguments: code 1, the old setting kept
        ctx.set_point_smoothing((1.0, 1.0, 1.0), 3.0)
        assert PS.same_bits(ctx.download_point_data(), Q)
        for sigma, truncate in (((1.0, -1.0, 1.0), 3.0), ((float("nan"), 1.0, 1.0), 3.0), ((1.0, 1.0, float("inf")), 3.0),
                                ((1.0, 1.0, 1.0), 0.0), ((1.0, 1.0, 1.0), 4.5), ((1.0, 5.4, 1.0), 3.0)):
            with pytest.raises(capi.DmiError) as e:
                ctx.set_point_smoothing(sigma, truncate)
            assert e.value.code == INVALID_ARGUMENT and "dmi_set_point_smoothing" in str(e.value)
            assert ctx.point_smoothing()[0].tolist() == [1.0, 1.0, 1.0] and ctx.point_smoothing()[1] == 3.0
        assert lib.dmi_set_point_smoothing(ctx._h, None, 3.0) == INVALID_ARGUMENT
        assert PS.same_bits(ctx.download_point_data(), Q) and ctx.point_smoothing_kernel_ms() > 0.0
        # new values in the grid with the setting on: the restatement of the new data
        cells2 = _cells((21, 13, 10), 8)
        ctx.upload_grid(cells2)
        Q2 = ctx.download_point_data()
        assert PS.same_bits(Q2, PS.smooth(_context_free_c2p(cells2), _weights3(1.0))) and not PS.same_bits(Q2, Q)
        assert lib.dmi_point_data_device_pointer(ctx._h, ctypes.byref(p)) == 0 and p.value == pointer
        # another setting, one pass instead of two: the result is still where the consumers look
        ctx.set_point_smoothing((0.0, 0.0, 1.0))
        assert PS.same_bits(ctx.download_point_data(), PS.smooth(_context_free_c2p(cells2), _weights3((0.0, 0.0, 1.0))))
        # off again: the bits of a context in which it was never set, and no kernel time
        ctx.set_point_smoothing(0.0)
        assert ctx.point_smoothing_kernel_ms() == 0.0
        assert PS.same_bits(ctx.download_point_data(), _context_free_c2p(cells2)) and ctx.point_smoothing_kernel_ms() == 0.0
        ctx.upload_grid(cells)
        assert PS.same_bits(ctx.download_point_data(), P)
    # a z-slab's context is refused, as the extraction refuses it
    grid = scene.default_grid((8, 8, 64))
    with capi.FusionContext(grid, scene.default_ray_potential(grid), z_first=32) as ctx:
        with pytest.raises(capi.DmiError) as e:
            ctx.set_point_smoothing(1.0)
        assert e.value.code == INVALID_ARGUMENT and "z_first" in str(e.value)


def _noisy_sphere_cells():
    z, y, x = np.mgrid[0:16, 0:20, 0:24].astype(np.float64)
    f = 6.3 - np.sqrt((x - 11.6) ** 2 + (y - 9.7) ** 2 + (z - 7.8) ** 2)
    return f + np.random.default_rng(9).normal(0.0, 1.2, size=f.shape)


@pytest.mark.gpu
def test_gpu_consumers_read_the_smoothed_field():
    cells = _noisy_sphere_cells()
    with _context(cells) as ctx:
        g = ctx.grid
        M = np.asarray(g.grid_matrix, dtype=np.float64).reshape(4, 4)
        v0, t0 = ctx.extract_isosurface(0.0)
        P, Q = _check(ctx, 1.0, 3.0)
        n, ids = ctx.iso_active_cells(0.0)
        assert np.array_equal(ids, R.emitting_cells(Q, 0.0)) and n == len(ids)
        v, t, nrm = ctx.extract_isosurface_with_normals(0.0)
        wv, wt, wn = RN.extract_with_normals(Q, 0.0, g.origin, g.spacing, M)
        assert v.tobytes() == wv.tobytes() and np.array_equal(t, wt) and nrm.tobytes() == wn.tobytes()
        v1, t1 = ctx.extract_isosurface(0.0)
        assert v1.tobytes() == wv.tobytes() and np.array_equal(t1, wt)
        # the smoothing does what it is for: fewer triangles than the noisy field's surface, and another mesh
        assert 0 < len(t) < len(t0)
        ctx.set_point_smoothing(0.0)
        v2, t2 = ctx.extract_isosurface(0.0)
        assert v2.tobytes() == v0.tobytes() and np.array_equal(t2, t0)


@pytest.mark.gpu
def test_gpu_cli_contour_smoothing_end_to_end(tmp_path):
    """dmi_reconstruction --extractMesh with and without --contourSmoothSigma 1 on a tiny scene: the volumes are the same bytes, and
    the mesh with the flag is the restatements' mesh of the smoothed point data of the .mha."""
    import test_cli as TC
    grid = scene.default_grid((24, 20, 16))
    rp = scene.default_ray_potential(grid)
    views = scene.make_views(4, 48, 36, seed=4, dense=True, with_best_cost=True)
    data = tmp_path / "data"
    data.mkdir()
    names = []
    for m in range(views.n):
        vti_writer.write_vti(str(data / f"frame_{m:04d}.vti"), {"Depths": views.depth[m], "Best Cost Values": views.best_cost[m]},
                             views.depth.shape[2], views.depth.shape[1], mode="appended-raw", header="UInt64")
        scene.write_krtd(str(data / f"frame_{m:04d}.krtd"), views.K4[m][:3, :3], views.RT4[m])
        names.append(f"frame_{m:04d}")
    (data / "vtiList.txt").write_text("".join(f"{i} {n}.vti\n" for i, n in enumerate(names)))
    (data / "kList.txt").write_text("".join(f"{i} {n}.krtd\n" for i, n in enumerate(names)))
    end = [grid.origin[a] + (grid.cell_dims[a] + 1) * grid.spacing[a] for a in range(3)]

    def run(name, flags):
        work = tmp_path / name                     # meta_image_volume.mha goes to the working directory
        work.mkdir()
        args = [capi.cli_binary(), "--dataFolder", str(data), "--gridDims"] + [str(c + 1) for c in grid.cell_dims] + \
               ["--gridOrigin"] + [repr(float(v)) for v in grid.origin] + ["--gridEnd"] + [repr(float(v)) for v in end] + \
               ["--rayThick", repr(rp.thickness), "--rayRho", repr(rp.rho), "--rayEta", repr(rp.eta), "--rayDelta", repr(rp.delta),
                "--threshBestCost", "0.7", "--contour", "0.25", "--outputGridFilename", str(work / "volume.vts"),
                "--outputMeshFilename", str(work / "mesh.vtp"), "--summary", "--extractMesh"] + flags
        r = subprocess.run(args, cwd=str(work), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr + r.stdout
        pd = capi.read_polydata(str(work / "mesh.vtp"))
        return work, args, pd.points.reshape(-1, 3), pd.connectivity.reshape(-1, 3), r.stdout, open(data / "summary.txt").read()

    w0, args, v0, t0, text0, summary0 = run("plain", [])
    assert "contour smoothing" not in text0 and "contour smoothing" not in summary0 and len(t0) > 100
    w1, _, v1, t1, text1, summary1 = run("smoothed", ["--contourSmoothSigma", "1", "--verbose"])
    for name in ("volume.vts", "meta_image_volume.mha"):
        assert open(w0 / name, "rb").read() == open(w1 / name, "rb").read(), name
    active = [x.split("  cells straddling the value  ")[1] for x in (summary0, summary1)]
    assert active[0].split("\n")[0] == active[1].split("\n")[0]
    o, _ = capi.cli_read_arguments(args)
    dims, _, pts = TC._read_mha(str(w0 / "meta_image_volume.mha"))
    P = pts.reshape(dims[2], dims[1], dims[0])
    M = np.array(o.grid_matrix).reshape(4, 4)
    pv, pt = R.extract(P, 0.25, o.grid_origin, o.grid_spacing, M)
    assert v0.tobytes() == pv.tobytes() and np.array_equal(t0, pt)
    wv, wt = R.extract(PS.smooth(P, _weights3(1.0)), 0.25, o.grid_origin, o.grid_spacing, M)
    assert v1.tobytes() == wv.tobytes() and np.array_equal(t1, wt)
    assert v1.tobytes() != v0.tobytes()
    line = [x for x in text1.splitlines() if x.startswith("contour smoothing:")]
    assert len(line) == 1 and "sigma 1 1 1 voxels, truncate 3, radii 3 3 3; " in line[0] and " ms of GPU kernels" in line[0], text1
    assert "  contour smoothing  sigma 1 1 1 voxels, truncate 3, radii 3 3 3, " in summary1
