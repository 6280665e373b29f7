"""dmi_smooth_isosurface: the CPU restatement (tests/isosurface_smooth_np.py) on hand-made meshes with exact
results and on a noisy sphere, the ABI and the CLI flags on the CPU; on the GPU every bit of the smoothed positions and normals
against the restatement applied to the GPU's own unsmoothed download."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import isosurface_components_np as C
import isosurface_np as R
import isosurface_smooth_np as S
import vti_writer
from cudadepthmapintegration_amd import capi, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 1   # DMI_ERR_INVALID_ARGUMENT (include/dmi.h)
PARAMS = [(1, 0.5, 0.0), (10, 0.5, -0.53), (3, 1.0, -1.0)]


# ---- the restatement on hand-made meshes: integer coordinates, every result exact ---------------------------------------------
TETRA = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int64)


def test_closed_tetrahedron_lands_on_the_mean_of_the_other_three():
    p = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, 6.0, 0.0], [0.0, 0.0, 9.0]])
    nbr, valence, fixed = S.adjacency(4, TETRA)
    assert valence.tolist() == [3, 3, 3, 3] and not fixed.any()
    assert nbr.tolist() == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]]
    out, _ = S.smooth(p, TETRA, 1, 1.0, 0.0)
    assert np.array_equal(out, np.array([[1.0, 2.0, 3.0], [0.0, 2.0, 3.0], [1.0, 0.0, 3.0], [1.0, 2.0, 0.0]]))
    # Jacobi: a step reads the previous step's positions only, so two iterations are one iteration applied twice
    assert np.array_equal(S.smooth(p, TETRA, 2, 1.0, 0.0)[0], S.smooth(out, TETRA, 1, 1.0, 0.0)[0])
    assert np.array_equal(S.smooth(out, TETRA, 1, 1.0, 0.0)[0][0], [2.0 / 3.0, 4.0 / 3.0, 2.0])
    # lambda then mu: one iteration is a step with each factor
    half, _ = S.smooth(p, TETRA, 1, 0.5, 0.0)
    assert np.array_equal(half, p + 0.5 * (out - p))
    assert np.array_equal(S.step(half, nbr, valence, ~fixed, -0.5), S.smooth(p, TETRA, 1, 0.5, -0.5)[0])


def test_open_fan_rim_is_fixed_and_only_the_hub_moves():
    rim = np.array([[4.0, 0.0, 0.0], [0.0, 4.0, 0.0], [-4.0, 0.0, 0.0], [0.0, -4.0, 8.0]])
    p = np.concatenate([[[1.0, 1.0, 5.0]], rim])
    fan = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]], dtype=np.int64)
    nbr, valence, fixed = S.adjacency(5, fan)
    assert fixed.tolist() == [False, True, True, True, True] and valence.tolist() == [4, 3, 3, 3, 3]
    out, _ = S.smooth(p, fan, 1, 1.0, 0.0)
    assert np.array_equal(out[1:], rim) and np.array_equal(out[0], [0.0, 0.0, 2.0])
    out, _ = S.smooth(p, fan, 1, 0.5, 0.0)
    assert np.array_equal(out[1:], rim) and np.array_equal(out[0], [0.5, 0.5, 3.5])
    # an open fan (a wedge missing): the hub is on the boundary too, nothing moves
    out, _ = S.smooth(p, fan[:3], 7, 0.5, -0.53)
    assert np.array_equal(out, p)


def test_isolated_vertex_degenerate_triangles_and_zero_iterations():
    p = np.arange(21, dtype=np.float64).reshape(7, 3) ** 2
    tris = np.concatenate([TETRA, [[4, 4, 4], [5, 4, 5]]]).astype(np.int64)       # 6 isolated; (4, 4, 4) names no edge
    nbr, valence, fixed = S.adjacency(7, tris)
    assert valence.tolist() == [3, 3, 3, 3, 1, 1, 0]
    assert fixed.tolist() == [False, False, False, False, True, True, False]     # (5, 4, 5) names {4, 5} as ONE triangle
    out, _ = S.smooth(p, tris, 3, 0.5, -0.53)
    assert np.array_equal(out[4:], p[4:]) and not np.array_equal(out[:4], p[:4])
    normals = np.ones((7, 3), dtype=np.float32)
    out, n = S.smooth(p, tris, 0, 0.5, -0.53, normals)
    assert np.array_equal(out, p) and n is normals
    # an edge two triangles name is no boundary edge; one named by three is none either
    two = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=np.int64)
    assert S.adjacency(5, two[:2])[2].tolist() == [True, True, True, True, False]
    nbr, valence, fixed = S.adjacency(5, two)
    assert fixed.all() and valence.tolist() == [4, 4, 2, 2, 2]
    empty = S.smooth(np.zeros((0, 3)), np.zeros((0, 3), np.int64), 5, 0.5, -0.53, np.zeros((0, 3), np.float32))
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3)


def test_geometric_normals_of_a_hand_made_mesh():
    p = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 2.0], [9.0, 9.0, 9.0]])
    tris = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int64)
    n = S.geometric_normals(p, tris)
    assert n.dtype == np.float32
    assert np.array_equal(n[1], [0.0, 0.0, 1.0]) and np.array_equal(n[3], [1.0, 0.0, 0.0]) and np.array_equal(n[4], [0.0, 0.0, 0.0])
    h = np.float32(4.0 / np.sqrt(32.0))
    assert np.array_equal(n[0], [h, 0.0, h]) and np.array_equal(n[2], [h, 0.0, h])


# ---- two properties on a noisy sphere -------------------------------------------------------------------------------------------
def _lattice(nx, ny, nz):
    z, y, x = np.mgrid[0:nz + 1, 0:ny + 1, 0:nx + 1].astype(np.float64)
    return x, y, z


def sphere_field(n=24, centre=(12.3, 11.8, 12.1), radius=8.4, noise=0.0, seed=5):
    x, y, z = _lattice(n, n, n)
    f = radius - np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
    if noise:
        f = f + np.random.default_rng(seed).normal(0.0, noise, size=f.shape)
    return f


def torus_field(n=28):
    x, y, z = _lattice(n, n, n)
    return 3.2 - np.sqrt((np.sqrt((x - 14.2) ** 2 + (y - 13.7) ** 2) - 8.1) ** 2 + (z - 14.4) ** 2)


def signed_volume(p, tris):
    a, b, c = p[tris[:, 0]], p[tris[:, 1]], p[tris[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def test_noisy_sphere_gets_rounder_and_taubin_keeps_its_volume_better():
    centre = np.array([12.3, 11.8, 12.1])
    verts, tris = R.extract(sphere_field(noise=0.15), 0.0)
    lab, _ = C.components(len(verts), tris)
    assert len(tris) > 1000 and not lab.any()                    # one closed component: the volume means something
    assert not S.adjacency(len(verts), tris)[2].any()

    def radial_rms(p):
        r = np.linalg.norm(p - centre, axis=1)
        return float(np.sqrt(np.mean((r - r.mean()) ** 2)))

    taubin, _ = S.smooth(verts, tris, 10, 0.5, -0.53)
    laplace, _ = S.smooth(verts, tris, 10, 0.5, 0.0)
    assert radial_rms(taubin) < radial_rms(verts)
    v0 = signed_volume(verts, tris)
    assert v0 > 0.0                                              # oriented from the inside to the outside
    assert abs(signed_volume(taubin, tris) - v0) < abs(signed_volume(laplace, tris) - v0)


def test_cross_product_points_the_way_the_gradient_normals_do():
    import isosurface_normals_np as RN
    verts, tris, normals = RN.extract_with_normals(sphere_field(), 0.0)
    g = S.geometric_normals(verts, tris).astype(np.float64)
    assert ((g * normals.astype(np.float64)).sum(1) > 0.9).all()


# ---- ABI and CLI flags ------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["dmi_smooth_isosurface", "dmi_get_isosurface_smooth_kernel_ms", "dmi_get_isosurface_smooth_pass_ms"]


def test_abi_has_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "dmi.h")).read()
    lib = ctypes.CDLL(capi.load()._name)
    for name in NEW_SYMBOLS:
        assert name + "(" in header and name in capi.ABI_SYMBOLS and hasattr(lib, name), name
    assert lib.dmi_abi_version() == 5
    # a null context is refused without a device
    assert capi.load().dmi_smooth_isosurface(None, 1, 0.5, -0.53) == INVALID_ARGUMENT
    assert capi.load().dmi_get_isosurface_smooth_kernel_ms(None, None) == INVALID_ARGUMENT
    assert capi.load().dmi_get_isosurface_smooth_pass_ms(None, None) == INVALID_ARGUMENT


BASE = ["Reconstruction", "--gridOrigin", "-2.29", "-2.24", "-2.2", "--gridEnd", "1.19", "1.67", "1.22", "--dataFolder", "data",
        "--outputGridFilename", "out.vts", "--outputMeshFilename", "mesh.vtp", "--rayThick", "0.1", "--gridDims", "10"]


def test_cli_smoothing_flags():
    o, text = capi.cli_read_arguments(BASE + ["--extractMesh"])
    assert o is not None and (o.mesh_smooth_iterations, o.mesh_smooth_lambda, o.mesh_smooth_mu) == (0, 0.5, -0.53), text
    o, text = capi.cli_read_arguments(BASE + ["--extractMesh", "--meshSmoothIterations", "25", "--meshSmoothLambda", "0.33", "--meshSmoothMu", "-0.34"])
    assert o is not None and (o.mesh_smooth_iterations, o.mesh_smooth_lambda, o.mesh_smooth_mu) == (25, 0.33, -0.34), text
    o, text = capi.cli_read_arguments(BASE + ["--extractMesh", "--meshSmoothIterations", "1000", "--meshSmoothLambda", "1", "--meshSmoothMu", "0"])
    assert o is not None and (o.mesh_smooth_iterations, o.mesh_smooth_lambda, o.mesh_smooth_mu) == (1000, 1.0, 0.0), text
    assert (o.extract_mesh, o.mesh_normals, o.mesh_min_component_triangles) == (1, 0, -1)
    for flag in (["--meshSmoothIterations", "5"], ["--meshSmoothIterations", "0"], ["--meshSmoothLambda", "0.5"], ["--meshSmoothMu", "-0.5"]):
        o, text = capi.cli_read_arguments(BASE + flag)
        first = text.split("\n")[0]
        assert o is None and first.startswith("Error : " + flag[0] + " needs --extractMesh"), text
    bad = [("--meshSmoothLambda", "0"), ("--meshSmoothLambda", "-0.5"), ("--meshSmoothLambda", "1.5"), ("--meshSmoothLambda", "nan"),
           ("--meshSmoothLambda", "inf"), ("--meshSmoothLambda", "x"), ("--meshSmoothMu", "0.1"), ("--meshSmoothMu", "nan"),
           ("--meshSmoothMu", "-inf"), ("--meshSmoothMu", ""), ("--meshSmoothIterations", "1001"), ("--meshSmoothIterations", "-1"),
           ("--meshSmoothIterations", "2.5"), ("--meshSmoothIterations", "nan")]
    for flag, value in bad:
        o, text = capi.cli_read_arguments(BASE + ["--extractMesh", flag, value])
        assert o is None and text.startswith("Bad value for " + flag), (flag, value, text)
    o, text = capi.cli_read_arguments(BASE + ["--extractMesh", "--meshSmoothIterations"])
    assert o is None and "needs a value" in text
    o, text = capi.cli_read_arguments(BASE + ["--help"])
    assert o is None and all(f in text for f in ("--meshSmoothIterations v", "--meshSmoothLambda v", "--meshSmoothMu v"))
    assert text.count("not in the reference") >= 9 and "geometric normals" in text
    # the tool itself: the usual exit status
    r = subprocess.run([capi.cli_binary()] + BASE[1:] + ["--meshSmoothIterations", "5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--meshSmoothIterations needs --extractMesh" in r.stderr
    r = subprocess.run([capi.cli_binary()] + BASE[1:] + ["--extractMesh", "--meshSmoothLambda", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "Bad value for --meshSmoothLambda" in r.stderr


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _cell_field(point_field):
    """A cell grid whose point data (the mean of the cells around a point) has the given field's shape: its mean over each cell."""
    s = point_field.shape
    return 0.125 * sum(point_field[dz:s[0] - 1 + dz, dy:s[1] - 1 + dy, dx:s[2] - 1 + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1))


def _sheared_rotated_matrix():
    M = np.array(scene.default_grid(4, rotated=True).grid_matrix, dtype=np.float64).reshape(4, 4).copy()
    shear = np.array([[1.0, 0.35, -0.2], [0.0, 1.3, 0.15], [0.0, 0.0, 0.8]])
    M[:3, :3] = M[:3, :3] @ shear
    M[:3, 3] = (0.4, -1.1, 2.5)
    return M


def _noisy(cells, sigma, seed):
    """Noise on the cells: the point data the surface is taken from averages eight of them."""
    return cells + np.random.default_rng(seed).normal(0.0, sigma, size=cells.shape)


def _case(name):
    """(cells [nz, ny, nx], grid matrix or None) of the named surface."""
    if name == "sphere":
        return _cell_field(sphere_field()), None
    if name == "torus":
        return _cell_field(torus_field()), None
    if name == "noisy_sphere":
        return _noisy(_cell_field(sphere_field()), 1.0, 1), None
    if name == "leaves_the_grid":
        return _noisy(_cell_field(sphere_field(centre=(3.1, 12.2, 20.4))), 0.5, 2), None
    if name == "nan":
        c = _noisy(_cell_field(sphere_field()), 1.0, 3)
        c[9:12, 3:8, 10:14] = np.nan
        c[0, 0, 0] = np.nan
        return c, None
    assert name == "sheared"
    return _noisy(_cell_field(sphere_field()), 0.7, 4), _sheared_rotated_matrix()


def _context(cells, matrix=None):
    nz, ny, nx = cells.shape
    grid = scene.default_grid((nx, ny, nz))
    if matrix is not None:
        grid = scene.GridDesc(grid.cell_dims, grid.origin, (0.05, 0.06, 0.045), matrix)
    ctx = capi.FusionContext(grid, scene.default_ray_potential(grid))
    ctx.upload_grid(cells)
    return ctx


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sphere", "torus", "noisy_sphere", "leaves_the_grid", "nan", "sheared"])
@pytest.mark.parametrize("normals", [False, True])
def test_gpu_smoothing_is_the_restatement_bit_for_bit(name, normals):
    cells, matrix = _case(name)
    with _context(cells, matrix) as ctx:
        for iterations, lam, mu in PARAMS:
            if normals:
                v0, t0, n0 = ctx.extract_isosurface_with_normals(0.0)
            else:
                (v0, t0), n0 = ctx.extract_isosurface(0.0), None
            assert len(t0) > 500
            want_v, want_n = S.smooth(v0, t0, iterations, lam, mu, n0)
            ctx.smooth_isosurface(iterations, lam, mu)
            v, t = ctx.download_isosurface()
            moved = int((v.view(np.uint64) != v0.view(np.uint64)).any(axis=1).sum())
            print(f"{name} ({iterations}, {lam}, {mu}): {len(v0)} vertices, {moved} moved, kernels {ctx.isosurface_smooth_pass_ms()}")
            assert _same_bits(t, t0)
            assert _same_bits(v, want_v), (name, iterations, lam, mu, int((v.view(np.uint64) != want_v.view(np.uint64)).any(axis=1).sum()))
            assert moved > 0 and ctx.isosurface_smooth_kernel_ms() > 0.0
            if normals:
                n = ctx.download_isosurface_normals()
                assert _same_bits(n, want_n), (name, iterations, lam, mu)
                if name == "sphere":                             # the cross product points the way the gradient normals do
                    assert ((n.astype(np.float64) * n0.astype(np.float64)).sum(1) > 0.0).all()
            else:
                with pytest.raises(capi.DmiError) as e:          # as before the call: the extraction had no normals
                    ctx.download_isosurface_normals()
                assert e.value.code == INVALID_ARGUMENT
            _, _, fixed = S.adjacency(len(v0), t0)
            assert _same_bits(v[fixed], v0[fixed])
            if name == "leaves_the_grid":
                assert fixed.any() and (v.view(np.uint64) != v0.view(np.uint64)).any(axis=1)[~fixed].any()
            elif name in ("sphere", "torus"):
                assert not fixed.any()
            if name == "nan":
                assert np.isfinite(v0).all()                     # NaN point values are outside: the mesh goes round them
        # the next extraction returns the unsmoothed mesh
        v, t = ctx.extract_isosurface(0.0)
        assert _same_bits(v, v0) and _same_bits(t, t0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [C.MIN_TRIANGLES, C.LARGEST])
def test_gpu_smoothing_after_and_before_the_component_filter(mode):
    cells = np.random.default_rng(17).uniform(-1.5, 2.5, size=(16, 20, 24))      # a soup of many components
    with _context(cells) as ctx:
        v0, t0, n0 = ctx.extract_isosurface_with_normals(1.0)
        lab, size = C.components(len(v0), t0)
        n_min = int(np.median(size[size > 0])) + 1
        assert int((size > 0).sum()) > 3
        kept = C.filter_mesh(v0, t0, n0, mode, n_min)
        assert ctx.filter_isosurface_components(mode, n_min) == kept["counts"] and 0 < kept["counts"][0] < len(v0)
        rid0, rsz0 = ctx.download_isosurface_regions()
        want_v, want_n = S.smooth(kept["vertices"], kept["triangles"], 10, 0.5, -0.53, kept["normals"])
        ctx.smooth_isosurface(10, 0.5, -0.53)
        v, t = ctx.download_isosurface()
        assert _same_bits(v, want_v) and _same_bits(t, kept["triangles"]) and _same_bits(ctx.download_isosurface_normals(), want_n)
        rid, rsz = ctx.download_isosurface_regions()
        assert _same_bits(rid, rid0) and _same_bits(rsz, rsz0) and _same_bits(rid, kept["region_id"])
        # a filter applied after smoothing takes the smoothed mesh: the kept vertices' smoothed bits
        again = C.filter_mesh(want_v, kept["triangles"], want_n, C.LARGEST)
        assert ctx.filter_isosurface_components(C.LARGEST) == again["counts"]
        v, t = ctx.download_isosurface()
        assert _same_bits(v, again["vertices"]) and _same_bits(t, again["triangles"])
        assert _same_bits(ctx.download_isosurface_normals(), again["normals"])
        # smoothing first, on a fresh extraction, then the filter
        v1, t1 = ctx.extract_isosurface(1.0)
        assert _same_bits(v1, v0)
        ctx.smooth_isosurface(3, 1.0, -1.0)
        sm, _ = S.smooth(v0, t0, 3, 1.0, -1.0)
        after = C.filter_mesh(sm, t0, None, mode, n_min)
        assert ctx.filter_isosurface_components(mode, n_min) == after["counts"]
        v, t = ctx.download_isosurface()
        assert _same_bits(v, after["vertices"]) and _same_bits(t, after["triangles"])


@pytest.mark.gpu
def test_gpu_smoothing_life_cycle_determinism_and_errors():
    cells = _noisy(_cell_field(sphere_field()), 1.0, 7)
    lib = capi.load()
    with _context(cells) as ctx:
        # before any extraction
        assert lib.dmi_smooth_isosurface(ctx._h, 1, 0.5, -0.53) == INVALID_ARGUMENT
        assert "no mesh" in lib.dmi_last_error(ctx._h).decode()
        v0, t0, n0 = ctx.extract_isosurface_with_normals(0.0)
        # iterations = 0: a success that changes nothing, normals included
        ctx.smooth_isosurface(0, 0.5, -0.53)
        v, t = ctx.download_isosurface()
        assert _same_bits(v, v0) and _same_bits(t, t0) and _same_bits(ctx.download_isosurface_normals(), n0)
        assert ctx.isosurface_smooth_kernel_ms() == 0.0
        # refused arguments leave the mesh as it was
        nan, inf = float("nan"), float("inf")
        for args in ((-1, 0.5, -0.53), (1001, 0.5, -0.53), (5, 0.0, -0.53), (5, -0.5, -0.53), (5, 1.0000001, -0.53), (5, nan, -0.53),
                     (5, inf, -0.53), (5, 0.5, 0.01), (5, 0.5, nan), (5, 0.5, -inf), (5, 0.5, inf), (0, 0.0, 0.0)):
            assert lib.dmi_smooth_isosurface(ctx._h, *args) == INVALID_ARGUMENT, args
            assert "dmi_smooth_isosurface" in lib.dmi_last_error(ctx._h).decode()
        assert lib.dmi_get_isosurface_smooth_kernel_ms(ctx._h, None) == INVALID_ARGUMENT
        assert lib.dmi_get_isosurface_smooth_pass_ms(ctx._h, None) == INVALID_ARGUMENT
        v, t = ctx.download_isosurface()
        assert _same_bits(v, v0) and _same_bits(t, t0) and _same_bits(ctx.download_isosurface_normals(), n0)
        # two calls on two fresh extractions of the same grid: identical bits; two calls in a row compose
        runs = []
        for _ in range(2):
            ctx.extract_isosurface_with_normals(0.0)
            ctx.smooth_isosurface(10, 0.5, -0.53)
            runs.append((ctx.download_isosurface()[0].tobytes(), ctx.download_isosurface_normals().tobytes()))
        assert runs[0] == runs[1]
        want_v, want_n = S.smooth(v0, t0, 10, 0.5, -0.53, n0)
        assert runs[0] == (want_v.tobytes(), want_n.tobytes())
        ctx.smooth_isosurface(2, 0.25, 0.0)
        twice_v, twice_n = S.smooth(want_v, t0, 2, 0.25, 0.0, want_n)
        assert _same_bits(ctx.download_isosurface()[0], twice_v) and _same_bits(ctx.download_isosurface_normals(), twice_n)
        passes = ctx.isosurface_smooth_pass_ms()
        assert set(passes) == {"adjacency", "steps", "normals"} and all(p >= 0.0 for p in passes.values())
        # a new extraction afterwards returns the unsmoothed mesh
        v, t, n = ctx.extract_isosurface_with_normals(0.0)
        assert _same_bits(v, v0) and _same_bits(t, t0) and _same_bits(n, n0)
        # an empty surface is a success
        ctx.reset_grid()
        v, t = ctx.extract_isosurface(1.0)
        assert v.shape == (0, 3)
        ctx.smooth_isosurface(5, 0.5, -0.53)
        assert ctx.download_isosurface()[0].shape == (0, 3)


def _filter_smooth_download(ctx, iso, normals, n_min):
    """The context's grid through extract -> filter -> smooth(3, 0.5, -0.53) -> download.  n_min None: the filter keeps the largest
    component; else it keeps those of >= n_min triangles, and a second filter after the smoothing keeps the largest.  Returns the
    unfiltered extraction (v0, t0, n0) and the final mesh (v, t, n, region ids, region sizes); n0 and n are None without normals."""
    if normals:
        v0, t0, n0 = ctx.extract_isosurface_with_normals(iso)
    else:
        (v0, t0), n0 = ctx.extract_isosurface(iso), None
    if n_min is None:
        ctx.filter_isosurface_components(C.LARGEST)
        ctx.smooth_isosurface(3, 0.5, -0.53)
    else:
        ctx.filter_isosurface_components(C.MIN_TRIANGLES, n_min)
        ctx.smooth_isosurface(3, 0.5, -0.53)
        ctx.filter_isosurface_components(C.LARGEST)
    v, t = ctx.download_isosurface()
    n = ctx.download_isosurface_normals() if normals else None
    return (v0, t0, n0), (v, t, n) + tuple(ctx.download_isosurface_regions())


def _filter_smooth_restated(v0, t0, n0, n_min):
    """What _filter_smooth_download returns second, from the CPU restatements applied to the unfiltered extraction."""
    if n_min is None:
        kept = C.filter_mesh(v0, t0, n0, C.LARGEST)
        v, n = S.smooth(kept["vertices"], kept["triangles"], 3, 0.5, -0.53, kept["normals"])
        return v, kept["triangles"], n, kept["region_id"], kept["region_size"]
    kept = C.filter_mesh(v0, t0, n0, C.MIN_TRIANGLES, n_min)
    v, n = S.smooth(kept["vertices"], kept["triangles"], 3, 0.5, -0.53, kept["normals"])
    big = C.filter_mesh(v, kept["triangles"], n, C.LARGEST)
    return big["vertices"], big["triangles"], big["normals"], big["region_id"], big["region_size"]


def _same_mesh(got, want):
    return all((g is None and w is None) or _same_bits(g, w) for g, w in zip(got, want)) and len(got) == len(want)


@pytest.mark.gpu
def test_gpu_mesh_buffers_grow_across_swaps_and_reach_a_steady_state():
    """One context of 24 x 20 x 16 cells takes a small mesh S with normals, a large one L without normals, L with normals (the
    normals' buffers grow while the vertex buffers, swapped by the filter and the smoother, are already large) and S again, each
    filtered and smoothed.  Every download is, bit for bit, what a fresh context gives for that field and what the restatements make of
    the unfiltered extraction; a second round of the four leaves info().device_bytes where the first left it."""
    x, y, z = _lattice(24, 20, 16)
    blob = lambda c, r: r - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
    small = _cell_field(np.maximum(blob((9.3, 9.8, 8.1), 3.3), blob((19.2, 6.4, 5.7), 1.7)))      # two spheres: LARGEST drops one
    large = np.random.default_rng(17).uniform(-1.5, 2.5, size=(16, 20, 24))                          # a soup of many components
    # (cells, iso, normals) of the four steps; n_min of the large field from a fresh context's extraction
    with _context(large) as ctx:
        v0, t0 = ctx.extract_isosurface(1.0)
    size = C.components(len(v0), t0)[1]
    n_min = int(np.median(size[size > 0])) + 1
    steps = [(small, 0.0, True, None), (large, 1.0, False, n_min), (large, 1.0, True, n_min), (small, 0.0, True, None)]
    want = []
    for cells, iso, normals, n_min_ in steps[:3]:
        with _context(cells) as ctx:
            raw, fresh = _filter_smooth_download(ctx, iso, normals, n_min_)
        assert _same_mesh(fresh, _filter_smooth_restated(*raw, n_min_))
        want.append((raw, fresh))
    want.append(want[0])
    n_small, n_large = len(want[0][0][1]), len(want[1][0][1])
    print(f"S: {n_small} triangles ({len(want[0][1][1])} kept), L: {n_large} triangles ({len(want[1][1][1])} kept), n_min {n_min}")
    assert 100 < n_small < 1000 and n_large > 4 * n_small and len(want[0][1][1]) < n_small
    assert _same_bits(want[1][0][0], want[2][0][0]) and _same_bits(want[1][1][0], want[2][1][0])   # normals or not: the same positions
    device_bytes = []
    with _context(small) as ctx:
        for _ in range(2):
            for (cells, iso, normals, n_min_), (raw, final) in zip(steps, want):
                ctx.upload_grid(cells)
                got_raw, got = _filter_smooth_download(ctx, iso, normals, n_min_)
                assert _same_mesh(got_raw, raw) and _same_mesh(got, final), (iso, normals)
            device_bytes.append(int(ctx.info().device_bytes))
    print(f"device_bytes after round one {device_bytes[0]}, after round two {device_bytes[1]}")
    assert device_bytes[0] == device_bytes[1] > 0


@pytest.mark.gpu
def test_gpu_timing_tool_smooth_record():
    """tools/gpu_isosurface_time.py --smooth: its record of a small fused scene is complete and agrees with the restatement."""
    import importlib.util
    import types
    spec = importlib.util.spec_from_file_location("gpu_isosurface_time", os.path.join(ROOT, "tools", "gpu_isosurface_time.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    grid = scene.default_grid((48, 40, 36))
    views = scene.make_views(5, 96, 72, seed=11, dense=True)
    with capi.FusionContext(grid, scene.default_ray_potential(grid)) as ctx:
        ctx.add_views(views)
        ctx.fuse()
        rec = tool.smooth_record(ctx, types.SimpleNamespace(iso=1.0, min_triangles=20, repeat=2, smooth=4, smooth_lambda=0.5, smooth_mu=-0.53))
    assert rec["host_matches_gpu"] and rec["iterations"] == 4
    for k in ("raw", "min"):
        r = rec[k]
        assert len(r["kernel_ms"]) == 2 and r["kernel_ms_min"] > 0 and r["over_extraction"] > 0 and r["vertices"] > 0
        assert set(r["pass_ms"][0]) == {"adjacency", "steps", "normals"} and r["step_ms"] > 0 and r["scratch_bytes"] > 0
        assert r["step_floor_bytes"] == 48 * r["vertices"] + 4 * (r["vertices"] + 1) + 4 * r["neighbour_entries"]


def _vtp_bytes(pts, tris, normals, contour):
    """The file dmi_reconstruction --extractMesh --meshNormals has always written, built here byte by byte."""
    import struct
    n, m = len(pts), len(tris)
    pb, cb, ob = 24 * n, 24 * m, 8 * m
    off = 24 + pb + cb + ob
    head = ('<?xml version="1.0"?>\n<VTKFile type="PolyData" version="1.0" byte_order="LittleEndian" header_type="UInt64">\n'
            f'  <PolyData>\n    <Piece NumberOfPoints="{n}" NumberOfVerts="0" NumberOfLines="0" NumberOfStrips="0" NumberOfPolys="{m}">\n'
            '      <PointData Normals="Normals" Scalars="reconstruction_scalar">\n        <DataArray type="Float32" Name="Normals" '
            f'NumberOfComponents="3" format="appended" offset="{off}"/>\n        <DataArray type="Float64" '
            f'Name="reconstruction_scalar" format="appended" offset="{off + 8 + 12 * n}"/>\n      </PointData>\n'
            '      <Points>\n        <DataArray type="Float64" Name="Points" NumberOfComponents="3" format="appended" offset="0"/>\n'
            f'      </Points>\n      <Polys>\n        <DataArray type="Int64" Name="connectivity" format="appended" offset="{8 + pb}"/>\n'
            f'        <DataArray type="Int64" Name="offsets" format="appended" offset="{16 + pb + cb}"/>\n      </Polys>\n    </Piece>\n'
            '  </PolyData>\n  <AppendedData encoding="raw">\n   _')
    body = struct.pack("<Q", pb) + pts.tobytes() + struct.pack("<Q", cb) + tris.tobytes() + struct.pack("<Q", ob) + \
        (3 * np.arange(1, m + 1, dtype=np.int64)).tobytes() + struct.pack("<Q", 12 * n) + normals.tobytes() + \
        struct.pack("<Q", 8 * n) + np.full(n, contour).tobytes()
    return head.encode() + body + b"\n  </AppendedData>\n</VTKFile>\n"


@pytest.mark.gpu
def test_gpu_cli_smoothing_end_to_end(tmp_path):
    """dmi_reconstruction --extractMesh --meshLargestComponent --meshNormals --meshSmoothIterations 5 on a small scene: the points
    and normals of mesh.vtp are the restatement applied to the same command's output without the smoothing flags, and that output is
    the file the tool wrote before the flags existed (the oracle's fused grid through the restatements, byte for byte)."""
    from oracle import oracle
    from helpers import oracle_params_from_scene
    import isosurface_normals_np as RN
    grid = scene.default_grid((24, 20, 16), rotated=True)
    rp = scene.default_ray_potential(grid)
    views = scene.make_views(5, 48, 36, seed=4, dense=True, with_best_cost=True)
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
    gm = np.asarray(grid.grid_matrix).reshape(4, 4)
    end = [grid.origin[a] + (grid.cell_dims[a] + 1) * grid.spacing[a] for a in range(3)]
    args = [capi.cli_binary(), "--dataFolder", str(data), "--gridDims"] + [str(c + 1) for c in grid.cell_dims] + \
           ["--gridOrigin"] + [repr(float(v)) for v in grid.origin] + ["--gridEnd"] + [repr(float(v)) for v in end] + \
           ["--gridVecX"] + [repr(float(v)) for v in gm[0, :3]] + ["--gridVecY"] + [repr(float(v)) for v in gm[1, :3]] + \
           ["--gridVecZ"] + [repr(float(v)) for v in gm[2, :3]] + \
           ["--rayThick", repr(rp.thickness), "--rayRho", repr(rp.rho), "--rayEta", repr(rp.eta), "--rayDelta", repr(rp.delta),
            "--threshBestCost", "0.7", "--contour", "0.25", "--outputGridFilename", str(tmp_path / "volume.vts"),
            "--outputMeshFilename", str(tmp_path / "mesh.vtp"), "--summary", "--extractMesh", "--meshLargestComponent", "--meshNormals"]

    def run(flags):
        r = subprocess.run(args + flags, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr + r.stdout
        pd = capi.read_polydata(str(tmp_path / "mesh.vtp"))
        return (pd.points, pd.connectivity.reshape(-1, 3), pd.point_data, r.stdout + r.stderr, open(data / "summary.txt").read(),
                open(tmp_path / "mesh.vtp", "rb").read())

    v0, t0, arrays0, text0, summary0, raw0 = run([])
    n0 = arrays0["Normals"]
    assert len(t0) > 100 and "mesh smoothing" not in text0 and "mesh smoothing" not in summary0   # (the paths name this test)
    # without the flags: the bytes of the parent commit's tool, from the oracle's grid and the restatements
    o, _ = capi.cli_read_arguments(args)
    g2 = scene.GridDesc(tuple(int(d) - 1 for d in o.grid_dims), tuple(o.grid_origin), tuple(o.grid_spacing), np.array(o.grid_matrix).reshape(4, 4))
    d = oracle.apply_depth_threshold(views.depth, views.best_cost, 0.7).reshape(views.depth.shape)
    fused, _, _ = oracle.fuse(oracle_params_from_scene(g2, rp, views), d, views.K4, views.RT4, n_threads=oracle.max_threads())
    wv, wt, wn = RN.extract_with_normals(oracle.cell_to_point(fused), 0.25, o.grid_origin, o.grid_spacing, np.array(o.grid_matrix).reshape(4, 4))
    big = C.filter_mesh(wv, wt, wn, C.LARGEST)
    assert raw0 == _vtp_bytes(big["vertices"], big["triangles"], big["normals"], 0.25)
    assert list(arrays0) == ["Normals", "reconstruction_scalar"]
    # with them
    want_v, want_n = S.smooth(v0, t0, 5, 0.5, -0.53, n0)
    v, t, arrays, text, summary, raw = run(["--meshSmoothIterations", "5"])
    assert _same_bits(v, want_v) and _same_bits(t, t0) and _same_bits(arrays["Normals"], want_n)
    assert list(arrays) == ["Normals", "reconstruction_scalar"] and np.all(arrays["reconstruction_scalar"] == 0.25)
    assert raw == _vtp_bytes(want_v, t0, want_n, 0.25)
    assert "mesh smoothing: 5 iterations, lambda 0.5, mu -0.53; " in text and " ms of GPU kernels" in text
    assert "  mesh smoothing  5 iterations, lambda 0.5, mu -0.53, " in summary
    want_v, want_n = S.smooth(v0, t0, 2, 1.0, 0.0, n0)
    v, t, arrays, text, summary, raw = run(["--meshSmoothIterations", "2", "--meshSmoothLambda", "1", "--meshSmoothMu", "0"])
    assert _same_bits(v, want_v) and _same_bits(arrays["Normals"], want_n)
    assert "mesh smoothing: 2 iterations, lambda 1, mu 0; " in text
    # lambda and mu alone (0 iterations): nothing is smoothed, the file is the unsmoothed one
    assert run(["--meshSmoothLambda", "0.3", "--meshSmoothMu", "-0.31"])[5] == raw0
