"""dmi_decimate_isosurface: the CPU restatement (tests/isosurface_decimate_np.py) on hand-made meshes with every
expected value written out and on a sphere and a torus, the ABI and the CLI flag on the CPU; on the GPU every bit of the decimated
vertices, triangles and normals against the restatement applied to the GPU's own download.

The weld-only cell size.  The definition refuses any cell size that gives more than 2^21 bins on an axis, and 1e-9 grid spacings
on a grid of 24 cells would be 2.4e10 bins: at that size the call is REFUSED, by the restatement and by the GPU, with a message
that names the smallest cell size the mesh accepts.  The tests assert exactly that, and then weld at the size the message names
(about 1e-5 spacings on these grids), where they assert what a weld is: one output vertex per distinct position."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import isosurface_components_np as C
import isosurface_decimate_np as D
import isosurface_np as R
import isosurface_smooth_np as S
import vti_writer
from cudadepthmapintegration_amd import capi, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 1   # DMI_ERR_INVALID_ARGUMENT (include/dmi.h)


def _i64(rows):
    return np.array(rows, dtype=np.int64).reshape(-1, 3)


# ---- the restatement on hand-made meshes: integer coordinates, every result exact ---------------------------------------------
def test_tiny_cell_welds_coincident_vertices_and_drops_the_zero_area_triangles():
    # A B C D and, coincident with B and C, B' C': two triangles along the edge B-C and the zero-area triangles between its copies
    p = np.array([[0.0, 0, 0], [4, 0, 0], [0, 4, 0], [4, 4, 0], [4, 0, 0], [0, 4, 0]])
    tris = _i64([[0, 1, 2], [1, 4, 2], [4, 3, 5], [4, 5, 2]])
    v, t, n = D.decimate(p, tris, 0.5)
    assert n is None
    assert np.array_equal(v, [[0.0, 0, 0], [4, 0, 0], [0, 4, 0], [4, 4, 0]])
    assert np.array_equal(t, [[0, 1, 2], [1, 3, 2]]) and t.dtype == np.int64 and v.dtype == np.float64
    cluster, count = D.clusters(p, 0.5)
    assert count == 4 and cluster.tolist() == [0, 1, 2, 3, 1, 2]
    v, t, n = D.decimate(p, tris, 0.5, np.zeros((6, 3), np.float32))             # with normals: the new mesh's geometric ones
    assert n.dtype == np.float32 and np.array_equal(n, [[0, 0, 1]] * 4)


TETRA = _i64([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])


def test_cell_larger_than_the_box_leaves_nothing_and_an_empty_mesh_is_a_success():
    p = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, 6.0, 0.0], [0.0, 0.0, 9.0]])
    v, t, n = D.decimate(p, TETRA, 9.5, np.ones((4, 3), np.float32))
    assert v.shape == (0, 3) and t.shape == (0, 3) and n.shape == (0, 3)
    assert D.bins(p, 9.5)[1] == [1, 1, 1] and D.bins(p, 9.0)[1] == [1, 1, 2]       # hi_2 = 9 is on the border: a bin of its own
    v, t, n = D.decimate(np.zeros((0, 3)), np.zeros((0, 3), np.int64), 1.0)
    assert v.shape == (0, 3) and t.shape == (0, 3) and n is None
    # a smaller cell keeps the tetrahedron as it is: four clusters of one, the vertices' own bits, renumbered by (b_2, b_1, b_0)
    v, t, _ = D.decimate(p, TETRA, 2.0)
    assert np.array_equal(v, p) and np.array_equal(t, TETRA)


def test_two_sided_sheet_keeps_the_lower_index_of_each_triple_with_its_vertex_order():
    corners = [[0.0, 0, 0], [4, 0, 0], [0, 4, 0], [4, 4, 0]]
    p = np.array(corners + [[x, y, 1.0] for x, y, _ in corners])                   # the bottom side, ids 0-3, and the top, ids 4-7
    tris = _i64([[4, 5, 6], [0, 2, 1], [1, 2, 3], [5, 7, 6]])                      # top, bottom, bottom, top
    v, t, _ = D.decimate(p, tris, 2.0)
    assert np.array_equal(v, [[0, 0, 0.5], [4, 0, 0.5], [0, 4, 0.5], [4, 4, 0.5]])
    assert np.array_equal(t, [[0, 1, 2], [1, 2, 3]])                               # index 0 as (0, 1, 2), index 2 as (1, 2, 3)
    v, t, _ = D.decimate(p, tris[[1, 0, 3, 2]], 2.0)                               # the other side first: its orientation stays
    assert np.array_equal(t, [[0, 2, 1], [1, 3, 2]])


def test_the_sum_is_made_left_to_right_in_ascending_id():
    big = 1e16
    p = np.array([[0.0, big, 0], [0, 1, 0], [0, 1, 0], [0, -big, 0], [1e17, 0, 0], [2e17, 5e17, 0]])
    v, t, _ = D.decimate(p, _i64([[0, 4, 5], [3, 5, 4]]), 1e17)
    assert D.clusters(p, 1e17)[0].tolist() == [0, 0, 0, 0, 1, 2]
    assert ((big + 1.0) + 1.0) + -big == 0.0 and ((big + -big) + 1.0) + 1.0 == 2.0  # another order differs
    assert np.array_equal(v, [[0, 0.0, 0], [1e17, 0, 0], [2e17, 5e17, 0]])
    assert np.array_equal(t, [[0, 1, 2]])                                          # (3, 5, 4) is the same set: index 0 stays
    v, _, _ = D.decimate(p[[0, 3, 1, 2, 4, 5]], _i64([[0, 4, 5]]), 1e17)           # ids in another order: another sum
    assert v[0, 1] == 0.5


def test_isolated_vertices_count_in_the_mean_and_are_output_only_with_a_triangle():
    p = np.array([[0.0, 0, 0], [4, 0, 0], [0, 4, 0], [1, 0, 0], [4, 4, 0]])         # 3 shares vertex 0's cell, 4 has its own
    tris = _i64([[0, 1, 2]])
    v, t, _ = D.decimate(p, tris, 2.0)
    assert D.clusters(p, 2.0) == (pytest.approx([0, 1, 2, 0, 3]), 4)
    assert np.array_equal(v, [[0.5, 0, 0], [4, 0, 0], [0, 4, 0]]) and np.array_equal(t, [[0, 1, 2]])
    # a triangle that names an id >= V (or below 0) is dropped; the vertices it names otherwise are not output for it
    v, t, _ = D.decimate(p, _i64([[0, 1, 2], [0, 1, 5], [1, 4, -1], [2, 4, 7]]), 2.0)
    assert np.array_equal(v, [[0.5, 0, 0], [4, 0, 0], [0, 4, 0]]) and np.array_equal(t, [[0, 1, 2]])


def test_bins_floor_at_a_border_at_the_upper_bound_and_divide_without_a_reciprocal():
    p = np.array([[0.0, 0, 0], [2, 0, 0], [4, 0, 0], [3.9999999999999996, 0, 0]])
    b, n = D.bins(p, 2.0)
    assert b[:, 0].tolist() == [0, 1, 2, 1] and n == [3, 1, 1]
    p = np.array([[0.0, -1, 5], [0.3, -1, 5]])
    b, n = D.bins(p, 0.1)
    assert 0.3 / 0.1 < 3.0 <= 0.3 * (1.0 / 0.1)                                     # the division, as rounded, stays below 3
    assert b.tolist() == [[0, 0, 0], [2, 0, 0]] and n == [3, 1, 1]


def test_refusals():
    p = np.array([[0.0, 0, 0], [2097151.0, 1, 0], [5, 5, 5]])
    assert D.bins(p, 1.0)[1] == [2097152, 6, 6]                                   # 2^21 bins: accepted
    q = p + [[0, 0, 0], [1, 0, 0], [0, 0, 0]]                                     # 2^21 + 1
    with pytest.raises(ValueError, match="2\\^21"):
        D.bins(q, 1.0)
    with pytest.raises(ValueError, match="smallest acceptable cell size for this mesh is 1.0000000000000002"):
        D.decimate(q, _i64([[0, 1, 2]]), 1.0)
    assert D.min_cell_size(q) == 1.0000000000000002 and D.bins(q, D.min_cell_size(q))[1][0] == 2097152
    with pytest.raises(ValueError, match="2\\^21"):
        D.decimate(p, _i64([[0, 1, 2]]), 5e-324)                                  # the quotient is an infinity
    for bad in (np.inf, -np.inf, np.nan):
        q = p.copy()
        q[2, 1] = bad
        with pytest.raises(ValueError, match="non-finite"):
            D.decimate(q, _i64([[0, 1, 2]]), 10.0)
    for h in (0.0, -1.0, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="cell_size"):
            D.decimate(p, _i64([[0, 1, 2]]), h)


# ---- properties on a sphere and a torus -------------------------------------------------------------------------------------------
def _lattice(nx, ny, nz):
    z, y, x = np.mgrid[0:nz + 1, 0:ny + 1, 0:nx + 1].astype(np.float64)
    return x, y, z


def sphere_field(n=24, centre=(12.3, 11.8, 12.1), radius=8.4):
    x, y, z = _lattice(n, n, n)
    return radius - np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)


def torus_field(n=28):
    x, y, z = _lattice(n, n, n)
    return 3.2 - np.sqrt((np.sqrt((x - 14.2) ** 2 + (y - 13.7) ** 2) - 8.1) ** 2 + (z - 14.4) ** 2)


def signed_volume(p, tris):
    a, b, c = p[tris[:, 0]], p[tris[:, 1]], p[tris[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def assert_clean(v, t):
    """No degenerate triangle, no duplicate triangle, no unreferenced vertex."""
    assert ((t >= 0) & (t < len(v))).all()
    assert (t[:, 0] != t[:, 1]).all() and (t[:, 1] != t[:, 2]).all() and (t[:, 2] != t[:, 0]).all()
    assert len(np.unique(np.sort(t, axis=1), axis=0)) == len(t)
    assert len(np.unique(t)) == len(v)


def assert_is_the_weld(v0, t0, v, t):
    """(v, t) is (v0, t0) with coincident vertices joined: one vertex per distinct position, and the triangles, as position triples in
    their stored order, are the input's without those that repeat a position and without the later ones of equal position sets."""
    distinct, inverse = np.unique(v0, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    assert len(v) == len(distinct) and len(np.unique(v, axis=0)) == len(v)
    by_position = inverse[t0]
    proper = (by_position[:, 0] != by_position[:, 1]) & (by_position[:, 1] != by_position[:, 2]) & (by_position[:, 2] != by_position[:, 0])
    idx = np.flatnonzero(proper)
    _, first = np.unique(np.sort(by_position[idx], axis=1), axis=0, return_index=True)
    stay = np.sort(idx[first])
    # (the mean of k equal numbers is their value up to the roundings of the k - 1 additions: x + x + x need not be 3 x)
    assert np.allclose(v[t], v0[t0[stay]], rtol=1e-14, atol=0.0)
    assert np.array_equal(v[t], v0[t0[stay]]) or len(v) < len(v0)                # nothing joined: every vertex keeps its bits


@pytest.mark.parametrize("field", [sphere_field, torus_field])
def test_sphere_and_torus_stay_clean_closed_and_get_coarser(field):
    v0, t0 = R.extract(field(), 0.0)                                              # unit spacing
    assert len(t0) > 1000 and signed_volume(v0, t0) > 0.0
    with pytest.raises(ValueError, match="2\\^21"):                                # 1e-9 spacings: beyond 2^21 bins (see the top)
        D.decimate(v0, t0, 1e-9)
    v, t, _ = D.decimate(v0, t0, D.min_cell_size(v0))
    assert_clean(v, t)
    assert_is_the_weld(v0, t0, v, t)
    assert len(v) <= len(v0) and signed_volume(v, t) > 0.0
    sizes = [len(v)]
    for h in (1.5, 4.0):
        v, t, n = D.decimate(v0, t0, h, np.zeros((len(v0), 3), np.float32))
        assert_clean(v, t)
        assert len(v) < len(v0) and 0 < len(t) < len(t0) and signed_volume(v, t) > 0.0
        assert ((n.astype(np.float64) * (v - v.mean(axis=0))).sum(1) > 0.0).mean() > 0.95 if field is sphere_field else True
        sizes.append(len(v))
    assert sizes[0] > sizes[1] > sizes[2]


# ---- ABI and CLI flag -------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["dmi_decimate_isosurface", "dmi_get_isosurface_decimate_kernel_ms", "dmi_get_isosurface_decimate_pass_ms"]


def test_abi_has_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "dmi.h")).read()
    lib = ctypes.CDLL(capi.load()._name)
    for name in NEW_SYMBOLS:
        assert name + "(" in header and name in capi.ABI_SYMBOLS and hasattr(lib, name), name
    assert lib.dmi_abi_version() == 5 and "#define DMI_ABI_VERSION 5 " in header
    # a null context is refused without a device
    n = ctypes.c_uint64(0)
    assert capi.load().dmi_decimate_isosurface(None, 1.0, ctypes.byref(n), ctypes.byref(n)) == INVALID_ARGUMENT
    assert "dmi_decimate_isosurface" in capi.load().dmi_last_error(None).decode()
    assert capi.load().dmi_get_isosurface_decimate_kernel_ms(None, None) == INVALID_ARGUMENT
    assert capi.load().dmi_get_isosurface_decimate_pass_ms(None, None) == INVALID_ARGUMENT


BASE = ["Reconstruction", "--gridOrigin", "-2.29", "-2.24", "-2.2", "--gridEnd", "1.19", "1.67", "1.22", "--dataFolder", "data",
        "--outputGridFilename", "out.vts", "--outputMeshFilename", "mesh.vtp", "--rayThick", "0.1", "--gridDims", "10"]


def test_cli_decimation_flag():
    o, text = capi.cli_read_arguments(BASE + ["--extractMesh"])
    assert o is not None and o.mesh_decimate_cell_size == 0.0, text
    o, text = capi.cli_read_arguments(BASE + ["--extractMesh", "--meshDecimateCellSize", "0.0375"])
    assert o is not None and o.mesh_decimate_cell_size == 0.0375, text
    assert (o.extract_mesh, o.mesh_normals, o.mesh_smooth_iterations, o.mesh_smooth_lambda, o.mesh_smooth_mu) == (1, 0, 0, 0.5, -0.53)
    o, text = capi.cli_read_arguments(BASE + ["--extractMesh", "--meshDecimateCellSize", "1e-12", "--meshSmoothIterations", "3"])
    assert o is not None and (o.mesh_decimate_cell_size, o.mesh_smooth_iterations) == (1e-12, 3), text
    o, text = capi.cli_read_arguments(BASE + ["--meshDecimateCellSize", "0.5"])
    assert o is None and text.split("\n")[0].startswith("Error : --meshDecimateCellSize needs --extractMesh"), text
    for value in ("0", "-1", "nan", "inf", "x", ""):
        o, text = capi.cli_read_arguments(BASE + ["--extractMesh", "--meshDecimateCellSize", value])
        assert o is None and text.startswith("Bad value for --meshDecimateCellSize"), (value, text)
    o, text = capi.cli_read_arguments(BASE + ["--extractMesh", "--meshDecimateCellSize"])
    assert o is None and "needs a value" in text
    o, text = capi.cli_read_arguments(BASE + ["--help"])
    assert o is None and "--meshDecimateCellSize v" in text
    assert "not in the reference" in text.split("--meshDecimateCellSize v")[1].split("--help")[0]
    # the tool itself: the usual exit status
    r = subprocess.run([capi.cli_binary()] + BASE[1:] + ["--meshDecimateCellSize", "0.5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--meshDecimateCellSize needs --extractMesh" in r.stderr
    r = subprocess.run([capi.cli_binary()] + BASE[1:] + ["--extractMesh", "--meshDecimateCellSize", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "Bad value for --meshDecimateCellSize" in r.stderr


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


def _shifted_sphere(centre):
    x, y, z = _lattice(24, 24, 24)
    return 8.4 - np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)


def _case(name):
    """(cells [nz, ny, nx], grid matrix or None) of the named surface."""
    if name == "sphere":
        return _cell_field(sphere_field()), None
    if name == "torus":
        return _cell_field(torus_field()), None
    if name == "noisy_sphere":
        return _noisy(_cell_field(sphere_field()), 1.0, 1), None
    if name == "leaves_the_grid":
        return _noisy(_cell_field(_shifted_sphere((3.1, 12.2, 20.4))), 0.5, 2), None
    if name == "nan":
        c = _noisy(_cell_field(sphere_field()), 1.0, 3)
        c[9:12, 3:8, 10:14] = np.nan
        c[0, 0, 0] = np.nan
        return c, None
    assert name == "sheared"
    return _noisy(_cell_field(sphere_field()), 0.7, 4), _sheared_rotated_matrix()


def _grid(cells, matrix=None):
    nz, ny, nx = cells.shape
    grid = scene.default_grid((nx, ny, nz))
    if matrix is not None:
        grid = scene.GridDesc(grid.cell_dims, grid.origin, (0.05, 0.06, 0.045), matrix)
    return grid


def _context(cells, matrix=None):
    grid = _grid(cells, matrix)
    ctx = capi.FusionContext(grid, scene.default_ray_potential(grid))
    ctx.upload_grid(cells)
    return ctx


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def two_bins_cell_size(v):
    """A cell size that gives exactly two bins on every axis of the positions v: eight clusters of hundreds of members.  A flat
    shape (the torus and the sheared sphere: one extent is below half the largest) has no such size; it gets two bins on its two
    long axes and one on the short one, four clusters."""
    extent = v.max(axis=0) - v.min(axis=0)
    long_axes = extent > extent.max() / 2
    h = float((extent.max() / 2 + extent[long_axes].min()) / 2)
    assert D.bins(v, h)[1] == [2 if a else 1 for a in long_axes] and long_axes.sum() >= 2
    return h


def cell_sizes(v, spacing):
    """The cell sizes of the bit-exactness test for positions v on a grid whose smallest spacing is `spacing`: name -> size."""
    return {"refused": 1e-9 * spacing, "weld": D.min_cell_size(v), "1.5": 1.5 * spacing, "4": 4.0 * spacing,
            "two_bins": two_bins_cell_size(v), "collapse": 1e6 * float((v.max(axis=0) - v.min(axis=0)).max())}


def _extract(ctx, normals, iso=0.0):
    if normals:
        return ctx.extract_isosurface_with_normals(iso)
    return ctx.extract_isosurface(iso) + (None,)


def _refused(ctx, cell_size):
    """The message of the refusal of decimate_isosurface(cell_size)."""
    with pytest.raises(capi.DmiError) as e:
        ctx.decimate_isosurface(cell_size)
    assert e.value.code == INVALID_ARGUMENT and "dmi_decimate_isosurface" in str(e.value)
    return str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sphere", "torus", "noisy_sphere", "leaves_the_grid", "nan", "sheared"])
@pytest.mark.parametrize("normals", [False, True])
def test_gpu_decimation_is_the_restatement_bit_for_bit(name, normals):
    cells, matrix = _case(name)
    spacing = min(_grid(cells, matrix).spacing)
    with _context(cells, matrix) as ctx:
        v0, t0, n0 = _extract(ctx, normals)
        assert len(t0) > 500
        for label, h in cell_sizes(v0, spacing).items():
            if label != "refused":
                v1, t1, n1 = _extract(ctx, normals)                                # each size on a fresh extraction
                assert _same_bits(v1, v0) and _same_bits(t1, t0)
            if label == "refused":                                                # more than 2^21 bins: the message names the weld's size
                with pytest.raises(ValueError, match="2\\^21"):
                    D.decimate(v0, t0, h, n0)
                text = _refused(ctx, h)
                assert "smallest acceptable cell size" in text and float(text.split()[-1]) == D.min_cell_size(v0), text
                v, t = ctx.download_isosurface()
                assert _same_bits(v, v0) and _same_bits(t, t0)
                continue
            want_v, want_t, want_n = D.decimate(v0, t0, h, n0)
            counts = ctx.decimate_isosurface(h)
            v, t = ctx.download_isosurface()
            print(f"{name} {label} (h = {h!r}): {len(v0)} -> {len(v)} vertices, {len(t0)} -> {len(t)} triangles, kernels {ctx.isosurface_decimate_pass_ms()}")
            assert counts == (len(v), len(t)) == (len(want_v), len(want_t))
            assert _same_bits(t, want_t), (name, label)
            assert _same_bits(v, want_v), (name, label, int((v.view(np.uint64) != want_v.view(np.uint64)).any(axis=1).sum()))
            if normals:
                assert _same_bits(ctx.download_isosurface_normals(), want_n), (name, label)
            else:
                with pytest.raises(capi.DmiError) as e:                            # as before the call: the extraction had no normals
                    ctx.download_isosurface_normals()
                assert e.value.code == INVALID_ARGUMENT
            with pytest.raises(capi.DmiError) as e:                                # no regions until a filter runs again
                ctx.download_isosurface_regions()
            assert e.value.code == INVALID_ARGUMENT and "no regions" in str(e.value)
            if label == "weld":
                assert_is_the_weld(v0, t0, v, t)
            elif label in ("1.5", "4"):
                assert 0 < len(t) < len(t0)
            elif label == "two_bins":
                assert D.clusters(v0, h)[1] == (4 if name in ("torus", "sheared") else 8) and 0 < len(v) <= 8
            else:
                assert counts == (0, 0)
            if len(v):
                assert_clean(v, t)


def quantised_cells():
    """Cells in steps of 1/2: many lattice points of the point data are exactly 0, so the surface at 0 has coincident vertices
    (t = 0 or 1) and zero-area triangles between them."""
    return np.round(2.0 * _cell_field(sphere_field())) / 2.0


@pytest.mark.gpu
def test_gpu_weld_joins_the_coincident_vertices_of_a_quantised_field():
    cells = quantised_cells()
    with _context(cells) as ctx:
        v0, t0, n0 = ctx.extract_isosurface_with_normals(0.0)
        assert len(np.unique(v0, axis=0)) < len(v0) - 20                          # there is something to weld
        h = D.min_cell_size(v0)
        want = D.decimate(v0, t0, h, n0)
        assert ctx.decimate_isosurface(h) == (len(want[0]), len(want[1])) and len(want[0]) < len(v0) and len(want[1]) < len(t0)
        v, t = ctx.download_isosurface()
        assert _same_bits(v, want[0]) and _same_bits(t, want[1]) and _same_bits(ctx.download_isosurface_normals(), want[2])
        assert_is_the_weld(v0, t0, v, t)
        assert_clean(v, t)


@pytest.mark.gpu
def test_gpu_decimation_composes_with_the_filter_and_the_smoother():
    cells = np.random.default_rng(17).uniform(-1.5, 2.5, size=(16, 20, 24))      # a soup of many components
    spacing = min(_grid(cells).spacing)
    with _context(cells) as ctx:
        v0, t0, n0 = ctx.extract_isosurface_with_normals(1.0)
        size = C.components(len(v0), t0)[1]
        n_min = int(np.median(size[size > 0])) + 1
        # filter(MIN) -> smooth(3, 0.5, -0.53) -> decimate(1.5)
        kept = C.filter_mesh(v0, t0, n0, C.MIN_TRIANGLES, n_min)
        sv, sn = S.smooth(kept["vertices"], kept["triangles"], 3, 0.5, -0.53, kept["normals"])
        want = D.decimate(sv, kept["triangles"], 1.5 * spacing, sn)
        assert ctx.filter_isosurface_components(C.MIN_TRIANGLES, n_min) == kept["counts"]
        ctx.smooth_isosurface(3, 0.5, -0.53)
        ctx.download_isosurface_regions()                                         # (still the filter's)
        assert ctx.decimate_isosurface(1.5 * spacing) == (len(want[0]), len(want[1])) and 0 < len(want[1]) < kept["counts"][1]
        v, t = ctx.download_isosurface()
        assert _same_bits(v, want[0]) and _same_bits(t, want[1]) and _same_bits(ctx.download_isosurface_normals(), want[2])
        with pytest.raises(capi.DmiError):
            ctx.download_isosurface_regions()
        # decimate -> filter(LARGEST) -> smooth, on a fresh extraction
        v1, t1, n1 = ctx.extract_isosurface_with_normals(1.0)
        assert _same_bits(v1, v0) and _same_bits(t1, t0) and _same_bits(n1, n0)
        dv, dt, dn = D.decimate(v0, t0, 1.5 * spacing, n0)
        big = C.filter_mesh(dv, dt, dn, C.LARGEST)
        sv, sn = S.smooth(big["vertices"], big["triangles"], 3, 0.5, -0.53, big["normals"])
        assert ctx.decimate_isosurface(1.5 * spacing) == (len(dv), len(dt))
        assert ctx.filter_isosurface_components(C.LARGEST) == big["counts"]
        rid, rsz = ctx.download_isosurface_regions()
        assert _same_bits(rid, big["region_id"]) and _same_bits(rsz, big["region_size"])
        ctx.smooth_isosurface(3, 0.5, -0.53)
        v, t = ctx.download_isosurface()
        assert _same_bits(v, sv) and _same_bits(t, big["triangles"]) and _same_bits(ctx.download_isosurface_normals(), sn)
        # a fresh extraction afterwards returns the original mesh
        v1, t1, n1 = ctx.extract_isosurface_with_normals(1.0)
        assert _same_bits(v1, v0) and _same_bits(t1, t0) and _same_bits(n1, n0)


@pytest.mark.gpu
def test_gpu_decimation_life_cycle_determinism_and_errors():
    cells = _noisy(_cell_field(sphere_field()), 1.0, 7)
    spacing = min(_grid(cells).spacing)
    lib = capi.load()
    n = ctypes.c_uint64(0)
    with _context(cells) as ctx:
        # before any extraction
        assert lib.dmi_decimate_isosurface(ctx._h, 1.0, ctypes.byref(n), ctypes.byref(n)) == INVALID_ARGUMENT
        assert "no mesh" in lib.dmi_last_error(ctx._h).decode() and "dmi_decimate_isosurface" in lib.dmi_last_error(ctx._h).decode()
        v0, t0, n0 = ctx.extract_isosurface_with_normals(0.0)
        ctx.filter_isosurface_components(C.MIN_TRIANGLES, 0)                      # keeps everything, leaves regions
        rid0, rsz0 = ctx.download_isosurface_regions()
        # refused arguments leave the mesh, its normals and its regions as they were
        box = float((v0.max(axis=0) - v0.min(axis=0)).max())
        for h in (0.0, -1.0, float("nan"), float("inf"), float("-inf"), box / 2 ** 22, 1e-9 * spacing, 5e-324):
            text = _refused(ctx, h)
            assert ("2^21" in text) == (h > 0 and h < 1.0), (h, text)
        assert lib.dmi_decimate_isosurface(ctx._h, 1.0, None, ctypes.byref(n)) == INVALID_ARGUMENT
        assert lib.dmi_decimate_isosurface(ctx._h, 1.0, ctypes.byref(n), None) == INVALID_ARGUMENT
        assert lib.dmi_get_isosurface_decimate_kernel_ms(ctx._h, None) == INVALID_ARGUMENT
        assert lib.dmi_get_isosurface_decimate_pass_ms(ctx._h, None) == INVALID_ARGUMENT
        v, t = ctx.download_isosurface()
        rid, rsz = ctx.download_isosurface_regions()
        assert _same_bits(v, v0) and _same_bits(t, t0) and _same_bits(ctx.download_isosurface_normals(), n0)
        assert _same_bits(rid, rid0) and _same_bits(rsz, rsz0)
        # the smallest accepted size is accepted
        assert ctx.decimate_isosurface(D.min_cell_size(v0))[0] > 0
        # two identical calls on identical fresh extractions: identical bytes (no race in the duplicate rule); times
        runs = []
        for _ in range(2):
            ctx.extract_isosurface_with_normals(0.0)
            ctx.decimate_isosurface(4.0 * spacing)
            runs.append(tuple(a.tobytes() for a in ctx.download_isosurface()) + (ctx.download_isosurface_normals().tobytes(),))
            passes = ctx.isosurface_decimate_pass_ms()
            assert list(passes) == ["clustering", "representatives", "triangles", "normals"] and all(p > 0.0 for p in passes.values())
            assert 0.0 < sum(passes.values()) <= ctx.isosurface_decimate_kernel_ms()
        assert runs[0] == runs[1]
        want = D.decimate(v0, t0, 4.0 * spacing, n0)
        assert runs[0] == tuple(a.tobytes() for a in want)
        # a second call takes the decimated mesh
        again = D.decimate(want[0], want[1], 9.0 * spacing, want[2])
        assert ctx.decimate_isosurface(9.0 * spacing) == (len(again[0]), len(again[1]))
        v, t = ctx.download_isosurface()
        assert _same_bits(v, again[0]) and _same_bits(t, again[1]) and _same_bits(ctx.download_isosurface_normals(), again[2])
        # everything collapses, then the empty mesh: successes; the second had nothing to do
        assert ctx.decimate_isosurface(1e6) == (0, 0)
        assert ctx.isosurface_decimate_kernel_ms() > 0.0 and ctx.isosurface_decimate_pass_ms()["normals"] == 0.0
        assert ctx.decimate_isosurface(1.0) == (0, 0)
        assert ctx.isosurface_decimate_kernel_ms() == 0.0 and set(ctx.isosurface_decimate_pass_ms().values()) == {0.0}
        assert ctx.download_isosurface()[0].shape == (0, 3)
        ctx.reset_grid()
        assert ctx.extract_isosurface(1.0)[0].shape == (0, 3)
        assert ctx.decimate_isosurface(1.0) == (0, 0) and ctx.isosurface_decimate_kernel_ms() == 0.0


@pytest.mark.gpu
def test_gpu_decimation_refuses_a_mesh_with_a_non_finite_coordinate():
    """A grid whose far corner overflows f64: if such a grid is accepted at all, its mesh has infinite coordinates and the
    decimation refuses it; if the grid or its extraction is refused, the restatement's test (test_refusals) stands alone."""
    cells = _cell_field(sphere_field())
    grid = scene.GridDesc((24, 24, 24), (1.79e308, 0.0, 0.0), (1e306, 1.0, 1.0), np.eye(4))
    try:
        ctx = capi.FusionContext(grid, scene.default_ray_potential(grid))
    except capi.DmiError:
        return
    with ctx:
        try:
            ctx.upload_grid(cells)
            v0, t0 = ctx.extract_isosurface(0.0)
        except capi.DmiError:
            return
        if np.isfinite(v0).all():
            return
        assert "non-finite" in _refused(ctx, 1.0)
        v, t = ctx.download_isosurface()
        assert _same_bits(v, v0) and _same_bits(t, t0)


@pytest.mark.gpu
def test_gpu_cli_decimation_end_to_end(tmp_path):
    """dmi_reconstruction --extractMesh --meshNormals --meshRegionIds --meshDecimateCellSize h on a small scene: the points,
    triangles and normals of mesh.vtp are the restatement applied to the same command's output without the flag, RegionId is the
    components restatement of the decimated mesh, and summary.txt carries the line."""
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
            "--outputMeshFilename", str(tmp_path / "mesh.vtp"), "--summary", "--extractMesh", "--meshNormals", "--meshRegionIds"]

    def run(flags):
        r = subprocess.run(args + flags, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr + r.stdout
        pd = capi.read_polydata(str(tmp_path / "mesh.vtp"))
        return pd.points, pd.connectivity.reshape(-1, 3), pd.point_data, r.stdout + r.stderr, open(data / "summary.txt").read()

    v0, t0, arrays0, text0, summary0 = run([])
    assert len(t0) > 100 and "mesh decimation" not in text0 and "mesh decimation" not in summary0
    assert list(arrays0) == ["Normals", "reconstruction_scalar", "RegionId"]
    assert _same_bits(arrays0["RegionId"], C.filter_mesh(v0, t0)["region_id"])
    o, _ = capi.cli_read_arguments(args)
    h = 1.5 * min(o.grid_spacing)
    want_v, want_t, want_n = D.decimate(v0, t0, h, arrays0["Normals"])
    assert 0 < len(want_t) < len(t0)
    v, t, arrays, text, summary = run(["--meshDecimateCellSize", repr(h)])
    assert _same_bits(v, want_v) and _same_bits(t, want_t) and _same_bits(arrays["Normals"], want_n)
    assert list(arrays) == ["Normals", "reconstruction_scalar", "RegionId"]
    assert arrays["reconstruction_scalar"].shape == (len(want_v),) and np.all(arrays["reconstruction_scalar"] == 0.25)
    assert _same_bits(arrays["RegionId"], C.filter_mesh(want_v, want_t)["region_id"])
    line = f"{len(v0)} vertices, {len(t0)} triangles before, {len(want_v)} vertices, {len(want_t)} triangles after"
    assert "mesh decimation: cell size " in text and line + "; " in text and " ms of GPU kernels" in text
    assert "  mesh decimation  cell size " in summary and line + ", " in summary
    # smoothing first, then the decimation, without the arrays' flags: points and triangles only
    plain = [a for a in args if a not in ("--meshNormals", "--meshRegionIds")]
    r = subprocess.run(plain + ["--meshSmoothIterations", "2", "--meshDecimateCellSize", repr(h)], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    pd = capi.read_polydata(str(tmp_path / "mesh.vtp"))
    want_v, want_t, _ = D.decimate(S.smooth(v0, t0, 2, 0.5, -0.53)[0], t0, h)
    assert _same_bits(pd.points, want_v) and _same_bits(pd.connectivity.reshape(-1, 3), want_t) and not list(pd.point_data)
