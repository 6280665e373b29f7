"""dmi_fill_isosurface_holes: the CPU restatement (tests/isosurface_holes_np.py) on hand-made meshes with exact
results, the ABI and the CLI flag on the CPU; on the GPU every bit of the filled mesh -- vertices, triangles, normals with and
without, and the four counts -- against the restatement applied to the GPU's own download before the call.

The loop sizes the GPU cases assert are what the restatements (isosurface_np, isosurface_holes_np) give on the CPU for the same
cells through the cell -> point pass the device runs.  Two of them differ from the figures of the issue that asked for this
feature: the smoothing tests' `leaves_the_grid` cells give ONE rim of 80 edges, and the plane with normal(0, 0.3) noise on its
cells, seed 3, ONE rim of 290; that issue's "4, 4, 4, 4, 96" and "4, 330" are what the restatement gives when noise of the POINT
lattice's shape is added to the point field and contoured directly, which no cell grid reproduces.  Both inputs are kept as
stated, with the sizes they really have, and a rougher sibling of each (`poke_rough`: 4, 4, 4, 4, 6, 100; `plane_rough`: 4, 374)
keeps what the figures were for: small rims filled beside a large one left, and a rim of more than 256 edges beside a small one."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import isosurface_components_np as C
import isosurface_decimate_np as D
import isosurface_holes_np as H
import isosurface_smooth_np as S
import test_isosurface_smooth as TS
import test_isosurface_support as TP
from cudadepthmapintegration_amd import capi, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 1   # DMI_ERR_INVALID_ARGUMENT (include/dmi.h)
MAX_EDGES_LIMIT = 1 << 20


def _fill(v, t, max_edges, normals=None):
    return H.fill(v, t, max_edges, normals)


# ---- the restatement on hand-made meshes: integer coordinates, every result exact ---------------------------------------------
def _sheet_with_a_square_hole():
    """A 4 x 4 lattice of vertices (id = 4 y + x), its nine quads split into (a, b, c), (a, c, d) counter-clockwise seen from +z,
    the middle quad left out: a hole with the rim 5, 6, 10, 9 at the heights 1, 2, 4, 9."""
    p = np.array([[x, y, 0.0] for y in range(4) for x in range(4)], dtype=np.float64)
    p[[5, 6, 10, 9], 2] = [1.0, 2.0, 4.0, 9.0]
    tris = []
    for y in range(3):
        for x in range(3):
            if (x, y) == (1, 1):
                continue
            a, b, c, d = 4 * y + x, 4 * y + x + 1, 4 * y + x + 5, 4 * y + x + 4
            tris += [[a, b, c], [a, c, d]]
    return p, np.array(tris, dtype=np.int64)


def test_square_hole_gets_its_centroid_and_four_triangles():
    p, tris = _sheet_with_a_square_hole()
    half, simple, complex_, nxt = H.boundary(16, tris)
    assert len(half) == 16 and simple.sum() == 16 and not complex_.any()
    # the hole's half-edges run against the sheet's orientation: 5 -> 9 -> 10 -> 6 -> 5
    assert [int(nxt[v]) for v in (5, 9, 10, 6)] == [9, 10, 6, 5]
    assert [h.tolist() for h in H.loops(16, tris)] == [[0, 1, 2, 3, 7, 11, 15, 14, 13, 12, 8, 4], [5, 9, 10, 6]]
    r = _fill(p, tris, 4)
    assert r["n_filled"] == 1 and r["boundary_edges_left"] == 12 and r["loop_sizes"] == [12, 4]
    assert np.array_equal(r["vertices"][:16], p) and np.array_equal(r["triangles"][:16], tris)
    assert np.array_equal(r["vertices"][16:], [[1.5, 1.5, 4.0]])                 # ((1 + 9) + 4) + 2 = 16, / 4
    assert r["triangles"][16:].tolist() == [[9, 5, 16], [10, 9, 16], [6, 10, 16], [5, 6, 16]]
    # oriented like the sheet: every new triangle's normal points to +z
    a, b, c = (r["vertices"][r["triangles"][16:, k]] for k in range(3))
    assert (np.cross(b - a, c - a)[:, 2] > 0).all()
    # max_edges = L - 1 against L, and the open sheet's own rim is a loop like any other
    assert _fill(p, tris, 3)["n_filled"] == 0 and np.array_equal(_fill(p, tris, 3)["triangles"], tris)
    both = _fill(p, tris, 12)
    assert _fill(p, tris, 11)["n_filled"] == 1 and both["n_filled"] == 2 and both["boundary_edges_left"] == 0
    assert len(both["vertices"]) == 18 and len(both["triangles"]) == 16 + 12 + 4
    assert both["triangles"][16].tolist() == [1, 0, 16] and both["triangles"][28].tolist() == [9, 5, 17]   # in loop order
    # idempotence
    again = _fill(both["vertices"], both["triangles"], 12)
    assert again["n_filled"] == 0 and np.array_equal(again["triangles"], both["triangles"])
    once = _fill(r["vertices"], r["triangles"], 4)
    assert once["n_filled"] == 0 and once["loop_sizes"] == [12]


CUBE = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0], [0, 0, 2], [2, 0, 2], [2, 2, 2], [0, 2, 2]], dtype=np.float64)
CUBE_QUADS = [(0, 3, 2, 1), (0, 1, 5, 4), (1, 2, 6, 5), (2, 3, 7, 6), (3, 0, 4, 7), (4, 5, 6, 7)]   # outward


def _quads(quads):
    return np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], dtype=np.int64)


def test_cube_with_a_face_missing_is_closed_outward():
    tris = _quads(CUBE_QUADS[:5])
    assert TS.signed_volume(CUBE, _quads(CUBE_QUADS)) == 8.0
    r = _fill(CUBE, tris, 4)
    assert r["n_filled"] == 1 and r["boundary_edges_left"] == 0 and r["loop_sizes"] == [4]
    assert np.array_equal(r["vertices"][8], [1.0, 1.0, 2.0]) and len(r["triangles"]) == 14
    assert r["filled"][0].tolist() == [4, 7, 6, 5] and r["triangles"][10:].tolist() == [[7, 4, 8], [6, 7, 8], [5, 6, 8], [4, 5, 8]]
    assert TS.signed_volume(r["vertices"], r["triangles"]) == 8.0                # a flat cap: the cube's volume, exactly
    assert not H.boundary(9, r["triangles"])[0].size


def test_tetrahedron_with_a_face_missing_gets_one_triangle_and_no_vertex():
    p = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, 6.0, 0.0], [0.0, 0.0, 9.0]])
    r = _fill(p, TS.TETRA[:3], 3)
    assert r["n_filled"] == 1 and np.array_equal(r["vertices"], p) and r["boundary_edges_left"] == 0
    assert r["filled"][0].tolist() == [1, 2, 3] and r["triangles"][3].tolist() == [1, 3, 2]      # (h_0, h_2, h_1): TETRA's own
    assert TS.signed_volume(p, r["triangles"]) == TS.signed_volume(p, TS.TETRA) != 0.0
    assert _fill(p, TS.TETRA[:3], 2)["n_filled"] == 0
    # an isolated triangle's rim is closed by its mirror image
    one = _fill(p, TS.TETRA[:1], 3)
    assert one["triangles"].tolist() == [[0, 1, 2], [0, 2, 1]] and one["boundary_edges_left"] == 0
    # a degenerate triangle and ids that are no vertices say nothing, and stay where they are
    junk = np.concatenate([TS.TETRA[:3], [[2, 2, 3], [0, 1, 4], [0, -1, 2], [3, 0, 3]]]).astype(np.int64)
    r2 = _fill(p, junk, 3)
    assert r2["n_filled"] == 1 and np.array_equal(r2["triangles"][:7], junk) and r2["triangles"][7].tolist() == [1, 3, 2]
    assert len(H.boundary(4, junk)[0]) == 3


def test_bow_tie_vertex_is_complex_and_neither_rim_is_filled():
    # two fans of four triangles (hubs 0 and 5) whose rims touch in vertex 1
    p = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [-2, 0, 0], [0, -2, 0], [4, 0, 0], [4, -2, 1], [6, 0, 0], [4, 2, 1]], dtype=np.float64)
    tris = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1], [5, 1, 6], [5, 6, 7], [5, 7, 8], [5, 8, 1]], dtype=np.int64)
    half, simple, complex_, _ = H.boundary(9, tris)
    assert len(half) == 8 and np.flatnonzero(complex_).tolist() == [1] and simple.sum() == 6
    assert H.loops(9, tris) == []
    r = _fill(p, tris, 64)
    assert r["n_filled"] == 0 and r["boundary_edges_left"] == 8 and np.array_equal(r["triangles"], tris)
    # apart, each rim is a loop
    apart = tris.copy()
    apart[4:][apart[4:] == 1] = 9
    p10 = np.concatenate([p, [[2.0, 0.0, 0.0]]])
    assert [h.tolist() for h in H.loops(10, apart)] == [[1, 2, 3, 4], [6, 7, 8, 9]]
    assert _fill(p10, apart, 4)["n_filled"] == 2


def test_an_edge_three_triangles_name_is_no_boundary():
    three = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=np.int64)
    half, simple, complex_, _ = H.boundary(5, three)
    edges = {tuple(sorted(e)) for e in half.tolist()}
    assert (0, 1) not in edges and len(half) == 6
    # 0 and 1 end three boundary half-edges each: complex, and every chain runs into them
    assert np.flatnonzero(complex_).tolist() == [0, 1] and H.loops(5, three) == []
    assert _fill(np.zeros((5, 3)), three, 64)["n_filled"] == 0
    two = H.boundary(4, three[:2])
    assert len(two[0]) == 4 and two[1].all() and [h.tolist() for h in H.loops(4, three[:2])] == [[0, 3, 1, 2]]


def test_normals_of_new_vertices_are_the_geometric_ones_and_the_old_rows_stay():
    p, tris = _sheet_with_a_square_hole()
    old = np.arange(48, dtype=np.float32).reshape(16, 3)
    r = _fill(p, tris, 12, old)
    assert r["normals"].dtype == np.float32 and np.array_equal(r["normals"][:16], old)
    assert np.array_equal(r["normals"][16:], S.geometric_normals(r["vertices"], r["triangles"])[16:])
    # (the outer rim's cap faces the other way: it closes the sheet from below)
    assert r["normals"][16].tolist() == [0.0, 0.0, -1.0] and r["normals"][17, 2] > 0
    assert _fill(p, tris, 12)["normals"] is None
    assert np.array_equal(_fill(p, tris, 3, old)["normals"], old)
    # non-finite coordinates propagate
    q = p.copy()
    q[5, 0] = np.nan
    assert np.isnan(_fill(q, tris, 4)["vertices"][16, 0]) and _fill(q, tris, 4)["vertices"][16, 1] == 1.5


# ---- ABI and CLI flag ---------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["dmi_fill_isosurface_holes", "dmi_get_isosurface_holes_kernel_ms", "dmi_get_isosurface_holes_pass_ms"]


def test_abi_has_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "dmi.h")).read()
    lib = ctypes.CDLL(capi.load()._name)
    for name in NEW_SYMBOLS:
        assert name + "(" in header and name in capi.ABI_SYMBOLS and hasattr(lib, name), name
    assert lib.dmi_abi_version() == 5 and "#define DMI_ABI_VERSION 5 " in header
    for name in ("fill_isosurface_holes", "isosurface_holes_kernel_ms", "isosurface_holes_pass_ms"):
        assert callable(getattr(capi.FusionContext, name)), name
    # a null context is refused without a device, and the message names the entry point
    L = capi.load()
    n = ctypes.c_uint64(0)
    assert L.dmi_fill_isosurface_holes(None, 16, ctypes.byref(n), ctypes.byref(n), None, None) == INVALID_ARGUMENT
    assert "dmi_fill_isosurface_holes" in L.dmi_last_error(None).decode()
    assert L.dmi_get_isosurface_holes_kernel_ms(None, None) == INVALID_ARGUMENT
    assert "dmi_get_isosurface_holes_kernel_ms" in L.dmi_last_error(None).decode()
    assert L.dmi_get_isosurface_holes_pass_ms(None, None) == INVALID_ARGUMENT
    assert "dmi_get_isosurface_holes_pass_ms" in L.dmi_last_error(None).decode()


def test_cli_fill_holes_flag():
    BASE = TS.BASE
    o, text = capi.cli_read_arguments(BASE + ["--extractMesh"])
    assert o is not None and o.mesh_fill_holes == 0, text
    for value, want in (("3", 3), ("16", 16), ("1048576", 1048576)):
        o, text = capi.cli_read_arguments(BASE + ["--extractMesh", "--meshFillHoles", value])
        assert o is not None and o.mesh_fill_holes == want, text
    # every earlier field keeps its place
    o, text = capi.cli_read_arguments(BASE + ["--extractMesh", "--meshFillHoles", "9", "--meshSmoothIterations", "25", "--meshNormals"])
    assert o is not None and (o.mesh_fill_holes, o.mesh_smooth_iterations, o.mesh_normals, o.extract_mesh, o.grid_auto_bounds_pixel_step) == (9, 25, 1, 1, 1)
    o, text = capi.cli_read_arguments(BASE + ["--meshFillHoles", "16"])
    assert o is None and text.split("\n")[0].startswith("Error : --meshFillHoles needs --extractMesh"), text
    for value in ("2", "0", "-1", "1048577", "2.5", "nan", "x", ""):
        o, text = capi.cli_read_arguments(BASE + ["--extractMesh", "--meshFillHoles", value])
        assert o is None and text.startswith("Bad value for --meshFillHoles"), (value, text)
    o, text = capi.cli_read_arguments(BASE + ["--extractMesh", "--meshFillHoles"])
    assert o is None and "needs a value" in text
    o, text = capi.cli_read_arguments(BASE + ["--help"])
    assert o is None and "--meshFillHoles v" in text and "vtkFillHolesFilter" in text
    # the tool itself: the usual exit status
    r = subprocess.run([capi.cli_binary()] + BASE[1:] + ["--meshFillHoles", "16"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--meshFillHoles needs --extractMesh" in r.stderr
    r = subprocess.run([capi.cli_binary()] + BASE[1:] + ["--extractMesh", "--meshFillHoles", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "Bad value for --meshFillHoles" in r.stderr


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
_same_bits = TP._same_bits


def _caps3():
    x, y, z = TS._lattice(16, 16, 16)
    f = None
    for c, r in (((8.2, 7.9, 14.9), 2.2), ((1.0, 8.1, 8.3), 2.9), ((14.9, 15.2, 8.0), 3.4)):
        g = r - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
        f = g if f is None else np.maximum(f, g)
    return TS._cell_field(f)


def _plane():
    x, y, z = TS._lattice(64, 64, 6)
    return TS._cell_field(3.1 + 0.013 * (x - 32) - 0.021 * (y - 32) - z)


def _soup():
    return np.random.default_rng(17).uniform(-1.5, 2.5, (8, 10, 12))


def _poke(sigma, seed):
    return TS._noisy(TS._cell_field(TS.sphere_field(centre=(3.1, 12.2, 20.4))), sigma, seed)


# name -> (cells, iso, the sorted loop sizes, complex vertices, {max_edges: (loops filled, boundary edges left)})
CASES = {
    "caps3": (_caps3, 0.0, [14, 22, 32], 0, {13: (0, 68), 14: (1, 54), 31: (2, 32), 32: (3, 0)}),
    "soup": (_soup, 1.0, [4] * 15 + [5, 5, 6, 6, 6, 6, 8, 8, 8, 10, 10, 10, 10, 10, 12, 12, 15], 0,
             {3: (0, 207), 4: (15, 147), 8: (24, 89), 64: (32, 0)}),
    "plane": (_plane, 0.0, [260], 0, {259: (0, 260), 260: (1, 0)}),
    "plane_noise": (lambda: TS._noisy(_plane(), 0.3, 3), 0.0, [290], 0, {289: (0, 290), 290: (1, 0)}),
    "plane_rough": (lambda: TS._noisy(_plane(), 1.0, 3), 0.0, [4, 374], 0, {4: (1, 374), 373: (1, 374), 374: (2, 0)}),
    "poke": (lambda: TS._case("leaves_the_grid")[0], 0.0, [80], 0, {16: (0, 80), 80: (1, 0)}),
    "poke_rough": (lambda: _poke(1.5, 10), 0.0, [4, 4, 4, 4, 6, 100], 0, {4: (4, 106), 16: (5, 100), 65536: (6, 0)}),
}


def _extract(ctx, iso, normals):
    if normals:
        return ctx.extract_isosurface_with_normals(iso)
    return ctx.extract_isosurface(iso) + (None,)


def _check_filled(ctx, got, want, v0, t0, normals):
    """The context's mesh and the call's four counts against the restatement's dict."""
    v, t = ctx.download_isosurface()
    assert got == (len(want["vertices"]), len(want["triangles"]), want["n_filled"], want["boundary_edges_left"]), got
    assert _same_bits(v, want["vertices"]), int((v.view(np.uint64) != want["vertices"].view(np.uint64)).any(axis=1).sum())
    assert _same_bits(t, want["triangles"])
    assert _same_bits(v[:len(v0)], v0) and _same_bits(t[:len(t0)], t0)
    if normals:
        assert _same_bits(ctx.download_isosurface_normals(), want["normals"])
    else:
        with pytest.raises(capi.DmiError) as e:                  # as before the call: the extraction had no normals
            ctx.download_isosurface_normals()
        assert e.value.code == INVALID_ARGUMENT


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("normals", [False, True])
def test_gpu_fill_is_the_restatement_bit_for_bit(name, normals):
    make, iso, sizes, n_complex, runs = CASES[name]
    with TS._context(make()) as ctx:
        for max_edges, (n_filled, left) in runs.items():
            v0, t0, n0 = _extract(ctx, iso, normals)
            want = _fill(v0, t0, max_edges, n0)
            # the case still exercises its branch
            assert sorted(want["loop_sizes"]) == sizes and int(H.boundary(len(v0), t0)[2].sum()) == n_complex, (name, sorted(want["loop_sizes"]))
            assert (want["n_filled"], want["boundary_edges_left"]) == (n_filled, left), (name, max_edges)
            got = ctx.fill_isosurface_holes(max_edges)
            print(f"{name} max_edges {max_edges}: {len(v0)} vertices, {len(t0)} triangles, {got}, kernels {ctx.isosurface_holes_pass_ms()}")
            _check_filled(ctx, got, want, v0, t0, normals)
            assert (ctx.isosurface_holes_kernel_ms() > 0.0) == (n_filled > 0)
            assert all((p > 0.0) == (n_filled > 0) for p in ctx.isosurface_holes_pass_ms().values())
        if name == "caps3":                                       # closed now, and oriented from the inside to the outside
            v, t = ctx.download_isosurface()
            assert not len(H.boundary(len(v), t)[0]) and TS.signed_volume(v, t) > 0.0
        # the next extraction returns the unfilled mesh
        v, t, _ = _extract(ctx, iso, normals)
        assert _same_bits(v, v0) and _same_bits(t, t0)


@pytest.mark.gpu
@pytest.mark.parametrize("normals", [False, True])
def test_gpu_fill_of_the_decimated_soup_leaves_the_complex_chains_open(normals):
    # (a grid of unit cells at the origin: the decimation's cell size 1.7 is in the lattice's own units, as the restatement's is)
    cells = _soup()
    grid = scene.GridDesc(cells.shape[::-1], (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), np.eye(4))
    with capi.FusionContext(grid, scene.default_ray_potential(grid)) as ctx:
        ctx.upload_grid(cells)
        for max_edges, n_filled in ((3, 2), (64, 10)):
            _extract(ctx, 1.0, normals)
            ctx.decimate_isosurface(1.7)
            v0, t0 = ctx.download_isosurface()
            n0 = ctx.download_isosurface_normals() if normals else None
            half, simple, complex_, _ = H.boundary(len(v0), t0)
            want = _fill(v0, t0, max_edges, n0)
            assert sorted(want["loop_sizes"]) == [3, 3, 4, 4, 4, 4, 5, 5, 5, 6] and int(complex_.sum()) == 8
            e = np.sort(np.concatenate([t0[:, [0, 1]], t0[:, [1, 2]], t0[:, [2, 0]]]), axis=1)
            assert int((np.unique(e, axis=0, return_counts=True)[1] > 2).sum()) == 6          # non-manifold edges
            assert want["n_filled"] == n_filled and want["boundary_edges_left"] == len(half) - (6 if max_edges == 3 else 43) > 0
            got = ctx.fill_isosurface_holes(max_edges)
            _check_filled(ctx, got, want, v0, t0, normals)


def _soup_context():
    return TS._context(_soup())


@pytest.mark.gpu
def test_gpu_fill_life_cycle_determinism_and_errors():
    lib = capi.load()
    n = [ctypes.c_uint64(0) for _ in range(4)]
    refs = [ctypes.byref(x) for x in n]
    with _soup_context() as ctx:
        # before any extraction
        assert lib.dmi_fill_isosurface_holes(ctx._h, 16, *refs) == INVALID_ARGUMENT
        assert "no mesh" in lib.dmi_last_error(ctx._h).decode()
        v0, t0, n0 = ctx.extract_isosurface_with_normals(1.0)

        def untouched():
            v, t = ctx.download_isosurface()
            return _same_bits(v, v0) and _same_bits(t, t0) and _same_bits(ctx.download_isosurface_normals(), n0)

        assert lib.dmi_fill_isosurface_holes(ctx._h, MAX_EDGES_LIMIT + 1, *refs) == INVALID_ARGUMENT
        assert "max_edges" in lib.dmi_last_error(ctx._h).decode() and untouched()
        assert lib.dmi_fill_isosurface_holes(ctx._h, 16, None, refs[1], None, None) == INVALID_ARGUMENT
        assert lib.dmi_fill_isosurface_holes(ctx._h, 16, refs[0], None, None, None) == INVALID_ARGUMENT and untouched()
        assert lib.dmi_get_isosurface_holes_kernel_ms(ctx._h, None) == INVALID_ARGUMENT
        assert lib.dmi_get_isosurface_holes_pass_ms(ctx._h, None) == INVALID_ARGUMENT
        # max_edges = 2: a success that changes nothing and drops nothing; n_filled and boundary_edges_left may be null
        ctx.filter_isosurface_components("min_triangles", 0)
        assert ctx.fill_isosurface_holes(2) == (len(v0), len(t0), 0, 207) and untouched()
        assert ctx.fill_isosurface_holes(3) == (len(v0), len(t0), 0, 207) and untouched()            # no loop of three edges
        assert len(ctx.download_isosurface_regions()[0]) == len(v0)
        assert ctx.isosurface_holes_kernel_ms() == 0.0 and set(ctx.isosurface_holes_pass_ms().values()) == {0.0}
        assert lib.dmi_fill_isosurface_holes(ctx._h, MAX_EDGES_LIMIT, refs[0], refs[1], None, None) == 0
        want = _fill(v0, t0, MAX_EDGES_LIMIT, n0)
        assert (n[0].value, n[1].value) == (len(want["vertices"]), len(want["triangles"]))
        ctx._mesh_counts = (int(n[0].value), int(n[1].value), 0)   # (the wrapper's own note of the sizes: it was gone round)
        _check_filled(ctx, (len(want["vertices"]), len(want["triangles"]), 32, 0), want, v0, t0, True)
        assert ctx.isosurface_holes_kernel_ms() > 0.0
        passes = ctx.isosurface_holes_pass_ms()
        assert set(passes) == {"boundary", "loops", "fill"} and all(p > 0.0 for p in passes.values())
        # a second call fills nothing and leaves the bits
        assert ctx.fill_isosurface_holes(64) == (len(want["vertices"]), len(want["triangles"]), 0, 0)
        _check_filled(ctx, (len(want["vertices"]), len(want["triangles"]), 32, 0), want, v0, t0, True)
        assert ctx.isosurface_holes_kernel_ms() == 0.0
        # two runs on two fresh extractions: identical bits; the next extraction returns the unfilled mesh
        runs = []
        for _ in range(2):
            v, t, nn = ctx.extract_isosurface_with_normals(1.0)
            assert _same_bits(v, v0) and _same_bits(t, t0) and _same_bits(nn, n0)
            ctx.fill_isosurface_holes(8)
            runs.append(tuple(a.tobytes() for a in ctx.download_isosurface()) + (ctx.download_isosurface_normals().tobytes(),))
        assert runs[0] == runs[1]
        # an empty surface is a success
        ctx.reset_grid()
        assert ctx.extract_isosurface(1.0)[0].shape == (0, 3)
        assert ctx.fill_isosurface_holes(16) == (0, 0, 0, 0) and ctx.download_isosurface()[0].shape == (0, 3)


@pytest.mark.gpu
def test_gpu_fill_then_filter_smoothing_and_decimation_take_the_filled_mesh():
    with _soup_context() as ctx:
        v0, t0, n0 = ctx.extract_isosurface_with_normals(1.0)
        filled = _fill(v0, t0, 8, n0)
        fv, ft, fn = filled["vertices"], filled["triangles"], filled["normals"]
        # a component filter
        assert ctx.fill_isosurface_holes(8)[2] == 24
        kept = C.filter_mesh(fv, ft, fn, C.LARGEST)
        assert ctx.filter_isosurface_components(C.LARGEST) == kept["counts"]
        v, t = ctx.download_isosurface()
        assert _same_bits(v, kept["vertices"]) and _same_bits(t, kept["triangles"]) and _same_bits(ctx.download_isosurface_normals(), kept["normals"])
        # a smoothing: the former rims of the filled loops move, the rims of the loops left open do not
        ctx.extract_isosurface_with_normals(1.0)
        ctx.fill_isosurface_holes(8)
        want_v, want_n = S.smooth(fv, ft, 3, 0.5, -0.53, fn)
        ctx.smooth_isosurface(3, 0.5, -0.53)
        v, t = ctx.download_isosurface()
        assert _same_bits(v, want_v) and _same_bits(t, ft) and _same_bits(ctx.download_isosurface_normals(), want_n)
        moved = (v.view(np.uint64) != fv.view(np.uint64)).any(axis=1)
        rims = np.concatenate(filled["filled"])
        still_open = np.unique(H.boundary(len(fv), ft)[0])
        assert not np.intersect1d(rims, still_open).size and len(still_open) == 89
        assert moved[rims].all() and moved[len(v0):].all() and not moved[still_open].any()
        before = S.smooth(v0, t0, 3, 0.5, -0.53)[0]              # without the fill those rims are pinned
        assert _same_bits(before[rims], v0[rims])
        # a decimation
        ctx.extract_isosurface_with_normals(1.0)
        ctx.fill_isosurface_holes(8)
        dv, dt, dn = D.decimate(fv, ft, 1.7, fn)
        assert ctx.decimate_isosurface(1.7) == (len(dv), len(dt))
        v, t = ctx.download_isosurface()
        assert _same_bits(v, dv) and _same_bits(t, dt) and _same_bits(ctx.download_isosurface_normals(), dn)


@pytest.mark.gpu
def test_gpu_fill_drops_regions_support_counts_and_colours():
    _, _, views, _ = TP._scene()
    ctx, v0, t0, n0 = TP._fusion_context(0.0)
    with ctx, capi.ColorContext() as c:
        c.add_views(scene.make_colors(TP.N_VIEWS, TP.W, TP.H, seed=5), views.K4, views.RT4)
        nv, nt = ctx.filter_isosurface_support(1, TP.TOLERANCE)
        v1, t1 = ctx.download_isosurface()
        n1 = ctx.download_isosurface_normals()
        want = _fill(v1, t1, 16, n1)
        assert want["n_filled"] > 5 and want["boundary_edges_left"] > 0 and int(H.boundary(nv, t1)[2].sum()) > 0

        def downloads():
            return list(ctx.download_isosurface_regions()) + [ctx.download_isosurface_support()] + list(ctx.download_isosurface_colors())

        def producers():
            ctx.filter_isosurface_components("min_triangles", 0)
            ctx.filter_isosurface_support(0, TP.TOLERANCE)
            ctx.color_isosurface(c)
            return downloads()

        first = producers()
        # a fill with nothing to do leaves all three valid
        assert ctx.fill_isosurface_holes(2)[2] == 0
        assert all(_same_bits(a, b) for a, b in zip(first, downloads()))
        got = ctx.fill_isosurface_holes(16)
        _check_filled(ctx, got, want, v1, t1, True)
        TP._refused(ctx.download_isosurface_regions, "dmi_download_isosurface_regions")
        TP._refused(ctx.download_isosurface_support, "dmi_download_isosurface_support")
        TP._refused(ctx.download_isosurface_colors, "dmi_download_isosurface_colors")
        after = producers()                                          # their producers run again on the filled mesh
        assert len(after[0]) == len(after[2]) == len(after[3]) == got[0]


@pytest.mark.gpu
def test_gpu_cli_fill_holes_end_to_end(tmp_path):
    """dmi_reconstruction --extractMesh --meshMinSupportViews 1 --meshFillHoles 16 --meshNormals on the support trim's scene: the
    .vtp is the API path's filled mesh, and its boundary edges, by the restatement, are the "left" the tool reports."""
    _, _, views, _ = TP._scene()
    data = tmp_path / "data"
    data.mkdir()
    lv, lk = scene.write_view_files(str(data), views)
    flags = ["--meshMinSupportViews", "1", "--meshSupportDepthTolerance", repr(TP.TOLERANCE), "--meshNormals"]
    r = TP._reconstruct(tmp_path, lv, lk, "filled", flags + ["--meshFillHoles", "16", "--verbose"])
    assert r.returncode == 0, r.stderr + r.stdout
    mesh = capi.read_polydata(str(tmp_path / "filled.vtp"))
    ctx, v, t, _ = TP._fusion_context(0.0)
    with ctx:
        ctx.filter_isosurface_support(1, TP.TOLERANCE)
        v1, t1 = ctx.download_isosurface()
        n1 = ctx.download_isosurface_normals()
    want = _fill(v1, t1, 16, n1)
    assert want["n_filled"] > 5 and len(want["vertices"]) > len(v1)
    points, tris = mesh.points.reshape(-1, 3), np.asarray(mesh.connectivity).reshape(-1, 3)
    assert _same_bits(points, want["vertices"]) and np.array_equal(tris, want["triangles"])
    assert list(mesh.point_data) == ["Normals", "reconstruction_scalar"]
    assert _same_bits(np.asarray(mesh.point_data["Normals"]).reshape(-1, 3), want["normals"])
    assert len(np.asarray(mesh.point_data["reconstruction_scalar"]).reshape(-1)) == len(points)
    left = len(H.boundary(len(points), tris)[0])
    assert left == want["boundary_edges_left"]
    line = [x for x in r.stdout.splitlines() if x.startswith("mesh holes:")]
    assert len(line) == 1 and f"at most 16 edges; {want['n_filled']} filled, {left} boundary edges left; " in line[0], r.stdout
    assert " ms of GPU kernels" in line[0]
    # with --meshRegionIds the components are labelled anew on the filled mesh: the restatement's labels of it
    r = TP._reconstruct(tmp_path, lv, lk, "labelled", flags + ["--meshFillHoles", "16", "--meshRegionIds"])
    assert r.returncode == 0, r.stderr + r.stdout
    labelled = capi.read_polydata(str(tmp_path / "labelled.vtp"))
    assert list(labelled.point_data) == ["Normals", "reconstruction_scalar", "RegionId"]
    assert _same_bits(labelled.points.reshape(-1, 3), want["vertices"])
    kept = C.filter_mesh(want["vertices"], want["triangles"], want["normals"], C.MIN_TRIANGLES, 0)
    assert _same_bits(np.asarray(labelled.point_data["RegionId"]).reshape(-1), kept["region_id"])
    # without the flag: the trimmed mesh, and no word about holes
    r = TP._reconstruct(tmp_path, lv, lk, "open", flags)
    assert r.returncode == 0 and "mesh holes" not in r.stdout, r.stderr + r.stdout
    assert _same_bits(capi.read_polydata(str(tmp_path / "open.vtp")).points.reshape(-1, 3), v1)
