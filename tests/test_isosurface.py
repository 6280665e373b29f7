"""dmi_extract_isosurface: the generated case table, the CPU restatement's topology, the .vtp writer and the
CLI flag on the CPU; the GPU mesh bit for bit against the restatement (tests/isosurface_np.py)."""
import ctypes
import os
import struct
import subprocess
from collections import Counter

import numpy as np
import pytest

import isosurface_np as R
from cudadepthmapintegration_amd import capi, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = R.T
INVALID_ARGUMENT = 1   # DMI_ERR_INVALID_ARGUMENT (include/dmi.h)


# ---- the table ---------------------------------------------------------------------------------------------------------
def test_committed_table_is_the_generators_output():
    assert open(T.OUT).read() == T.render()


def test_table_bound_and_histogram():
    assert T.MAX_TRIS == 5
    assert [T.TRI_COUNT.count(n) for n in range(6)] == [2, 16, 50, 80, 76, 32]
    assert T.TRI_COUNT[0] == 0 and T.TRI_COUNT[255] == 0


@pytest.mark.parametrize("case", range(256))
def test_case_uses_exactly_its_crossed_edges_and_follows_the_face_rule(case):
    crossed = {e for e in range(12) if ((case >> T.edge_corners(e)[0]) & 1) != ((case >> T.edge_corners(e)[1]) & 1)}
    tris = T.TRIS[case]
    used = {e for t in tris for e in t}
    assert used == crossed
    assert len(tris) <= T.MAX_TRIS
    # the directed boundary of the case's triangles is the union of its face segments: every boundary edge of the fan
    # lies on a face and pairs two crossed edges of that face as the face rule says
    half = Counter()
    for a, b, c in tris:
        for p, q in ((a, b), (b, c), (c, a)):
            half[(p, q)] += 1
    boundary = {pq for pq, n in half.items() if half.get((pq[1], pq[0]), 0) < n}
    want = set()
    for d, s, cyc in T.FACES:
        ins = [(case >> c) & 1 for c in cyc]
        face_edges = [e for e in crossed if set(T.edge_corners(e)) <= set(cyc)]
        segs = T.face_segments(case, (d, s, cyc))
        assert len(face_edges) == 2 * len(segs)
        if len(face_edges) == 4:   # ambiguous: the two segments each cut off one inside corner
            assert ins in ([1, 0, 1, 0], [0, 1, 0, 1])
            for p, q in segs:
                shared = set(T.edge_corners(p)) & set(T.edge_corners(q))
                assert len(shared) == 1 and (case >> shared.pop()) & 1
        want |= set(segs)
    assert boundary == want


# ---- the restatement's surfaces ----------------------------------------------------------------------------------------
def _edge_use(tris):
    half = Counter()
    for a, b, c in tris.tolist():
        half[(a, b)] += 1
        half[(b, c)] += 1
        half[(c, a)] += 1
    return half


def test_random_field_is_closed_and_oriented_away_from_the_outer_faces():
    rng = np.random.default_rng(5)
    P = rng.standard_normal((32, 18, 25))          # 24 x 17 x 31 cells
    verts, tris = R.extract(P, 0.1)
    assert tris.size and tris.min() >= 0 and tris.max() < len(verts)
    nz, ny, nx = (s - 1 for s in P.shape)
    lo, hi = np.zeros(3), np.array([nx, ny, nz], dtype=float)

    def on_face(v):
        return bool(np.any(verts[v] == lo) or np.any(verts[v] == hi))
    half = _edge_use(tris)
    for (a, b), n in half.items():
        back = half.get((b, a), 0)
        if on_face(a) and on_face(b) and back == 0:
            # a mesh edge without its twin: only on the grid's outer faces, where the surface ends
            same_face = np.any((verts[a] == verts[b]) & ((verts[a] == lo) | (verts[a] == hi)))
            assert same_face and n == 1
            continue
        assert n == 1 and back == 1, (a, b)


def _grid(n):
    z, y, x = np.mgrid[0:n + 1, 0:n + 1, 0:n + 1].astype(np.float64)
    return x, y, z


def _chi(verts, tris):
    half = _edge_use(tris)
    assert all(n == 1 and half.get((b, a), 0) == 1 for (a, b), n in half.items())
    return len(verts) - len(half) // 2 + len(tris)


def test_sphere_euler_characteristic_area_and_orientation():
    x, y, z = _grid(40)
    c, r = 20.0, 12.3
    P = r - np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2)     # inside (>= 0) = the ball
    verts, tris = R.extract(P, 0.0)
    assert _chi(verts, tris) == 2
    A = verts[tris]
    cr = np.cross(A[:, 1] - A[:, 0], A[:, 2] - A[:, 0])
    area = 0.5 * np.linalg.norm(cr, axis=1).sum()
    assert abs(area / (4 * np.pi * r * r) - 1) < 0.01
    vol = np.einsum("ij,ij->i", A[:, 0] - c, cr).sum() / 6     # normals point from inside to outside: positive
    assert vol > 0 and abs(vol / (4 / 3 * np.pi * r ** 3) - 1) < 0.02


def test_torus_euler_characteristic():
    x, y, z = _grid(40)
    P = 4.2 - np.sqrt((np.sqrt((x - 20) ** 2 + (y - 20) ** 2) - 11) ** 2 + (z - 20) ** 2)
    verts, tris = R.extract(P, 0.0)
    assert _chi(verts, tris) == 0


def test_touching_spheres_resolve_ambiguous_faces_by_the_rule():
    """Two balls whose surfaces meet between two lattice points: the face between them has two diagonal inside corners,
    which the rule separates -- two spheres (chi = 4), not one merged surface (chi = 2)."""
    P2 = np.full((6, 6, 6), -1.0)
    P2[2, 2, 2] = P2[3, 3, 2] = 1.0                 # diagonal inside corners of one face (z = 2)
    verts, tris = R.extract(P2, 0.0)
    assert _chi(verts, tris) == 4
    P2[2, 3, 2] = 1.0                               # connected: one surface
    verts, tris = R.extract(P2, 0.0)
    assert _chi(verts, tris) == 2


# ---- host side: the .vtp writer and the flag ---------------------------------------------------------------------------
def read_vtp(path):
    raw = open(path, "rb").read()
    head, _, tail = raw.partition(b'<AppendedData encoding="raw">\n   _')
    text = head.decode()
    assert 'type="PolyData"' in text and 'header_type="UInt64"' in text and 'byte_order="LittleEndian"' in text
    n_pts = int(text.split('NumberOfPoints="')[1].split('"')[0])
    n_polys = int(text.split('NumberOfPolys="')[1].split('"')[0])
    offs = [int(v) for v in (text.split(f'Name="{name}"')[1].split('offset="')[1].split('"')[0]
                             for name in ("Points", "connectivity", "offsets"))]
    arrays = []
    for off, dt in zip(offs, (np.float64, np.int64, np.int64)):
        (nb,) = struct.unpack_from("<Q", tail, off)
        arrays.append(np.frombuffer(tail, dtype=dt, count=nb // 8, offset=off + 8))
    assert tail.endswith(b"\n  </AppendedData>\n</VTKFile>\n")
    pts, conn, offsets = arrays
    assert np.array_equal(offsets, 3 * np.arange(1, n_polys + 1))
    return pts.reshape(n_pts, 3), conn.reshape(n_polys, 3)


def test_write_polydata_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    pts = rng.standard_normal((37, 3))
    pts[3] = np.nan
    tris = rng.integers(0, 37, size=(51, 3)).astype(np.int64)
    capi.write_polydata(str(tmp_path / "m.vtp"), pts, tris)
    p, t = read_vtp(str(tmp_path / "m.vtp"))
    assert p.tobytes() == pts.tobytes() and t.tobytes() == tris.tobytes()
    capi.write_polydata(str(tmp_path / "e.vtp"), np.zeros((0, 3)), np.zeros((0, 3), np.int64))
    p, t = read_vtp(str(tmp_path / "e.vtp"))
    assert p.shape == (0, 3) and t.shape == (0, 3)
    L = capi.load_host()
    assert L.dmi_write_polydata(os.fsencode(str(tmp_path / "x.vtp")), None, -1, None, 0) == 0
    assert L.dmi_write_polydata(os.fsencode(str(tmp_path / "no_such_dir" / "x.vtp")), None, 0, None, 0) == 0


BASE = ["Reconstruction", "--gridOrigin", "-2.29", "-2.24", "-2.2", "--gridEnd", "1.19", "1.67", "1.22", "--dataFolder", "data",
        "--outputGridFilename", "out.vts", "--outputMeshFilename", "mesh.vtp", "--rayThick", "0.1", "--gridDims", "10"]


def test_cli_extract_mesh_flag_parses_and_defaults_off():
    o, text = capi.cli_read_arguments(BASE)
    assert o is not None and o.extract_mesh == 0, text
    o, text = capi.cli_read_arguments(BASE + ["--extractMesh"])
    assert o is not None and o.extract_mesh == 1, text
    o, text = capi.cli_read_arguments(BASE + ["--help"])
    assert o is None and "--extractMesh" in text


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def _mesh_check(ctx, grid, iso):
    pts = ctx.download_point_data()
    verts, tris = ctx.extract_isosurface(iso)
    wv, wt = R.extract(pts, iso, grid.origin, grid.spacing, np.asarray(grid.grid_matrix).reshape(4, 4))
    from helpers import bits_equal
    assert verts.shape == wv.shape and bits_equal(verts, wv), iso
    assert np.array_equal(tris, wt), iso
    # the cells that emit triangles are the pre-pass's ids
    n, ids = ctx.iso_active_cells(iso)
    assert np.array_equal(ids, R.emitting_cells(pts, iso))
    return verts, tris


def _cells(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.5, 2.5, size=shape)


@pytest.mark.gpu
@pytest.mark.parametrize("cells,rotated", [((1, 1, 1), False), ((70, 33, 17), True), ((130, 5, 40), False), ((64, 64, 64), False),
                                           ((300, 3, 2), True)])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_gpu_mesh_bit_exact_random_and_sphere(cells, rotated, dtype):
    grid = scene.default_grid(cells, rotated=rotated)
    nx, ny, nz = cells
    c = _cells((nz, ny, nx), seed=nx + 7 * ny + 3 * nz)
    if dtype == "f32":
        c = c.astype(np.float32).astype(np.float64)
    with capi.FusionContext(grid, scene.default_ray_potential(grid), grid_dtype=dtype) as ctx:
        ctx.upload_grid(c)
        for iso in (1.0, 0.0, 0.37):
            _mesh_check(ctx, grid, iso)
        # a sphere SDF
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        s = 0.4 * max(cells) - np.sqrt((i - nx / 2) ** 2 + (j - ny / 2) ** 2 + (k - nz / 2) ** 2)
        if dtype == "f32":
            s = s.astype(np.float32).astype(np.float64)
        ctx.upload_grid(s)
        v1, t1 = _mesh_check(ctx, grid, 0.0)
        # a second call gives the same bits; the kernel time is reported
        v2, t2 = ctx.extract_isosurface(0.0)
        assert v1.tobytes() == v2.tobytes() and np.array_equal(t1, t2)
        assert ctx.isosurface_kernel_ms() > 0.0


@pytest.mark.gpu
def test_gpu_mesh_nan_and_iso_on_lattice_values():
    grid = scene.default_grid((40, 23, 19), rotated=True)
    nx, ny, nz = grid.cell_dims
    c = np.round(_cells((nz, ny, nx), seed=9) * 2) / 2      # values on a 0.5 lattice: iso 1.0 hits point values exactly
    c[3:6, 4:9, 10:20] = np.nan
    c[0, 0, 0] = np.nan
    with capi.FusionContext(grid, scene.default_ray_potential(grid)) as ctx:
        ctx.upload_grid(c)
        pts = ctx.download_point_data()
        assert np.isnan(pts).any() and (pts == 1.0).any()
        verts, tris = _mesh_check(ctx, grid, 1.0)
        tri_pts = verts[tris]
        degenerate = np.all(tri_pts[:, 0] == tri_pts[:, 1], axis=1) | np.all(tri_pts[:, 1] == tri_pts[:, 2], axis=1)
        assert degenerate.any()                             # t = 0 vertices collapse triangles; they are kept
        _mesh_check(ctx, grid, 0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("iso", [1.0, 0.0])
def test_gpu_mesh_of_a_fused_scene(iso):
    grid = scene.default_grid((48, 40, 36))
    ray = scene.default_ray_potential(grid)
    views = scene.make_views(5, 96, 72, seed=11, dense=True)
    with capi.FusionContext(grid, ray) as ctx:
        ctx.add_views(views)
        ctx.fuse()
        verts, tris = _mesh_check(ctx, grid, iso)
        assert len(tris) > 100


@pytest.mark.gpu
def test_gpu_mesh_follows_the_grid_and_refuses_bad_calls():
    grid = scene.default_grid((30, 20, 10))
    ray = scene.default_ray_potential(grid)
    lib = capi.load()
    nv, nt = ctypes.c_uint64(7), ctypes.c_uint64(7)
    with capi.FusionContext(grid, ray) as ctx:
        dv = np.zeros(3)
        dt = np.zeros(3, dtype=np.int64)
        # download before any extraction
        rc = lib.dmi_download_isosurface(ctx._h, capi._dp(dv), dt.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
        assert rc == INVALID_ARGUMENT
        ctx.upload_grid(_cells((10, 20, 30), seed=3))
        v0, t0 = _mesh_check(ctx, grid, 1.0)
        assert len(t0) > 0
        assert lib.dmi_extract_isosurface(ctx._h, float("nan"), ctypes.byref(nv), ctypes.byref(nt)) == INVALID_ARGUMENT
        assert lib.dmi_extract_isosurface(ctx._h, 1.0, None, ctypes.byref(nt)) == INVALID_ARGUMENT
        assert lib.dmi_extract_isosurface(ctx._h, 1.0, ctypes.byref(nv), ctypes.byref(nt)) == 0
        assert lib.dmi_download_isosurface(ctx._h, None, dt.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) == INVALID_ARGUMENT
        assert lib.dmi_get_isosurface_kernel_ms(ctx._h, None) == INVALID_ARGUMENT
        # the grid changes: the mesh follows it
        ctx.reset_grid()
        v, t = ctx.extract_isosurface(1.0)
        assert v.shape == (0, 3) and t.shape == (0, 3)        # an empty surface is a success
        views = scene.make_views(3, 64, 48, seed=2, dense=True)
        ctx.add_views(views)
        ctx.fuse()
        _mesh_check(ctx, grid, 1.0)
    with capi.FusionContext(grid, ray, z_first=8) as ctx:
        assert lib.dmi_extract_isosurface(ctx._h, 1.0, ctypes.byref(nv), ctypes.byref(nt)) == INVALID_ARGUMENT


@pytest.mark.gpu
def test_gpu_mesh_full_size_cfg3_speckle():
    """512^3, the speckle scene of bench.py --full's cfg 3: totals equal the restatement's counts; the triangles of 4096
    sampled cells and their vertices are bit-exact."""
    from helpers import bits_equal
    grid = scene.default_grid(512)
    ray = scene.default_ray_potential(grid)
    # the first 32 of the 256 views of bench.py's cfg 3 speckle scene (1280 x 720, best-cost threshold applied)
    views, thr = scene.make_scene_views("speckle", 256, 1280, 720, seed=1000, view_range=(0, 32), noise_sigma=float(max(grid.spacing)))
    with capi.FusionContext(grid, ray) as ctx:
        ctx.add_views(views, threshold=thr)
        ctx.fuse()
        pts = ctx.download_point_data()
        verts, tris = ctx.extract_isosurface(1.0)
    nv, nt = R.counts(pts, 1.0)
    assert (len(verts), len(tris)) == (nv, nt) and nt > 1000
    cells = R.emitting_cells(pts, 1.0)
    rng = np.random.default_rng(7)
    pick = np.sort(rng.choice(cells, size=min(4096, len(cells)), replace=False))
    n_tri = R.TRI_COUNT.astype(np.uint8)[R.cell_cases(pts >= 1.0).reshape(-1)]
    first = (np.cumsum(n_tri, dtype=np.int64) - n_tri)[pick]        # each sampled cell's first triangle
    want_tris, ids, want_verts = R.sampled_cells(pts, 1.0, pick, grid.origin, grid.spacing, np.asarray(grid.grid_matrix).reshape(4, 4))
    got = np.concatenate([tris[f:f + int(n)] for f, n in zip(first, n_tri[pick])])
    assert np.array_equal(got, want_tris)
    assert bits_equal(verts[ids], want_verts)


@pytest.mark.gpu
def test_gpu_cli_extract_mesh_end_to_end(tmp_path):
    """dmi_reconstruction --extractMesh: mesh.vtp holds the restatement applied to the oracle's fused grid, bit for bit, and the
    summary reports its size."""
    from oracle import oracle
    from helpers import bits_equal, oracle_params_from_scene
    grid = scene.default_grid((24, 20, 16), rotated=True)
    rp = scene.default_ray_potential(grid)
    views = scene.make_views(5, 48, 36, seed=4, dense=True, with_best_cost=True)
    data = tmp_path / "data"
    data.mkdir()
    lv, lk = scene.write_view_files(str(data), views)
    gm = np.asarray(grid.grid_matrix).reshape(4, 4)
    end = [grid.origin[a] + (grid.cell_dims[a] + 1) * grid.spacing[a] for a in range(3)]
    args = [capi.cli_binary(), "--dataFolder", str(data), "--depthMapFile", os.path.basename(lv), "--KRTFile", os.path.basename(lk),
            "--gridDims"] + [str(c + 1) for c in grid.cell_dims] + ["--gridOrigin"] + [repr(float(v)) for v in grid.origin] + \
           ["--gridEnd"] + [repr(float(v)) for v in end] + ["--gridVecX"] + [repr(float(v)) for v in gm[0, :3]] + \
           ["--gridVecY"] + [repr(float(v)) for v in gm[1, :3]] + ["--gridVecZ"] + [repr(float(v)) for v in gm[2, :3]] + \
           ["--rayThick", repr(rp.thickness), "--rayRho", repr(rp.rho), "--rayEta", repr(rp.eta), "--rayDelta", repr(rp.delta),
            "--threshBestCost", "0.7", "--contour", "0.25", "--outputGridFilename", str(tmp_path / "volume.vts"),
            "--outputMeshFilename", str(tmp_path / "mesh.vtp"), "--summary", "--extractMesh"]
    r = subprocess.run(args, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "is NOT written" not in r.stdout + r.stderr
    o, _ = capi.cli_read_arguments(args)
    g2 = scene.GridDesc(tuple(int(d) - 1 for d in o.grid_dims), tuple(o.grid_origin), tuple(o.grid_spacing), np.array(o.grid_matrix).reshape(4, 4))
    d = oracle.apply_depth_threshold(views.depth, views.best_cost, 0.7).reshape(views.depth.shape)
    want, _, _ = oracle.fuse(oracle_params_from_scene(g2, rp, views), d, views.K4, views.RT4, n_threads=oracle.max_threads())
    pts = oracle.cell_to_point(want)
    wv, wt = R.extract(pts, 0.25, o.grid_origin, o.grid_spacing, np.array(o.grid_matrix).reshape(4, 4))
    v, t = read_vtp(str(tmp_path / "mesh.vtp"))
    assert len(wt) > 0
    assert v.shape == wv.shape and bits_equal(v, wv) and np.array_equal(t, wt)
    summary = open(data / "summary.txt").read()
    assert f"mesh vertices  {len(wv)}\n" in summary and f"mesh triangles  {len(wt)}\n" in summary
    assert f"{len(wv)} vertices, {len(wt)} triangles" in r.stdout + r.stderr
