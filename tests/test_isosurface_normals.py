"""dmi_extract_isosurface_normals: the CPU restatement's normals on spheres and under sheared and mirrored grid
matrices, the .vtp writer's point arrays and the --meshNormals flag on the CPU; the GPU normals bit for bit against the
restatement (tests/isosurface_normals_np.py), next to the plain call's mesh."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import isosurface_normals_np as RN
import isosurface_np as R
from cudadepthmapintegration_amd import capi, scene

INVALID_ARGUMENT = 1   # DMI_ERR_INVALID_ARGUMENT (include/dmi.h)


def _sphere(n, spacing, origin=(0.0, 0.0, 0.0), frac=0.35):
    """Signed distance to a sphere (inside >= 0) on an n^3-cell lattice: (P, centre, radius) in lattice-space coordinates."""
    ext = np.array([n * s for s in spacing])
    c = np.asarray(origin) + ext / 2
    r = frac * ext.min()
    k, j, i = np.meshgrid(*[np.arange(n + 1)] * 3, indexing="ij")
    x = np.stack([origin[0] + i * spacing[0], origin[1] + j * spacing[1], origin[2] + k * spacing[2]], -1)
    return r - np.linalg.norm(x - c, axis=-1), c, r


def _unit(v):
    return v / np.linalg.norm(v, axis=1)[:, None]


def _world_radial(verts, M, c):
    """The exact outward normal of the sphere at each world vertex: inverse(A)^T (x - c) with x the lattice-space point."""
    A = M[:3, :3]
    x = np.linalg.solve(A, (verts - M[:3, 3]).T).T
    return _unit((np.linalg.inv(A).T @ (x - c).T).T)


def _interior(P, pts, margin=2):
    nz, ny, nx = (s - 1 for s in P.shape)
    k, j, i = pts[:, 0], pts[:, 1], pts[:, 2]
    return (i >= margin) & (i <= nx - margin - 1) & (j >= margin) & (j <= ny - margin - 1) & (k >= margin) & (k <= nz - margin - 1)


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_normal_matrix_is_the_identity_for_the_identity_and_inverse_transpose_up_to_a_positive_factor():
    assert RN.normal_matrix(np.eye(4)).tobytes() == np.eye(3).tobytes()
    rng = np.random.default_rng(3)
    for _ in range(20):
        M = np.eye(4)
        M[:3, :3] = rng.standard_normal((3, 3))
        Nm = RN.normal_matrix(M)
        want = np.linalg.inv(M[:3, :3]).T
        f = Nm / want
        assert np.all(f > 0) and np.allclose(f, f[0, 0], rtol=1e-9)


@pytest.mark.parametrize("n,spacing", [(24, (1.0, 1.0, 1.0)), (30, (0.5, 1.0, 0.8)), (20, (0.07, 0.05, 0.11))])
def test_sphere_normals_are_radial_and_agree_with_the_faces(n, spacing):
    P, c, r = _sphere(n, spacing)
    verts, tris, normals = RN.extract_with_normals(P, 0.0, (0.0, 0.0, 0.0), spacing, np.eye(4))
    verts0, tris0 = R.extract(P, 0.0, (0.0, 0.0, 0.0), spacing, np.eye(4))
    assert verts.tobytes() == verts0.tobytes() and np.array_equal(tris, tris0)
    assert normals.dtype == np.float32 and normals.shape == verts.shape
    assert np.allclose(np.linalg.norm(normals.astype(np.float64), axis=1), 1.0, atol=1e-6)
    pts, _ = RN.vertex_edges(P, 0.0)
    away = _interior(P, pts)
    assert away.sum() > 100
    cos = np.einsum("ij,ij->i", normals[away].astype(np.float64), _unit(verts[away] - c))
    assert np.degrees(np.arccos(np.clip(cos.min(), -1, 1))) < 3.0
    # every vertex normal of a non-degenerate triangle lies on the side its (inside -> outside) face normal points to
    T = verts[tris]
    f = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    area = np.linalg.norm(f, axis=1)
    ok = area > 1e-9 * area.max()
    side = np.einsum("tvi,ti->tv", normals[tris].astype(np.float64), f)[ok]
    assert (side > 0).all(axis=1).mean() >= 0.99


SHEARED = np.array([[0.0, 2.5, 0.0, 0.3], [-0.7, 0.0, 0.0, -1.0], [0.0, 0.0, 1.3, 2.0], [0.0, 0.0, 0.0, 1.0]])   # det > 0
MIRRORED = np.array([[1.7, 0.0, 0.0, 0.0], [0.0, 0.0, 0.6, 0.5], [0.0, 2.2, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]])   # det < 0


@pytest.mark.parametrize("M", [SHEARED, MIRRORED], ids=["sheared", "mirrored"])
def test_world_normals_are_perpendicular_to_the_world_mesh_and_point_outward(M):
    """Orthogonal axes of different lengths, one set mirrored: the normals go through inverse(A)^T, not A.  Using A instead
    breaks the perpendicularity test below (checked here, so the test is known to catch it)."""
    assert (np.linalg.det(M[:3, :3]) < 0) == (M is MIRRORED)
    spacing = (0.5, 1.0, 0.8)
    P, c, r = _sphere(40, spacing)
    verts, tris, normals = RN.extract_with_normals(P, 0.0, (0.0, 0.0, 0.0), spacing, M)
    n = normals.astype(np.float64)
    # outward: along the exact normal of the (ellipsoidal) world surface
    cos = np.einsum("ij,ij->i", n, _world_radial(verts, M, c))
    pts, _ = RN.vertex_edges(P, 0.0)
    assert cos.min() > 0 and np.degrees(np.arccos(np.clip(cos[_interior(P, pts)].min(), -1, 1))) < 3.0
    # perpendicular to the world triangle edges at each vertex
    T = verts[tris]
    e = np.concatenate([T[:, 1] - T[:, 0], T[:, 2] - T[:, 1], T[:, 0] - T[:, 2]])
    at = np.concatenate([tris[:, 0], tris[:, 1], tris[:, 2]])
    length = np.linalg.norm(e, axis=1)
    ok = length > 1e-9 * length.max()

    def off_plane(normal):
        return np.abs(np.einsum("ij,ij->i", normal[at[ok]], e[ok])) / length[ok]
    good = off_plane(n)
    assert good.mean() < 0.06 and np.percentile(good, 99) < 0.25
    Nm_wrong = M[:3, :3]                                    # the grid matrix itself where inverse(A)^T belongs
    g = RN.neg_gradient(P, pts, spacing)
    wrong = _unit((Nm_wrong @ g.T).T)
    assert off_plane(wrong).mean() > 3 * good.mean()


def test_nan_lattice_values_and_flat_fields():
    P = np.full((5, 6, 7), -1.0)
    P[2, 2:4, 2:5] = 1.0
    P[2, 3, 3] = np.nan
    verts, tris, normals = RN.extract_with_normals(P, 0.0)
    assert np.isnan(normals).any() and not np.isnan(verts).any()
    finite = ~np.isnan(normals).any(axis=1)
    assert np.allclose(np.linalg.norm(normals[finite].astype(np.float64), axis=1), 1.0, atol=1e-6)
    # a zero gradient at both ends leaves n = w = 0 (no division)
    P = np.zeros((3, 3, 4))
    P[:, :, 2:] = 1.0
    P[:, :, 1] = 1.0                                   # iso 1: the crossed x edges run from value 0 to 1
    _, _, normals = RN.extract_with_normals(P, 1.0)
    assert np.isfinite(normals).all()


# ---- host side: the .vtp writer and the flag ---------------------------------------------------------------------------
def read_vtp_point_data(path):
    """(points, triangles, Normals [n, 3] f32, reconstruction_scalar [n] f64) of a .vtp written with normals."""
    raw = open(path, "rb").read()
    head, _, tail = raw.partition(b'<AppendedData encoding="raw">\n   _')
    text = head.decode()
    assert '<PointData Normals="Normals" Scalars="reconstruction_scalar">' in text
    assert '<DataArray type="Float32" Name="Normals" NumberOfComponents="3" format="appended"' in text
    assert '<DataArray type="Float64" Name="reconstruction_scalar" format="appended"' in text
    n_pts = int(text.split('NumberOfPoints="')[1].split('"')[0])
    n_polys = int(text.split('NumberOfPolys="')[1].split('"')[0])
    names = ("Points", "connectivity", "offsets", "Normals", "reconstruction_scalar")
    dts = (np.float64, np.int64, np.int64, np.float32, np.float64)
    arrays = []
    for name, dt in zip(names, dts):
        off = int(text.split(f'Name="{name}"')[1].split('offset="')[1].split('"')[0])
        (nb,) = struct.unpack_from("<Q", tail, off)
        arrays.append(np.frombuffer(tail, dtype=dt, count=nb // np.dtype(dt).itemsize, offset=off + 8))
    assert tail.endswith(b"\n  </AppendedData>\n</VTKFile>\n")
    pts, conn, offsets, normals, scalar = arrays
    assert np.array_equal(offsets, 3 * np.arange(1, n_polys + 1))
    return pts.reshape(n_pts, 3), conn.reshape(n_polys, 3), normals.reshape(n_pts, 3), scalar


def test_write_polydata_with_normals_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    pts = rng.standard_normal((37, 3))
    tris = rng.integers(0, 37, size=(51, 3)).astype(np.int64)
    normals = rng.standard_normal((37, 3)).astype(np.float32)
    normals[5] = np.float32(-0.0)
    normals[6, 1] = np.nan
    capi.write_polydata_with_normals(str(tmp_path / "m.vtp"), pts, tris, normals, 0.25)
    p, t, n, s = read_vtp_point_data(str(tmp_path / "m.vtp"))
    assert p.tobytes() == pts.tobytes() and t.tobytes() == tris.tobytes() and n.tobytes() == normals.tobytes()
    assert s.shape == (37,) and np.all(s == 0.25)
    # the plain writer's file is the head of this one: the same bytes up to the point data and the appended tail
    capi.write_polydata(str(tmp_path / "plain.vtp"), pts, tris)
    plain = open(tmp_path / "plain.vtp", "rb").read()
    assert b"<PointData" not in plain
    capi.write_polydata_with_normals(str(tmp_path / "e.vtp"), np.zeros((0, 3)), np.zeros((0, 3), np.int64),
                                     np.zeros((0, 3), np.float32), 1.0)
    p, t, n, s = read_vtp_point_data(str(tmp_path / "e.vtp"))
    assert p.shape == (0, 3) and t.shape == (0, 3) and n.shape == (0, 3) and s.shape == (0,)
    L = capi.load_host()
    assert L.dmi_write_polydata_with_normals(os.fsencode(str(tmp_path / "x.vtp")), None, -1, None, 0, None, 1.0) == 0
    assert L.dmi_write_polydata_with_normals(os.fsencode(str(tmp_path / "x.vtp")), None, 0, None, -2, None, 1.0) == 0
    assert L.dmi_write_polydata_with_normals(os.fsencode(str(tmp_path / "no_such_dir" / "x.vtp")), None, 0, None, 0, None, 1.0) == 0


BASE = ["Reconstruction", "--gridOrigin", "-2.29", "-2.24", "-2.2", "--gridEnd", "1.19", "1.67", "1.22", "--dataFolder", "data",
        "--outputGridFilename", "out.vts", "--outputMeshFilename", "mesh.vtp", "--rayThick", "0.1", "--gridDims", "10"]


def test_cli_mesh_normals_flag_needs_extract_mesh():
    o, text = capi.cli_read_arguments(BASE)
    assert o is not None and o.mesh_normals == 0, text
    o, text = capi.cli_read_arguments(BASE + ["--extractMesh"])
    assert o is not None and o.extract_mesh == 1 and o.mesh_normals == 0, text
    o, text = capi.cli_read_arguments(BASE + ["--extractMesh", "--meshNormals"])
    assert o is not None and o.extract_mesh == 1 and o.mesh_normals == 1, text
    o, text = capi.cli_read_arguments(BASE + ["--meshNormals"])
    assert o is None and "--meshNormals" in text.split("\n")[0] and "--extractMesh" in text.split("\n")[0]
    o, text = capi.cli_read_arguments(BASE + ["--help"])
    assert o is None and "--meshNormals" in text


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def _normals_check(ctx, grid, iso):
    """The normals call against the plain call (vertices and triangles, bit for bit) and the restatement (normals)."""
    from helpers import bits_equal
    pts = ctx.download_point_data()
    v0, t0 = ctx.extract_isosurface(iso)
    verts, tris, normals = ctx.extract_isosurface_with_normals(iso)
    assert verts.tobytes() == v0.tobytes() and np.array_equal(tris, t0), iso
    M = np.asarray(grid.grid_matrix).reshape(4, 4)
    wv, wt, wn = RN.extract_with_normals(pts, iso, grid.origin, grid.spacing, M)
    assert verts.shape == wv.shape and bits_equal(verts, wv) and np.array_equal(tris, wt), iso
    assert normals.dtype == np.float32 and normals.shape == wn.shape and bits_equal(normals, wn), iso
    return verts, tris, normals


def _cells(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.5, 2.5, size=shape)


@pytest.mark.gpu
@pytest.mark.parametrize("cells,rotated", [((1, 1, 1), False), ((70, 33, 17), True), ((130, 5, 40), False), ((64, 64, 64), False),
                                           ((300, 3, 2), True)])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_gpu_normals_bit_exact_random_and_sphere(cells, rotated, dtype):
    grid = scene.default_grid(cells, rotated=rotated)
    nx, ny, nz = cells
    c = _cells((nz, ny, nx), seed=nx + 7 * ny + 3 * nz)
    if dtype == "f32":
        c = c.astype(np.float32).astype(np.float64)
    with capi.FusionContext(grid, scene.default_ray_potential(grid), grid_dtype=dtype) as ctx:
        ctx.upload_grid(c)
        for iso in (1.0, 0.0, 0.37):
            _normals_check(ctx, grid, iso)
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        s = 0.4 * max(cells) - np.sqrt((i - nx / 2) ** 2 + (j - ny / 2) ** 2 + (k - nz / 2) ** 2)
        if dtype == "f32":
            s = s.astype(np.float32).astype(np.float64)
        ctx.upload_grid(s)
        v1, t1, n1 = _normals_check(ctx, grid, 0.0)
        # a second call gives the same bits; the kernel time is reported
        v2, t2, n2 = ctx.extract_isosurface_with_normals(0.0)
        assert v1.tobytes() == v2.tobytes() and np.array_equal(t1, t2) and n1.tobytes() == n2.tobytes()
        assert ctx.isosurface_kernel_ms() > 0.0


@pytest.mark.gpu
def test_gpu_normals_nan_and_iso_on_lattice_values():
    grid = scene.default_grid((40, 23, 19), rotated=True)
    nx, ny, nz = grid.cell_dims
    c = np.round(_cells((nz, ny, nx), seed=9) * 2) / 2
    c[3:6, 4:9, 10:20] = np.nan
    c[0, 0, 0] = np.nan
    with capi.FusionContext(grid, scene.default_ray_potential(grid)) as ctx:
        ctx.upload_grid(c)
        _, _, normals = _normals_check(ctx, grid, 1.0)
        assert np.isnan(normals).any()
        _normals_check(ctx, grid, 0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("iso", [1.0, 0.0])
def test_gpu_normals_of_a_fused_scene(iso):
    grid = scene.default_grid((48, 40, 36))
    views = scene.make_views(5, 96, 72, seed=11, dense=True)
    with capi.FusionContext(grid, scene.default_ray_potential(grid)) as ctx:
        ctx.add_views(views)
        ctx.fuse()
        _, tris, _ = _normals_check(ctx, grid, iso)
        assert len(tris) > 100


@pytest.mark.gpu
@pytest.mark.parametrize("M", [SHEARED, MIRRORED], ids=["sheared", "mirrored"])
def test_gpu_normals_under_sheared_and_mirrored_grid_matrices(M):
    n = 40
    grid = scene.GridDesc((n, n, n), (-1.0, -1.0, -1.0), (0.05, 0.06, 0.045), M.copy())
    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    s = 13.0 - np.sqrt((1.0 * (i - 19.5)) ** 2 + (1.2 * (j - 19.5)) ** 2 + (0.9 * (k - 19.5)) ** 2)
    with capi.FusionContext(grid, scene.default_ray_potential(grid)) as ctx:
        ctx.upload_grid(s)
        verts, tris, normals = _normals_check(ctx, grid, 0.0)
        assert len(tris) > 1000 and np.isfinite(normals).all()


@pytest.mark.gpu
def test_gpu_normals_refuse_bad_calls():
    grid = scene.default_grid((30, 20, 10))
    ray = scene.default_ray_potential(grid)
    lib = capi.load()
    nv, nt = ctypes.c_uint64(7), ctypes.c_uint64(7)
    fp = ctypes.POINTER(ctypes.c_float)
    dn = np.zeros(3, dtype=np.float32)
    with capi.FusionContext(grid, ray) as ctx:
        # before any extraction
        assert lib.dmi_download_isosurface_normals(ctx._h, dn.ctypes.data_as(fp)) == INVALID_ARGUMENT
        ctx.upload_grid(_cells((10, 20, 30), seed=3))
        # after a plain extraction
        v, t = ctx.extract_isosurface(1.0)
        assert len(t) > 0
        assert lib.dmi_download_isosurface_normals(ctx._h, dn.ctypes.data_as(fp)) == INVALID_ARGUMENT
        # after a normals extraction: works; a null pointer does not
        _, _, n1 = _normals_check(ctx, grid, 1.0)
        assert lib.dmi_download_isosurface_normals(ctx._h, None) == INVALID_ARGUMENT
        assert lib.dmi_extract_isosurface_normals(ctx._h, float("nan"), ctypes.byref(nv), ctypes.byref(nt)) == INVALID_ARGUMENT
        assert lib.dmi_extract_isosurface_normals(ctx._h, 1.0, None, ctypes.byref(nt)) == INVALID_ARGUMENT
        assert lib.dmi_extract_isosurface_normals(ctx._h, 1.0, ctypes.byref(nv), None) == INVALID_ARGUMENT
        # calls refused for their arguments leave the last mesh as it was, as dmi_extract_isosurface's do
        again = np.empty_like(n1)
        assert lib.dmi_download_isosurface_normals(ctx._h, again.ctypes.data_as(fp)) == 0
        assert again.tobytes() == n1.tobytes()
        # a later plain extraction drops the normals
        ctx.extract_isosurface(1.0)
        assert lib.dmi_download_isosurface_normals(ctx._h, dn.ctypes.data_as(fp)) == INVALID_ARGUMENT
        # an empty surface is a success
        ctx.reset_grid()
        v, t, n = ctx.extract_isosurface_with_normals(1.0)
        assert v.shape == (0, 3) and t.shape == (0, 3) and n.shape == (0, 3)
    with capi.FusionContext(grid, ray, z_first=8) as ctx:
        assert lib.dmi_extract_isosurface_normals(ctx._h, 1.0, ctypes.byref(nv), ctypes.byref(nt)) == INVALID_ARGUMENT


@pytest.mark.gpu
def test_gpu_normals_full_size_cfg3_speckle():
    """512^3, the first 32 views of bench.py --full's cfg-3 speckle scene: totals equal the restatement's counts, the mesh is
    the plain call's, and the normals of the vertices of 4096 sampled cells are bit-exact."""
    from helpers import bits_equal
    grid = scene.default_grid(512)
    ray = scene.default_ray_potential(grid)
    views, thr = scene.make_scene_views("speckle", 256, 1280, 720, seed=1000, view_range=(0, 32), noise_sigma=float(max(grid.spacing)))
    with capi.FusionContext(grid, ray) as ctx:
        ctx.add_views(views, threshold=thr)
        ctx.fuse()
        pts = ctx.download_point_data()
        v0, t0 = ctx.extract_isosurface(1.0)
        verts, tris, normals = ctx.extract_isosurface_with_normals(1.0)
    assert verts.tobytes() == v0.tobytes() and np.array_equal(tris, t0)
    del v0, t0
    nv, nt = R.counts(pts, 1.0)
    assert (len(verts), len(tris), len(normals)) == (nv, nt, nv) and nt > 1000
    cells = R.emitting_cells(pts, 1.0)
    rng = np.random.default_rng(7)
    pick = np.sort(rng.choice(cells, size=min(4096, len(cells)), replace=False))
    M = np.asarray(grid.grid_matrix).reshape(4, 4)
    _, ids, want_verts = R.sampled_cells(pts, 1.0, pick, grid.origin, grid.spacing, M)
    assert bits_equal(verts[ids], want_verts)
    want = RN.sampled_normals(pts, 1.0, ids, grid.spacing, M)
    assert bits_equal(normals[ids], want)


@pytest.mark.gpu
def test_gpu_cli_mesh_normals_end_to_end(tmp_path):
    """dmi_reconstruction --extractMesh --meshNormals: mesh.vtp's Normals are the restatement's over the oracle's fused grid,
    bit for bit, and its scalar array is the contour value; without --meshNormals the file has no point data."""
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
    r = subprocess.run(args + ["--meshNormals"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    o, _ = capi.cli_read_arguments(args + ["--meshNormals"])
    g2 = scene.GridDesc(tuple(int(d) - 1 for d in o.grid_dims), tuple(o.grid_origin), tuple(o.grid_spacing), np.array(o.grid_matrix).reshape(4, 4))
    d = oracle.apply_depth_threshold(views.depth, views.best_cost, 0.7).reshape(views.depth.shape)
    want, _, _ = oracle.fuse(oracle_params_from_scene(g2, rp, views), d, views.K4, views.RT4, n_threads=oracle.max_threads())
    pts = oracle.cell_to_point(want)
    wv, wt, wn = RN.extract_with_normals(pts, 0.25, o.grid_origin, o.grid_spacing, np.array(o.grid_matrix).reshape(4, 4))
    v, t, n, s = read_vtp_point_data(str(tmp_path / "mesh.vtp"))
    assert len(wt) > 0
    assert v.shape == wv.shape and bits_equal(v, wv) and np.array_equal(t, wt)
    assert n.shape == wn.shape and bits_equal(n, wn)
    assert np.all(s == 0.25)
    assert f"{len(wv)} vertices, {len(wt)} triangles" in r.stdout + r.stderr
    summary_with = open(data / "summary.txt").read()
    # the same run without --meshNormals: no point data, the same mesh
    r = subprocess.run(args, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    raw = open(tmp_path / "mesh.vtp", "rb").read()
    assert b"<PointData" not in raw
    from test_isosurface import read_vtp
    v2, t2 = read_vtp(str(tmp_path / "mesh.vtp"))
    assert v2.tobytes() == v.tobytes() and np.array_equal(t2, t)
    # the summary's lines are those of --extractMesh alone, apart from the command line and the times
    summary = open(data / "summary.txt").read()

    def steady(text):
        lines = text.split("time\n")[0].splitlines()
        return lines[:1] + lines[2:]                        # without the command line itself
    assert steady(summary_with) == steady(summary)
