"""dmi_filter_isosurface_components: the CPU restatement (tests/isosurface_components_np.py) against independent
labellings and on known shapes, the ABI, the CLI flags and the .vtp writer's RegionId array on the CPU; on the GPU every count and
every array of the filtered mesh against the restatement applied to the GPU's own unfiltered download, twice."""
import ctypes
import os
import struct
import subprocess
import time
from collections import Counter

import numpy as np
import pytest

import isosurface_components_np as C
import isosurface_normals_np as RN
import isosurface_np as R
from cudadepthmapintegration_amd import capi, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 1   # DMI_ERR_INVALID_ARGUMENT (include/dmi.h)
MIN, LARGEST = C.MIN_TRIANGLES, C.LARGEST


# ---- the restatement against independent labellings ----------------------------------------------------------------------
def _union_find_labels(n, tris):
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    for a, b, c in np.asarray(tris).reshape(-1, 3).tolist():
        for p, q in ((a, b), (a, c)):
            rp, rq = find(p), find(q)
            if rp != rq:
                parent[max(rp, rq)] = min(rp, rq)
    return np.array([find(v) for v in range(n)], dtype=np.int64)


def _soup(seed, n, m):
    """m random triangles over n vertices whose ids are mostly near each other: many components, some vertices unreferenced,
    some triangles degenerate."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n, size=m)
    t = np.stack([a, np.clip(a + rng.integers(-2, 3, size=m), 0, n - 1), np.clip(a + rng.integers(-2, 3, size=m), 0, n - 1)], -1)
    return t.astype(np.int64)


def _random_field_mesh(shape=(13, 12, 11), seed=3, iso=1.0):
    rng = np.random.default_rng(seed)
    return R.extract(rng.uniform(-1.5, 2.5, size=shape), iso)


@pytest.mark.parametrize("seed", range(6))
def test_restatement_equals_a_plain_union_find(seed):
    n = 40 + 37 * seed
    tris = _soup(seed, n, n // 2 + 11 * seed)
    lab, size = C.components(n, tris)
    want = _union_find_labels(n, tris)
    assert np.array_equal(lab, want)
    assert np.array_equal(size, np.bincount(want[tris[:, 0]], minlength=n))
    verts, mt = _random_field_mesh(seed=seed)
    assert np.array_equal(C.labels(len(verts), mt), _union_find_labels(len(verts), mt))
    # a path given from its far end: the deepest tree a hooking order can make
    n = 300
    chain = np.stack([np.arange(n - 1, 0, -1), np.arange(n - 2, -1, -1), np.arange(n - 2, -1, -1)], -1)
    assert not C.labels(n, chain).any()


@pytest.mark.parametrize("case", ["soup", "field48"])
def test_restatement_equals_scipy_connected_components(case):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    if case == "soup":
        n, tris = 5000, _soup(11, 5000, 4000)
    else:
        verts, tris = _random_field_mesh((33, 41, 49), seed=1)
        n = len(verts)
    i = np.concatenate([tris[:, 0], tris[:, 0], tris[:, 1]])
    j = np.concatenate([tris[:, 1], tris[:, 2], tris[:, 2]])
    g = sp.coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(n, n))
    k, cls = connected_components(g, directed=False)
    lab, size = C.components(n, tris)
    class_min = np.full(k, n, dtype=np.int64)
    np.minimum.at(class_min, cls, np.arange(n))
    assert np.array_equal(lab, class_min[cls])                       # the same partition, labelled by each class's minimum
    tri_per_class = np.bincount(cls[tris[:, 0]], minlength=k)
    assert np.array_equal(size[class_min], tri_per_class) and size.sum() == len(tris)
    assert C.filter_mesh(np.zeros((n, 3)), tris)["counts"][2] == k


# ---- known shapes ------------------------------------------------------------------------------------------------------------
def _lattice(nx, ny, nz):
    z, y, x = np.mgrid[0:nz + 1, 0:ny + 1, 0:nx + 1].astype(np.float64)
    return x, y, z


def three_spheres_field(nx=44, ny=30, nz=28):
    x, y, z = _lattice(nx, ny, nz)
    f = np.full(x.shape, -np.inf)
    for cx, cy, cz, r in ((10.2, 14.1, 13.3, 8.3), (26.4, 12.2, 12.1, 5.6), (37.3, 20.4, 15.2, 4.1)):
        f = np.maximum(f, r - np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2))
    return f


def eight_tubes_field(nx=20, ny=34, nz=18):
    """Eight tubes along x whose axes differ by whole lattice steps: their meshes are translates, so their sizes tie."""
    x, y, z = _lattice(nx, ny, nz)
    f = np.full(x.shape, -np.inf)
    for jy in range(4):
        for kz in range(2):
            f = np.maximum(f, 2.3 - np.sqrt((y - (4.4 + 8 * jy)) ** 2 + (z - (4.6 + 8 * kz)) ** 2))
    return f


def winding_tube_field(nx=40, ny=36, nz=24):
    """One tube that goes back and forth along x through every (y, z) lane of the grid: one component whose vertex graph has a
    diameter of the order of the whole path."""
    x, y, z = _lattice(nx, ny, nz)
    inside = np.zeros(x.shape, dtype=bool)
    lanes = [(j, k) for k in range(3, nz - 2, 6) for j in (range(3, ny - 2, 6) if (k // 6) % 2 == 0 else reversed(range(3, ny - 2, 6)))]
    for n, (j, k) in enumerate(lanes):
        inside |= (np.abs(y - j) <= 1) & (np.abs(z - k) <= 1) & (x >= 3) & (x <= nx - 3)
        if n + 1 < len(lanes):                                   # the bend to the next lane, at alternating ends
            j2, k2 = lanes[n + 1]
            xe = nx - 3 if n % 2 == 0 else 3
            inside |= (np.abs(x - xe) <= 1) & (y >= min(j, j2) - 1) & (y <= max(j, j2) + 1) & (z >= min(k, k2) - 1) & (z <= max(k, k2) + 1)
    return np.where(inside, 1.0, -1.0)


def _edge_use(tris):
    half = Counter()
    for a, b, c in tris.tolist():
        half[(a, b)] += 1
        half[(b, c)] += 1
        half[(c, a)] += 1
    return half


def _closed_chi(verts, tris):
    half = _edge_use(tris)
    assert all(n == 1 and half.get((b, a), 0) == 1 for (a, b), n in half.items())     # every edge once in each direction
    return len(verts) - len(half) // 2 + len(tris)


def test_three_spheres():
    verts, tris = R.extract(three_spheres_field(), 0.0)
    lab, size = C.components(len(verts), tris)
    sizes = np.sort(size[size > 0])
    assert len(sizes) == 3 and sizes[0] < sizes[1] < sizes[2]
    big = C.filter_mesh(verts, tris, mode=LARGEST)
    assert big["counts"] == (int((lab == lab[np.argmax(size)]).sum()), int(sizes[2]), 3, 1)
    assert _closed_chi(big["vertices"], big["triangles"]) == 2
    assert np.array_equal(big["region_id"], np.zeros(len(big["vertices"]), np.int64)) and big["region_size"].tolist() == [sizes[2]]
    two = C.filter_mesh(verts, tris, mode=MIN, min_triangles=int(sizes[0]) + 1)
    assert two["counts"][2:] == (3, 2) and two["counts"][1] == sizes[1] + sizes[2]
    assert _closed_chi(two["vertices"], two["triangles"]) == 4
    assert C.filter_mesh(verts, tris, mode=MIN, min_triangles=int(sizes[1]) + 1)["counts"][3] == 1


def test_eight_equal_tubes_tie_goes_to_the_smallest_label():
    verts, tris = R.extract(eight_tubes_field(), 0.0)
    lab, size = C.components(len(verts), tris)
    roots = np.flatnonzero(lab == np.arange(len(verts)))
    assert len(roots) == 8 and len(set(size[roots].tolist())) == 1 and roots[0] == 0
    out = C.filter_mesh(verts, tris, mode=LARGEST)
    assert out["counts"] == (int((lab == 0).sum()), int(size[0]), 8, 1)
    assert out["vertices"].tobytes() == verts[lab == 0].tobytes()


def test_winding_tube_is_one_component():
    verts, tris = R.extract(winding_tube_field(), 0.0)
    assert C.filter_mesh(verts, tris, mode=LARGEST)["counts"] == (len(verts), len(tris), 1, 1)
    assert _closed_chi(verts, tris) == 2


def test_random_field_has_thousands_of_components():
    rng = np.random.default_rng(48 + 7 * 40 + 3 * 32)
    verts, tris = R.extract(rng.uniform(-1.5, 2.5, size=(33, 41, 49)), 1.0)      # 48 x 40 x 32 cells
    lab, size = C.components(len(verts), tris)
    assert ((lab[tris[:, 0]] == lab[tris[:, 1]]) & (lab[tris[:, 0]] == lab[tris[:, 2]])).all()
    unref = np.ones(len(verts), dtype=bool)
    unref[tris.reshape(-1)] = False
    assert not unref.any()                                        # every marching-cubes vertex is named by a triangle
    n_comp = int((lab == np.arange(len(verts))).sum())
    assert n_comp > 1000 and size.sum() == len(tris) and size[size > 0].min() >= 1
    for n in (0, 2, 3, 10, 1000, len(tris) + 1):
        out = C.filter_mesh(verts, tris, mode=MIN, min_triangles=n)
        assert out["counts"][1] == out["region_size"].sum() == size[size >= max(n, 1)].sum()
        assert out["counts"][2] == n_comp and out["counts"][3] == len(out["region_size"])
    assert C.filter_mesh(verts, tris, mode=MIN, min_triangles=len(tris) + 1)["counts"] == (0, 0, n_comp, 0)


def test_unreferenced_vertex_and_degenerate_links():
    verts = np.arange(24, dtype=np.float64).reshape(8, 3)
    tris = np.array([[5, 6, 7], [1, 2, 3], [3, 3, 5]], dtype=np.int64)    # 0 and 4 unreferenced; (3, 3, 5) joins the two parts
    lab, size = C.components(8, tris)
    assert lab.tolist() == [0, 1, 1, 1, 4, 1, 1, 1] and size.tolist() == [0, 3, 0, 0, 0, 0, 0, 0]
    out = C.filter_mesh(verts, tris, mode=MIN, min_triangles=0)
    assert out["counts"] == (8, 3, 3, 3) and out["region_id"].tolist() == [0, 1, 1, 1, 2, 1, 1, 1]
    assert out["region_size"].tolist() == [0, 3, 0] and np.array_equal(out["triangles"], tris)
    out = C.filter_mesh(verts, tris, mode=MIN, min_triangles=1)
    assert out["counts"] == (6, 3, 3, 1) and out["triangles"].tolist() == [[3, 4, 5], [0, 1, 2], [2, 2, 3]]
    assert out["vertices"].tobytes() == verts[[1, 2, 3, 5, 6, 7]].tobytes()
    # without the degenerate triangle the parts are two components; a tie, so LARGEST keeps the smaller label
    out = C.filter_mesh(verts, tris[:2], mode=LARGEST)
    assert out["counts"] == (3, 1, 4, 1) and out["triangles"].tolist() == [[0, 1, 2]] and out["vertices"].tobytes() == verts[1:4].tobytes()
    # LARGEST of a mesh without triangles keeps vertex 0's component; of no mesh at all, nothing
    assert C.filter_mesh(verts, tris[:0], mode=LARGEST)["counts"] == (1, 0, 8, 1)
    assert C.filter_mesh(verts[:0], tris[:0], mode=LARGEST)["counts"] == (0, 0, 0, 0)


def test_order_remapping_region_ids_idempotence_and_composition():
    verts, tris = _random_field_mesh((17, 19, 23), seed=8)
    rng = np.random.default_rng(0)
    normals = rng.standard_normal(verts.shape).astype(np.float32)
    lab, size = C.components(len(verts), tris)
    n = int(np.median(size[size > 0])) + 1
    out = C.filter_mesh(verts, tris, normals, MIN, n)
    keep_v = size[lab] >= n
    old = np.flatnonzero(keep_v)                                   # ascending old ids
    assert out["vertices"].tobytes() == verts[old].tobytes() and out["normals"].tobytes() == normals[old].tobytes()
    keep_t = keep_v[tris[:, 0]]
    assert np.array_equal(old[out["triangles"]], tris[keep_t])     # original order, remapped ids
    kept_labels = np.unique(lab[old])                              # ascending labels -> 0, 1, 2, ...
    assert np.array_equal(kept_labels[out["region_id"]], lab[old]) and np.array_equal(out["region_size"], size[kept_labels])
    again = C.filter_mesh(out["vertices"], out["triangles"], out["normals"], MIN, n)
    for k in ("vertices", "triangles", "normals", "region_id", "region_size"):
        assert again[k].tobytes() == out[k].tobytes(), k
    assert again["counts"] == out["counts"][:2] + (out["counts"][3],) * 2
    big = C.filter_mesh(verts, tris, normals, LARGEST)
    assert big["counts"][1] >= n
    both = C.filter_mesh(out["vertices"], out["triangles"], out["normals"], LARGEST)
    for k in ("vertices", "triangles", "normals", "region_id", "region_size"):
        assert both[k].tobytes() == big[k].tobytes(), k


# ---- ABI, CLI flags, writer -----------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["dmi_filter_isosurface_components", "dmi_download_isosurface_regions", "dmi_get_isosurface_filter_kernel_ms",
               "dmi_get_isosurface_filter_pass_ms", "dmi_get_isosurface_filter_cas_retries"]


def test_abi_has_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "dmi.h")).read()
    lib = ctypes.CDLL(capi.load()._name)
    for name in NEW_SYMBOLS:
        assert name + "(" in header and name in capi.ABI_SYMBOLS and hasattr(lib, name), name
    assert "DMI_COMPONENTS_MIN_TRIANGLES = 0, DMI_COMPONENTS_LARGEST = 1" in header
    assert lib.dmi_abi_version() == 5
    host = open(os.path.join(ROOT, "include", "dmi_host.h")).read()
    assert "dmi_write_polydata_with_arrays(" in host and "dmi_write_polydata_with_arrays" in capi.HOST_ABI_SYMBOLS
    assert hasattr(lib, "dmi_write_polydata_with_arrays")
    # null pointers and a null context are refused without a device
    assert capi.load().dmi_filter_isosurface_components(None, 0, 0, None, None, None, None) == INVALID_ARGUMENT
    assert capi.load().dmi_download_isosurface_regions(None, None, None) == INVALID_ARGUMENT
    assert capi.load().dmi_get_isosurface_filter_kernel_ms(None, None) == INVALID_ARGUMENT


BASE = ["Reconstruction", "--gridOrigin", "-2.29", "-2.24", "-2.2", "--gridEnd", "1.19", "1.67", "1.22", "--dataFolder", "data",
        "--outputGridFilename", "out.vts", "--outputMeshFilename", "mesh.vtp", "--rayThick", "0.1", "--gridDims", "10"]


def test_cli_component_flags():
    o, text = capi.cli_read_arguments(BASE + ["--extractMesh"])
    assert o is not None and (o.mesh_min_component_triangles, o.mesh_largest_component, o.mesh_region_ids) == (-1, 0, 0), text
    o, text = capi.cli_read_arguments(BASE + ["--extractMesh", "--meshMinComponentTriangles", "120"])
    assert o is not None and (o.mesh_min_component_triangles, o.mesh_largest_component, o.mesh_region_ids) == (120, 0, 0), text
    o, text = capi.cli_read_arguments(BASE + ["--extractMesh", "--meshMinComponentTriangles", "0", "--meshLargestComponent", "--meshRegionIds"])
    assert o is not None and (o.mesh_min_component_triangles, o.mesh_largest_component, o.mesh_region_ids) == (0, 1, 1), text
    assert (o.extract_mesh, o.mesh_normals) == (1, 0)
    for flag in (["--meshMinComponentTriangles", "5"], ["--meshLargestComponent"], ["--meshRegionIds"]):
        o, text = capi.cli_read_arguments(BASE + flag)
        first = text.split("\n")[0]
        assert o is None and first.startswith("Error : " + flag[0] + " needs --extractMesh"), text
    for bad in ("-3", "x", "1.5", "", "+2", "1e3"):
        o, text = capi.cli_read_arguments(BASE + ["--extractMesh", "--meshMinComponentTriangles", bad])
        assert o is None and text.startswith("Bad value for --meshMinComponentTriangles"), (bad, text)
    o, text = capi.cli_read_arguments(BASE + ["--extractMesh", "--meshMinComponentTriangles"])
    assert o is None and "needs a value" in text
    o, text = capi.cli_read_arguments(BASE + ["--help"])
    assert o is None and all(f in text for f in ("--meshMinComponentTriangles v", "--meshLargestComponent", "--meshRegionIds"))


def vtp_bytes(pts, tris, normals=None, contour=0.0):
    """The file dmi_write_polydata / dmi_write_polydata_with_normals wrote before RegionId existed, built here byte by byte."""
    n, m = len(pts), len(tris)
    pb, cb, ob = 24 * n, 24 * m, 8 * m
    head = ('<?xml version="1.0"?>\n<VTKFile type="PolyData" version="1.0" byte_order="LittleEndian" header_type="UInt64">\n'
            f'  <PolyData>\n    <Piece NumberOfPoints="{n}" NumberOfVerts="0" NumberOfLines="0" NumberOfStrips="0" NumberOfPolys="{m}">\n')
    if normals is not None:
        off = 24 + pb + cb + ob
        head += ('      <PointData Normals="Normals" Scalars="reconstruction_scalar">\n        <DataArray type="Float32" Name="Normals" '
                 f'NumberOfComponents="3" format="appended" offset="{off}"/>\n        <DataArray type="Float64" '
                 f'Name="reconstruction_scalar" format="appended" offset="{off + 8 + 12 * n}"/>\n      </PointData>\n')
    head += ('      <Points>\n        <DataArray type="Float64" Name="Points" NumberOfComponents="3" format="appended" offset="0"/>\n'
             f'      </Points>\n      <Polys>\n        <DataArray type="Int64" Name="connectivity" format="appended" offset="{8 + pb}"/>\n'
             f'        <DataArray type="Int64" Name="offsets" format="appended" offset="{16 + pb + cb}"/>\n      </Polys>\n    </Piece>\n'
             '  </PolyData>\n  <AppendedData encoding="raw">\n   _')
    body = struct.pack("<Q", pb) + pts.tobytes() + struct.pack("<Q", cb) + tris.tobytes() + struct.pack("<Q", ob) + \
        (3 * np.arange(1, m + 1, dtype=np.int64)).tobytes()
    if normals is not None:
        body += struct.pack("<Q", 12 * n) + normals.tobytes() + struct.pack("<Q", 8 * n) + np.full(n, contour).tobytes()
    return head.encode() + body + b"\n  </AppendedData>\n</VTKFile>\n"


def _mesh_for_files(seed=2, n=37, m=51):
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((n, 3))
    tris = rng.integers(0, max(n, 1), size=(m, 3)).astype(np.int64)
    normals = rng.standard_normal((n, 3)).astype(np.float32)
    rid = rng.integers(0, 1 << 40, size=n).astype(np.int64)
    return pts, tris, normals, rid


@pytest.mark.parametrize("n,m", [(37, 51), (0, 0)])
def test_writer_old_entry_points_write_the_bytes_they_always_wrote(tmp_path, n, m):
    pts, tris, normals, rid = _mesh_for_files(n=n, m=m)
    f = str(tmp_path / "m.vtp")
    capi.write_polydata(f, pts, tris)
    assert open(f, "rb").read() == vtp_bytes(pts, tris)
    capi.write_polydata_with_normals(f, pts, tris, normals, 0.25)
    assert open(f, "rb").read() == vtp_bytes(pts, tris, normals, 0.25)
    # the new entry point without region ids writes those very files
    capi.write_polydata_with_arrays(f, pts, tris)
    assert open(f, "rb").read() == vtp_bytes(pts, tris)
    capi.write_polydata_with_arrays(f, pts, tris, normals, 0.25)
    assert open(f, "rb").read() == vtp_bytes(pts, tris, normals, 0.25)


@pytest.mark.parametrize("n,m", [(37, 51), (0, 0)])
def test_writer_region_ids_round_trip_through_the_vtp_reader(tmp_path, n, m):
    pts, tris, normals, rid = _mesh_for_files(n=n, m=m)
    f = str(tmp_path / "m.vtp")
    capi.write_polydata_with_arrays(f, pts, tris, region_ids=rid)
    pd = capi.read_polydata(f)                       # the reader behind dmi_coloration
    assert pd.points.tobytes() == pts.tobytes() and pd.connectivity.tobytes() == tris.tobytes()
    assert list(pd.point_data) == ["RegionId"] and pd.point_data["RegionId"].dtype == np.int64
    assert np.array_equal(pd.point_data["RegionId"], rid) and pd.point_designations == [("Scalars", "RegionId")]
    raw = open(f, "rb").read()
    plain = vtp_bytes(pts, tris)
    cut = plain.index(b"      <Points>")
    assert raw[:cut] == plain[:cut] and raw.endswith(struct.pack("<Q", 8 * n) + rid.tobytes() + b"\n  </AppendedData>\n</VTKFile>\n")
    capi.write_polydata_with_arrays(f, pts, tris, normals, 0.5, rid)
    pd = capi.read_polydata(f)
    assert list(pd.point_data) == ["Normals", "reconstruction_scalar", "RegionId"]
    assert pd.point_data["Normals"].tobytes() == normals.tobytes() and np.all(pd.point_data["reconstruction_scalar"] == 0.5)
    assert np.array_equal(pd.point_data["RegionId"], rid) and len(pd.point_data["reconstruction_scalar"]) == n
    assert pd.point_designations == [("Normals", "Normals"), ("Scalars", "reconstruction_scalar")]
    assert pd.points.tobytes() == pts.tobytes() and pd.connectivity.tobytes() == tris.tobytes()
    L = capi.load_host()
    assert L.dmi_write_polydata_with_arrays(os.fsencode(str(tmp_path / "x.vtp")), None, -1, None, 0, None, 1.0, None) == 0
    assert L.dmi_write_polydata_with_arrays(os.fsencode(str(tmp_path / "no_such_dir" / "x.vtp")), None, 0, None, 0, None, 1.0, None) == 0


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
def _extract(ctx, iso, normals):
    if normals:
        v, t, n = ctx.extract_isosurface_with_normals(iso)
        return {"vertices": v, "triangles": t, "normals": n}
    v, t = ctx.extract_isosurface(iso)
    return {"vertices": v, "triangles": t, "normals": None}


def _run_steps(ctx, iso, normals, steps, want_of=None):
    """One extraction and the filters `steps` on the GPU: every count and array after every step against the restatement applied
    to the GPU's own unfiltered mesh (when want_of is given: a cache of restatement results), and all the bytes for the rerun."""
    mesh = _extract(ctx, iso, normals)
    got_bytes = []
    for i, (mode, n) in enumerate(steps):
        counts = ctx.filter_isosurface_components(mode, n)
        gv, gt = ctx.download_isosurface()
        rid, rsz = ctx.download_isosurface_regions()
        gn = ctx.download_isosurface_normals() if normals else None
        got_bytes.append((counts, gv.tobytes(), gt.tobytes(), rid.tobytes(), rsz.tobytes(), None if gn is None else gn.tobytes()))
        if want_of is None:
            continue
        key = (iso, normals, tuple(steps[:i + 1]))
        if key not in want_of:
            want_of[key] = C.filter_mesh(mesh["vertices"], mesh["triangles"], mesh["normals"], mode, n)
        mesh = want_of[key]
        assert counts == mesh["counts"], (steps, i, counts, mesh["counts"])
        assert gv.shape == mesh["vertices"].shape and gv.tobytes() == mesh["vertices"].tobytes(), (steps, i)
        assert gt.shape == mesh["triangles"].shape and np.array_equal(gt, mesh["triangles"]), (steps, i)
        assert np.array_equal(rid, mesh["region_id"]) and np.array_equal(rsz, mesh["region_size"]), (steps, i)
        if normals:
            assert gn.shape == mesh["normals"].shape and gn.tobytes() == mesh["normals"].tobytes(), (steps, i)
    return got_bytes


def _all_step_lists(ctx, iso, normals):
    """The issue's list for one surface: MIN(0), MIN(1), MIN at the median size, MIN(T + 1), LARGEST, MIN then LARGEST, and the
    same call twice -- each after a fresh extraction, each run twice with the same bytes."""
    mesh = _extract(ctx, iso, False)
    lab, size = C.components(len(mesh["vertices"]), mesh["triangles"])
    median = int(np.median(size[size > 0])) if len(mesh["triangles"]) else 1
    t1 = len(mesh["triangles"]) + 1
    lists = [[(MIN, 0)], [(MIN, 1)], [(MIN, median)], [(MIN, t1)], [(LARGEST, 0)], [(MIN, median), (LARGEST, 0)],
             [(LARGEST, 0), (LARGEST, 0)], [(MIN, median), (MIN, median)], [(MIN, 0), (MIN, 0)]]
    cache = {}
    for steps in lists:
        first = _run_steps(ctx, iso, normals, steps, cache)
        second = _run_steps(ctx, iso, normals, steps)
        assert first == second, steps
        if len(steps) == 2 and steps[0] == steps[1]:              # idempotent: the second call changes nothing
            assert first[0][1:] == first[1][1:] and first[1][0][:2] == first[0][0][:2], steps
    # a fresh extraction after a filter is the full mesh again, bit for bit
    again = _extract(ctx, iso, False)
    assert again["vertices"].tobytes() == mesh["vertices"].tobytes() and np.array_equal(again["triangles"], mesh["triangles"])
    return len(mesh["triangles"])


def _cells(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.5, 2.5, size=shape)


@pytest.mark.gpu
@pytest.mark.parametrize("cells,rotated", [((1, 1, 1), False), ((70, 33, 17), True), ((130, 5, 40), False), ((64, 64, 64), False)])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("normals", [False, True])
def test_gpu_components_random_field(cells, rotated, dtype, normals):
    grid = scene.default_grid(cells, rotated=rotated)
    nx, ny, nz = cells
    c = _cells((nz, ny, nx), seed=nx + 7 * ny + 3 * nz)
    if dtype == "f32":
        c = c.astype(np.float32).astype(np.float64)
    with capi.FusionContext(grid, scene.default_ray_potential(grid), grid_dtype=dtype) as ctx:
        ctx.upload_grid(c)
        for iso in (1.0, 0.0, 0.37):
            _all_step_lists(ctx, iso, normals)


def _cell_field(point_field):
    """A cell grid whose point data (the mean of the 8 cells around a point) has the sign structure of the given shape: the
    shape's field sampled at the cell centres."""
    return 0.125 * sum(point_field[dz:point_field.shape[0] - 1 + dz, dy:point_field.shape[1] - 1 + dy, dx:point_field.shape[2] - 1 + dx]
                       for dz in (0, 1) for dy in (0, 1) for dx in (0, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["three_spheres", "winding_tube", "eight_tubes", "nan_and_lattice_iso"])
@pytest.mark.parametrize("normals", [False, True])
def test_gpu_components_known_shapes(shape, normals):
    iso = 0.0
    if shape == "three_spheres":
        c, want_components = _cell_field(three_spheres_field()), 3
    elif shape == "winding_tube":
        c, want_components = _cell_field(winding_tube_field(100, 72, 48)), 1
    elif shape == "eight_tubes":
        c, want_components = _cell_field(eight_tubes_field()), 8
    else:
        c = np.round(_cells((19, 23, 40), seed=9) * 2) / 2        # values on a 0.5 lattice: iso 1.0 hits point values exactly
        c[3:6, 4:9, 10:20] = np.nan
        c[0, 0, 0] = np.nan
        iso, want_components = 1.0, None
    nz, ny, nx = c.shape
    grid = scene.default_grid((nx, ny, nz), rotated=shape != "eight_tubes")
    with capi.FusionContext(grid, scene.default_ray_potential(grid)) as ctx:
        ctx.upload_grid(c)
        assert _all_step_lists(ctx, iso, normals) > 100
        v, t = ctx.extract_isosurface(iso)
        counts = ctx.filter_isosurface_components(MIN, 0)
        if want_components is not None:
            assert counts == (len(v), len(t), want_components, want_components)
        else:
            tri_pts = v[t]
            assert (np.all(tri_pts[:, 0] == tri_pts[:, 1], axis=1) | np.all(tri_pts[:, 1] == tri_pts[:, 2], axis=1)).any()
        if shape == "eight_tubes":                                 # a tie: the component of vertex 0 stays
            rid, rsz = ctx.download_isosurface_regions()
            assert len(set(rsz.tolist())) == 1
            assert ctx.filter_isosurface_components(LARGEST)[:2] == (int((rid == 0).sum()), int(rsz[0]))
            assert ctx.download_isosurface()[0].tobytes() == v[rid == 0].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("iso", [1.0, 0.0])
def test_gpu_components_of_a_fused_scene(iso):
    grid = scene.default_grid((48, 40, 36))
    ray = scene.default_ray_potential(grid)
    views = scene.make_views(5, 96, 72, seed=11, dense=True)
    with capi.FusionContext(grid, ray) as ctx:
        ctx.add_views(views)
        ctx.fuse()
        assert _all_step_lists(ctx, iso, True) > 100


@pytest.mark.gpu
def test_gpu_components_life_cycle_and_errors():
    grid = scene.default_grid((30, 20, 10))
    ray = scene.default_ray_potential(grid)
    lib = capi.load()
    u64 = ctypes.c_uint64
    a, b, c, d = u64(7), u64(7), u64(7), u64(7)
    refs = [ctypes.byref(x) for x in (a, b, c, d)]
    i64p = ctypes.POINTER(ctypes.c_int64)
    rid = np.zeros(16, dtype=np.int64)
    with capi.FusionContext(grid, ray) as ctx:
        # before any extraction
        assert lib.dmi_filter_isosurface_components(ctx._h, 0, 0, *refs) == INVALID_ARGUMENT
        assert "no mesh" in lib.dmi_last_error(ctx._h).decode()
        assert lib.dmi_download_isosurface_regions(ctx._h, rid.ctypes.data_as(i64p), None) == INVALID_ARGUMENT
        ctx.upload_grid(_cells((10, 20, 30), seed=3))
        v0, t0 = ctx.extract_isosurface(1.0)
        assert len(t0) > 0
        # a region download before any filter; null pointers; a bad mode
        assert lib.dmi_download_isosurface_regions(ctx._h, rid.ctypes.data_as(i64p), None) == INVALID_ARGUMENT
        assert "no regions" in lib.dmi_last_error(ctx._h).decode()
        for k in range(4):
            args = list(refs)
            args[k] = None
            assert lib.dmi_filter_isosurface_components(ctx._h, 0, 0, *args) == INVALID_ARGUMENT
        for mode in (2, -1, 77):
            assert lib.dmi_filter_isosurface_components(ctx._h, mode, 0, *refs) == INVALID_ARGUMENT
            assert "unknown mode" in lib.dmi_last_error(ctx._h).decode()
        assert lib.dmi_get_isosurface_filter_kernel_ms(ctx._h, None) == INVALID_ARGUMENT
        assert lib.dmi_get_isosurface_filter_pass_ms(ctx._h, None) == INVALID_ARGUMENT
        # none of the refused calls touched the mesh
        v, t = ctx.download_isosurface()
        assert v.tobytes() == v0.tobytes() and np.array_equal(t, t0)
        want = C.filter_mesh(v0, t0, None, LARGEST)
        assert ctx.filter_isosurface_components(LARGEST) == want["counts"]
        assert lib.dmi_download_isosurface_regions(ctx._h, None, None) == 0          # neither array wanted
        passes = ctx.isosurface_filter_pass_ms()
        assert ctx.isosurface_filter_kernel_ms() > 0.0 and all(p >= 0.0 for p in passes.values())
        with pytest.raises(capi.DmiError):                                              # the extraction had no normals
            ctx.download_isosurface_normals()
        # the next extraction replaces the filtered mesh, and the regions go with it
        v, t = ctx.extract_isosurface(1.0)
        assert v.tobytes() == v0.tobytes() and np.array_equal(t, t0)
        assert lib.dmi_download_isosurface_regions(ctx._h, rid.ctypes.data_as(i64p), None) == INVALID_ARGUMENT
        # an empty surface: a success, and so is its filter in both modes
        ctx.reset_grid()
        v, t = ctx.extract_isosurface(1.0)
        assert v.shape == (0, 3) and t.shape == (0, 3)
        assert ctx.filter_isosurface_components(MIN, 5) == (0, 0, 0, 0)
        assert ctx.filter_isosurface_components(LARGEST) == (0, 0, 0, 0)
        r, s = ctx.download_isosurface_regions()
        assert r.shape == (0,) and s.shape == (0,)
        # after reset_grid + a fusion + an extraction the filter sees the new mesh
        views = scene.make_views(3, 64, 48, seed=2, dense=True)
        ctx.add_views(views)
        ctx.fuse()
        v1, t1, n1 = ctx.extract_isosurface_with_normals(1.0)
        want = C.filter_mesh(v1, t1, n1, LARGEST)
        assert len(t1) > 0 and ctx.filter_isosurface_components(LARGEST) == want["counts"]
        assert ctx.download_isosurface()[0].tobytes() == want["vertices"].tobytes()
        assert ctx.download_isosurface_normals().tobytes() == want["normals"].tobytes()


@pytest.mark.gpu
def test_gpu_components_full_size_cfg3_speckle():
    """512^3, the first 32 views of the speckle scene of bench.py --full's cfg 3 (the set-up of
    test_gpu_mesh_full_size_cfg3_speckle), MIN(0) and LARGEST: the WHOLE filtered mesh -- vertices, normals, triangles, RegionId,
    RegionSize and the counts -- equals the restatement applied to the GPU's unfiltered download.  Size used: the full 512^3
    (4.34 M vertices, 8.62 M triangles, 15 264 components); the restatement takes 1.0-1.2 s per filter on 16 CPUs (printed)."""
    grid = scene.default_grid(512)
    ray = scene.default_ray_potential(grid)
    views, thr = scene.make_scene_views("speckle", 256, 1280, 720, seed=1000, view_range=(0, 32), noise_sigma=float(max(grid.spacing)))
    with capi.FusionContext(grid, ray) as ctx:
        ctx.add_views(views, threshold=thr)
        ctx.fuse()
        v, t, n = ctx.extract_isosurface_with_normals(1.0)
        assert len(t) > 1000
        for mode in (MIN, LARGEST):
            t0 = time.perf_counter()
            want = C.filter_mesh(v, t, n, mode, 0)
            dt = time.perf_counter() - t0
            runs = []
            for _ in range(2):
                if runs:
                    ctx.extract_isosurface_with_normals(1.0)
                counts = ctx.filter_isosurface_components(mode, 0)
                gv, gt = ctx.download_isosurface()
                rid, rsz = ctx.download_isosurface_regions()
                runs.append((counts, gv.tobytes(), gt.tobytes(), ctx.download_isosurface_normals().tobytes(), rid.tobytes(), rsz.tobytes()))
            print(f"full size {mode}: {len(v)} vertices, {len(t)} triangles -> counts {counts}; restatement {dt:.1f} s; "
                  f"GPU filter {ctx.isosurface_filter_kernel_ms():.3f} ms {ctx.isosurface_filter_pass_ms()}")
            assert runs[0] == runs[1]
            assert counts == want["counts"]
            assert runs[0][1] == want["vertices"].tobytes() and runs[0][2] == want["triangles"].tobytes()
            assert runs[0][3] == want["normals"].tobytes()
            assert runs[0][4] == want["region_id"].tobytes() and runs[0][5] == want["region_size"].tobytes()


@pytest.mark.gpu
def test_gpu_timing_tool_components_record():
    """tools/gpu_isosurface_time.py --components: its record of a small fused scene is complete and agrees with the restatement."""
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
        rec = tool.components_record(ctx, types.SimpleNamespace(iso=1.0, min_triangles=20, repeat=2))
        v, t = ctx.extract_isosurface(1.0)
    lab, size = C.components(len(v), t)
    sizes = size[size > 0]
    assert rec["host_matches_gpu"] and sum(rec["size_histogram"].values()) == len(sizes)
    assert rec["largest_sizes"][0] == sizes.max()
    assert rec["min0"]["counts"] == {"vertices": len(v), "triangles": len(t), "components": len(sizes), "components_kept": len(sizes)}
    assert rec["mid"]["counts"]["components_kept"] == int((sizes >= 20).sum()) and rec["largest"]["counts"]["triangles"] == sizes.max()
    for k in ("min0", "mid", "largest"):
        assert len(rec[k]["kernel_ms"]) == 2 and rec[k]["kernel_ms_min"] > 0 and rec[k]["over_extraction"] > 0
        assert set(rec[k]["pass_ms"][0]) == {"labels", "sizes", "scans", "compaction"} and all(c >= 0 for c in rec[k]["cas_retries"])
    assert rec["floor_bytes"] == 72 * len(t) + 96 * len(v)


def read_vtp_arrays(path):
    pd = capi.read_polydata(path)
    return pd.points, pd.connectivity.reshape(-1, 3), pd.point_data


@pytest.mark.gpu
def test_gpu_cli_components_end_to_end(tmp_path):
    """dmi_reconstruction --extractMesh --meshNormals --meshLargestComponent --meshRegionIds: mesh.vtp's arrays are the
    restatement applied to the oracle's fused grid, the summary names the component counts, and dmi_coloration colours the file."""
    from oracle import oracle
    from helpers import bits_equal, oracle_params_from_scene
    grid = scene.default_grid((24, 20, 16), rotated=True)
    rp = scene.default_ray_potential(grid)
    views = scene.make_views(5, 48, 36, seed=4, dense=True, with_best_cost=True)
    colors = scene.make_colors(5, 48, 36, seed=5)
    data = tmp_path / "data"
    data.mkdir()
    lv, lk = scene.write_view_files(str(data), views, colors)
    gm = np.asarray(grid.grid_matrix).reshape(4, 4)
    end = [grid.origin[a] + (grid.cell_dims[a] + 1) * grid.spacing[a] for a in range(3)]
    args = [capi.cli_binary(), "--dataFolder", str(data), "--depthMapFile", os.path.basename(lv), "--KRTFile", os.path.basename(lk),
            "--gridDims"] + [str(c + 1) for c in grid.cell_dims] + ["--gridOrigin"] + [repr(float(v)) for v in grid.origin] + \
           ["--gridEnd"] + [repr(float(v)) for v in end] + ["--gridVecX"] + [repr(float(v)) for v in gm[0, :3]] + \
           ["--gridVecY"] + [repr(float(v)) for v in gm[1, :3]] + ["--gridVecZ"] + [repr(float(v)) for v in gm[2, :3]] + \
           ["--rayThick", repr(rp.thickness), "--rayRho", repr(rp.rho), "--rayEta", repr(rp.eta), "--rayDelta", repr(rp.delta),
            "--threshBestCost", "0.7", "--contour", "0.25", "--outputGridFilename", str(tmp_path / "volume.vts"),
            "--outputMeshFilename", str(tmp_path / "mesh.vtp"), "--summary", "--extractMesh", "--meshNormals"]
    o, _ = capi.cli_read_arguments(args)
    g2 = scene.GridDesc(tuple(int(d) - 1 for d in o.grid_dims), tuple(o.grid_origin), tuple(o.grid_spacing), np.array(o.grid_matrix).reshape(4, 4))
    d = oracle.apply_depth_threshold(views.depth, views.best_cost, 0.7).reshape(views.depth.shape)
    fused, _, _ = oracle.fuse(oracle_params_from_scene(g2, rp, views), d, views.K4, views.RT4, n_threads=oracle.max_threads())
    pts = oracle.cell_to_point(fused)
    wv, wt, wn = RN.extract_with_normals(pts, 0.25, o.grid_origin, o.grid_spacing, np.array(o.grid_matrix).reshape(4, 4))
    lab, size = C.components(len(wv), wt)
    n_mid = int(np.median(size[size > 0])) + 1

    def run(flags):
        r = subprocess.run(args + flags, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr + r.stdout
        return r.stdout + r.stderr, open(data / "summary.txt").read()

    def check(want, found, text, summary, region_ids):
        v, t, arrays = read_vtp_arrays(str(tmp_path / "mesh.vtp"))
        assert v.shape == want["vertices"].shape and bits_equal(v, want["vertices"]) and np.array_equal(t, want["triangles"])
        assert bits_equal(arrays["Normals"], want["normals"]) and np.all(arrays["reconstruction_scalar"] == 0.25)
        assert list(arrays) == ["Normals", "reconstruction_scalar"] + (["RegionId"] if region_ids else [])
        if region_ids:
            assert arrays["RegionId"].dtype == np.int64 and np.array_equal(arrays["RegionId"], want["region_id"])
        nv, nt, _, kept = want["counts"]
        assert f"mesh vertices  {nv}\n" in summary and f"mesh triangles  {nt}\n" in summary
        assert f"mesh components found  {found}\n" in summary and f"mesh components kept  {kept}\n" in summary
        assert f"mesh vertices before the component filter  {len(wv)}\n" in summary
        assert f"mesh triangles before the component filter  {len(wt)}\n" in summary
        assert f"mesh components: {found} found, {kept} kept; {len(wv)} vertices, {len(wt)} triangles before, {nv} vertices, {nt} triangles after" in text

    all_kept = C.filter_mesh(wv, wt, wn, MIN, 0)
    found = all_kept["counts"][2]
    assert found >= 1 and len(wt) > 0
    big = C.filter_mesh(wv, wt, wn, LARGEST)
    text, summary = run(["--meshLargestComponent", "--meshRegionIds"])
    check(big, found, text, summary, True)
    # the file goes through dmi_coloration, RegionId carried along
    out = str(tmp_path / "colored.vtp")
    r = subprocess.run([capi.coloration_cli_binary(), "--input", str(tmp_path / "mesh.vtp"), "--output", out, "--krtd", lk, "--vti", lv],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    col = capi.read_polydata(out)
    assert np.array_equal(col.point_data["RegionId"], big["region_id"]) and col.points.tobytes() == big["vertices"].tobytes()
    want_col = oracle.color_mesh(col.points, colors, views.K4, views.RT4)
    for name, w in zip(("MeanColoration", "MedianColoration", "NbProjectedDepthMap"), want_col):
        assert np.array_equal(col.point_data[name], w), name
    # labels only; by size; by size, then the largest
    text, summary = run(["--meshRegionIds"])
    check(all_kept, found, text, summary, True)
    mid = C.filter_mesh(wv, wt, wn, MIN, n_mid)
    text, summary = run(["--meshMinComponentTriangles", str(n_mid)])
    check(mid, found, text, summary, False)
    both = C.filter_mesh(mid["vertices"], mid["triangles"], mid["normals"], LARGEST)
    text, summary = run(["--meshMinComponentTriangles", str(n_mid), "--meshLargestComponent", "--meshRegionIds"])
    check(both, found, text, summary, True)
    # without a component flag nothing about components is said
    text, summary = run([])
    assert "mesh components" not in summary and "component filter" not in summary and "mesh components" not in text
