"""dmi_decimate_isosurface_placed with DMI_DECIMATE_QUADRIC: the CPU restatement
(tests/isosurface_decimate_quadric_np.py) on hand-made meshes and on a box and a sphere, the ABI and the CLI flag on the CPU; on
the GPU every bit of the decimated vertices, triangles and normals against the restatement applied to the GPU's own download, the
old entry against the new one, the life cycle, the composition with the other mesh stages and the command line."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import coloration_depth_np as CD
import isosurface_components_np as C
import isosurface_decimate_np as D
import isosurface_decimate_quadric_np as Q
import isosurface_np as R
import isosurface_smooth_np as S
import test_isosurface_decimate as T
import vti_writer
from cudadepthmapintegration_amd import capi, scene

ROOT = T.ROOT
INVALID_ARGUMENT = T.INVALID_ARGUMENT
_i64, _same_bits = T._i64, T._same_bits


def _reps(p, tris, h, details=None):
    """Every cluster's quadric representative and mean (whether a triangle survives in it or not)."""
    p = np.asarray(p, dtype=np.float64)
    cluster, count = D.clusters(p, h)
    return Q.representatives(p, _i64(tris), cluster, count, h, details), D.representatives(p, cluster, count), cluster


# ---- the restatement on hand-made meshes -------------------------------------------------------------------------------------------
def test_flat_patch_isolated_vertices_and_zero_area_triangles_give_the_mean():
    p = np.array([[0.0, 0, 1], [1, 0, 1], [0, 1, 1], [1, 1, 1],                    # a flat patch in cell (0, 0, 0), z = 1
                  [10, 10, 10], [10.5, 10, 10.25],                                # two isolated vertices in one cell
                  [20, 20, 20], [20.5, 20, 20], [21, 20, 20], [20.25, 20, 20]])   # collinear: triangles of no area
    tris = [[0, 1, 2], [1, 3, 2], [6, 7, 8], [6, 9, 8]]
    details = {}
    reps, mean, cluster = _reps(p, tris, 4.0, details)
    assert cluster.tolist() == [0, 0, 0, 0, 1, 1, 2, 2, 2, 2] and details["corners"].tolist() == [6, 0, 6]
    assert details["solved"].tolist() == [True, False, False]
    assert np.array_equal(details["y"][0] - mean[0], [0.0, 0.0, 0.0])             # d = 0: x = +-0
    assert _same_bits(reps, mean)
    assert np.array_equal(mean, [[0.5, 0.5, 1], [10.25, 10, 10.125], [20.4375, 20, 20]])
    # through decimate: the patch with a skirt to two other cells survives as its mean
    p2 = np.vstack([p[:4], [[6.0, 0, 1], [0, 6, 1]]])
    v, t, _ = Q.decimate(p2, _i64([[0, 1, 2], [1, 3, 2], [1, 4, 5]]), 4.0)
    assert _same_bits(v, D.decimate(p2, _i64([[0, 1, 2], [1, 3, 2], [1, 4, 5]]), 4.0)[0]) and len(t) == 1


def test_three_orthogonal_planes_meet_at_their_apex():
    # planes x = 1, y = 1, z = 1, a triangle of area 1/2 in each, none touching the apex (1, 1, 1); an isolated vertex at the
    # origin sets the bounds and counts in the mean.  A = 3 I (every triangle thrice), tr = 9: lambda_min = tr / 3, the bias of
    # (A + mu I)^-1 A is mu / (lambda_min + mu) < 3 * 2^-10
    p = np.array([[0.0, 0, 0], [1, 2, 2], [1, 3, 2], [1, 2, 3], [2, 1, 2], [3, 1, 2], [2, 1, 3], [2, 2, 1], [3, 2, 1], [2, 3, 1]])
    tris = [[1, 2, 3], [4, 6, 5], [7, 8, 9]]
    details = {}
    reps, mean, cluster = _reps(p, tris, 4.0, details)
    assert len(reps) == 1 and details["solved"].all() and not details["clamped"].any()
    apex = np.array([1.0, 1.0, 1.0])
    off = float(np.linalg.norm(apex - mean[0]))
    assert off > 1.0
    assert np.linalg.norm(reps[0] - apex) <= 3 * 2.0 ** -10 * off + 16 * np.finfo(np.float64).eps
    assert np.linalg.norm(reps[0] - apex) < np.linalg.norm(mean[0] - apex) / 300


def test_the_corner_sums_are_made_left_to_right_in_ascending_corner_index():
    # u = (0, 0, 1), v = (a, b, 0): n = (-b, a, 0) and n0 n1 = -a b.  Three triangles in one cell with n0 n1 = 1e16, 1, -1e16
    p = np.array([[0.0, 0, 0], [0, 0, 1], [1e8, -1e8, 0], [1, -1, 0], [1e8, 1e8, 0]])
    tris = _i64([[0, 1, 2], [0, 1, 3], [0, 1, 4]])
    big = 1e16
    assert (((big + big) + big) + 1.0) + 1.0 == 3e16 and 3e16 + 3.0 != 3e16      # another order differs
    cluster, count = D.clusters(p, 1e9)
    assert count == 1
    mean = D.representatives(p, cluster, count)
    A, g, corners = Q.corner_sums(p, tris, cluster, count, mean)
    assert corners.tolist() == [9] and A[0, 1] == 0.0                             # 3e16 + 1 + 1 + 1 - 3e16
    A2, _, _ = Q.corner_sums(p, tris[[0, 2, 1]], cluster, count, mean)            # triangles in another order: another sum
    assert A2[0, 1] == 3.0
    assert A[0, 0] == A2[0, 0] == 3e16 + 3e16 and A[0, 5] == 0.0
    # and g: the corners of one triangle are consecutive, the triangles ascend
    n = np.array([[1e8, 1e8, 0], [1, 1, 0], [-1e8, 1e8, 0]])
    d = -((n[:, 0] * (0 - mean[0, 0]) + n[:, 1] * (0 - mean[0, 1])) + n[:, 2] * (0 - mean[0, 2]))
    want = n[0] * d[0]
    for k in (0, 0, 1, 1, 1, 2, 2, 2):
        want = want + n[k] * d[k]
    assert np.array_equal(g[0], want) and g[0, 0] != 0.0 and g[0, 1] != 0.0


# ---- a box and a sphere --------------------------------------------------------------------------------------------------------------
BOX_CENTRE, BOX_HALF = np.array([12.3, 11.8, 12.1]), np.array([7.4, 6.3, 5.6])


def box_field(n=24):
    x, y, z = T._lattice(n, n, n)
    return -np.maximum(np.maximum(np.abs(x - 12.3) - 7.4, np.abs(y - 11.8) - 6.3), np.abs(z - 12.1) - 5.6)


def box_distance(p, shift=0.0):
    """The distance of every point to the surface of the box."""
    q = np.abs(p - (BOX_CENTRE + shift)) - BOX_HALF
    return np.abs(np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(axis=1), 0.0))


def rms(x):
    return float(np.sqrt(np.mean(np.square(x))))


@pytest.fixture(scope="module")
def box_mesh():
    v0, t0 = R.extract(box_field(), 0.0)                                          # unit spacing
    assert len(t0) > 1000 and T.signed_volume(v0, t0) > 0.0
    v0.setflags(write=False)
    t0.setflags(write=False)
    return v0, t0


@pytest.mark.parametrize("h", [3.0, 4.0])
def test_box_keeps_its_edges_and_corners(box_mesh, h):
    v0, t0 = box_mesh
    mv, mt, _ = D.decimate(v0, t0, h)
    details = {}
    v, t, n = Q.decimate(v0, t0, h, np.zeros((len(v0), 3), np.float32), details=details)
    assert _same_bits(t, mt) and len(v) == len(mv) and n.shape == (len(v), 3) and n.dtype == np.float32
    T.assert_clean(v, t)
    assert T.signed_volume(v, t) > 0.0
    assert (v >= details["lower"]).all() and (v <= details["upper"]).all()
    mean_rms, quadric_rms = rms(box_distance(mv)), rms(box_distance(v))
    print(f"box, cell size {h}: rms distance to the box {mean_rms:.4f} (mean) -> {quadric_rms:.4f} (quadric), "
          f"{int(details['solved'].sum())} of {len(v)} solved, {int(details['clamped'].sum())} clamped")
    assert quadric_rms <= mean_rms / 4
    assert T.signed_volume(v, t) > T.signed_volume(mv, mt)                        # the mean shrinks a convex shape


def test_a_box_rotated_about_two_axes_is_closer_too():
    """The box at 0.85 of its size (it stays inside the lattice), turned by 0.5 rad about z and then 0.3 rad about x: no face is
    parallel to the cells.  The figures are printed; asserted is that the quadric placement is the closer one."""
    ca, sa, cb, sb = np.cos(0.5), np.sin(0.5), np.cos(0.3), np.sin(0.3)
    M = np.array([[1, 0, 0], [0, cb, -sb], [0, sb, cb]]) @ np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1]])
    half = 0.85 * BOX_HALF
    x, y, z = T._lattice(24, 24, 24)
    local = (np.stack([x, y, z], axis=-1) - BOX_CENTRE) @ M.T
    v0, t0 = R.extract(-np.max(np.abs(local) - half, axis=-1), 0.0)
    assert len(t0) > 1000 and T.signed_volume(v0, t0) > 0.0

    def distance(p):
        q = np.abs((p - BOX_CENTRE) @ M.T) - half
        return np.abs(np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(axis=1), 0.0))

    for h in (3.0, 4.0):
        mv, mt, _ = D.decimate(v0, t0, h)
        v, t, _ = Q.decimate(v0, t0, h)
        assert _same_bits(t, mt) and len(v) == len(mv)
        T.assert_clean(v, t)
        a, b = rms(distance(mv)), rms(distance(v))
        print(f"rotated box, cell size {h}: rms distance to the box {a:.4f} (mean) -> {b:.4f} (quadric)")
        assert b < a


def test_the_clamp_is_taken_and_holds(box_mesh):
    v0, t0 = box_mesh
    details = {}
    v, t, _ = Q.decimate(v0, t0, 1.5, details=details)
    assert details["clamped"].sum() >= 1
    assert (v >= details["lower"]).all() and (v <= details["upper"]).all()
    y = details["y"][details["clamped"]]
    assert ((y < details["lower"][details["clamped"]]) | (y > details["upper"][details["clamped"]])).any(axis=1).all()


def test_sphere_is_no_further_from_its_radius():
    v0, t0 = R.extract(T.sphere_field(), 0.0)
    centre = np.array([12.3, 11.8, 12.1])
    for h in (3.0, 4.0):
        mv, mt, _ = D.decimate(v0, t0, h)
        v, t, _ = Q.decimate(v0, t0, h)
        assert _same_bits(t, mt) and len(v) == len(mv)
        T.assert_clean(v, t)
        a, b = rms(np.linalg.norm(mv - centre, axis=1) - 8.4), rms(np.linalg.norm(v - centre, axis=1) - 8.4)
        print(f"sphere, cell size {h}: rms radial error {a:.4f} (mean) -> {b:.4f} (quadric)")
        assert b <= a


def test_a_shift_of_five_million_loses_nothing(box_mesh):
    v0, t0 = box_mesh
    v, t, _ = Q.decimate(v0, t0, 3.0)
    w, u, _ = Q.decimate(v0 + 5e6, t0, 3.0)
    assert _same_bits(u, t) and len(w) == len(v)
    assert np.abs((w - 5e6) - v).max() <= 1e-6
    assert rms(box_distance(w, 5e6)) <= rms(box_distance(D.decimate(v0 + 5e6, t0, 3.0)[0], 5e6)) / 4


def test_refusals():
    p = np.array([[0.0, 0, 0], [2097151.0, 1, 0], [5, 5, 5]])
    tri = _i64([[0, 1, 2]])
    Q.decimate(p, tri, 1.0)                                                       # 2^21 bins: accepted
    with pytest.raises(ValueError, match="2\\^21"):
        Q.decimate(p + [[0, 0, 0], [1, 0, 0], [0, 0, 0]], tri, 1.0)
    for bad in (np.inf, -np.inf, np.nan):
        q = p.copy()
        q[2, 1] = bad
        with pytest.raises(ValueError, match="non-finite"):
            Q.decimate(q, tri, 10.0)
    for h in (0.0, -1.0, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="cell_size"):
            Q.decimate(p, tri, h)
        with pytest.raises(ValueError, match="cell_size"):
            Q.decimate(np.zeros((0, 3)), np.zeros((0, 3), np.int64), h)
    for placement in (-1, 2, 7):
        with pytest.raises(ValueError, match="placement"):
            Q.decimate(p, tri, 10.0, placement=placement)
    # 3 T >= 2^32 (a view of one triangle, no memory behind it): refused for the quadric placement only
    many = np.broadcast_to(np.zeros((1, 3), np.int64), ((1 << 32) // 3 + 1, 3))
    with pytest.raises(ValueError, match="3 T >= 2\\^32"):
        Q.decimate(p, many, 10.0)
    assert _same_bits(Q.decimate(p, tri, 2.0, placement=Q.MEAN)[0], D.decimate(p, tri, 2.0)[0])
    assert Q.decimate(np.zeros((0, 3)), np.zeros((0, 3), np.int64), 1.0)[0].shape == (0, 3)


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------
def test_abi_python_and_cli_know_the_placement():
    header = open(os.path.join(ROOT, "include", "dmi.h")).read()
    lib = ctypes.CDLL(capi.load()._name)
    assert "int dmi_decimate_isosurface_placed(dmi_context *ctx, double cell_size, int32_t placement," in header
    assert "#define DMI_DECIMATE_MEAN 0\n" in header and "#define DMI_DECIMATE_QUADRIC 1\n" in header
    assert "dmi_decimate_isosurface_placed" in capi.ABI_SYMBOLS and hasattr(lib, "dmi_decimate_isosurface_placed")
    assert (capi.DMI_DECIMATE_MEAN, capi.DMI_DECIMATE_QUADRIC) == (Q.MEAN, Q.QUADRIC) == (0, 1)
    assert lib.dmi_abi_version() == 5
    n = ctypes.c_uint64(0)
    assert capi.load().dmi_decimate_isosurface_placed(None, 1.0, 1, ctypes.byref(n), ctypes.byref(n)) == INVALID_ARGUMENT
    assert "dmi_decimate_isosurface_placed" in capi.load().dmi_last_error(None).decode()
    # an unknown placement is a ValueError before any call (nothing of the context is touched)
    with pytest.raises(ValueError, match="placement"):
        capi.FusionContext.decimate_isosurface(object(), 1.0, "median")
    with pytest.raises(ValueError, match="placement"):
        capi.FusionContext.decimate_isosurface(object(), 1.0, placement=1)
    o, text = capi.cli_read_arguments(T.BASE + ["--extractMesh", "--meshDecimateCellSize", "0.5"])
    assert o is not None and o.mesh_decimate_quadric == 0 and o.mesh_decimate_cell_size == 0.5, text
    o, text = capi.cli_read_arguments(T.BASE + ["--extractMesh", "--meshDecimateCellSize", "0.5", "--meshDecimateQuadric"])
    assert o is not None and o.mesh_decimate_quadric == 1 and o.mesh_decimate_cell_size == 0.5, text
    assert o.mesh_coloration_depth_from_mesh == 0 and o.mesh_coloration == 0
    o, text = capi.cli_read_arguments(T.BASE + ["--extractMesh", "--meshDecimateQuadric"])
    assert o is None and text.split("\n")[0].startswith("Error : --meshDecimateQuadric needs --meshDecimateCellSize"), text
    assert "--meshDecimateCellSize v" in text                                     # the help text follows
    o, text = capi.cli_read_arguments(T.BASE + ["--help"])
    assert o is None and "--meshDecimateQuadric" in text
    assert "not in the reference" in text.split("--meshDecimateQuadric")[1].split("--meshColoration")[0]
    r = subprocess.run([capi.cli_binary()] + T.BASE[1:] + ["--extractMesh", "--meshDecimateQuadric"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--meshDecimateQuadric needs --meshDecimateCellSize" in r.stderr


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _case(name):
    if name == "box":
        return T._cell_field(box_field()), None
    return T._case(name)


def _refused(ctx, cell_size, placement="quadric"):
    with pytest.raises(capi.DmiError) as e:
        ctx.decimate_isosurface(cell_size, placement)
    assert e.value.code == INVALID_ARGUMENT and "dmi_decimate_isosurface_placed" in str(e.value)
    return str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sphere", "torus", "noisy_sphere", "leaves_the_grid", "nan", "sheared", "box"])
@pytest.mark.parametrize("normals", [False, True])
def test_gpu_quadric_decimation_is_the_restatement_bit_for_bit(name, normals):
    cells, matrix = _case(name)
    spacing = min(T._grid(cells, matrix).spacing)
    with T._context(cells, matrix) as ctx:
        v0, t0, n0 = T._extract(ctx, normals)
        assert len(t0) > 500
        moved = 0
        for label, h in T.cell_sizes(v0, spacing).items():
            if label == "refused":
                continue
            v1, t1, n1 = T._extract(ctx, normals)                                  # each size on a fresh extraction
            assert _same_bits(v1, v0) and _same_bits(t1, t0)
            details = {}
            want_v, want_t, want_n = Q.decimate(v0, t0, h, n0, details=details)
            counts = ctx.decimate_isosurface(h, "quadric")
            v, t = ctx.download_isosurface()
            print(f"{name} {label} (h = {h!r}): {len(v0)} -> {len(v)} vertices, {len(t0)} -> {len(t)} triangles, "
                  f"{int(details['clamped'].sum()) if details else 0} clamped, kernels {ctx.isosurface_decimate_pass_ms()}")
            assert counts == (len(v), len(t)) == (len(want_v), len(want_t))
            assert _same_bits(t, want_t), (name, label)
            assert _same_bits(v, want_v), (name, label, int((v.view(np.uint64) != want_v.view(np.uint64)).any(axis=1).sum()))
            if normals:
                assert _same_bits(ctx.download_isosurface_normals(), want_n), (name, label)
            else:
                with pytest.raises(capi.DmiError) as e:
                    ctx.download_isosurface_normals()
                assert e.value.code == INVALID_ARGUMENT
            with pytest.raises(capi.DmiError) as e:                                # no regions until a filter runs again
                ctx.download_isosurface_regions()
            assert e.value.code == INVALID_ARGUMENT and "no regions" in str(e.value)
            mean_v, mean_t, _ = D.decimate(v0, t0, h)
            assert _same_bits(t, mean_t)                                          # only the coordinates change
            if label == "weld":
                # One vertex per distinct position.  Every plane of such a cluster passes through its mean, so d is what the
                # roundings leave of an exact 0: |d| <= 8 eps |n| |q| with a margin of 8 for the cross product's own roundings,
                # |g| <= sum |n| |d|, and |(A + mu I)^-1| <= 1 / mu = 2^10 / sum |n|^2: |x| <= 2^10 * 64 eps * max |q|
                assert len(v) == len(np.unique(v0, axis=0)) and len(np.unique(v, axis=0)) == len(v)
                extent = float((v0.max(axis=0) - v0.min(axis=0)).max())
                assert np.abs(v - mean_v).max() <= 2.0 ** 10 * 64 * np.finfo(np.float64).eps * extent
                assert (np.bincount(D.clusters(v0, h)[0]) == 1).mean() > 0.5      # most clusters have one member
            elif label in ("1.5", "4"):
                assert 0 < len(t) < len(t0)
                moved += int((v != mean_v).any(axis=1).sum())
            elif label == "two_bins":
                assert D.clusters(v0, h)[1] == (4 if name in ("torus", "sheared") else 8) and 0 < len(v) <= 8
                assert details["corners"].max() > 1000                            # a lane walks thousands of corners
            else:
                assert counts == (0, 0)
            if len(v):
                T.assert_clean(v, t)
                assert (v >= details["lower"]).all() and (v <= details["upper"]).all()
        assert moved > 0                                                          # the placement is not the mean's


@pytest.mark.gpu
def test_gpu_mean_through_the_new_entry_is_the_old_entry_and_no_state_leaks():
    cells, _ = _case("noisy_sphere")
    spacing = min(T._grid(cells).spacing)
    h = 2.0 * spacing

    def result(ctx):
        return tuple(a.tobytes() for a in ctx.download_isosurface()) + (ctx.download_isosurface_normals().tobytes(),)

    with T._context(cells) as ctx:
        v0, t0, n0 = ctx.extract_isosurface_with_normals(0.0)
        old_counts = ctx.decimate_isosurface(h)
        old = result(ctx)
        assert old == tuple(a.tobytes() for a in D.decimate(v0, t0, h, n0))
        ctx.extract_isosurface_with_normals(0.0)
        assert ctx.decimate_isosurface(h, "mean") == old_counts and result(ctx) == old   # (the binding's "mean" is the old entry)
        ctx.extract_isosurface_with_normals(0.0)
        n = (ctypes.c_uint64(0), ctypes.c_uint64(0))
        assert capi.load().dmi_decimate_isosurface_placed(ctx._h, h, capi.DMI_DECIMATE_MEAN, ctypes.byref(n[0]), ctypes.byref(n[1])) == 0
        assert (int(n[0].value), int(n[1].value)) == old_counts
        ctx._mesh_counts = old_counts + (0,)                                       # (the binding's own record of the mesh's sizes)
        assert result(ctx) == old
        ctx.extract_isosurface_with_normals(0.0)
        assert ctx.decimate_isosurface(h, "quadric") == old_counts
        quadric = result(ctx)
        assert quadric[1] == old[1] and quadric[0] != old[0]
        assert quadric == tuple(a.tobytes() for a in Q.decimate(v0, t0, h, n0))
        ctx.extract_isosurface_with_normals(0.0)                                   # the old entry after a quadric call
        assert ctx.decimate_isosurface(h) == old_counts and result(ctx) == old
        # without normals too, where the key arrays are sized by the placement alone
        ctx.extract_isosurface(0.0)
        assert ctx.decimate_isosurface(h, "quadric") == old_counts
        assert tuple(a.tobytes() for a in ctx.download_isosurface()) == quadric[:2]
        ctx.extract_isosurface(0.0)
        assert ctx.decimate_isosurface(h) == old_counts
        assert tuple(a.tobytes() for a in ctx.download_isosurface()) == old[:2]


@pytest.mark.gpu
def test_gpu_quadric_decimation_life_cycle_determinism_and_errors():
    cells = T._noisy(T._cell_field(T.sphere_field()), 1.0, 7)
    spacing = min(T._grid(cells).spacing)
    lib = capi.load()
    n = ctypes.c_uint64(0)
    with T._context(cells) as ctx:
        assert lib.dmi_decimate_isosurface_placed(ctx._h, 1.0, 1, ctypes.byref(n), ctypes.byref(n)) == INVALID_ARGUMENT
        assert "no mesh" in lib.dmi_last_error(ctx._h).decode() and "dmi_decimate_isosurface_placed" in lib.dmi_last_error(ctx._h).decode()
        v0, t0, n0 = ctx.extract_isosurface_with_normals(0.0)
        ctx.filter_isosurface_components(C.MIN_TRIANGLES, 0)                      # keeps everything, leaves regions
        rid0, rsz0 = ctx.download_isosurface_regions()
        # refused arguments leave the mesh, its normals and its regions as they were
        for placement in (-1, 2, 1 << 20):
            assert lib.dmi_decimate_isosurface_placed(ctx._h, 4.0 * spacing, placement, ctypes.byref(n), ctypes.byref(n)) == INVALID_ARGUMENT
            text = lib.dmi_last_error(ctx._h).decode()
            assert "dmi_decimate_isosurface_placed" in text and "placement" in text and str(placement) in text
        box = float((v0.max(axis=0) - v0.min(axis=0)).max())
        for h in (0.0, -1.0, float("nan"), float("inf"), float("-inf"), box / 2 ** 22, 1e-9 * spacing, 5e-324):
            text = _refused(ctx, h)
            assert ("2^21" in text) == (h > 0 and h < 1.0), (h, text)
        assert lib.dmi_decimate_isosurface_placed(ctx._h, 1.0, 1, None, ctypes.byref(n)) == INVALID_ARGUMENT
        assert lib.dmi_decimate_isosurface_placed(ctx._h, 1.0, 1, ctypes.byref(n), None) == INVALID_ARGUMENT
        v, t = ctx.download_isosurface()
        rid, rsz = ctx.download_isosurface_regions()
        assert _same_bits(v, v0) and _same_bits(t, t0) and _same_bits(ctx.download_isosurface_normals(), n0)
        assert _same_bits(rid, rid0) and _same_bits(rsz, rsz0)
        # two identical calls on identical fresh extractions: identical bytes; times
        runs = []
        for _ in range(2):
            ctx.extract_isosurface_with_normals(0.0)
            ctx.filter_isosurface_components(C.MIN_TRIANGLES, 0)
            ctx.decimate_isosurface(4.0 * spacing, "quadric")
            runs.append(tuple(a.tobytes() for a in ctx.download_isosurface()) + (ctx.download_isosurface_normals().tobytes(),))
            passes = ctx.isosurface_decimate_pass_ms()
            assert list(passes) == ["clustering", "representatives", "triangles", "normals"] and all(p > 0.0 for p in passes.values())
            assert 0.0 < sum(passes.values()) <= ctx.isosurface_decimate_kernel_ms()
            with pytest.raises(capi.DmiError) as e:                                # regions are refused after success, as for the mean
                ctx.download_isosurface_regions()
            assert e.value.code == INVALID_ARGUMENT and "no regions" in str(e.value)
            with pytest.raises(capi.DmiError) as e:                                # ... and colours
                ctx.download_isosurface_colors()
            assert e.value.code == INVALID_ARGUMENT
        assert runs[0] == runs[1]
        want = Q.decimate(v0, t0, 4.0 * spacing, n0)
        assert runs[0] == tuple(a.tobytes() for a in want)
        # a second call takes the decimated mesh
        again = Q.decimate(want[0], want[1], 9.0 * spacing, want[2])
        assert ctx.decimate_isosurface(9.0 * spacing, "quadric") == (len(again[0]), len(again[1]))
        v, t = ctx.download_isosurface()
        assert _same_bits(v, again[0]) and _same_bits(t, again[1]) and _same_bits(ctx.download_isosurface_normals(), again[2])
        # everything collapses, then the empty mesh: successes; the second had nothing to do
        assert ctx.decimate_isosurface(1e6, "quadric") == (0, 0)
        assert ctx.isosurface_decimate_kernel_ms() > 0.0 and ctx.isosurface_decimate_pass_ms()["normals"] == 0.0
        assert ctx.decimate_isosurface(1.0, "quadric") == (0, 0)
        assert ctx.isosurface_decimate_kernel_ms() == 0.0 and set(ctx.isosurface_decimate_pass_ms().values()) == {0.0}
        assert ctx.download_isosurface()[0].shape == (0, 3)
        ctx.reset_grid()
        assert ctx.extract_isosurface(1.0)[0].shape == (0, 3)
        assert ctx.decimate_isosurface(1.0, "quadric") == (0, 0) and ctx.isosurface_decimate_kernel_ms() == 0.0


@pytest.mark.gpu
def test_gpu_quadric_decimation_refuses_a_mesh_with_a_non_finite_coordinate():
    """A grid whose far corner overflows f64: 1.79e308 + k 1e306 is an infinity from k = 1 on, and the sphere starts at k = 3, so
    no vertex of its mesh has a finite x.  Both placements refuse it through the new entry, and the mesh, its normals and
    the regions of a filter are bit for bit what they were."""
    cells = T._cell_field(T.sphere_field())
    grid = scene.GridDesc((24, 24, 24), (1.79e308, 0.0, 0.0), (1e306, 1.0, 1.0), np.eye(4))
    assert np.isinf(1.79e308 + 1e306)
    with capi.FusionContext(grid, scene.default_ray_potential(grid)) as ctx:
        ctx.upload_grid(cells)
        v0, t0, n0 = ctx.extract_isosurface_with_normals(0.0)
        assert len(t0) > 500 and not np.isfinite(v0[:, 0]).any()                   # infinities, and NaN where two were interpolated
        kept = ctx.filter_isosurface_components(C.MIN_TRIANGLES, 0)                # keeps everything, leaves regions
        assert kept[:2] == (len(v0), len(t0))
        rid0, rsz0 = ctx.download_isosurface_regions()
        for placement in ("quadric", "mean"):
            if placement == "quadric":
                assert "non-finite" in _refused(ctx, 1.0)
            else:                                                                 # the mean through the new entry
                n = ctypes.c_uint64(0)
                assert capi.load().dmi_decimate_isosurface_placed(ctx._h, 1.0, capi.DMI_DECIMATE_MEAN, ctypes.byref(n), ctypes.byref(n)) == INVALID_ARGUMENT
                text = capi.load().dmi_last_error(ctx._h).decode()
                assert "non-finite" in text and "dmi_decimate_isosurface_placed" in text
            v, t = ctx.download_isosurface()
            rid, rsz = ctx.download_isosurface_regions()
            assert _same_bits(v, v0) and _same_bits(t, t0) and _same_bits(ctx.download_isosurface_normals(), n0)
            assert _same_bits(rid, rid0) and _same_bits(rsz, rsz0)


@pytest.mark.gpu
def test_gpu_quadric_decimation_composes_with_the_filter_the_smoother_and_the_coloration():
    grid = scene.default_grid((24, 20, 16), rotated=True)
    rp = scene.default_ray_potential(grid)
    views = scene.make_views(5, 48, 36, seed=4, dense=True)
    colors = scene.make_colors(5, 48, 36, seed=5)
    spacing = min(grid.spacing)
    with capi.FusionContext(grid, rp) as ctx, capi.ColorContext() as cc:
        ctx.add_views(views)
        ctx.fuse()
        cc.add_views(colors, views.K4, views.RT4)
        v0, t0, n0 = ctx.extract_isosurface_with_normals(0.25)
        size = C.components(len(v0), t0)[1]
        n_min = int(np.median(size[size > 0])) + 1
        kept = C.filter_mesh(v0, t0, n0, C.MIN_TRIANGLES, n_min)
        sv, sn = S.smooth(kept["vertices"], kept["triangles"], 3, 0.5, -0.53, kept["normals"])
        want = Q.decimate(sv, kept["triangles"], 1.5 * spacing, sn)
        assert ctx.filter_isosurface_components(C.MIN_TRIANGLES, n_min) == kept["counts"]
        ctx.smooth_isosurface(3, 0.5, -0.53)
        assert ctx.decimate_isosurface(1.5 * spacing, "quadric") == (len(want[0]), len(want[1])) and 0 < len(want[1]) < kept["counts"][1]
        v, t = ctx.download_isosurface()
        assert _same_bits(v, want[0]) and _same_bits(t, want[1]) and _same_bits(ctx.download_isosurface_normals(), want[2])
        assert not _same_bits(v, D.decimate(sv, kept["triangles"], 1.5 * spacing)[0])
        assert ctx.color_isosurface(cc) == len(v)
        wanted = CD.color_mesh_depth_np(want[0], colors, None, views.K4, views.RT4, None)
        for a, b in zip(ctx.download_isosurface_colors(), wanted):
            assert _same_bits(np.ascontiguousarray(a), np.ascontiguousarray(b))
        assert (wanted[2] > 0).any()
        # quadric decimation -> filter(LARGEST) -> smooth, on a fresh extraction
        v1, t1, n1 = ctx.extract_isosurface_with_normals(0.25)
        assert _same_bits(v1, v0) and _same_bits(t1, t0) and _same_bits(n1, n0)
        dv, dt, dn = Q.decimate(v0, t0, 1.5 * spacing, n0)
        big = C.filter_mesh(dv, dt, dn, C.LARGEST)
        sv, sn = S.smooth(big["vertices"], big["triangles"], 3, 0.5, -0.53, big["normals"])
        assert ctx.decimate_isosurface(1.5 * spacing, "quadric") == (len(dv), len(dt))
        assert ctx.filter_isosurface_components(C.LARGEST) == big["counts"]
        ctx.smooth_isosurface(3, 0.5, -0.53)
        v, t = ctx.download_isosurface()
        assert _same_bits(v, sv) and _same_bits(t, big["triangles"]) and _same_bits(ctx.download_isosurface_normals(), sn)


@pytest.mark.gpu
def test_gpu_cli_quadric_decimation_end_to_end(tmp_path):
    """dmi_reconstruction --extractMesh --meshDecimateCellSize h --meshDecimateQuadric on the scene of
    test_gpu_cli_decimation_end_to_end: mesh.vtp is the Python call's result on the same fused grid, bit for bit, and the log and
    summary.txt say "quadric placement"; without the flag the files and lines are the mean placement's, as they were."""
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
            "--outputMeshFilename", str(tmp_path / "mesh.vtp"), "--summary", "--extractMesh", "--meshNormals"]

    def run(flags):
        r = subprocess.run(args + flags, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr + r.stdout
        pd = capi.read_polydata(str(tmp_path / "mesh.vtp"))
        return pd.points, pd.connectivity.reshape(-1, 3), pd.point_data, r.stdout + r.stderr, open(data / "summary.txt").read()

    o, _ = capi.cli_read_arguments(args)
    h = 1.5 * min(o.grid_spacing)
    g2 = scene.GridDesc(tuple(int(d) - 1 for d in o.grid_dims), tuple(o.grid_origin), tuple(o.grid_spacing), np.array(o.grid_matrix).reshape(4, 4))
    v0, t0, arrays0, _, _ = run([])
    with capi.FusionContext(g2, rp) as ctx:                                       # the Python calls, on the same fused grid
        ctx.add_views(views, threshold=0.7)
        ctx.fuse()
        pv, pt, pn = ctx.extract_isosurface_with_normals(0.25)
        assert _same_bits(pv, v0) and _same_bits(pt, t0) and _same_bits(pn, arrays0["Normals"])
        mean_counts = ctx.decimate_isosurface(h)
        mean = ctx.download_isosurface() + (ctx.download_isosurface_normals(),)
        ctx.extract_isosurface_with_normals(0.25)
        assert ctx.decimate_isosurface(h, "quadric") == mean_counts
        quadric = ctx.download_isosurface() + (ctx.download_isosurface_normals(),)
    assert 0 < len(mean[1]) < len(t0) and not _same_bits(mean[0], quadric[0])
    want = Q.decimate(v0, t0, h, arrays0["Normals"])
    assert all(_same_bits(a, b) for a, b in zip(quadric, want))
    v, t, arrays, text, summary = run(["--meshDecimateCellSize", repr(h), "--meshDecimateQuadric"])
    assert _same_bits(v, quadric[0]) and _same_bits(t, quadric[1]) and _same_bits(arrays["Normals"], quadric[2])
    assert list(arrays) == ["Normals", "reconstruction_scalar"]
    line = f"{len(v0)} vertices, {len(t0)} triangles before, {len(v)} vertices, {len(t)} triangles after"
    assert f"mesh decimation: cell size {h:g}, quadric placement; {line}; " in text
    assert f"  mesh decimation  cell size {h:g}, quadric placement, {line}, " in summary
    quadric_file = open(tmp_path / "mesh.vtp", "rb").read()
    # without the flag: the mean placement's, the line as it always was
    v, t, arrays, text, summary = run(["--meshDecimateCellSize", repr(h)])
    assert _same_bits(v, mean[0]) and _same_bits(t, mean[1]) and _same_bits(arrays["Normals"], mean[2])
    assert "quadric placement" not in text and "quadric placement" not in summary
    assert f"mesh decimation: cell size {h:g}; {line}; " in text and f"  mesh decimation  cell size {h:g}, {line}, " in summary
    mean_file = open(tmp_path / "mesh.vtp", "rb").read()
    assert mean_file != quadric_file
    expected = str(tmp_path / "expected.vtp")                                    # the file the writer makes of the Python call's result
    capi.write_polydata_with_normals(expected, mean[0], mean[1], mean[2], 0.25)
    assert open(expected, "rb").read() == mean_file
