"""The window column's reciprocals come from one Newton step per voxel (fusion_tile.hip): its error is the square
of c.z's relative step between two voxels of a column, which the scenes of the other tests keep tiny (cameras three grid widths
away).  Here the cameras stand next to and inside the grid: bricks whose c.z grows by up to kWinCzRatio = 1.25 from one corner to
the other still get windows, and a camera plane cuts the grid along steep columns (the gathering columns: c.z crosses zero inside a
brick).  The bar is the usual one: the oracle's grid, bit for bit."""
import numpy as np
import pytest

from cudadepthmapintegration_amd import capi, scene
from oracle import oracle
from helpers import bits_equal, oracle_params_from_scene

pytestmark = pytest.mark.gpu

FX = capi.VARIANT_FIXED_TILE_SHAPE
WA = capi.VARIANT_WINDOWS_ALWAYS
DIMS = (96, 80, 64)
W, H = 320, 240
TK = 16  # shape 0: bricks of 8 x 8 x 16 voxels


def _views(positions, targets, focal_scale, hole_seed):
    """Pinhole cameras at `positions` looking at `targets` over the sphere scene with a background, 10 % of the pixels without a
    depth, scattered."""
    K = np.eye(4)
    K[0, 0] = K[1, 1] = focal_scale * W
    K[0, 2] = W / 2.0 - 1.75  # principal point off the centre
    K[1, 2] = H / 2.0
    n = len(positions)
    depth = np.empty((n, H, W))
    K4 = np.empty((n, 4, 4))
    RT4 = np.empty((n, 4, 4))
    for m in range(n):
        RT4[m] = scene.look_at_rt(np.asarray(positions[m], dtype=np.float64), target=targets[m])
        K4[m] = K
        depth[m] = scene.render_sphere_depth(K[:3, :3], RT4[m], W, H, background=2.4)
    depth[np.random.default_rng(hole_seed).random(depth.shape) < 0.1] = -1.0
    return scene.Views(depth, K4, RT4)


def _near_views():
    """Eight cameras on a sphere of radius 1.45 around the grid cube [-1, 1]^3 (its faces are 0.45 away, its corners behind the
    cameras) and one inside the cube, all with a wide field of view: a brick's footprint stays within a window's 32 x 64 pixels
    down to c.z = 0.6."""
    rng = np.random.default_rng(5)
    pos = list(scene.camera_positions(8, radius=1.45)) + [np.array([0.78, 0.12, 0.06])]
    targets = [0.02 * rng.standard_normal(3) for _ in pos]
    return _views(pos, targets, focal_scale=0.25, hole_seed=11)


def _cutting_views():
    """Cameras inside the cube looking along the grid's k axis, a little tilted: the plane c.z = 0 cuts the grid, and c.z changes
    sign within a brick along its columns (a brick's 16 voxels are half a unit of c.z here)."""
    pos = [np.array([0.31, -0.22, -0.17]), np.array([-0.4, 0.3, 0.23]), np.array([0.1, 0.55, -0.52]), np.array([-0.66, -0.61, 0.05]),
           np.array([0.7, 0.2, 0.4]), np.array([-0.2, -0.1, -0.75]), np.array([0.0, 0.72, 0.7]), np.array([0.5, -0.7, -0.3])]
    tilt = [(0.12, 0.05), (-0.2, 0.1), (0.05, -0.3), (0.3, 0.25), (-0.1, -0.15), (0.02, 0.01), (0.4, -0.1), (-0.25, 0.3)]
    sign = [1, -1, 1, -1, -1, 1, -1, 1]
    targets = [p + np.array([tx, ty, float(s)]) for p, (tx, ty), s in zip(pos, tilt, sign)]
    return _views(pos, targets, focal_scale=0.35, hole_seed=12)


def _brick_corner_cz(grid, views):
    """c.z at the eight corner VOXELS of every brick of 8 x 8 x TK voxels (those that lie inside the grid) for every view:
    shape (views, bricks_z, bricks_y, bricks_x, 8), and the corners' world positions."""
    nx, ny, nz = grid.cell_dims
    o, s = np.asarray(grid.origin), np.asarray(grid.spacing)
    G = np.asarray(grid.grid_matrix)
    bx, by, bz = np.arange(nx // 8), np.arange(ny // 8), np.arange(nz // TK)
    BZ, BY, BX = np.meshgrid(bz, by, bx, indexing="ij")
    corners = []
    for dk in (0, TK - 1):
        for dj in (0, 7):
            for di in (0, 7):
                idx = np.stack([BX * 8 + di, BY * 8 + dj, BZ * TK + dk], axis=-1)
                g = o + (idx + 0.5) * s
                corners.append(g @ G[:3, :3].T + G[:3, 3])
    world = np.stack(corners, axis=-2)  # (bz, by, bx, 8, 3)
    cz = np.einsum("mc,zyxkc->mzyxk", views.RT4[:, 2, :3], world) + views.RT4[:, 2, 3][:, None, None, None, None]
    return cz, world


def _window_candidates(grid, rp, views):
    """(ratio, view, bx, by, bz) of the pairs that a window should serve, by a test stricter than the library's: every corner in
    front of the camera, the corners' pixels well inside the image and within 28 x 56 pixels, and every depth of that rectangle (and
    three pixels around it) missing or further behind the brick than delta.  Sorted by c.z ratio, largest first."""
    cz, world = _brick_corner_cz(grid, views)
    out = []
    for m in range(views.n):
        zmin, zmax = cz[m].min(axis=-1), cz[m].max(axis=-1)
        ratio = np.where(zmin > 0, zmax / np.where(zmin > 0, zmin, 1.0), np.inf)
        for b in np.argwhere((ratio > 1.15) & (ratio < 1.24)):
            w = world[tuple(b)]
            c = w @ views.RT4[m, :3, :3].T + views.RT4[m, :3, 3]
            u = views.K4[m, 0, 0] * c[:, 0] / c[:, 2] + views.K4[m, 0, 2]
            v = views.K4[m, 1, 1] * c[:, 1] / c[:, 2] + views.K4[m, 1, 2]
            x0, x1, y0, y1 = int(np.floor(u.min())) - 3, int(np.ceil(u.max())) + 3, int(np.floor(v.min())) - 3, int(np.ceil(v.max())) + 3
            if x0 < 0 or y0 < 0 or x1 >= W or y1 >= H or x1 - x0 >= 28 + 6 or y1 - y0 >= 56 + 6:
                continue
            d = views.depth[m, y0:y1 + 1, x0:x1 + 1]
            if np.all((d == -1.0) | (d - zmax[tuple(b)] > 1.5 * rp.delta)):
                out.append((float(ratio[tuple(b)]), m, int(b[2]), int(b[1]), int(b[0])))
    return sorted(out, reverse=True)


@pytest.fixture(scope="module")
def near_scene():
    return _near_views()


@pytest.fixture(scope="module")
def cutting_scene():
    return _cutting_views()


def _oracle_grid(grid, rp, views):
    want, _, map_hits = oracle.fuse(oracle_params_from_scene(grid, rp, views), views.depth, views.K4, views.RT4, n_threads=oracle.max_threads())
    # (on the CPU, with the oracle alone: the scene is not an empty one)
    assert int(np.count_nonzero(map_hits)) == views.n and np.count_nonzero(want) > want.size // 20, (map_hits, np.count_nonzero(want))
    return want


@pytest.mark.parametrize("rotated", [False, True])
def test_windows_next_to_the_cameras(near_scene, rotated):
    """Bricks whose c.z varies by a factor between 1.15 and kWinCzRatio get windows (one such brick is fused as a grid of its own:
    exactly one window pair), and the whole grid is the oracle's with the default shapes, 16-voxel columns and windows forced."""
    grid = scene.default_grid(DIMS, rotated=rotated)
    rp = scene.default_ray_potential(grid)
    views = near_scene
    want = _oracle_grid(grid, rp, views)
    cands = _window_candidates(grid, rp, views)
    assert cands, "no brick with a c.z ratio above 1.15 whose footprint lies in free space"
    served = []
    for ratio, m, bx, by, bz in [cands[q * (len(cands) - 1) // 3] for q in range(4)]:  # from the largest ratio to the smallest
        # the brick as a grid of its own, fused with its view alone: one (brick, view) pair
        o = tuple(grid.origin[a] + (bx * 8, by * 8, bz * TK)[a] * grid.spacing[a] for a in range(3))
        one = scene.GridDesc((8, 8, TK), o, grid.spacing, grid.grid_matrix)
        with capi.FusionContext(one, rp, kernel_variant=FX | WA) as ctx:
            ctx.add_views(views.subset(m, m + 1))
            ctx.fuse()
            served.append((ratio, ctx.window_pair_count()))
    assert any(n == 1 and ratio > 1.15 for ratio, n in served), served
    for variant in (0, FX, WA):
        with capi.FusionContext(grid, rp, kernel_variant=variant) as ctx:
            ctx.add_views(views)
            ctx.fuse()
            out = ctx.download_grid()
            n_win = ctx.window_pair_count()
        assert bits_equal(out, want), (rotated, variant)
        assert n_win > 0, (rotated, variant)


@pytest.mark.parametrize("rotated", [False, True])
def test_camera_planes_through_the_grid(cutting_scene, rotated):
    """Columns along the viewing direction of cameras inside the grid: c.z passes through zero inside a brick (checked here on the
    brick corners), tier 1's reciprocal meets non-positive c.z on the gathering columns, and the grid is the oracle's."""
    grid = scene.default_grid(DIMS, rotated=rotated)
    rp = scene.default_ray_potential(grid)
    views = cutting_scene
    want = _oracle_grid(grid, rp, views)
    cz, _ = _brick_corner_cz(grid, views)
    # the two ends of a column (corner k of the first plane and of the last): opposite signs, and steep (most of a brick's c.z range)
    crossing = (cz[..., :4] * cz[..., 4:] < 0) & (np.abs(cz[..., 4:] - cz[..., :4]) > 0.4)
    assert all(crossing[m].any() for m in range(views.n)), crossing.reshape(views.n, -1).sum(axis=1)
    for variant in (0, FX, WA):
        with capi.FusionContext(grid, rp, kernel_variant=variant) as ctx:
            ctx.add_views(views)
            ctx.fuse()
            assert bits_equal(ctx.download_grid(), want), (rotated, variant)
