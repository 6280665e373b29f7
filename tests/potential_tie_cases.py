"""Scenes for tests/test_potential_tie_cases.py and tests/test_gpu_potential_ties.py: the VALUE side of the fusion at its ties.

The reference decides what a voxel accumulates with strict compares (cu:105-120: |diff| > delta, |diff| > thick, diff > 0,
diff != 0) on diff = c.z - depth.  Rendered spheres and random poses never put diff exactly on +-delta, +-thick or 0; the scenes
here do, on whole layers of voxels, with numbers that are all dyadic so that c.z, the depth and diff are exact doubles:

  * a grid of 16 x 16 cells across the viewing axis and 64 along it (two 32-boxes, four 16-bricks, eight 8-bricks), spacing 1/16,
    with the identity grid matrix or a signed permutation (the library's rotated path; c.z stays exact);
  * six camera families, one per grid axis and direction, rotation rows of 0 and +-1, 8 units in front of the grid's middle:
    along the viewing axis c.z(L) = 8 + s g(L) exactly, one value per layer L;
  * one view per layer L0 from 6 layers before the grid to 6 behind it, whose depth map is the constant c.z(L0): layer L has
    diff = s (L - L0) / 16, so every tie meets every alignment to bricks, boxes and the grid's ends;
  * variants: the image split at a column that is no multiple of 8 between c.z(L0) and c.z(L0 + 8); a tenth of the pixels
    without a depth; the principal point shifted so that the grid's picture leaves the image; K[2][2] = 2 (general K);
  * the outward-rounding scenes: depths that are no f32 values, 2^-46 on the near side of a tie, so that a min/max pyramid
    rounded to nearest instead of outward proves a brick free (or behind) that is not;
  * the range-ends scene: patches of +-inf, +-0, negative, subnormal, just-not-sentinel and huge depths in rendered maps.

The views of a tie scene are ordered in GROUPS of four whose L0 are 19 layers apart: fused alone, a group gives every layer at
most one value of the column's ramp or plateau beside a few free-space constants, so that a one-ulp error of a view (0.9 for
0.8999999999999999 at |diff| == thick) is not rounded away in a sum of 76 views (test_potential_tie_cases proves it sees it).

Helpers only; every expectation is the oracle's."""
import functools

import numpy as np

from cudadepthmapintegration_amd import scene
from oracle import oracle, oracle_np
from helpers import oracle_params_from_scene

S = 1.0 / 16.0        # spacing on every axis
NA, NC = 64, 16       # cells along / across the viewing axis
DIST = 8.0            # RT[2][3] in the grid's own frame: c.z = DIST + s g
W, H = 96, 80
F = 192.0
PC = (48.25, 39.75)   # dyadic; the grid's picture is within 16 pixels of it
MARGIN = 6            # layers before and behind the grid that get a view of their own
GROUP_STRIDE = 19     # (NA + 2 MARGIN) / 4: the L0 of a group's four views are this far apart
SPLIT_X = 45          # the split variant's column: no multiple of 8, inside the picture of every layer
SPLIT_LAYERS = 8
E1, E2 = 2.0 ** -46, 2.0 ** -45

FAMILIES = ("+i", "-i", "+j", "-j", "+k", "-k")
GRIDS = ("identity", "permutation")
# rows gridVecX/Y/Z of the signed permutation (w = G g): every entry 0 or +-1, none on the diagonal, a dyadic translation
PERMUTATION = np.array([[0.0, -1.0, 0.0, 0.25], [0.0, 0.0, 1.0, -0.5], [-1.0, 0.0, 0.0, 0.125], [0.0, 0.0, 0.0, 1.0]])

PARAM_SETS = {
    "main": scene.RayPotential(thickness=3 * S, rho=0.9, eta=0.03, delta=5 * S),
    "thick_zero": scene.RayPotential(thickness=0.0, rho=0.9, eta=0.03, delta=5 * S),       # diff == 0: the reference's NaN (cu:119)
    "delta_zero": scene.RayPotential(thickness=3 * S, rho=0.9, eta=0.03, delta=0.0),
    "delta_eq_thick": scene.RayPotential(thickness=3 * S, rho=0.9, eta=0.03, delta=3 * S),
    "delta_lt_thick": scene.RayPotential(thickness=5 * S, rho=0.9, eta=0.03, delta=3 * S),
    "rho_neg_eta_neg": scene.RayPotential(thickness=3 * S, rho=-0.9, eta=-0.03, delta=5 * S),  # free-space constant < 0
    "rho_neg_eta_pos": scene.RayPotential(thickness=3 * S, rho=-0.9, eta=0.03, delta=5 * S),   # free-space constant > 0
}

# the principal points of the border variants, with a focal length of 2 F (the picture is 60 pixels wide at the nearest layer):
# the picture starts 22 pixels left of the image (within the validity maps' margin of 32), or ends 40 pixels below it
BORDER_PC = {"border_in_margin": (8.25, 39.75), "border_beyond_margin": (48.25, 90.25)}
KINDS = ("plain", "split", "holes", "split_holes", "general_k") + tuple(BORDER_PC) + tuple(k + "_holes" for k in BORDER_PC)


def axis_of(family):
    return "ijk".index(family[1])


def sign_of(family):
    return 1.0 if family[0] == "+" else -1.0


def grid_for(family, grid_kind):
    a = axis_of(family)
    dims, origin = [NC] * 3, [-0.5] * 3
    dims[a], origin[a] = NA, -2.0
    G = np.eye(4) if grid_kind == "identity" else PERMUTATION.copy()
    return scene.GridDesc(tuple(dims), tuple(origin), (S, S, S), G)


def layer_coordinate(family, L):
    """g(L): the grid-frame coordinate of layer L's voxel centres along the viewing axis (any integer L, also outside the grid)."""
    return -2.0 + (L + 0.5) * S


def cz_of_layer(family, L, rt23=DIST):
    """The exact c.z of every voxel of layer L: rt23 + s g(L)."""
    return rt23 + sign_of(family) * layer_coordinate(family, L)


def camera(grid, family, f=F, pc=PC, rt23=DIST, k22=1.0):
    """K, RT of the family's camera: it looks along s e_a of the grid's own frame from rt23 in front of the plane g_a = 0, and
    is carried into the world by the grid matrix.  k22 scales K's three rows alike (h.z = k22 c.z: the same pixels)."""
    a, s = axis_of(family), sign_of(family)
    Rg = np.zeros((3, 3))
    Rg[0, (a + 1) % 3] = 1.0
    Rg[1, (a + 2) % 3] = s
    Rg[2, a] = s
    Tg = np.array([0.0, 0.0, rt23])
    G = np.asarray(grid.grid_matrix, dtype=np.float64)
    RT = np.eye(4)
    RT[:3, :3] = Rg @ G[:3, :3].T
    RT[:3, 3] = Tg - RT[:3, :3] @ G[:3, 3]
    K = np.eye(4)
    K[0, 0] = K[1, 1] = f * k22
    K[0, 2], K[1, 2], K[2, 2] = pc[0] * k22, pc[1] * k22, k22
    return K, RT


def view_layers():
    """L0 of every view of a tie scene, in the scene's order: groups of four, GROUP_STRIDE layers apart."""
    return sorted(range(-MARGIN, NA + MARGIN), key=lambda L: ((L + MARGIN) % GROUP_STRIDE, L))


def groups():
    """(first, count) of every group of views."""
    n = NA + 2 * MARGIN
    assert n % GROUP_STRIDE == 0
    per = n // GROUP_STRIDE
    return [(g * per, per) for g in range(GROUP_STRIDE)]


@functools.lru_cache(maxsize=None)
def tie_scene(family, grid_kind, kind="plain"):
    """(grid, views) of a tie scene.  The arrays are shared between tests: read only."""
    assert kind in KINDS, kind
    grid = grid_for(family, grid_kind)
    base = kind[:-len("_holes")] if kind.endswith("_holes") else kind
    if base in BORDER_PC:
        K, RT = camera(grid, family, f=2.0 * F, pc=BORDER_PC[base])
    elif base == "general_k":
        K, RT = camera(grid, family, k22=2.0)
    else:
        K, RT = camera(grid, family)
    layers = view_layers()
    depth = np.empty((len(layers), H, W))
    for m, L0 in enumerate(layers):
        depth[m] = cz_of_layer(family, L0)
        if base == "split":
            depth[m][:, SPLIT_X:] = cz_of_layer(family, L0 + SPLIT_LAYERS)
    if kind.endswith("holes"):
        depth[np.random.default_rng(97 + FAMILIES.index(family)).random(depth.shape) < 0.1] = -1.0
    views = scene.Views(depth, np.tile(K, (len(layers), 1, 1)), np.tile(RT, (len(layers), 1, 1)))
    for arr in (views.depth, views.K4, views.RT4):
        arr.setflags(write=False)
    return grid, views


# ---- the outward-rounding scenes -------------------------------------------------------------------------------------------------
ROUNDING_POSITIONS = {"free": (7, 15, 31, 63), "behind": (8, 16, 32, 0)}  # as seen from the camera: last / first layer of an
                                                                          # 8-brick, a 16-brick, a 32-box, the grid


def layer_at_position(family, p):
    """The grid's layer that is the p-th as seen from the family's camera."""
    return p if sign_of(family) > 0 else NA - 1 - p


ROUNDING_OFFSETS = (E1, 2.0 ** -30)  # e1 (e2 = 2 e1).  2^-46 is an ulp's breadth from the tie; 2^-30 is far beyond the 2 cz_err by
                                     # which the classification widens c.z on a rotated grid, and still 2^-10
                                     # of the f32 spacing at these depths: there the rounding decides on the permutation grid too


@functools.lru_cache(maxsize=None)
def rounding_scene(family, grid_kind):
    """(grid, views, sides, layers, F, e1): view m is of side sides[m] ("free" / "behind") and aims at layer layers[m]; F[m] is
    the f32 value its depth, F -+ 2 e1[m], narrows to.
      free:   RT[2][3] = 8 - e1, c.z(L) = F - delta - e1: c.z - depth = -delta + e1 (not free), c.z - F < -delta;
      behind: RT[2][3] = 8 + e1, c.z(L) = F + delta + e1: c.z - depth = +delta - e1 (not behind), c.z - F > +delta."""
    grid = grid_for(family, grid_kind)
    delta = PARAM_SETS["main"].delta
    sides, layers, Fs, e1s, Ks, RTs, depth = [], [], [], [], [], [], []
    for e1 in ROUNDING_OFFSETS:
        for side, positions in ROUNDING_POSITIONS.items():
            sg = -1.0 if side == "free" else 1.0
            for p in positions:
                L = layer_at_position(family, p)
                K, RT = camera(grid, family, rt23=DIST + sg * e1)
                f32_depth = cz_of_layer(family, L) - sg * delta        # = c.z(L) -+ delta -+ e1 with the view's own RT[2][3]
                sides.append(side), layers.append(L), Fs.append(f32_depth), e1s.append(e1), Ks.append(K), RTs.append(RT)
                depth.append(np.full((H, W), f32_depth + sg * 2.0 * e1))
    views = scene.Views(np.stack(depth), np.stack(Ks), np.stack(RTs))
    for arr in (views.depth, views.K4, views.RT4):
        arr.setflags(write=False)
    return grid, views, tuple(sides), tuple(layers), np.array(Fs), np.array(e1s)


def narrowed(views):
    """The views as a store of f32 depths holds them."""
    with np.errstate(over="ignore"):
        d = views.depth.astype(np.float32).astype(np.float64)
    return scene.Views(d, views.K4, views.RT4)


# ---- depth values at the ends of the range ---------------------------------------------------------------------------------------
FLT_MAX = float(np.finfo(np.float32).max)
RANGE_END_VALUES = {
    "plus_inf": np.inf, "minus_inf": -np.inf, "zero": 0.0, "minus_zero": -0.0, "negative": -2.5,
    "f64_subnormal": 2.0 ** -1060, "f32_subnormal": 2.0 ** -140,
    "just_above_sentinel": float(np.nextafter(-1.0, 0.0)), "just_below_sentinel": float(np.nextafter(-1.0, -np.inf)),
    "flt_max": FLT_MAX, "twice_flt_max": 2.0 * FLT_MAX,
}
PATCH = (12, 12)  # pixels: columns, rows


@functools.lru_cache(maxsize=None)
def range_ends_scene():
    """(grid, ray potential, views, names [n, H, W] of object: the special value's name or None).  Rendered maps of the sphere
    scene (random poses, f32-inexact depths) with every other patch of 12 x 12 pixels holding one of RANGE_END_VALUES."""
    grid = scene.default_grid((24, 20, 28))
    rp = scene.default_ray_potential(grid)
    v = scene.make_views(6, 96, 72, seed=11, dense=True)
    depth = v.depth * (1.0 + 2.0 ** -30)      # no f32 values: auto storage keeps f64
    names = np.full(depth.shape, None, dtype=object)
    keys = list(RANGE_END_VALUES)
    q = 0
    for m in range(v.n):
        for py in range(72 // PATCH[1]):
            for px in range(96 // PATCH[0]):
                if (px + py + m) % 2:
                    continue
                key = keys[q % len(keys)]
                q += 1
                sl = (m, slice(py * PATCH[1], (py + 1) * PATCH[1]), slice(px * PATCH[0], (px + 1) * PATCH[0]))
                depth[sl] = RANGE_END_VALUES[key]
                names[sl] = key
    views = scene.Views(depth, v.K4, v.RT4)
    for arr in (views.depth, views.K4, views.RT4):
        arr.setflags(write=False)
    return grid, rp, views, names


# ---- what the reference sees ---------------------------------------------------------------------------------------------------
def project(grid, views):
    """(c.z, pixel column, pixel row, inside) per view and voxel, [n, nz, ny, nx], in the reference's order of operations
    (oracle_np): `inside` says that the voxel passes cu:177 and cu:192-197, its pixel is (px, py), table entry [H-1-py, px]."""
    nx, ny, nz = grid.cell_dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    g = [grid.origin[a] + (idx + 0.5) * grid.spacing[a] for a, idx in enumerate((i, j, k))]
    w = oracle_np._rows(np.asarray(grid.grid_matrix, dtype=np.float64), *g)
    cz, px, py, ok = [], [], [], []
    for m in range(views.n):
        c = oracle_np._rows(views.RT4[m], *w)
        h = oracle_np._rows(views.K4[m], *c)
        with np.errstate(divide="ignore", invalid="ignore"):
            ru, rv = oracle_np._round_half_away(h[0] / h[2]), oracle_np._round_half_away(h[1] / h[2])
        inside = ~(h[2] < 0) & (ru >= 0) & (rv >= 0) & (ru < views.width) & (rv < views.height)
        cz.append(c[2]), ok.append(inside)
        px.append(np.where(inside, ru, 0).astype(np.int64)), py.append(np.where(inside, rv, 0).astype(np.int64))
    return np.stack(cz), np.stack(px), np.stack(py), np.stack(ok)


def image_coordinates(grid, views, m=0):
    """u, v of every voxel centre in view m (fp64, the reference's order of operations), [nz, ny, nx]."""
    nx, ny, nz = grid.cell_dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    g = [grid.origin[a] + (idx + 0.5) * grid.spacing[a] for a, idx in enumerate((i, j, k))]
    c = oracle_np._rows(views.RT4[m], *oracle_np._rows(np.asarray(grid.grid_matrix, dtype=np.float64), *g))
    h = oracle_np._rows(views.K4[m], *c)
    return h[0] / h[2], h[1] / h[2]


def layers_first(grid, family, a):
    """a [..., nz, ny, nx] with the viewing axis moved to the front of the three: [..., layer, 16, 16]."""
    return np.moveaxis(a, a.ndim - 1 - axis_of(family), a.ndim - 3)


def oracle_grid(grid, rp, views, first=0, count=None, init=None, count_hits=True):
    """The C oracle's (grid, voxel hits, map hits) of views [first, first + count)."""
    v = views if count is None and first == 0 else views.subset(first, first + count)
    return oracle.fuse(oracle_params_from_scene(grid, rp, v), v.depth, v.K4, v.RT4, init_grid=init, count_hits=count_hits,
                       n_threads=oracle.max_threads())


def numpy_grid(grid, rp, views, first=0, count=None, init=None):
    v = views if count is None and first == 0 else views.subset(first, first + count)
    return oracle_np.fuse(grid.cell_dims, grid.origin, grid.spacing, grid.grid_matrix, rp.thickness, rp.rho, rp.eta, rp.delta,
                          v.depth, v.K4, v.RT4, init_grid=init)


@functools.lru_cache(maxsize=None)
def init_grid(n_voxels):
    """An uploaded grid: random normal values, a tenth of them -0.0."""
    rng = np.random.default_rng(5)
    g = rng.standard_normal(n_voxels)
    g[rng.random(n_voxels) < 0.1] = -0.0
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def expected(family, grid_kind, kind, param_set, with_init=False, narrow=False):
    """What the GPU tests compare with: {"all": (grid, voxel hits, map hits), "groups": [grid per group]}; computed once."""
    grid, views = tie_scene(family, grid_kind, kind)
    if narrow:
        views = narrowed(views)
    rp = PARAM_SETS[param_set]
    init = init_grid(grid.n_voxels) if with_init else None
    return {"all": oracle_grid(grid, rp, views, init=init),
            "groups": [oracle_grid(grid, rp, views, f, c, init=init, count_hits=False)[0] for f, c in groups()]}
