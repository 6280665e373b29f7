"""The clouds of test_depth_points_scale.py and their CPU references, each computed once and left unchanged: clouds of 2^20 + 4321
points for the thinning at chosen key widths, a base cloud for the neighbour count with two strays that set the search grid's key
width, a cloud of 270 001 points, and the room scene's cloud of 1 228 800 points with its filtered and its thinned successors."""
import functools

import numpy as np

import depth_points_np as P
import depth_points_radius_binned_np as B
import depth_points_radius_np as R
import depth_points_thin_np as T
from view_set_model import ViewSetModel
from cudadepthmapintegration_amd import scene

P0 = (1 << 20) + 4321        # above rocPRIM's merge-sort limit (2^20 items) and above every stride cap of the passes
INPUT_NAMES = ("xyz", "normal", "view", "pixel", "count")

# ---- the thinning: key_bits -> (bins, cell size, min_points, the optional arrays that are absent) ----
THIN_CASES = {
    8: ((8, 8, 4), 0.25, 1, ()),
    12: ((16, 16, 16), 0.3, 1, ()),
    15: ((28, 28, 28), 1.7, 1, ()),
    16: ((40, 40, 40), 0.3, 1, ()),
    21: ((128, 128, 128), 0.25, 3, ()),
    24: ((256, 256, 256), 1.7, 1, ("normal", "pixel")),
    30: ((1 << 20, 1 << 10, 1), 0.3, 1, ()),
    40: ((1 << 20, 1 << 20, 1), 0.25, 1, ()),
    63: (((1 << 21) - 1,) * 3, 0.3, 1, ()),
}


def _frozen(arrays):
    for a in arrays.values():
        if a is not None:
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=1)   # (50 MB a case: a test asks for its own case's alone)
def thin_cloud(bits):
    """P0 points on the lattice of a quarter cell, so ties on cell borders abound; the first two points are opposite corners, so the
    bins are exactly the case's.  Where the grid has more cells than a quarter of the points, the points fall into that many cells
    drawn from it: about four members a cell at every key width, so the order of a cell's members (the sort's stability) shows in
    the sums.  Normals, views, pixels and counts as test_depth_points_thin.py's random clouds have them."""
    bins, h, _, absent = THIN_CASES[bits]
    rng = np.random.default_rng(7000 + bits)
    cells = bins[0] * bins[1] * bins[2]
    if cells <= P0 // 4:
        cell = np.stack([rng.integers(0, n, P0) for n in bins], axis=1)
    else:
        pool = np.stack([rng.integers(0, n, P0 // 4) for n in bins], axis=1)
        cell = pool[rng.integers(0, len(pool), P0)]
    lattice = 4 * cell + rng.integers(0, 4, (P0, 3))
    lattice[0] = 0
    lattice[1] = [4 * n - 1 for n in bins]
    xyz = lattice.astype(np.float64) * (h / 4)
    normal = rng.normal(size=(P0, 3)).astype(np.float32)
    normal /= np.linalg.norm(normal, axis=1, keepdims=True).astype(np.float32)
    normal[rng.random(P0) < 0.2] = 0.0
    view = np.sort(rng.integers(0, 12, P0)).astype(np.int32)
    pixel = rng.integers(0, 1 << 20, P0).astype(np.int32)
    count = rng.integers(0, 12, P0).astype(np.int32)
    cloud = dict(xyz=xyz, normal=normal, view=view, pixel=pixel, count=count)
    for name in absent:
        cloud[name] = None
    return _frozen(cloud)


@functools.lru_cache(maxsize=1)
def thinned(bits):
    """(arrays, report) of depth_points_thin_np.thin for the case."""
    _, h, min_points, _ = THIN_CASES[bits]
    cloud = thin_cloud(bits)
    arrays, report = T.thin(*(cloud[name] for name in INPUT_NAMES), cell_size=h, min_points=min_points)
    return _frozen(arrays), report


def thin_key_bits(bits):
    """key_bits of depth_points_thin_rules.h for the case's cloud, restated from the restatement's bins."""
    _, n = T.bins(thin_cloud(bits)["xyz"], THIN_CASES[bits][1])
    return (n[0] * n[1] * n[2] - 1).bit_length(), tuple(n)


# ---- the neighbour count ----
RADIUS = 0.3
SLACK = 1 + 2.0 ** -10       # radius_rules::kCellSlack
BASE_LATTICE = (120, 960, 960)   # quarter radii: a slab of 30 x 240 x 240 search cells, 57 600 rows of about 18 points
# key_bits of the search grid -> (the strays (X, 0, 0) and (0, Y, Z) in radii, min_neighbors)
RADIUS_CASES = {
    21: ((33.0, 243.0, 0.0), 1),
    24: ((250.0, 243.0, 0.0), 0),
    28: ((1300.0, 650.0, 0.0), 4),
    30: ((2600.0, 1300.0, 0.0), 1),
    40: ((80000.0, 40000.0, 0.0), 4),
    63: ((2.0e6, 2.0e6, 2.0e6), 0),
}
SMALL_POINTS = 270001
SMALL_LATTICE = (40, 1000, 1000)   # 10 x 250 x 250 search cells: 62 500 rows of about 4 points


def _lattice_cloud(seed, n_points, lattice):
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.integers(0, n, n_points) for n in lattice], axis=1).astype(np.float64) * (RADIUS / 4)
    xyz[0] = 0.0                                         # the corners: the extents are exactly the lattice's
    xyz[1] = (np.array(lattice) - 1) * (RADIUS / 4)
    xyz.setflags(write=False)
    return xyz


@functools.lru_cache(maxsize=None)
def radius_base():
    """P0 - 2 points on the lattice of a quarter radius: exact ties at the radius abound."""
    return _lattice_cloud(8000, P0 - 2, BASE_LATTICE)


@functools.lru_cache(maxsize=None)
def radius_base_counts():
    neighbors = B.count_neighbors(radius_base(), RADIUS)
    neighbors.setflags(write=False)
    return neighbors


@functools.lru_cache(maxsize=None)
def radius_small():
    return _lattice_cloud(8001, SMALL_POINTS, SMALL_LATTICE)


@functools.lru_cache(maxsize=None)
def radius_small_counts():
    neighbors = B.count_neighbors(radius_small(), RADIUS)
    neighbors.setflags(write=False)
    return neighbors


def radius_cloud(bits):
    """The base cloud followed by the case's two strays."""
    (x, y, z), _ = RADIUS_CASES[bits]
    return np.concatenate([radius_base(), np.array([[x, 0.0, 0.0], [0.0, y, z]]) * RADIUS])


def search_grid(xyz, radius=RADIUS):
    """(bins, key_bits, cell size) of the device's search grid (radius_rules::cell_size_of and bins_of_extent), for a cloud no
    axis of which reaches 2^21 bins: no cell is enlarged."""
    h = radius * SLACK
    extent = xyz.max(axis=0) - xyz.min(axis=0)
    n = [int(np.floor(e / h)) + 1 for e in extent]
    assert max(n) < 1 << 21
    return n, (n[0] * n[1] * n[2] - 1).bit_length(), h


def search_units(xyz, radius=RADIUS, group=64):
    """The work units of the count kernel (radius_rules::unit_head): runs of at most `group` points within a (b_1, b_2) row."""
    n, _, h = search_grid(xyz, radius)
    b = np.floor((xyz - xyz.min(axis=0)) / h).astype(np.int64)
    _, per_row = np.unique(b[:, 2] * n[1] + b[:, 1], return_counts=True)
    return int(((per_row + group - 1) // group).sum())


# ---- the chain on the resident view set ----
ROOM = dict(n=4, W=640, H=480, seed=1)
BUILD = dict(dedupe=False, abs_tolerance=0.0, rel_tolerance=0.02, min_views=0)
# name -> (radius, min_neighbors).  "counted": the counts stay below one wave's 64 and nothing is dropped -- no radius of this scene
# has both a maximum below 64 and more than 2^20 points with a neighbour (the cameras stand close to some walls and far from
# others: 951 952 points have a neighbour at 0.003, where the maximum is 63; at 0.0031 it is 65).  "dropped": 159 165 points go, more
# than 2^20 stay, and the densest point has 81 neighbours.
CHAIN_CASES = {"counted": (0.003, 0), "dropped": (0.0034, 1)}
CHAIN_CELLS = {"counted": (0.01, 2), "dropped": (0.005, 1)}   # name -> (cell size, min_points) of the thinning behind the filter
CHAIN_WAVE_CELL_POINTS = 8   # the view set's knob: tens of thousands of cells then go to the wave pass, which strides


@functools.lru_cache(maxsize=None)
def room_views():
    return scene.make_room_views(ROOM["n"], ROOM["W"], ROOM["H"], seed=ROOM["seed"])


@functools.lru_cache(maxsize=None)
def chain_built():
    views = room_views()
    model = ViewSetModel()
    model.add(views, None)
    arrays, report = P.build_points(model.depth, views.K4, views.RT4, **BUILD)
    return _frozen(arrays), report


@functools.lru_cache(maxsize=None)
def chain_counts(name):
    neighbors = B.count_neighbors(chain_built()[0]["xyz"], CHAIN_CASES[name][0])
    neighbors.setflags(write=False)
    return neighbors


@functools.lru_cache(maxsize=None)
def chain_filtered(name):
    cloud, _ = chain_built()
    neighbors = chain_counts(name)
    keep = neighbors >= CHAIN_CASES[name][1]
    arrays = {k: np.ascontiguousarray(cloud[k][keep]) for k in INPUT_NAMES}
    arrays["neighbors"] = neighbors[keep]
    return _frozen(arrays), R.report_of(neighbors, CHAIN_CASES[name][1])


@functools.lru_cache(maxsize=None)
def chain_thinned(name):
    cloud, _ = chain_filtered(name)
    cell_size, min_points = CHAIN_CELLS[name]
    arrays, report = T.thin(*(cloud[k] for k in INPUT_NAMES), cell_size=cell_size, min_points=min_points)
    return _frozen(arrays), report
