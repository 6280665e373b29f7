"""The radius neighbour count of include/dmi.h (dmi_count_point_neighbors, dmi_views_filter_points_radius), restated
in numpy straight from the definition: brute force over all pairs, no grid.  Every operation is an f64 numpy operation of its own, so
each is rounded once and nothing is contracted."""
import numpy as np

REPORT_NAMES = ("points_in", "points_kept", "isolated", "max_neighbors", "neighbor_sum")   # distance_tests and kernel_ms are the device's
ROWS = 512   # queries per block of the pair matrix


def count_neighbors(xyz, radius):
    """neighbors uint32 [P]: steps 1 to 4."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    if not np.isfinite(xyz).all():
        raise ValueError("non-finite coordinate")
    radius = np.float64(radius)
    with np.errstate(over="ignore", under="ignore"):
        r2 = radius * radius
    if not (radius > 0 and np.isfinite(r2) and r2 >= np.finfo(np.float64).tiny):
        raise ValueError("radius")
    p = len(xyz)
    out = np.zeros(p, dtype=np.uint32)
    with np.errstate(over="ignore"):
        for first in range(0, p, ROWS):
            q = xyz[first:first + ROWS]
            d0 = xyz[None, :, 0] - q[:, None, 0]
            d1 = xyz[None, :, 1] - q[:, None, 1]
            d2 = xyz[None, :, 2] - q[:, None, 2]
            near = ((d0 * d0 + d1 * d1) + d2 * d2) <= r2
            rows = np.arange(len(q))
            near[rows, first + rows] = False   # never its own neighbour: by index
            out[first:first + ROWS] = near.sum(axis=1)
    return out


def filter_radius(arrays, radius, min_neighbors):
    """(arrays of the kept points with `neighbors` added, report): steps 5 to 7.  `arrays` is a dict with xyz and whatever else the
    cloud carries."""
    if min_neighbors < 0:
        raise ValueError("min_neighbors")
    neighbors = count_neighbors(arrays["xyz"], radius)
    keep = neighbors >= min_neighbors
    out = {name: np.ascontiguousarray(a[keep]) for name, a in arrays.items() if name != "neighbors"}
    out["neighbors"] = neighbors[keep]
    return out, report_of(neighbors, min_neighbors)


def report_of(neighbors, min_neighbors):
    return dict(points_in=len(neighbors), points_kept=int((neighbors >= min_neighbors).sum()), isolated=int((neighbors == 0).sum()),
                max_neighbors=int(neighbors.max()) if len(neighbors) else 0, neighbor_sum=int(neighbors.astype(np.uint64).sum()))
