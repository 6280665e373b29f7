"""A model of the resident view set made of the context-free calls: it keeps the depths on the host, runs every step
through capi.filter_depth_speckles / fill_depth_holes / smooth_depths / filter_depth_consistency / estimate_scene_bounds with no
best costs, and counts the step's report with numpy from the arrays those calls return -- what include/dmi.h says a dmi_view_set
must reproduce byte for byte.  In the manner of fusion_sequence_model.py: the tests replay one sequence on both and compare after
every step."""
import numpy as np

from cudadepthmapintegration_amd import capi, scene

STEP_CALLS = {"speckles": capi.filter_depth_speckles, "holes": capi.fill_depth_holes, "smooth": capi.smooth_depths,
              "consistency": capi.filter_depth_consistency}


def normalised(depth, best_cost=None, threshold=None):
    """What dmi_views_add stores: the depth where it is valid and its cost does not exceed the threshold, -1 elsewhere."""
    d = np.asarray(depth, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        keep = (d > 0.0) & (d < np.inf)
        if best_cost is not None and threshold is not None:
            keep &= ~(np.asarray(best_cost, dtype=np.float64) > threshold)
    return np.where(keep, d, -1.0)


def groups_of_sizes(size, select=None):
    """A group of s pixels shows s times among the sizes: the pixels of size s, over s, are the groups of that size."""
    s = size[(size > 0) if select is None else (size > 0) & select]
    values, pixels = np.unique(s, return_counts=True)
    assert np.all(pixels % values == 0)
    return int((pixels // values).sum())


def step_report(name, params, before, after, aux):
    """include/dmi.h's table, from the arrays of the context-free call."""
    r = dict(valid_before=int((before > 0).sum()), valid_after=int((after > 0).sum()), changed=int((before != after).sum()),
             groups=0, groups_kept=0, aux_sum=0)
    if name == "speckles":
        r["groups"], r["groups_kept"] = groups_of_sizes(aux), groups_of_sizes(aux, aux >= params["min_pixels"])
    elif name == "holes":
        r["groups"], r["groups_kept"] = groups_of_sizes(aux), groups_of_sizes(aux, after != -1.0)
    elif name == "smooth":
        r["aux_sum"] = int(aux[after > 0].astype(np.int64).sum())
    return r


class ViewSetModel:
    def __init__(self, device=0):
        self.device = device
        self.depth = self.K4 = self.RT4 = None

    def add(self, views, threshold=None):
        d = normalised(views.depth, views.best_cost, threshold)
        k, rt = np.asarray(views.K4, dtype=np.float64), np.asarray(views.RT4, dtype=np.float64)
        if self.depth is None:
            self.depth, self.K4, self.RT4 = d, k.copy(), rt.copy()
        else:
            self.depth = np.concatenate([self.depth, d])
            self.K4, self.RT4 = np.concatenate([self.K4, k]), np.concatenate([self.RT4, rt])

    def views(self):
        return scene.Views(self.depth, self.K4, self.RT4, None)

    def step(self, name, params):
        """Runs the step; returns (report, aux)."""
        out, aux, ms = STEP_CALLS[name](self.views(), device=self.device, **params)
        report = step_report(name, params, self.depth, out.depth, aux)
        self.depth = out.depth
        return report, aux

    def bounds(self, params):
        lo, hi, count, ms = capi.estimate_scene_bounds(self.views(), device=self.device, **params)
        return lo, hi, count
