"""Sequences of calls on ONE capi.FusionContext against a replay by the oracle (tests/fusion_sequence_model.py).  The randomised
fusion tests elsewhere go through capi.fuse_once -- a fresh context, one add_views, one fuse, one download -- while a context
carries state whose only purpose is to skip work on LATER calls: the deferred zero fill of a reset, the per-layer "is zero" flags
that decide init_from_grid, "the grid holds no -0.0" (fusion_launch_rules.h: zero_free), the record tables that grow as a unit,
the views' hit counters that keep their counts across a growth, the promotion of the depth store to f64 in mid-life, the validity
of the point data, and the class / order / cz tables that are kept while they hold what is needed.  A wrong flag there gives a
wrong grid on the second or the fifth call of a context, never on the first.

A seeded generator (generate) yields a configuration -- scene, grid type, grid form, hit counters, ray potential, launch rules --
and 8-14 operations; the context runs them, the model replays them.  After every operation the generator marks "observe", and
always after the last, the downloaded grid (f64: bit for bit; f32: by value), download_hits() of a counting context and
info().n_views are compared with the model; at operations marked "points" download_point_data() is compared with
oracle.cell_to_point(model grid) too.  The generator, not the runner, decides where to look: a download flushes the deferred fill
and would hide what the deferral gets wrong.  fuse_download returns the grid, which is compared whenever it is called.

Shapes: 24 x 24 x 64 cells (two DMI_SLAB_ALIGNMENT units: the slabs (0, 32) and (32, 32)), axis-aligned or rotated; images of
40 x 24, after a clear_views sometimes 56 x 32; up to 140 views.  Scenes: the dense sphere (scene.make_views), and the speckle
scene of tests/test_fusion_context_reuse.py step 4 -- a best-cost threshold leaves a tenth of the pixels without a depth, every
depth moved 4 units back so that the whole grid lies in free space and the window column runs; where the launch rules allow
windows at all (no hit counters, an f32 depth store, every resident view thresholded, no uploaded grid, brick classes on) such a
sequence must show window_pair_count() > 0 at least once.  Depth storage AUTO; a batch whose depths lie one f64 ulp above f32
values promotes the store.  Half the seeds count hits; every seed runs with brick classes on (conftest.py), a quarter of them
once more under the shipped launch rules (helpers.shipped_defaults), which their first batch is sized for.

Batch sizes are steered towards the record tables' capacity (fusion_launch_rules.h: record_capacity, restated in one line
here and checked against the numbers of tests/cpp/fusion_launch_rules_host.cpp): some fuse of a sequence finds as many views as the
tables hold records, or one fewer, or one more.  At "as many" the window column's prefetch of the next view's record would
read past a table that was not grown; the rule grows it.

test_the_generator_covers_what_it_is_for (CPU) holds the generator to its purpose: every kind of operation in a fifth of the
sequences at least, a fuse at views == capacity in four, a promotion in three, and in EVERY sequence a fuse whose grid is read
by a later fuse with nothing looking at the grid in between.

SEEDS = 32.  Measured on an MI355X: the whole file (32 seeds, 8 of them once more under the shipped rules, 10 directed cases)
takes 4.4 s, the slowest case 0.49 s; the oracle replay of all 32 seeds alone takes about 5 s on one CPU thread, less on the
threads a test machine gives it."""
import functools

import numpy as np
import pytest

from cudadepthmapintegration_amd import capi, scene
from fusion_sequence_model import FusionSequenceModel, ModelRefusal, same_grid
from helpers import bits_equal, shipped_defaults

SEEDS = 32
DIMS = (24, 24, 64)
SMALL, LARGE = (40, 24), (56, 32)
POOL = {SMALL: 140, LARGE: 70}   # views a sequence may hold at each image size
KINDS = ("add", "fuse", "fuse_range", "fuse_slab", "fuse_download", "reset", "upload", "clear", "cell_to_point", "refused")
FUSES = ("fuse", "fuse_range", "fuse_slab", "fuse_download")
BRICKS_NEED_VIEWS = 48   # shipped rules: a launch of fewer views into this grid (72 bricks) runs without classes, so without windows


def record_capacity(n):
    return max(64, 2 * n)   # fusion_launch_rules.h: record_capacity


def records_held(held, n):
    """the records every table holds after a fuse finds n views and `held` records: kept while the window table holds n + 1"""
    return held if held >= n + 1 else record_capacity(n)


# ---- scenes -----------------------------------------------------------------------------------------------------------
RAYS = {"default": None, "thin": (0.05, 0.8, 0.03, 0.2), "thin_negative_eta": (0.05, 0.8, -0.2, 0.2)}


def _ray(name, grid):
    return scene.default_ray_potential(grid) if RAYS[name] is None else scene.RayPotential(*RAYS[name])


@functools.lru_cache(maxsize=None)
def _pool(kind, size):
    """(views with best-cost values, threshold) -- a sequence's resident views are always the first n of a pool"""
    n = POOL[size]
    if kind == "speckle":
        v, threshold = scene.make_scene_views("speckle", n, *size, seed=23, speckle=0.1)
        v.depth[...] = np.where(v.depth > 0, (v.depth + 4.0).astype(np.float32), v.depth)   # (f32 values still)
    else:
        v, threshold = scene.make_views(n, *size, seed=21, dense=True, with_best_cost=True), 0.9
    for a in (v.depth, v.K4, v.RT4, v.best_cost):
        a.setflags(write=False)
    return v, threshold


def _batch(kind, size, lo, hi, how):
    """views [lo, hi) of the pool as add_views takes them: how = plain (no threshold), thresholded, or inexact -- every depth one
    f64 ulp above its f32 value, which AUTO storage can only keep in an f64 store"""
    pool, threshold = _pool(kind, size)
    v = pool.subset(lo, hi)
    if how == "thresholded":
        return v, threshold
    depth = np.where(v.depth > 0, np.nextafter(v.depth, np.inf), v.depth) if how == "inexact" else v.depth
    return scene.Views(depth, v.K4, v.RT4, None), None


def _uploaded_grid(seed):
    rng = np.random.default_rng([int(seed), 5])
    g = rng.standard_normal(DIMS[::-1])
    what = rng.random(g.shape)
    g[what < 0.25] = -0.0
    g[what > 0.8] = 0.0
    return g


# ---- the generator ----------------------------------------------------------------------------------------------------
def config(seed):
    """The speckle scene keeps the axis-aligned grid (its sequences are for the window column); half the dense ones are rotated."""
    speckle = (seed // 4) % 2 == 1
    return dict(seed=seed, count_hits=seed % 2 == 1, grid_dtype="f32" if (seed // 2) % 2 else "f64", scene="speckle" if speckle else "dense",
                rotated=not speckle and (seed // 8) % 2 == 1, shipped=seed % 8 in (2, 5),
                ray=("default", "thin", "thin_negative_eta", "default")[(seed // 3) % 4])


class _Tracker:
    """What the generator must know of a sequence to steer it and to say what it covers (none of it is compared with the library)."""

    def __init__(self, cfg):
        self.cfg, self.size, self.hows, self.held = cfg, SMALL, [], 0
        self.uploaded = False   # since the last reset (or the context's creation)

    @property
    def n(self):
        return sum(h[1] for h in self.hows)

    def fused(self, op, count):
        """a fuse of `count` > 0 views reaches the launch: the record tables are brought to the resident views"""
        if self.held:
            op["views_minus_capacity"] = self.n - self.held
        self.held = records_held(self.held, self.n)
        c = self.cfg
        op["windows_possible"] = (c["scene"] == "speckle" and not c["count_hits"] and not c["rotated"] and not self.uploaded and
                                  all(h[0] == "thresholded" for h in self.hows) and (count >= BRICKS_NEED_VIEWS or not c["shipped"]))


def _unobserved_chain(ops):
    """a fuse whose grid a later fuse reads -- no reset or upload between them -- with nothing looking at the grid in between"""
    unseen = set()   # the halves of the grid (layers 0-31, 32-63) that hold a fuse's sums nobody has looked at
    for op in ops:
        halves = set()
        if op["kind"] in FUSES and op.get("count", 1) > 0:
            halves = {z0 // 32 for z0, _ in op["slabs"]} if op["kind"] == "fuse_slab" else {0, 1}
        if halves & unseen:
            return True
        if op["kind"] in ("reset", "upload"):
            unseen = set()
        unseen |= halves
        if op.get("observe") or op.get("points") or op["kind"] in ("fuse_download", "cell_to_point"):
            unseen = set()
    return False


def _generate(cfg, attempt):
    rng = np.random.default_rng([cfg["seed"], attempt, 20])
    t = _Tracker(cfg)
    n_ops = int(rng.integers(8, 15))
    ops = []

    def add(clear):
        if clear:
            t.size = LARGE if rng.random() < 0.5 else SMALL
            t.hows = []
        room = POOL[t.size] - t.n
        targets = [c for c in (t.held - 1, t.held, t.held + 1) if t.n < c <= POOL[t.size]] if t.held else []
        if targets and rng.random() < 0.7:
            k = int(rng.choice(targets)) - t.n
        else:
            k = int(rng.integers(1, min(room, 40) + 1))
        first_of_speckle = cfg["scene"] == "speckle" and not ops
        if first_of_speckle and cfg["shipped"]:
            k = max(k, BRICKS_NEED_VIEWS + int(rng.integers(0, 8)))
        how = "thresholded" if first_of_speckle else str(rng.choice(["plain", "thresholded", "inexact"], p=[0.4, 0.42, 0.18]))
        # (a promotion: an f32 store with views in it meets a batch it cannot hold)
        op = dict(kind="clear" if clear else "add", size=t.size, lo=t.n, hi=t.n + k, how=how,
                  promotes=how == "inexact" and t.n > 0 and not any(h[0] == "inexact" for h in t.hows))
        t.hows.append((how, k))
        return op

    def a_range():
        first = int(rng.integers(0, t.n))
        count = t.n - first if rng.random() < 0.4 else int(rng.integers(0, t.n - first + 1))
        return first, count

    weights = dict(add=2.0, fuse=2.0, fuse_range=1.6, fuse_slab=1.6, fuse_download=1.4, reset=1.3, upload=1.0, clear=0.9, cell_to_point=0.9, refused=1.0)
    while len(ops) < n_ops:
        if not ops:
            kind = "add"
        elif len(ops) == 1 and cfg["scene"] == "speckle":
            kind = str(rng.choice(["fuse", "fuse_slab"]))   # the window column's launch: before any upload, promotion or plain batch
        else:
            kind = str(rng.choice(KINDS, p=np.array([weights[k] for k in KINDS]) / sum(weights.values())))
        if kind == "add":
            if POOL[t.size] - t.n < 1:
                continue
            op = add(False)
        elif kind == "clear":
            op = add(True)
        elif kind == "fuse":
            op = dict(kind=kind)
            t.fused(op, t.n)
        elif kind == "fuse_range":
            first, count = a_range()
            op = dict(kind=kind, first=first, count=count)
            if count:
                t.fused(op, count)
        elif kind == "fuse_slab":
            op = dict(kind=kind, slabs=[[(0, 32)], [(32, 32)], [(0, 32), (32, 32)], [(32, 32), (0, 32)]][int(rng.integers(0, 4))])
            t.fused(op, t.n)
        elif kind == "fuse_download":
            first, count = a_range()
            if rng.random() < 0.25:
                count = 0
            op = dict(kind=kind, first=first, count=count, n_slabs=int(rng.integers(1, 3)))
            if count:
                t.fused(op, count)
        elif kind == "reset":
            op = dict(kind=kind, times=2 if rng.random() < 0.3 else 1)
            t.uploaded = False
        elif kind == "upload":
            op = dict(kind=kind, grid_seed=int(rng.integers(0, 1 << 30)))
            t.uploaded = True
        elif kind == "cell_to_point":
            op = dict(kind=kind)
        else:
            what = str(rng.choice(["range_past_the_end", "range_starts_past_the_end", "slab_off_alignment", "slab_past_the_grid"]))
            call = {"range_past_the_end": ("fuse", int(rng.integers(0, t.n)), 0), "range_starts_past_the_end": ("fuse", t.n + 1, 0),
                    "slab_off_alignment": ("fuse_slab", 16, 16), "slab_past_the_grid": ("fuse_slab", 32, 64)}[what]
            if what == "range_past_the_end":
                call = ("fuse", call[1], t.n - call[1] + 1)
            op = dict(kind=kind, call=call)
        op["observe"] = bool(rng.random() < 0.28)
        op["points"] = bool(rng.random() < 0.14)
        ops.append(op)
    ops[-1]["observe"] = True
    return ops


@functools.lru_cache(maxsize=None)
def generate(seed):
    cfg = config(seed)
    for attempt in range(200):
        ops = _generate(cfg, attempt)
        if _unobserved_chain(ops):
            return cfg, ops
    raise AssertionError(f"seed {seed}: no sequence with an unobserved fuse-to-fuse chain in 200 attempts")


# ---- the runner -------------------------------------------------------------------------------------------------------
def _compare(ctx, model, cfg, where, points):
    np_dtype = np.float64 if cfg["grid_dtype"] == "f64" else np.float32
    if points:   # first: the point data is then the reader that meets a deferred fill, not the download below
        assert bits_equal(ctx.download_point_data(), model.point_data()), (where, "point data")
    assert same_grid(ctx.download_grid(np_dtype), model), (where, "grid")
    assert int(ctx.info().n_views) == model.n_views, (where, "n_views")
    if cfg["count_hits"]:
        voxel_hits, map_hits = ctx.download_hits()
        assert np.array_equal(voxel_hits, model.voxel_hits), (where, "voxel hits")
        if model.map_hits_known:
            assert np.array_equal(map_hits, model.map_hits), (where, "view hits", map_hits, model.map_hits)


def run_sequence(cfg, ops, shipped=False):
    grid = scene.default_grid(DIMS, rotated=cfg["rotated"])
    ray = _ray(cfg["ray"], grid)
    model = FusionSequenceModel(grid, ray, grid_dtype=cfg["grid_dtype"], count_hits=cfg["count_hits"])
    np_dtype = np.float64 if cfg["grid_dtype"] == "f64" else np.float32
    options = dict(grid_dtype=cfg["grid_dtype"], count_hits=cfg["count_hits"], depth_storage="auto")
    if shipped:
        with shipped_defaults():
            ctx = capi.FusionContext(grid, ray, **options)
    else:
        ctx = capi.FusionContext(grid, ray, **options)
    window_pairs, windows_possible, inexact = [], False, False
    with ctx:
        for q, op in enumerate(ops):
            kind, where = op["kind"], (cfg["seed"], q, op["kind"])
            if kind in ("add", "clear"):
                if kind == "clear":
                    ctx.clear_views()
                    model.clear_views()
                    inexact = False
                views, threshold = _batch(cfg["scene"], op["size"], op["lo"], op["hi"], op["how"])
                ctx.add_views(views, threshold)
                model.add_views(views, threshold)
                inexact = inexact or op["how"] == "inexact"
                assert ctx.info().depth_storage_in_use == (capi.DMI_DEPTH_F64 if inexact else capi.DMI_DEPTH_F32), where
            elif kind == "fuse":
                ctx.fuse()
                model.fuse()
            elif kind == "fuse_range":
                ctx.fuse(op["first"], op["count"])
                model.fuse(op["first"], op["count"])
            elif kind == "fuse_slab":
                for z0, zc in op["slabs"]:
                    ctx.fuse_slab(z0, zc)
                    model.fuse_slab(z0, zc)
            elif kind == "fuse_download":
                got = ctx.fuse_download(op["first"], op["count"], dtype=np_dtype, n_slabs=op["n_slabs"])
                model.fuse_download(op["first"], op["count"])
                assert same_grid(got, model), (where, "the grid fuse_download returns")
            elif kind == "reset":
                for _ in range(op["times"]):
                    ctx.reset_grid()
                    model.reset_grid()
            elif kind == "upload":
                g = np.full(DIMS[::-1], -0.0) if op["grid_seed"] is None else _uploaded_grid(op["grid_seed"])
                ctx.upload_grid(g)
                model.upload_grid(g)
            elif kind == "cell_to_point":
                ctx.cell_to_point()
            else:
                name, a, b = op["call"]
                with pytest.raises(capi.DmiError):
                    getattr(ctx, name)(a, b)
                with pytest.raises(ModelRefusal):
                    getattr(model, name)(a, b)
            if op.get("windows_possible"):
                windows_possible = True
                window_pairs.append(ctx.window_pair_count())
            if op.get("observe") or op.get("points") or q == len(ops) - 1:
                _compare(ctx, model, cfg, where, op.get("points"))
    assert not windows_possible or max(window_pairs) > 0, (cfg["seed"], "the window column never ran", window_pairs)


# ---- the seeds --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(SEEDS))
def test_a_sequence_of_calls_is_its_replay(seed):
    run_sequence(*generate(seed))


SHIPPED_SEEDS = [seed for seed in range(SEEDS) if config(seed)["shipped"]]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SHIPPED_SEEDS)
def test_a_sequence_of_calls_is_its_replay_under_the_shipped_launch_rules(seed):
    """a quarter of the seeds once more, without conftest.py's "brick classes always": launches of fewer than 48 views into this
    grid take the zero row, the others the class tables -- a sequence crosses from one to the other as its views arrive"""
    run_sequence(*generate(seed), shipped=True)


def test_the_capacity_rule_restated_here_is_the_headers():
    """the numbers of tests/cpp/fusion_launch_rules_host.cpp (which checks csrc/fusion_launch_rules.h against them)"""
    want = {1: 64, 31: 64, 32: 64, 33: 66, 63: 126, 64: 128, 65: 130, 129: 258, 130: 260, 131: 262}
    assert {n: record_capacity(n) for n in want} == want
    # fuse at 32 views, then at 64: the 64 records held do not hold the window table's 65 -> grown; at 63 they do
    assert records_held(0, 32) == 64 and records_held(64, 63) == 64 and records_held(64, 64) == 128 and records_held(64, 65) == 130
    for a in range(1, 141):
        for b in range(a, 141):
            assert records_held(records_held(0, a), b) >= b + 1


def test_the_generator_covers_what_it_is_for():
    sequences = [generate(seed) for seed in range(SEEDS)]
    assert all(8 <= len(ops) <= 14 for _, ops in sequences)
    for kind in KINDS:
        with_kind = sum(any(op["kind"] == kind for op in ops) for _, ops in sequences)
        assert with_kind * 5 >= SEEDS, (kind, with_kind)
    at = {d: sum(any(op.get("views_minus_capacity") == d for op in ops) for _, ops in sequences) for d in (-1, 0, 1)}
    assert at[0] >= 4 and at[-1] >= 1 and at[1] >= 1, at
    promotions = sum(any(op.get("promotes") for op in ops) for _, ops in sequences)
    assert promotions >= 3, promotions
    assert all(_unobserved_chain(ops) for _, ops in sequences)
    for cfg, ops in sequences:
        if cfg["scene"] == "speckle" and not cfg["count_hits"] and not cfg["rotated"]:
            assert any(op.get("windows_possible") for op in ops), cfg
        assert max(op["hi"] for op in ops if "hi" in op) <= 140
    # both grid types, both grid forms, both scenes, with and without counters, and the shipped rules in a quarter
    for key, values in (("grid_dtype", {"f32", "f64"}), ("rotated", {False, True}), ("scene", {"dense", "speckle"}), ("count_hits", {False, True})):
        assert {cfg[key] for cfg, _ in sequences} == values
    assert sum(cfg["count_hits"] for cfg, _ in sequences) * 2 == SEEDS and sum(cfg["shipped"] for cfg, _ in sequences) * 4 == SEEDS
    assert sum(any(op["kind"] == "clear" and op["size"] == LARGE for op in ops) for _, ops in sequences) >= 3
    assert sum(any(op["kind"] == "reset" and op["times"] == 2 for op in ops) for _, ops in sequences) >= 3
    assert sum(any(op["kind"] == "fuse_download" and op["count"] == 0 for op in ops) for _, ops in sequences) >= 3


# ---- the directed sequences -------------------------------------------------------------------------------------------
def _cfg(**kw):
    cfg = dict(seed="directed", count_hits=False, grid_dtype="f64", scene="dense", rotated=False, shipped=False, ray="default")
    cfg.update(kw)
    return cfg


def _add(lo, hi, how="plain", size=SMALL, clear=False, **kw):
    return dict(kind="clear" if clear else "add", size=size, lo=lo, hi=hi, how=how, **kw)


def _fuse(**kw):
    return dict(kind="fuse", **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("grid_dtype", ["f64", "f32"])
def test_views_equal_to_the_record_capacity_through_the_window_column(grid_dtype):
    """add 32, fuse, add 32, fuse: 64 views find tables of 64 records, and the window column's last view prefetches record 64 -- the
    rule grows the tables to 128 first.  One more view; then 128 views, as many as the tables hold again, with persistent
    workgroups (96 views and more); then 130, what 65 views' growth would have held under the capacity alone."""
    ops = [_add(0, 32, "thresholded"), _fuse(windows_possible=True), _add(32, 64, "thresholded"), _fuse(windows_possible=True, observe=True),
           _add(64, 65, "thresholded"), _fuse(windows_possible=True), _add(65, 128, "thresholded"), _fuse(windows_possible=True, observe=True),
           _add(128, 130, "thresholded"), _fuse(windows_possible=True, observe=True, points=True)]
    run_sequence(_cfg(scene="speckle", grid_dtype=grid_dtype), ops)


@pytest.mark.gpu
@pytest.mark.parametrize("count_hits", [False, True])
def test_a_slab_after_a_reset_leaves_zeros_in_the_other_half(count_hits):
    """fuse, reset, fuse_slab(32, 32): the reset's fill is deferred, the slab writes its own layers only -- the lower half must read as
    zeros, not as the first fuse's sums."""
    ops = [_add(0, 20), _fuse(), dict(kind="reset", times=1), dict(kind="fuse_slab", slabs=[(32, 32)], observe=True),
           dict(kind="fuse_slab", slabs=[(0, 32)], observe=True, points=True)]
    run_sequence(_cfg(count_hits=count_hits), ops)


@pytest.mark.gpu
@pytest.mark.parametrize("ray", ["thin", "thin_negative_eta"])
def test_negative_zeros_come_and_go_with_uploads_and_resets(ray):
    """upload(-0.0), fuse(range), reset, fuse(range), upload(-0.0), fuse_slab: "the grid holds no -0.0" must be off, on, and off again
    -- a voxel far behind every surface, or missed by every view, keeps the -0.0 of an uploaded grid only if the +0.0 adds are
    really made.  (-0.0 everywhere: the uploaded grid, not _uploaded_grid's mixture.)"""
    minus = dict(kind="upload", grid_seed=None)
    ops = [_add(0, 50), minus, dict(kind="fuse_range", first=10, count=40, observe=True), dict(kind="reset", times=1),
           dict(kind="fuse_range", first=0, count=30), dict(kind="fuse_range", first=30, count=20, observe=True), minus,
           dict(kind="fuse_slab", slabs=[(32, 32), (0, 32)], observe=True)]
    run_sequence(_cfg(ray=ray), ops)


@pytest.mark.gpu
def test_a_refused_call_does_not_eat_the_pending_fill():
    """fuse, reset, a refused fuse and a refused slab, point data: zeros, through the second reader of the grid"""
    ops = [_add(0, 12), _fuse(), dict(kind="reset", times=1), dict(kind="refused", call=("fuse", 5, 8)),
           dict(kind="refused", call=("fuse_slab", 16, 16), points=True), dict(kind="fuse_range", first=2, count=10, observe=True, points=True)]
    run_sequence(_cfg(count_hits=True), ops)


@pytest.mark.gpu
def test_hit_counts_survive_views_added_past_the_counters():
    """fuse 40 views, add 30 more, read the hits before the next fuse: the views' counters hold 64 entries until a fusion grows them,
    and the download answered 70 views with zeros for all of them, the 40 counted ones included (found by seed 3)."""
    ops = [_add(0, 40), _fuse(), _add(40, 70, observe=True), _fuse(observe=True)]
    run_sequence(_cfg(count_hits=True), ops)


@pytest.mark.gpu
@pytest.mark.parametrize("grid_dtype", ["f64", "f32"])
def test_views_of_another_size_fuse_onto_the_fused_grid(grid_dtype):
    """fuse, point data, fuse again (the point data must follow), clear_views, views of 56 x 32 -- one batch of them inexact: the store
    is promoted --, fuse onto the fused grid, point data."""
    ops = [_add(0, 30, "thresholded"), _fuse(points=True), dict(kind="fuse_range", first=5, count=25, points=True),
           _add(0, 20, "plain", LARGE, clear=True), _add(20, 26, "inexact", LARGE), _fuse(observe=True, points=True)]
    run_sequence(_cfg(grid_dtype=grid_dtype, rotated=True), ops)
