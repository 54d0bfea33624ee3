"""Cost-to-go fields on the GPU (gvom_cost_to_go: k_ctg_seed, k_ctg_relax, k_ctg_dirs, k_travcost; DeviceMaps.cost_to_go,
Gvom.cost_to_go_of, Gvom.cost_to_go_of_device) against the referee of tests/costfield_ref.py: the field, the directions, the cost
map and the call's info with tolerance 0 -- everything is integer.  Synthetic maps on grids of 16, 31, 32, 33, 50, 64, 65, 100 and
129 cells (one partial tile; each side of the tile edges 16, 32, 64; ragged last tiles; exactly 2 x 2 tiles; 4 x 4 with a ragged
rim; 5 x 5 with a last tile one cell wide), 1024 cells (32 x 32 tiles) against Dijkstra and 4096 cells (128 x 128 tiles, the
largest map accepted) against a closed form and the Bellman check of tests/costfield_ref.py,
the obstacle scenes end to end through combine_maps_device() on rings of one and two slots, an early stop, snapshots, the product
pool, errors, and a torch consumer in a child process.  tests/test_costfield_cpu.py holds the census of every input.

Wall time on the MI355X (pytest --durations, one run): 129 cells 0.30 s (100 cells: 0.18 s); 1024 cells open / random / random_cut /
seventeen_goals 2.08 / 1.66 / 0.87 / 1.73 s (Dijkstra included; 33 / 49 / 35 / 29 rounds); 4096 cells open 1.90 s (129 rounds, 48,896
tile relaxations), random 9.77 s (171 rounds, 601,562 tile relaxations; about half of it is the Bellman check on the host)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import clearance_ref as cr
import costfield_ref as cf
import obstacle_scenes as ob

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = cf.UNREACHED


def _params(xy, res=0.4, buffer_size=1):
    return (res, 0.2, xy, 8, buffer_size, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)


@pytest.fixture(scope="module")
def gvom():
    import gvom as mod
    rc, info = mod.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    assert mod.PRODUCT_COSTFIELD == 7
    return mod


@pytest.fixture(scope="module")
def handles(gvom):
    return {xy: gvom.Gvom(*_params(xy), voxel_statistics=False) for xy in cf.SIZES}


class _Device(object):
    """int32 arrays in device memory through the HIP runtime the library is linked against"""

    def __init__(self):
        self.rt = ctypes.CDLL("libamdhip64.so")
        self.rt.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.rt.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.rt.hipFree.argtypes = [ctypes.c_void_p]
        self.held = []

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = ctypes.c_void_p()
        assert self.rt.hipMalloc(ctypes.byref(p), a.nbytes) == 0
        assert self.rt.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0           # host to device, blocking
        self.held.append(p)
        return p.value

    def free(self):
        for p in self.held:
            self.rt.hipFree(p)
        self.held = []


def _hold(f, c, D, d, info, what, converged=True):
    """a DeviceCostField against the referee: the three parts and the info, exactly"""
    with f:
        cost, direction, cell = f.copy_to_host()
    xy = D.shape[0]
    assert cost.dtype == np.int32 and direction.dtype == np.uint8 and cell.dtype == np.uint16, what
    assert cost.shape == direction.shape == cell.shape == (xy, xy) and cost.flags.f_contiguous and direction.flags.f_contiguous, what
    assert np.array_equal(cell, np.asarray(c)), "%s: the cost map differs in %d cells" % (what, int((cell != np.asarray(c)).sum()))
    if not np.array_equal(cost, D):
        bad = np.argwhere(cost != D)
        raise AssertionError("%s: the field differs in %d cells, first (%d, %d): got %d, referee %d" % (
            what, len(bad), bad[0][0], bad[0][1], cost[tuple(bad[0])], D[tuple(bad[0])]))
    if not np.array_equal(direction, d):
        bad = np.argwhere(direction != d)
        raise AssertionError("%s: the directions differ in %d cells, first (%d, %d): got %d, referee %d" % (
            what, len(bad), bad[0][0], bad[0][1], direction[tuple(bad[0])], d[tuple(bad[0])]))
    assert (f.converged, f.reached, f.goals_seeded) == (converged, info[0], info[1]), (what, f.converged, f.reached, f.goals_seeded, info)
    assert f.rounds >= 1, what
    return cost, direction


@pytest.mark.parametrize("xy", cf.SIZES)
def test_synthetic_maps_match_the_referee_exactly(handles, xy):
    g = handles[xy]
    rounds = {}
    for name, (c, goals, cap) in cf.patterns(xy).items():
        D, d, info = cf.expected(xy, name)
        f = g.cost_to_go_of(c, goals, max_cost=cap or None)
        assert f.cost.shape == (xy, xy) and f.cost.strides == f.direction.strides == f.cell_cost.strides == (1, xy), name
        rounds[name] = f.rounds
        _hold(f, c, D, d, info, "xy %d, %s" % (xy, name))
    if xy > 64:
        assert rounds["serpentine"] > rounds["open"]              # the wavefront crosses a tile boundary per corridor
    assert rounds["all_blocked"] == 1 and rounds["single_free_goal"] == 1


# ---- beyond 4 x 4 tiles: 1024 cells (32 x 32 tiles) and 4096 (128 x 128, the largest map the call accepts) ---------------------------
# 129 cells (5 x 5 tiles, the last one cell wide) run every pattern above, as a member of cf.SIZES.

@pytest.fixture(scope="module")
def large_handles(gvom):
    made = {}

    def get(xy):
        if xy not in made:
            made.clear()                                           # (one large mapper at a time)
            made[xy] = gvom.Gvom(0.4, 0.2, xy, 1, 1, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1, voxel_statistics=False)
        return made[xy]
    yield get
    made.clear()


@pytest.mark.parametrize("name", ["open", "random", "random_cut", "seventeen_goals"])
def test_1024_cells_match_dijkstra(large_handles, name):
    xy = 1024
    g = large_handles(xy)
    c, goals, cap, D, d, info = cf.large_expected(xy, name)
    f = g.cost_to_go_of(np.asfortranarray(c), goals, max_cost=cap or None)
    print(xy, name, "rounds", f.rounds, "tile relaxations", g.get_tuning("cost_to_go_tiles"))
    assert f.rounds >= (32 if name == "open" else 2)               # (open: from the corner goal the wavefront crosses the 32 tiles of a side, one a round)
    _hold(f, c, D, d, info, "xy %d, %s" % (xy, name))
    if name == "random_cut":
        full = cf.large_expected(xy, "random")[3]
        assert 0.25 * info[0] < ((full != U) & (D == U)).sum() < 3 * info[0]      # the cap cuts about half of the reachable cells off


def test_4096_cells_open_map_matches_the_closed_form(large_handles):
    """one goal in the corner of an all-ones map of 128 x 128 tiles: D = 14 min(dx, dy) + 10 |dx - dy| (cf.open_field, pinned to
    Dijkstra by tests/test_costfield_cpu.py); the far corner holds 14 * 4095"""
    xy = 4096
    g = large_handles(xy)
    c, goals = cf.large_patterns(xy)["open"]
    D = cf.open_field(xy)
    assert D[xy - 1, xy - 1] == 14 * (xy - 1) and D[xy - 1, 0] == 10 * (xy - 1)
    f = g.cost_to_go_of(np.asfortranarray(c), goals)
    print(xy, "open: rounds", f.rounds, "tile relaxations", g.get_tuning("cost_to_go_tiles"))
    assert f.rounds >= 128
    _hold(f, c, D, cf.directions(D, c), (xy * xy, 1), "xy 4096, open")


def test_4096_cells_random_map_passes_the_bellman_check(large_handles):
    """random costs, a quarter of the cells blocked, 128 x 128 tiles: the field is held to cf.bellman -- the conditions that make
    a field THE cost-to-go field, pinned to Dijkstra on the small maps -- and the directions, reached and goals_seeded to it"""
    xy = 4096
    g = large_handles(xy)
    c, goals = cf.large_patterns(xy)["random"]
    f = g.cost_to_go_of(np.asfortranarray(c), goals)
    print(xy, "random: rounds", f.rounds, "tile relaxations", g.get_tuning("cost_to_go_tiles"))
    with f:
        cost, direction, cell = f.copy_to_host()
    assert cost.dtype == np.int32 and cost.shape == direction.shape == cell.shape == (xy, xy)
    assert np.array_equal(cell, c)
    bad, d = cf.bellman(cost, c, goals)
    assert bad == {}, bad
    if not np.array_equal(direction, d):
        wrong = np.argwhere(direction != d)
        raise AssertionError("the directions differ in %d cells, first (%d, %d): got %d, referee %d" % (
            len(wrong), wrong[0][0], wrong[0][1], direction[tuple(wrong[0])], d[tuple(wrong[0])]))
    reached = int((cost != U).sum())
    assert (f.converged, f.reached, f.goals_seeded) == (True, reached, 1) and f.rounds >= 64
    assert 0.7 * xy * xy < reached < 0.76 * xy * xy                # (a quarter is blocked; the free cells percolate, a few pockets aside)
    assert not np.array_equal(cost, cost.T)


@pytest.mark.parametrize("xy", [33, 100])
def test_the_result_does_not_depend_on_inner_bound_or_batch(gvom, xy):
    """a tile that runs out of sweeps marks itself active again; a batch may end in the middle of the solve"""
    g = gvom.Gvom(*_params(xy), voxel_statistics=False)
    for inner, batch in (((1, 1),) if xy == 33 else ()) + ((3, 16), (7, 5)):
        g.set_tuning("cost_to_go_inner", inner)
        g.set_tuning("cost_to_go_batch", batch)
        for name in ("serpentine", "random", "walls_cut", "diagonal_wall"):
            c, goals, cap = cf.patterns(xy)[name]
            D, d, info = cf.expected(xy, name)
            _hold(g.cost_to_go_of(c, goals, max_cost=cap or None), c, D, d, info, "xy %d, %s, inner %d, batch %d" % (xy, name, inner, batch))
    assert g.get_tuning("cost_to_go_tiles") > 0


@pytest.mark.parametrize("xy", [31, 65])
def test_device_cost_maps_are_read_in_place_and_clamped(handles, xy):
    g, dev = handles[xy], _Device()
    try:
        for name in ("random", "diagonal_wall", "seventeen_goals"):
            c, goals, cap = cf.patterns(xy)[name]
            D, d, info = cf.expected(xy, name)
            ptr = dev.upload(np.asfortranarray(c).T)                   # cell (x, y) at [y * xy + x]
            _hold(g.cost_to_go_of_device(ptr, goals), c, D, d, info, "device, xy %d, %s" % (xy, name))
        c, goals, _ = cf.patterns(xy)["random"]
        wild = c.astype(np.int64)
        wild[c == 0] = -7
        wild[c > 60000] += 10 ** 6
        clamped = np.clip(wild, 0, 65535).astype(np.int32)
        assert (clamped == 65535).sum() > 10 and (wild < 0).sum() > 10
        D = cf.dijkstra(clamped, goals)
        ptr = dev.upload(np.asfortranarray(wild.astype(np.int32)).T)
        _hold(g.cost_to_go_of_device(ptr, goals), clamped, D, cf.directions(D, clamped), cf.info(D, clamped, goals), "clamped")
        # the same values in a HOST map are refused before anything is enqueued
        pid, bad = ctypes.c_int64(-1), np.asfortranarray(wild.astype(np.int32))
        gl = np.ascontiguousarray(goals, np.int32)
        rc = g._lib.gvom_cost_to_go(g._h, -1, None, bad.ctypes.data_as(ctypes.c_void_p), 0, gl.ctypes.data_as(ctypes.c_void_p), len(gl),
                                    0, 0, 0, ctypes.byref(pid), None)
        assert rc == -1 and pid.value == -1 and b"outside 0 .. 65535" in g._lib.gvom_last_error(g._h)
    finally:
        dev.free()


def test_memory_orders_and_integer_types(handles):
    g, xy = handles[50], 50
    c, goals, _ = cf.patterns(xy)["random"]
    D, d, info = cf.expected(xy, "random")
    assert not np.array_equal(D, D.T)                              # an [x, y] / [y, x] mix-up would show
    for name, a in (("fortran", np.asfortranarray(c)), ("int64", c.astype(np.int64)), ("uint16", c.astype(np.uint16)),
                    ("float", c.astype(np.float64)), ("view", np.ascontiguousarray(c.T).T)):
        _hold(g.cost_to_go_of(a, goals.astype(np.int64)), c, D, d, info, name)
    _hold(g.cost_to_go_of(c, tuple(goals[0])), c, D, d, info, "one goal as a pair")
    _hold(g.cost_to_go_of(c, goals, max_cost=2 ** 30), c, D, d, info, "max_cost 2^30")


def test_paths_follow_the_directions_to_a_goal(handles):
    g, xy = handles[100], 100
    for name in ("random", "seventeen_goals", "walls"):
        c, goals, _ = cf.patterns(xy)[name]
        D, _, _ = cf.expected(xy, name)
        f = g.cost_to_go_of(c, goals)
        reached = np.argwhere(D != U)
        rng = np.random.default_rng(5)
        seeded = {(int(x), int(y)) for x, y in goals if c[x, y] > 0}
        for x, y in reached[rng.choice(len(reached), 64, replace=False)]:
            path = f.path_from((x, y))
            assert path[0] == (x, y) and path[-1] in seeded, (name, x, y)
            assert cf.path_cost(path, c) == D[x, y], (name, x, y)
        bx, by = np.argwhere(D == U)[0]
        assert f.path_from((bx, by)) is None
        with pytest.raises(ValueError):
            f.path_from((xy, 0))
        f.release()


def test_an_early_stop_leaves_upper_bounds_and_a_second_call_finishes(gvom):
    xy = 100
    g = gvom.Gvom(*_params(xy), voxel_statistics=False)
    c, goals, _ = cf.patterns(xy)["serpentine"]
    D, d, info = cf.expected(xy, "serpentine")
    f = g.cost_to_go_of(c, goals, max_rounds=1)
    assert not f.converged and f.rounds == 1 and f.goals_seeded == 1
    cost, direction, cell = f.copy_to_host()
    finite = cost != U
    assert finite.any() and not finite[D == U].any() and (cost[finite] >= D[finite]).all() and f.reached == int(finite.sum()) < info[0]
    assert np.array_equal(cell, c) and ((direction < 8) | np.isin(direction, (cf.GOAL, cf.UNSETTLED, cf.NONE))).all()
    assert np.array_equal(direction == cf.NONE, ~finite) and np.array_equal(direction == cf.GOAL, cost == 0)
    if (direction == cf.UNSETTLED).any():
        x, y = np.argwhere(direction == cf.UNSETTLED)[0]
        with pytest.raises(RuntimeError, match="unsettled"):
            f.path_from((x, y))
    f.release()
    few = g.cost_to_go_of(c, goals, max_rounds=3)
    assert not few.converged and few.rounds == 3 and f.reached <= few.reached < info[0]
    few.release()
    _hold(g.cost_to_go_of(c, goals, max_rounds=0), c, D, d, info, "the same call to the end")
    done = g.cost_to_go_of(c, goals, max_rounds=10 ** 6)
    assert done.converged and done.rounds < 10 ** 6
    _hold(done, c, D, d, info, "a bound that is not reached")


def _scene(gvom, name):
    g = gvom.Gvom(*ob.params(name), voxel_statistics=False)
    for pc, ego in ob.scans(name):
        g.process_pointcloud(pc, ego)
    return g, np.array(ob.scans(name)[-1][1][:2])


@pytest.mark.parametrize("name", cf.SCENES)
def test_scenes_end_to_end_through_device_map_sets(gvom, name):
    """the cost map of the set's own maps (travcost on their host copies and on the clearance the existing clearance() returns) and
    the field on it, for every variant: no inflation / one cell / 2.5 cells x unknown free / blocked / priced, with soft and
    roughness weights; goals in world metres"""
    g, ego = _scene(gvom, name)
    res, xy = g.xy_resolution, g.xy_size
    goals_m = ego + np.array([(0.0, 0.0), (5.0, 3.1), (-6.0, -4.2), (2.2, -7.0), (-11.9, 11.9)])
    reached = []
    with g.combine_maps_device() as m:
        pos, neg, vis, rough = (a.copy_to_host() for a in (m.positive, m.negative, m.visibility, m.roughness))
        cells = cf.world_to_cells(goals_m, res, m.origin)
        assert ((cells >= 0) & (cells < xy)).all() and len({tuple(c) for c in cells}) == len(cells)
        for v in cf.VARIANTS:
            what = "%s %r" % (name, v)
            P = cf.variant_params(v, res, cr.max_cells2_of)
            with m.clearance(cf.SCENE_THRESHOLD, include_negative=v["include_negative"], max_distance=v["inflation_radius"]) as clr:
                d2 = clr.squared_cells.copy_to_host()
            c = cf.travcost(pos, neg, vis, rough, d2, P)
            D = cf.dijkstra(c, cells)
            f = m.cost_to_go(goals_m, density_threshold=cf.SCENE_THRESHOLD, roughness_range=cf.ROUGHNESS_RANGE, **v)
            _hold(f, c, D, cf.directions(D, c), cf.info(D, c, cells), what)
            reached.append(int((D != U).sum()))
        c = cf.travcost(pos, neg, vis, rough, None, dict(density_threshold=12.5, base=4))
        D = cf.dijkstra(c, cells[:2], 3000)
        f = m.cost_to_go(cells[:2], goals_in_cells=True, density_threshold=12.5, base=4, max_cost=3000)
        _hold(f, c, D, cf.directions(D, c), cf.info(D, c, cells[:2]), name + ", goals in cells, threshold 12.5, max_cost")
        assert 0 < (D != U).sum() < (c > 0).sum()
    assert min(reached[:6]) > 500 and len(set(reached)) >= 5, reached


def test_device_pointer_of_a_torch_style_cost_map_equals_the_host_route(gvom):
    """graded inflation is the caller's: a cost map built from the clearance product, handed over by device pointer"""
    g, ego = _scene(gvom, "one_round")
    dev = _Device()
    try:
        with g.combine_maps_device() as m:
            with m.clearance(cf.SCENE_THRESHOLD, max_distance=2.0) as clr:
                d2 = clr.squared_cells.copy_to_host()
        graded = np.where(d2 == 0, 0, 1 + 4000 // np.clip(d2, 1, 4000)).astype(np.int32)
        cells = cf.world_to_cells([ego], g.xy_resolution, m.origin)
        D = cf.dijkstra(graded, cells)
        want = (graded, D, cf.directions(D, graded), cf.info(D, graded, cells))
        a = g.cost_to_go_of(graded, cells)
        b = g.cost_to_go_of_device(dev.upload(np.asfortranarray(graded).T), cells)
        assert a.product_id != b.product_id and a.cost.ptr != b.cost.ptr
        _hold(a, *want, "host route")
        _hold(b, *want, "device route")
    finally:
        dev.free()


def test_a_cost_field_is_a_snapshot(gvom):
    name = "one_round"
    g = gvom.Gvom(*ob.params(name), voxel_statistics=False)
    scans = ob.scans(name)
    g.process_pointcloud(*scans[0])
    m = g.combine_maps_device()
    goal = [(32, 32)]
    held = m.cost_to_go(goal, goals_in_cells=True, soft_weight=10)
    m.release()
    before = held.copy_to_host()
    for pc, ego in scans[1:]:
        g.process_pointcloud(pc, ego)
        m = g.combine_maps_device()
        later = m.cost_to_go(goal, goals_in_cells=True, soft_weight=10)
        assert later.cost.ptr != held.cost.ptr
        now = later.copy_to_host()
        later.release()
        m.release()
    after = held.copy_to_host()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert not np.array_equal(now[0], after[0])                  # the map has moved on; the held product has not


def test_pool_capacity_reuse_and_no_allocation_in_steady_state(gvom):
    xy = 64
    g = gvom.Gvom(*_params(xy), voxel_statistics=False)
    assert g.get_tuning("cost_to_go") == 1 and g.get_tuning("cost_to_go_allocations") == 0
    c, goals, _ = cf.patterns(xy)["random"]
    want = (c,) + cf.expected(xy, "random")
    first = g.cost_to_go_of(c, goals)
    assert g.get_tuning("cost_to_go_allocations") == 3          # the product set, the work buffer, the host staging buffer
    assert g.get_tuning("device_product_sets") == 1 and g.get_tuning("device_map_sets") == 0
    ptr = first.cost.ptr
    first.release()
    for _ in range(3):                                         # released: everything is reused
        with g.cost_to_go_of(c, goals) as f:
            assert f.cost.ptr == ptr
            _hold(f, *want, "reused set")
    assert g.get_tuning("cost_to_go_allocations") == 3 and g.get_tuning("device_product_sets") == 1
    held = [g.cost_to_go_of(c, goals) for _ in range(4)]
    assert len({f.cost.ptr for f in held}) == 4 and g.get_tuning("device_product_sets") == 4
    with pytest.raises(gvom.GvomBackendError, match="all 4 device product sets of this kind"):
        g.cost_to_go_of(c, goals)
    pid, cc, gl = ctypes.c_int64(-1), np.asfortranarray(c), np.ascontiguousarray(goals, np.int32)
    rc = g._lib.gvom_cost_to_go(g._h, -1, None, cc.ctypes.data_as(ctypes.c_void_p), 0, gl.ctypes.data_as(ctypes.c_void_p), len(gl), 0, 0, 0,
                                ctypes.byref(pid), None)
    assert rc == -4 and pid.value == -1                        # GVOM_ERR_CAPACITY
    allocs = g.get_tuning("cost_to_go_allocations")
    assert allocs == 6
    held[2].release()
    with g.cost_to_go_of(c, goals) as f:
        _hold(f, *want, "after a release")
    assert g.get_tuning("device_product_sets") == 4 and g.get_tuning("cost_to_go_allocations") == allocs
    for k in (0, 1, 3):                                        # (the set of held[2] has been handed out again: its id is stale)
        _hold(held[k], *want, "held")
    with pytest.raises(gvom.GvomBackendError, match="unknown or stale device product id"):
        held[2].copy_to_host()
    # a clearance product of the same handle lives in the same pool, under its own kind
    g.clearance_of(c).release()
    assert g.get_tuning("device_product_sets") == 5


def test_errors(gvom):
    name = "one_round"
    g = gvom.Gvom(*ob.params(name), voxel_statistics=False)
    xy = g.xy_size
    cost = np.ones((xy, xy), np.int32, order="F")
    cp = cost.ctypes.data_as(ctypes.c_void_p)
    goal = np.array([[3, 4]], np.int32)
    gp = goal.ctypes.data_as(ctypes.c_void_p)
    pid = ctypes.c_int64(-1)
    P = gvom.GvomCtgParams(50.0, 0.0, 0.0, 0, 1, 0, 0, 0)

    def raw(set_id=-1, params=None, c=cp, goals=gp, n=1, max_cost=0, max_rounds=0, flags=0, out=pid):
        return g._check(g._lib.gvom_cost_to_go(g._h, set_id, ctypes.byref(params) if params is not None else None, c, 0, goals, n, max_cost,
                                               max_rounds, flags, ctypes.byref(out) if out is not None else None, None))
    assert raw() == 0
    g._check(g._lib.gvom_device_product_export(g._h, pid.value, 0, ctypes.c_void_p(gvom._STREAM_NOSYNC), ctypes.byref(ctypes.c_void_p()),
                                               ctypes.byref(ctypes.c_int32()), (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()))
    g._check(g._lib.gvom_device_product_release(g._h, pid.value, ctypes.c_void_p(gvom._STREAM_NOSYNC)))
    for kw, word in ((dict(set_id=10 ** 9, params=P, c=None), "unknown or stale device map set id"), (dict(set_id=1, params=P), "not both"),
                     (dict(c=None), "a map set id or a cost map"), (dict(set_id=1, c=None), "a map set id or a cost map|needs the cost parameters"),
                     (dict(goals=None), "goals"), (dict(n=0), "goals"), (dict(n=65537), "goals"), (dict(max_cost=-1), "max_cost"),
                     (dict(max_cost=2 ** 30 + 1), "max_cost"), (dict(max_rounds=-1), "max_rounds"), (dict(flags=4), "unknown flag bits")):
        with pytest.raises(gvom.GvomBackendError, match=word):
            raw(**kw)
    assert g._lib.gvom_cost_to_go(g._h, -1, None, cp, 0, gp, 1, 0, 0, 0, None, None) == gvom.GVOM_ERR_INVALID        # NULL product_id
    for bad in ((xy, 0), (0, xy), (-1, 5), (5, -1)):
        out = np.array([[3, 4], bad], np.int32)
        with pytest.raises(gvom.GvomBackendError, match="outside the window"):
            raw(goals=out.ctypes.data_as(ctypes.c_void_p), n=2)
    with pytest.raises(gvom.GvomBackendError, match="gvom_cost_to_go"):
        g._device_product(gvom.PRODUCT_COSTFIELD)
    sets = g.get_tuning("device_product_sets")
    assert sets == 1
    scans = ob.scans(name)
    g.process_pointcloud(*scans[0])
    m = g.combine_maps_device()
    old = m.set_id
    for field, value in (("density_threshold", float("nan")), ("base", 0), ("soft_weight", -1), ("soft_weight", 65536), ("unknown_cost", 65536),
                         ("rough_weight", 65536), ("inflation_cells2", -1)):
        bad = gvom.GvomCtgParams(50.0, 0.0, 0.0, 0, 1, 0, 0, 0)
        setattr(bad, field, value)
        with pytest.raises(gvom.GvomBackendError, match="bad cost parameters"):
            raw(set_id=old, params=bad, c=None)
    for lo, hi in ((0.0, 0.0), (1.0, 0.0), (float("-inf"), 0.0), (0.0, float("nan"))):
        with pytest.raises(gvom.GvomBackendError, match="bad cost parameters"):
            raw(set_id=old, params=gvom.GvomCtgParams(50.0, lo, hi, 0, 1, 0, 0, 1), c=None)
    assert raw(set_id=old, params=gvom.GvomCtgParams(50.0, 1.0, 0.0, 0, 1, 0, 0, 0), c=None) == 0      # (the range is not read without a weight)
    m.cost_to_go([(3, 4)], goals_in_cells=True).release()
    m.release()
    g.process_pointcloud(*scans[1])
    g.combine_maps_device().release()                           # the unheld set was recycled: its id is stale
    with pytest.raises(gvom.GvomBackendError, match="unknown or stale device map set id"):
        raw(set_id=old, params=P, c=None)
    assert g.get_tuning("device_product_sets") == sets
    sharded = gvom.Gvom(*_params(64), voxel_statistics=False, _shard=(0, 2))
    with pytest.raises(gvom.GvomBackendError, match="sharded handles are not supported"):
        sharded.cost_to_go_of(np.ones((64, 64), np.int32), [(1, 1)])


def test_maps_of_more_than_4096_cells_a_side_are_refused(gvom):
    xy = 4100
    g = gvom.Gvom(0.4, 0.2, xy, 1, 1, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1, voxel_statistics=False)
    cost = np.ones((xy, xy), np.int32, order="F")
    goal, pid = np.array([[3, 4]], np.int32), ctypes.c_int64(-1)
    rc = g._lib.gvom_cost_to_go(g._h, -1, None, cost.ctypes.data_as(ctypes.c_void_p), 0, goal.ctypes.data_as(ctypes.c_void_p), 1, 0, 0, 0,
                                ctypes.byref(pid), None)
    assert rc == -4 and pid.value == -1 and b"4096" in g._lib.gvom_last_error(g._h)
    assert g.get_tuning("cost_to_go_allocations") == 0


def _torch_case(name):
    """One case per fresh child process that imports torch BEFORE the library is loaded (one HIP runtime in the process)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_costfield_torch.py"), name],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "CASE OK " + name in r.stdout, r.stdout[-4000:]


def test_dlpack_zero_copy_through_torch():
    _torch_case("zero_copy")


def test_consumer_gathers_directions_on_its_own_stream():
    _torch_case("consumer_stream")
