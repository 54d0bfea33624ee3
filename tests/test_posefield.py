"""Pose fields on the GPU (gvom_pose_field: k_cspace, k_pose_seed, k_pose_relax, k_pose_actions; DeviceCostField.pose_field,
Gvom.pose_field_of, Gvom.pose_field_of_device, Gvom.set_primitives) against the referee of tests/posefield_ref.py: the pose cost
volume, the field, the actions and the call's info with tolerance 0 -- everything is integer.  The cases of posefield_ref.cases()
(grids on each side of the solver's 8-cell tile edge, ragged and one-cell last tiles, H = 1 .. 64, halos 1, 3 and 4, footprints of
1 cell, 65 cells and a car, random and arc tables, inner bounds and batch sizes, a cap), the shipped 2-D solver as a degenerate
case, the rollout kernel's pose cost, 256 cells x 16 headings against the Bellman check, the obstacle scenes end to end on rings of
one and two slots, an early stop, snapshots, the product pool, errors, paths, and a torch consumer in a child process.
tests/test_posefield_cpu.py holds the census of every input.

Wall time on the MI355X (pytest --durations, one run): the torch child 2.4 s, every other test 0.25 s or less (256 cells x 16 headings:
0.19 s, 36 rounds, 11,631 tile relaxations); the file 4.4 s."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import costfield_ref as cf
import obstacle_scenes as ob
import posefield_ref as ref
import rollouts_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = ref.UNREACHED


def _params(xy, res=0.5, buffer_size=1):
    return (res, 0.2, xy, 8, buffer_size, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)


@pytest.fixture(scope="module")
def gvom():
    import gvom as mod
    rc, info = mod.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    assert mod.PRODUCT_POSEFIELD == 20
    return mod


class _Device(object):
    """arrays in device memory through the HIP runtime the library is linked against"""

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


def _mapper(gvom, q, res=0.5):
    g = gvom.Gvom(*_params(q["xy"], res), voxel_statistics=False)
    g.set_footprint(q["footprint"])
    g.set_primitives(q["table"])
    return g


def _hold(f, want, what, release=True):
    """a DevicePoseField against the referee's (C, D, action, seeds, info): the three volumes and the info, exactly"""
    C, D, A, seeds, info = want
    cost, action, pose_cost = f.copy_to_host()
    print(what, "rounds", f.rounds, "reached", f.reached, "seeded", f.goals_seeded)
    assert cost.dtype == np.int32 and action.dtype == np.uint8 and pose_cost.dtype == np.uint16, what
    assert cost.shape == action.shape == pose_cost.shape == D.shape and f.cost.shape == D.shape, what
    H, xy, _ = D.shape
    assert f.cost.strides == f.action.strides == f.pose_cost.strides == (xy * xy, 1, xy), what
    assert np.array_equal(pose_cost, C), "%s: the pose cost volume differs in %d states" % (what, int((pose_cost != C).sum()))
    if not np.array_equal(cost, D):
        bad = np.argwhere(cost != D)
        h, x, y = bad[0]
        raise AssertionError("%s: the field differs in %d states, first at h %d cell (%d, %d): %d, the referee has %d"
                             % (what, len(bad), h, x, y, cost[h, x, y], D[h, x, y]))
    assert np.array_equal(action, A), "%s: the actions differ in %d states" % (what, int((action != A).sum()))
    assert f.converged and f.rounds >= 1 and (f.reached, f.goals_seeded) == info, (what, f.converged, f.rounds, f.reached, f.goals_seeded, info)
    if release:
        f.release()


@pytest.mark.parametrize("i", range(len(ref.cases())), ids=[q["name"].replace(" ", "_") for q in ref.cases()])
def test_cases_match_the_referee_exactly(gvom, i):
    q = ref.cases()[i]
    g = _mapper(gvom, q)
    assert g.get_tuning("pose_field") == 1 and g.get_tuning("primitives") == 1
    g.set_tuning("pose_field_inner", q["inner"])
    g.set_tuning("pose_field_batch", q["batch"])
    goals = ref.goals_for_binding(q["goals"], q["H"])
    _hold(g.pose_field_of(q["c"], goals, max_cost=q["max_cost"]), ref.expected(i), q["name"])
    assert g.get_tuning("pose_field_tiles") > 0 and g.get_tuning("pose_field_rounds") >= 1
    dev = _Device()
    try:                                            # the same map in device memory, int32 [y][x], read in place
        ptr = dev.upload(np.asfortranarray(q["c"].astype(np.int32)).T)
        _hold(g.pose_field_of_device(ptr, goals, max_cost=q["max_cost"]), ref.expected(i), q["name"] + ", device route")
    finally:
        dev.free()


def test_the_result_does_not_depend_on_inner_bound_or_batch(gvom):
    i = [k for k, q in enumerate(ref.cases()) if q["name"].startswith("xy20 H16 point arcs")][0]
    q = ref.cases()[i]
    g = _mapper(gvom, q)
    goals = ref.goals_for_binding(q["goals"], q["H"])
    rounds = []
    for inner, batch in ((1, 1), (3, 5), (1, 16), (0, 0)):
        g.set_tuning("pose_field_inner", inner)
        g.set_tuning("pose_field_batch", batch)
        assert (g.get_tuning("pose_field_inner"), g.get_tuning("pose_field_batch")) == (inner, batch)
        f = g.pose_field_of(q["c"], goals)
        rounds.append(f.rounds)
        _hold(f, ref.expected(i), "inner %d batch %d" % (inner, batch))
    assert rounds[0] > rounds[-1]                    # one sweep a round takes more rounds to the same field


def test_one_heading_and_eight_steps_are_the_shipped_solver(gvom):
    """H = 1, a one-cell footprint and the eight steps in CTG_STEPS order with w = 5 and 7 on a map without a blocked cell (the 2-D
    solver's corner rule then never applies): the same field, and the same first steps but for the goal code"""
    xy = 33
    rng = np.random.default_rng(5)
    c = rng.integers(1, 3000, (xy, xy)).astype(np.uint16)
    g = gvom.Gvom(*_params(xy), voxel_statistics=False)
    g.set_footprint(ref.point_footprint(1))
    g.set_primitives(ref.steps_table())
    goals = [(4, 29), (30, 2)]
    with g.cost_to_go_of(c, goals) as two, g.pose_field_of(c, goals) as three:
        D2, d2, _ = two.copy_to_host()
        D3, a3, C3 = three.copy_to_host()
    assert np.array_equal(C3[0], c) and np.array_equal(D3[0], D2)
    assert np.array_equal(a3[0], np.where(d2 == gvom.CTG_GOAL, gvom.POSE_GOAL, d2))
    assert (d2 == gvom.CTG_GOAL).sum() == 2 and (D2 < U).all()


def test_the_pose_cost_volume_is_what_the_rollout_kernel_computes(gvom):
    """two kernels held against each other: k_cspace and k_rollouts at the cell centres with yaw 2 pi h / H"""
    i = [k for k, q in enumerate(ref.cases()) if q["name"] == "xy40 H16 car arcs random"][0]
    q = ref.cases()[i]
    g = _mapper(gvom, q)
    xy, H = q["xy"], q["H"]
    with g.pose_field_of(q["c"], q["goals"][:, :2]) as f, g.score_rollouts_of(q["c"], ref.centre_poses(xy, H, g.xy_resolution)) as r:
        C = f.pose_cost.copy_to_host()
        _, pc = r.copy_to_host()
    assert np.array_equal(C, pc.reshape(H, xy, xy)) and np.array_equal(C, ref.expected(i)[0])
    assert 0 < (C == 0).sum() < C.size


def test_256_cells_and_16_headings_pass_the_bellman_check(gvom):
    xy, H = 256, 16
    car = gvom.rectangle_footprint(xy_resolution=ref.CAR_RES, headings=H, **ref.CAR)
    table = gvom.arc_primitives(H, 3.0, ref.CAR_RES, reach=3, reverse_weight=3.0)
    c = ref.cost_map(xy, 21, zeros=0.003)
    goals = np.array([(200, 40, -1), (30, 220, -1), (128, 128, -1)], np.int32)
    g = gvom.Gvom(*_params(xy), voxel_statistics=False)
    g.set_footprint(car)
    g.set_primitives(table)
    with g.pose_field_of(c, goals[:, :2]) as f:
        D, A, C = f.copy_to_host()
        info = (f.converged, f.reached, f.goals_seeded)
        print("256 x 16: rounds", f.rounds, "tile relaxations", g.get_tuning("pose_field_tiles"), "reached", f.reached)
    want_C = ref.volume(c, car)
    seeds = ref.seed_mask(want_C, goals)
    assert np.array_equal(C, want_C)
    assert ref.bellman_violations(want_C, table, D, seeds) == 0
    assert np.array_equal(A, ref.actions(want_C, table, D, seeds))
    assert info == (True, int((D < U).sum()), int(seeds.sum())) and seeds.sum() > 0
    assert (D < U).sum() > 0.2 * D.size and ((want_C != 0) & (D == U)).sum() > 0


def test_an_early_stop_leaves_upper_bounds_and_a_second_call_finishes(gvom):
    i = [k for k, q in enumerate(ref.cases()) if q["name"] == "xy40 H16 car arcs random"][0]
    q = ref.cases()[i]
    g = _mapper(gvom, q)
    g.set_tuning("pose_field_inner", 2)
    goals = ref.goals_for_binding(q["goals"], q["H"])
    C, D, A, seeds, info = ref.expected(i)
    with g.pose_field_of(q["c"], goals, max_rounds=3) as f:
        cost, action, _ = f.copy_to_host()
        assert not f.converged and f.rounds == 3 and f.goals_seeded == info[1]
    finite = cost < U
    assert finite.sum() > seeds.sum() and (cost[finite] >= D[finite]).all() and (D[finite] < U).all() and (cost != D).any()
    assert (cost[seeds] == 0).all() and set(np.unique(action[~finite])) == {ref.NONE}
    assert ((action == ref.UNSETTLED) | (action == ref.GOAL) | (action < 3))[finite].all()
    _hold(g.pose_field_of(q["c"], goals), ref.expected(i), "after the early stop")


def _scene(gvom, name):
    g = gvom.Gvom(*ob.params(name), voxel_statistics=False)
    for pc, ego in ob.scans(name):
        g.process_pointcloud(pc, ego)
    return g, np.array(ob.scans(name)[-1][1][:2])


@pytest.mark.parametrize("name", cf.SCENES)
def test_scenes_end_to_end_through_device_map_sets(gvom, name):
    """combine_maps_device() -> cost_to_go() without inflation -> pose_field(), after the ego has moved; goals in world metres with a yaw"""
    g, ego = _scene(gvom, name)
    H = 16
    car = gvom.rectangle_footprint(xy_resolution=g.xy_resolution, headings=H, front=1.6, rear=0.6, half_width=0.5)
    table = gvom.arc_primitives(H, 2.0, g.xy_resolution, reach=3, reverse_weight=2.0)
    g.set_footprint(car)
    g.set_primitives(table)
    goals_m = np.concatenate([ego + np.array([(0.0, 0.0), (5.0, 3.1), (-6.0, -4.2)]), [[0.0], [math.pi / 2], [-2.0]]], axis=1)
    with g.combine_maps_device() as m:
        assert np.abs(m.origin[:2]).max() > 0                                         # the window has moved with the ego
        with m.cost_to_go(goals_m[:, :2], density_threshold=cf.SCENE_THRESHOLD, soft_weight=3) as field:
            c = field.cell_cost.copy_to_host()
            f = field.pose_field(goals_m)
            cells = gvom._pose_goals(goals_m, g.xy_size, H, (g.xy_resolution, m.origin))
    assert cells[:, 2].tolist() == [0, 4, 11] and (f.origin == m.origin).all()
    C = ref.volume(c, car)
    seeds = ref.seed_mask(C, cells)
    D = ref.relax(C, table, seeds)
    _hold(f, (C, D, ref.actions(C, table, D, seeds), seeds, (int((D < U).sum()), int(seeds.sum()))), name)
    assert (D < U).sum() > 2000 and ((C == 0) & (c != 0)[None]).sum() > 1000


def test_a_pose_field_is_a_snapshot(gvom):
    i = 1
    q = ref.cases()[i]
    g = _mapper(gvom, q)
    goals = ref.goals_for_binding(q["goals"], q["H"])
    held = g.pose_field_of(q["c"], goals)
    before = held.copy_to_host()
    g.set_primitives(ref.random_table(q["H"], 2, 77))
    g.set_footprint(rollouts_ref.patch_table(q["H"], 5))
    other = g.pose_field_of(np.ascontiguousarray(q["c"][::-1]), goals)
    assert other.cost.ptr != held.cost.ptr and not np.array_equal(other.copy_to_host()[0], before[0])
    other.release()
    g.process_pointcloud(np.zeros((10, 3), np.float32) + 1.5, (0.0, 0.0, 0.0))
    g.combine_maps()
    assert all(np.array_equal(a, b) for a, b in zip(before, held.copy_to_host()))
    _hold(held, ref.expected(i), "held across set_primitives, set_footprint, a scan and a combine", release=False)
    assert held.path_from(*[int(v) for v in np.argwhere(ref.expected(i)[1] == 0)[0][[1, 2, 0]]]) is not None      # (its own table, not the new one)
    held.release()


def test_pool_capacity_reuse_and_no_allocation_in_steady_state(gvom):
    i = 4
    q = ref.cases()[i]
    g = gvom.Gvom(*_params(q["xy"]), voxel_statistics=False)
    assert g.get_tuning("pose_field_allocations") == 0
    g.set_footprint(q["footprint"])
    g.set_primitives(q["table"])
    assert g.get_tuning("pose_field_allocations") == 1           # the table
    goals = ref.goals_for_binding(q["goals"], q["H"])
    first = g.pose_field_of(q["c"], goals)
    assert g.get_tuning("pose_field_allocations") == 4           # + the product set, the work buffer, the host staging buffer
    ptr = first.cost.ptr
    first.release()
    for _ in range(3):                                           # released: everything is reused
        g.set_primitives(q["table"])
        with g.pose_field_of(q["c"], goals) as f:
            assert f.cost.ptr == ptr
    assert g.get_tuning("pose_field_allocations") == 4 and g.get_tuning("device_product_sets") == 1
    held = [g.pose_field_of(q["c"], goals) for _ in range(4)]
    assert len({f.cost.ptr for f in held}) == 4 and g.get_tuning("device_product_sets") == 4
    with pytest.raises(gvom.GvomBackendError, match="all 4 device product sets of this kind"):
        g.pose_field_of(q["c"], goals)
    allocs = g.get_tuning("pose_field_allocations")
    assert allocs == 7
    held[2].release()
    _hold(g.pose_field_of(q["c"], goals), ref.expected(i), "after a release")
    assert g.get_tuning("device_product_sets") == 4 and g.get_tuning("pose_field_allocations") == allocs
    for k in (0, 1, 3):
        _hold(held[k], ref.expected(i), "held")
    with pytest.raises(gvom.GvomBackendError, match="unknown or stale device product id"):
        held[2].copy_to_host()


def test_errors(gvom):
    xy, H = 20, 8
    g = gvom.Gvom(*_params(xy), voxel_statistics=False)
    c = np.full((xy, xy), 3, np.uint16)
    table = ref.random_table(H, 3, 1, most=5)
    with pytest.raises(ValueError, match="no primitive table"):
        g.pose_field_of(c, [(1, 1)])
    g.set_primitives(table)
    with pytest.raises(ValueError, match="no footprint table"):
        g.pose_field_of(c, [(1, 1)])
    g.set_footprint(ref.point_footprint(4))
    with pytest.raises(ValueError, match="another number of headings"):
        g.pose_field_of(c, [(1, 1)])
    g.set_footprint(rollouts_ref.patch_table(65, 3))
    with pytest.raises(gvom.GvomBackendError, match="more than 64 headings"):
        g.pose_field_of(c, [(1, 1)])
    g.set_footprint(ref.point_footprint(H))
    g.pose_field_of(c, [(1, 1)]).release()
    sets = g.get_tuning("device_product_sets")
    for bad in ([(xy, 0)], [(0, -1)], [(1, 1, float("nan"))], np.zeros((0, 2)), np.zeros((3, 4))):
        with pytest.raises(ValueError):
            g.pose_field_of(c, bad)
    for kw in (dict(max_cost=0), dict(max_cost=2 ** 30 + 1), dict(max_rounds=-1), dict(max_cost=1.5)):
        with pytest.raises(ValueError):
            g.pose_field_of(c, [(1, 1)], **kw)
    for bad in (np.full((xy, xy + 1), 3), np.full((xy, xy), 65536), np.full((xy, xy), -1), None):
        with pytest.raises(ValueError):
            g.pose_field_of(bad, [(1, 1)])
    with pytest.raises(ValueError):
        g.pose_field_of_device(0, [(1, 1)])
    with pytest.raises(ValueError, match="outside the limits"):
        g.set_primitives((np.array([0, 1] + [1] * (H - 1)), np.array([(5, 0, 0, 1)])))
    # the C ABI's own checks
    pid, info = ctypes.c_int64(7), (ctypes.c_int64 * 4)()
    cc = np.asfortranarray(c.astype(np.int32))
    cp = cc.ctypes.data_as(ctypes.c_void_p)

    def raw(field=-1, cost=cp, goals=(1, 1, -1), n=1, max_cost=0, max_rounds=0, out=pid):
        gl = np.array(goals, np.int32)
        return g._check(g._lib.gvom_pose_field(g._h, field, cost, 0, gl.ctypes.data_as(ctypes.c_void_p) if n >= 0 else None, abs(n), max_cost,
                                               max_rounds, ctypes.byref(out) if out is not None else None, info))
    assert raw() == 0 and pid.value > 0
    field = g.cost_to_go_of(c, [(1, 1)])
    assert raw(field=field.product_id, cost=None) == 0 and pid.value > 0
    for kw, word in ((dict(cost=None), "give a cost field id or a cost map"), (dict(field=field.product_id), "not both"),
                     (dict(field=12345, cost=None), "unknown or stale cost field id"), (dict(field=10 ** 9, cost=None), "unknown or stale cost field id"),
                     (dict(goals=(xy, 1, -1)), "outside the window"), (dict(goals=(1, -1, 0)), "outside the window"),
                     (dict(goals=(1, 1, H)), "not one of the table's"), (dict(n=0), "between 1 and 65536 goals"), (dict(n=-1), "between 1 and 65536 goals"),
                     (dict(n=65537), "between 1 and 65536 goals"), (dict(max_cost=-1), "max_cost outside"), (dict(max_cost=2 ** 30 + 1), "max_cost outside"),
                     (dict(max_rounds=-1), "max_rounds must not be negative")):
        pid.value = 7
        with pytest.raises(gvom.GvomBackendError, match=word):
            raw(**kw)
        assert pid.value == -1, kw
    assert g._lib.gvom_pose_field(g._h, -1, cp, 0, np.array((1, 1, -1), np.int32).ctypes.data_as(ctypes.c_void_p), 1, 0, 0, None, info) == gvom.GVOM_ERR_INVALID   # NULL product_id
    bad_cost = np.asfortranarray(np.full((xy, xy), 70000, np.int32))
    with pytest.raises(gvom.GvomBackendError, match="outside 0 .. 65535"):
        raw(cost=bad_cost.ctypes.data_as(ctypes.c_void_p))
    # the id of another kind of product is no cost field; a released field whose set has been handed out again is stale
    with g.clearance_of(np.zeros((xy, xy), np.int32)) as clr:
        with pytest.raises(gvom.GvomBackendError, match="unknown or stale cost field id"):
            raw(field=clr.product_id, cost=None)
    with g.pose_field_of(c, [(1, 1)]) as other:
        with pytest.raises(gvom.GvomBackendError, match="unknown or stale cost field id"):
            raw(field=other.product_id, cost=None)
    old = field.product_id
    field.release()
    g.cost_to_go_of(c, [(2, 2)]).release()
    with pytest.raises(gvom.GvomBackendError, match="unknown or stale cost field id"):
        raw(field=old, cost=None)
    with pytest.raises(ValueError, match="unknown or stale cost field id"):
        field.pose_field([(1, 1)], goals_in_cells=True)
    sharded = gvom.Gvom(*_params(64), voxel_statistics=False, _shard=(0, 2))
    sharded.set_footprint(ref.point_footprint(H))
    sharded.set_primitives(table)
    with pytest.raises(ValueError, match="sharded handles are not supported"):
        sharded.pose_field_of(np.ones((64, 64), np.uint16), [(1, 1)])
    assert sharded.get_tuning("device_product_sets") == 0
    st, pr = table
    for k, col, value in ((0, 0, 5), (0, 1, -5), (0, 2, H), (0, 2, -1), (0, 3, 0), (0, 3, 256)):
        p2 = pr.copy()
        p2[k, col] = value
        assert g._lib.gvom_primitives_set(g._h, H, st.ctypes.data_as(ctypes.c_void_p), p2.ctypes.data_as(ctypes.c_void_p)) == -1
    assert g._lib.gvom_primitives_set(g._h, 65, st.ctypes.data_as(ctypes.c_void_p), pr.ctypes.data_as(ctypes.c_void_p)) == -1
    assert g._lib.gvom_primitives_set(g._h, H, None, pr.ctypes.data_as(ctypes.c_void_p)) == -1
    assert g.get_tuning("primitives") == 1                       # a refused table leaves the one in place
    assert g._lib.gvom_device_product(g._h, gvom.PRODUCT_POSEFIELD, 0, ctypes.byref(pid)) == -1
    assert g.get_tuning("device_product_sets") == sets + 2        # the cost field's and the clearance product's: no refused call made a set


def test_windows_beyond_the_limits_are_refused(gvom):
    goal, info = np.array([(1, 1, -1)], np.int32), (ctypes.c_int64 * 4)()

    def refused(g, xy, word):
        cost, pid = np.ones((xy, xy), np.int32, order="F"), ctypes.c_int64(7)
        rc = g._lib.gvom_pose_field(g._h, -1, cost.ctypes.data_as(ctypes.c_void_p), 0, goal.ctypes.data_as(ctypes.c_void_p), 1, 0, 0, ctypes.byref(pid), info)
        assert rc == -4 and pid.value == -1 and word in g._lib.gvom_last_error(g._h), (rc, g._lib.gvom_last_error(g._h))      # GVOM_ERR_CAPACITY
        assert g.get_tuning("pose_field_allocations") == 1 and g.get_tuning("device_product_sets") == 0                      # (the table only)
    big = gvom.Gvom(0.4, 0.2, 4100, 1, 1, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1, voxel_statistics=False)
    big.set_footprint(ref.point_footprint(1))
    big.set_primitives(ref.steps_table())
    refused(big, 4100, b"more than 4096 cells")
    del big
    wide = gvom.Gvom(0.4, 0.2, 2052, 1, 1, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1, voxel_statistics=False)       # 64 x 2052^2 > 2^28
    wide.set_footprint(ref.point_footprint(64))
    wide.set_primitives(ref.random_table(64, 1, 0, most=2))
    refused(wide, 2052, b"2^28 states")


def test_paths_follow_the_actions_to_a_seeded_state(gvom):
    i = [k for k, q in enumerate(ref.cases()) if q["name"] == "xy40 H16 car arcs+reverse gap"][0]
    q = ref.cases()[i]
    g = _mapper(gvom, q)
    C, D, A, seeds, _ = ref.expected(i)
    f = g.pose_field_of(q["c"], ref.goals_for_binding(q["goals"], q["H"]))
    rng = np.random.default_rng(3)
    reached = np.argwhere((D < U) & ~seeds)
    n_back = 0
    for h, x, y in reached[rng.choice(len(reached), 60, replace=False)]:
        path = f.path_from(x, y, h)
        assert path[0] == (x, y, h) and seeds[path[-1][2], path[-1][0], path[-1][1]]
        assert ref.path_price(path, C, q["table"]) == D[h, x, y]
        n_back += any(A[ph, px, py] >= 3 for px, py, ph in path[:-1])
    assert n_back > 0                                            # some of them back up
    h, x, y = np.argwhere((D == U) & (C != 0))[0]
    assert f.path_from(x, y, h) is None and f.path_from(0, 0, 0) is None
    gx, gy, gh = (int(v) for v in q["goals"][0])
    assert f.path_from(gx, gy, gh) == [(gx, gy, gh)]
    with pytest.raises(ValueError):
        f.path_from(q["xy"], 0, 0)
    f.release()
    g.set_tuning("pose_field_inner", 1)
    with g.pose_field_of(q["c"], ref.goals_for_binding(q["goals"], q["H"]), max_rounds=2) as early:
        act = early.action.copy_to_host()
        assert not early.converged
        for h, x, y in np.argwhere(act == ref.UNSETTLED)[:5]:          # (which states are unsettled after two rounds is the schedule's; the CPU test has a fixed one)
            with pytest.raises(RuntimeError, match="unsettled"):
                early.path_from(x, y, h)


def test_a_torch_consumer_gathers_terminal_costs():
    """a fresh child process that imports torch BEFORE the library is loaded (one HIP runtime in the process)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_posefield_torch.py")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "CASE OK terminal_costs" in r.stdout, r.stdout[-4000:]
