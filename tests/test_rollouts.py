"""Rollout scoring on the GPU (gvom_footprint_set, gvom_score_rollouts: k_rollouts; Gvom.set_footprint, DeviceCostField.score_rollouts,
Gvom.score_rollouts_of, Gvom.score_rollouts_of_device) against the referee of tests/rollouts_ref.py: the summary and the pose costs
with tolerance 0 -- everything is integer.  Synthetic maps of 16, 33, 64 and 100 cells (random, free, blocked, one blocked cell),
footprints of 1, 63, 64, 65, 128, 129 and 1000 cells per heading (each side of the 64-lane and the 256-cell boundaries of the lane
loop) with 1, 7 and 64 headings and an asymmetric table, K x T of 1 x 1, 1 x 65, 3 x 64, 65 x 7, 257 x 33 and 2 x 4096, with and without a
cost-to-go field, through host and device pointers; a car footprint on 1024 cells at a negative origin; the largest map (4096
cells) at its far corner; the obstacle scenes end to end through combine_maps_device().cost_to_go().score_rollouts() after the ego
has moved; snapshots, the product pool, errors, and a torch consumer in a child process.  tests/test_rollouts_cpu.py holds the
census of every input."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import costfield_ref as cf
import obstacle_scenes as ob
import rollouts_ref as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(xy, res=0.4, buffer_size=1, zs=8):
    return (res, 0.2, xy, zs, buffer_size, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)


@pytest.fixture(scope="module")
def gvom():
    import gvom as mod
    rc, info = mod.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    assert mod.PRODUCT_ROLLOUTS == 10
    return mod


@pytest.fixture(scope="module")
def handles(gvom):
    return {xy: gvom.Gvom(*_params(xy, rr.RES[xy]), voxel_statistics=False) for xy in rr.SIZES}


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


def _hold(r, want, what):
    """a DeviceRollouts against the referee's (summary, pose_cost, ...): both parts, exactly"""
    with r:
        summary, cost = r.copy_to_host()
    assert summary.dtype == np.int32 and cost.dtype == np.uint16, what
    assert summary.shape == want[0].shape and cost.shape == want[1].shape, (what, summary.shape, cost.shape)
    if not np.array_equal(cost, want[1]):
        bad = np.argwhere(cost != want[1])
        raise AssertionError("%s: the pose costs differ in %d poses, first (%d, %d): got %d, referee %d" % (
            what, len(bad), bad[0][0], bad[0][1], cost[tuple(bad[0])], want[1][tuple(bad[0])]))
    if not np.array_equal(summary, want[0]):
        bad = np.argwhere((summary != want[0]).any(axis=1))
        raise AssertionError("%s: the summaries differ in %d rollouts, first %d: got %r, referee %r" % (
            what, len(bad), bad[0][0], summary[bad[0][0]].tolist(), want[0][bad[0][0]].tolist()))
    return summary, cost


def _run(g, q, dev, device=None):
    """one case through the host or the device route"""
    g.set_footprint(q["table"])
    if q["device"] if device is None else device:
        K, T = q["poses"].shape[:2]
        cp = dev.upload(np.asfortranarray(q["c"]).T)                       # cell (x, y) at [y * xy + x]
        dp = None if q["D"] is None else dev.upload(np.asfortranarray(q["D"]).T)
        return g.score_rollouts_of_device(cp, dev.upload(q["poses"]), K, T, cost_to_go_ptr=dp, origin=q["origin"])
    return g.score_rollouts_of(q["c"], q["poses"], cost_to_go=q["D"], origin=q["origin"])


@pytest.mark.parametrize("shape", rr.SHAPES, ids=lambda s: "%dx%d" % s)
def test_synthetic_inputs_match_the_referee_exactly(handles, shape):
    dev = _Device()
    try:
        for q, want in zip(rr.cases(shape), rr.expected(shape)):
            r = _run(handles[q["xy"]], q, dev)
            assert r.summary.shape == (shape[0], 4) and r.pose_cost.shape == shape and r.summary.strides == (4, 1) and r.pose_cost.strides == (shape[1], 1)
            assert r.summary.ptr % 256 == 0 and r.pose_cost.ptr % 256 == 0
            _hold(r, want, q["name"])
    finally:
        dev.free()


def test_host_and_device_routes_agree_with_and_without_a_field(handles):
    """every case of one shape through BOTH routes, and a case with a field scored again without it: only the terminals change"""
    dev = _Device()
    shape = (65, 7)
    try:
        for q, want in zip(rr.cases(shape), rr.expected(shape)):
            g = handles[q["xy"]]
            for device in (False, True):
                _hold(_run(g, q, dev, device), want, "%s, %s route" % (q["name"], "device" if device else "host"))
            if q["D"] is not None:
                bare = dict(q, D=None)
                summary, _ = _hold(_run(g, bare, dev, True), rr.score(q["c"], q["poses"], q["table"], q["res"], q["origin_cells"], None), q["name"] + ", no field")
                assert (summary[:, 3] == rr.UNREACHED).all() and np.array_equal(summary[:, :3], want[0][:, :3])
    finally:
        dev.free()


def test_memory_orders_and_number_types(handles):
    q = [q for q in rr.cases((257, 33)) if q["D"] is not None and "random" in q["name"]][0]
    g = handles[q["xy"]]
    want = rr.score(q["c"], q["poses"], q["table"], q["res"], q["origin_cells"], q["D"])
    assert not np.array_equal(q["c"], q["c"].T)
    g.set_footprint((q["table"][0].astype(np.int64), q["table"][1].astype(np.int32)))          # raw arrays of other integer types
    for name, c, D in (("fortran", np.asfortranarray(q["c"]), np.asfortranarray(q["D"])), ("int64", q["c"].astype(np.int64), q["D"].astype(np.int64)),
                       ("float", q["c"].astype(np.float64), q["D"].astype(np.float64)), ("view", np.ascontiguousarray(q["c"].T).T, q["D"])):
        _hold(g.score_rollouts_of(c, q["poses"].astype(np.float64), cost_to_go=D, origin=q["origin"]), want, name)
    _hold(g.score_rollouts_of(q["c"], np.asfortranarray(q["poses"]), cost_to_go=q["D"], origin=np.array(q["origin"] + (0.0,))), want, "fortran poses, 3-d origin")


@pytest.fixture(scope="module")
def large_handles(gvom):
    made = {}

    def get(xy):
        if xy not in made:
            made.clear()                                           # (one large mapper at a time)
            made[xy] = gvom.Gvom(*_params(xy, rr.RES[xy], zs=1), voxel_statistics=False)
        return made[xy]
    yield get
    made.clear()


def _car(gvom, xy):
    car = gvom.rectangle_footprint(rr.CAR["front"], rr.CAR["rear"], rr.CAR["half_width"], rr.RES[xy], headings=64)
    return car, (car[0].tobytes(), car[1].tobytes(), 64)


def test_1024_cells_with_a_car_footprint_at_a_negative_origin(gvom, large_handles):
    xy = 1024
    g = large_handles(xy)
    car, key = _car(gvom, xy)
    q, want = rr.large_case(xy, key)
    assert q["poses"].shape == (1024, 64, 3) and 300 < np.diff(car[0]).mean() < 360
    dev = _Device()
    try:
        summary, cost = _hold(_run(g, q, dev, True), want, "xy 1024, device route")
        _hold(_run(g, q, dev, False), want, "xy 1024, host route")
    finally:
        dev.free()
    assert all((summary[:, 0] == s).sum() >= 10 for s in (rr.CLEAR, rr.COLLISION, rr.LEFT_WINDOW)) and (cost > 0).mean() > 0.3


def test_4096_cells_the_largest_map_at_its_far_corner(gvom, large_handles):
    xy = 4096
    g = large_handles(xy)
    car, key = _car(gvom, xy)
    q, want = rr.large_case(xy, key)
    cx, cy, _, valid = rr.pose_frame(q["poses"], q["res"], q["origin_cells"], 64)
    assert valid.all() and cx.max() >= xy - 8 and cy.max() >= xy - 8 and cx.min() > xy - 200       # cell indices next to 2^24
    dev = _Device()
    try:
        summary, cost = _hold(_run(g, q, dev, True), want, "xy 4096")
    finally:
        dev.free()
    assert (cost > 0).sum() > 100 and (summary[:, 0] == rr.LEFT_WINDOW).any() and (summary[:, 3] != rr.UNREACHED).any()


def _scene(gvom, name):
    g = gvom.Gvom(*ob.params(name), voxel_statistics=False)
    for pc, ego in ob.scans(name):
        g.process_pointcloud(pc, ego)
    return g, np.array(ob.scans(name)[-1][1][:2])


@pytest.mark.parametrize("name", cf.SCENES)
def test_scenes_end_to_end_through_cost_fields(gvom, name):
    """combine_maps_device().cost_to_go(...).score_rollouts(...) after the ego has moved (the window's origin is not zero), against
    the referee fed with the field's own host copies"""
    g, ego = _scene(gvom, name)
    res, xy = g.xy_resolution, g.xy_size
    table = gvom.rectangle_footprint(0.9, 0.5, 0.45, res, headings=16, margin=0.1)
    g.set_footprint(table)
    dev = _Device()
    try:
        with g.combine_maps_device() as m:
            oc = tuple(int(v) for v in np.round(np.asarray(m.origin)[:2] / res))
            assert oc != (0, 0)
            with m.cost_to_go([ego + (5.0, 3.1), ego - (6.0, 4.2)], density_threshold=cf.SCENE_THRESHOLD, soft_weight=3, unknown=40) as f:
                assert np.array_equal(f.origin, m.origin)
                D, _, c = f.copy_to_host()
                poses = rr.arc_poses(200, 40, xy, res, oc, 77, spread=6.0, centre=tuple(np.floor(ego / res).astype(int) - oc))
                poses[7, 20] = np.nan
                want = rr.score(c, poses, table, res, oc, D)
                summary, cost = _hold(f.score_rollouts(poses), want, name)
                # the same maps by pointer: the field's own parts, read in place
                by_pointer = g.score_rollouts_of_device(f.cell_cost.ptr, dev.upload(poses), 200, 40, cost_to_go_ptr=f.cost.ptr, origin=m.origin)
                _hold(by_pointer, want, name + ", by pointer")
    finally:
        dev.free()
    print(name, "status counts", np.bincount(summary[:, 0], minlength=4).tolist(), "finite terminals", int((summary[:, 3] != rr.UNREACHED).sum()))
    assert (cost > 0).any() and (summary[:, 0] == rr.COLLISION).any() and summary[7, 1] <= 20 and len(np.unique(cost)) > 2


def test_a_rollout_product_is_a_snapshot(gvom):
    name = "one_round"
    g = gvom.Gvom(*ob.params(name), voxel_statistics=False)
    scans = ob.scans(name)
    res, xy = g.xy_resolution, g.xy_size
    g.set_footprint(gvom.disc_footprint(0.5, res))
    g.process_pointcloud(*scans[0])
    with g.combine_maps_device() as m:
        f = m.cost_to_go([(32, 32)], goals_in_cells=True, soft_weight=10)
        oc = tuple(int(v) for v in np.round(np.asarray(m.origin)[:2] / res))
    poses = rr.arc_poses(64, 30, xy, res, oc, 5)
    held = f.score_rollouts(poses)
    f.release()
    before = held.copy_to_host()
    assert (before[1] > 0).any() and (before[1] == 0).any()
    for pc, ego in scans[1:]:
        g.process_pointcloud(pc, ego)
        with g.combine_maps_device() as m:
            with m.cost_to_go([(32, 32)], goals_in_cells=True, soft_weight=10) as f2:
                g.set_footprint(gvom.rectangle_footprint(1.5, 0.5, 0.6, res, headings=8))
                later = f2.score_rollouts(poses)
                assert later.summary.ptr != held.summary.ptr
                now = later.copy_to_host()
                later.release()
    after = held.copy_to_host()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert not np.array_equal(now[1], after[1])                    # the map and the footprint have moved on; the held product has not


def test_pool_capacity_reuse_and_no_allocation_in_steady_state(gvom):
    xy = 64
    g = gvom.Gvom(*_params(xy, rr.RES[xy]), voxel_statistics=False)
    assert g.get_tuning("rollouts") == 1 and g.get_tuning("footprint") == 0 and g.get_tuning("rollout_allocations") == 0
    q = [q for q in rr.cases((65, 7)) if q["xy"] == xy][0]
    want = rr.score(q["c"], q["poses"], q["table"], q["res"], q["origin_cells"], q["D"])
    g.set_footprint(q["table"])
    assert g.get_tuning("footprint") == 1
    call = lambda poses=q["poses"]: g.score_rollouts_of(q["c"], poses, cost_to_go=q["D"], origin=q["origin"])
    first = call()
    assert g.get_tuning("rollout_allocations") == 2             # the product set and the host staging buffer
    assert g.get_tuning("device_product_sets") == 1
    ptr = first.summary.ptr
    first.release()
    for _ in range(3):                                         # released: everything is reused
        with call() as r:
            assert r.summary.ptr == ptr
            _hold(r, want, "reused set")
    assert g.get_tuning("rollout_allocations") == 2 and g.get_tuning("device_product_sets") == 1
    # replacing the footprint between calls: the next call scores with the new table
    other = rr.asymmetric_table(7)
    g.set_footprint(other)
    _hold(call(), rr.score(q["c"], q["poses"], other, q["res"], q["origin_cells"], q["D"]), "after set_footprint")
    g.set_footprint(q["table"])
    assert g.get_tuning("rollout_allocations") == 2
    # a larger shape gives the small set up for one that holds it
    big = np.concatenate([q["poses"]] * 40, axis=0)
    with call(big) as r:
        assert r.summary.shape == (65 * 40, 4)
        _hold(r, tuple(np.concatenate([w] * 40, axis=0) for w in want[:2]), "a larger K")
    grown = g.get_tuning("rollout_allocations")
    assert grown > 2 and g.get_tuning("device_product_sets") == 1
    with call() as r:                                           # the smaller shape fits the larger set
        _hold(r, want, "the smaller shape again")
    assert g.get_tuning("rollout_allocations") == grown
    held = [call() for _ in range(4)]
    assert len({r.summary.ptr for r in held}) == 4 and g.get_tuning("device_product_sets") == 4
    with pytest.raises(gvom.GvomBackendError, match="all 4 device product sets of this kind"):
        call()
    held[2].release()
    allocs = g.get_tuning("rollout_allocations")
    with call() as r:
        _hold(r, want, "after a release")
    assert g.get_tuning("device_product_sets") == 4 and g.get_tuning("rollout_allocations") == allocs
    for k in (0, 1, 3):                                        # (the set of held[2] has been handed out again: its id is stale)
        _hold(held[k], want, "held")
    with pytest.raises(gvom.GvomBackendError, match="unknown or stale device product id"):
        held[2].copy_to_host()


def test_errors(gvom):
    xy = 64
    g = gvom.Gvom(*_params(xy), voxel_statistics=False)
    cost = np.ones((xy, xy), np.uint16)
    poses = np.zeros((2, 3, 3), np.float32)
    with pytest.raises(ValueError, match="no footprint table is set"):
        g.score_rollouts_of(cost, poses)
    assert g.get_tuning("rollout_allocations") == 0
    g.set_footprint(gvom.disc_footprint(0.5, 0.4))
    pid = ctypes.c_int64(-1)
    oc = (ctypes.c_int64 * 2)(0, 0)
    cp, pp = cost.ctypes.data_as(ctypes.c_void_p), poses.ctypes.data_as(ctypes.c_void_p)

    def raw(field=-1, c=cp, D=None, p=pp, K=2, T=3, origin=oc, out=pid):
        return g._check(g._lib.gvom_score_rollouts(g._h, field, c, D, p, K, T, 0, origin, ctypes.byref(out) if out is not None else None))
    assert raw() == 0
    g._check(g._lib.gvom_device_product_export(g._h, pid.value, 0, ctypes.c_void_p(gvom._STREAM_NOSYNC), ctypes.byref(ctypes.c_void_p()),
                                               ctypes.byref(ctypes.c_int32()), (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()))
    g._check(g._lib.gvom_device_product_release(g._h, pid.value, ctypes.c_void_p(gvom._STREAM_NOSYNC)))
    far = (ctypes.c_int64 * 2)(1 << 41, 0)
    for kw, word in ((dict(field=10 ** 9, c=None), "unknown or stale cost field id"), (dict(field=pid.value, c=None), "unknown or stale cost field id"),
                     (dict(field=1), "not both"), (dict(c=None), "a cost field id or a cell-cost map"), (dict(p=None), "poses"),
                     (dict(origin=None), "origin_cells"), (dict(T=0), "T outside"), (dict(T=4097), "T outside"), (dict(K=0), "K must be"),
                     (dict(K=(1 << 26) // 3 + 1), "2\\^26 poses"), (dict(origin=far), "2\\^40")):
        with pytest.raises(gvom.GvomBackendError, match=word):
            raw(**kw)
        assert pid.value == -1
    assert g._lib.gvom_score_rollouts(g._h, -1, cp, None, pp, 2, 3, 0, oc, None) == gvom.GVOM_ERR_INVALID        # NULL product_id
    assert g._lib.gvom_score_rollouts(g._h, -1, cp, None, pp, (1 << 26) // 3 + 1, 3, 0, oc, ctypes.byref(pid)) == -4   # GVOM_ERR_CAPACITY
    with pytest.raises(gvom.GvomBackendError, match="gvom_score_rollouts"):
        g._device_product(gvom.PRODUCT_ROLLOUTS)
    with pytest.raises(gvom.GvomBackendError, match="unknown product kind"):
        g._device_product(9)
    # a stale field: released and recycled by the next solve
    f = g.cost_to_go_of(np.ones((xy, xy), np.int32), [(1, 1)])
    old = f.product_id
    f.score_rollouts(poses).release()
    f.release()
    g.cost_to_go_of(np.ones((xy, xy), np.int32), [(2, 2)]).release()
    with pytest.raises(gvom.GvomBackendError, match="unknown or stale cost field id"):
        raw(field=old, c=None)
    # bad tables, as the library itself sees them
    st, of = np.array([0, 2], np.int32), np.zeros((2, 2), np.int16)
    fs = lambda H, s, o: g._lib.gvom_footprint_set(g._h, H, s.ctypes.data_as(ctypes.c_void_p) if s is not None else None,
                                                   o.ctypes.data_as(ctypes.c_void_p) if o is not None else None)
    assert fs(1, st, of) == 0
    for H, s, o in ((0, st, of), (1025, st, of), (1, None, of), (1, st, None), (1, np.array([1, 2], np.int32), of), (1, np.array([0, 0], np.int32), of),
                    (1, np.array([0, 16385], np.int32), of), (2, np.array([0, 2, 1], np.int32), of)):
        assert fs(H, s, o) == gvom.GVOM_ERR_INVALID
        assert g.get_tuning("footprint") == 1                   # a refused table leaves the one that is set
    many = np.concatenate([[0], np.cumsum(np.full(257, 16384))]).astype(np.int32)
    assert fs(257, many, of) == -4                               # more than 2^22 offsets: refused before anything is read
    sharded = gvom.Gvom(*_params(64), voxel_statistics=False, _shard=(0, 2))
    with pytest.raises(ValueError, match="sharded handles are not supported"):
        sharded.score_rollouts_of(cost, poses)


def test_maps_of_more_than_4096_cells_a_side_are_refused(gvom):
    xy = 4100
    g = gvom.Gvom(0.4, 0.2, xy, 1, 1, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1, voxel_statistics=False)
    g.set_footprint(gvom.disc_footprint(0.5, 0.4))
    with pytest.raises(gvom.GvomBackendError, match="4096"):
        g.score_rollouts_of_device(1 << 20, 1 << 21, 1, 1)
    assert g.get_tuning("rollout_allocations") == 0


def _torch_case(name):
    """One case per fresh child process that imports torch BEFORE the library is loaded (one HIP runtime in the process)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_rollouts_torch.py"), name],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "CASE OK " + name in r.stdout, r.stdout[-4000:]


def test_a_torch_planner_picks_its_rollout_on_a_side_stream():
    _torch_case("planner")
