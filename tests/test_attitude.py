"""Terrain attitude scoring on the GPU (gvom_chassis_set, gvom_score_attitude: k_attitude_ground, k_attitude; Gvom.set_chassis,
DeviceMaps.score_attitude, Gvom.score_attitude_of, Gvom.score_attitude_of_device) against the referee of tests/attitude_ref.py: the
summary, the three values per pose and the pose status with tolerance 0 -- every float64 operation is one IEEE operation in the
header's order.  Synthetic grounds of 16, 33, 64 and 100 cells (flat, a plane, terraces, random with 10 % unknown in every way a
cell can be, all unknown), footprints of 1, 63, 64, 65, 256, 257 and 1000 cells per heading (each side of the 64-lane and the
256-cell boundaries of the lane loop) with 1, 7 and 64 headings and an asymmetric table, K x T of 1 x 1, 1 x 65, 3 x 64, 65 x 7, 257 x 33
and 2 x 4096, through host and device pointers; a stored value one float32 ulp above, on and below each limit; a car on 1024 cells at
a negative origin; the obstacle scenes through combine_maps_device().score_attitude() after the ego has moved, with and without the
inferred ground; snapshots, the product pool, errors, and a torch consumer in a child process.  tests/test_attitude_cpu.py holds the
census of every input."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import attitude_ref as ar
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
    assert mod.PRODUCT_ATTITUDE == 14
    return mod


@pytest.fixture(scope="module")
def handles(gvom):
    return {xy: gvom.Gvom(*_params(xy, rr.RES[xy]), voxel_statistics=False) for xy in ar.SIZES}


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


def _chassis(gvom, ch):
    """the binding's chassis of a referee Chassis: the limits are the referee's float32 numbers, bit for bit"""
    c = gvom.chassis(ch.front_axle, ch.rear_axle, ch.track, ch.belly_height)
    c.max_pitch, c.max_roll, c.min_clearance = ch.max_pitch, ch.max_roll, ch.min_clearance
    return c


def _hold(r, want, what):
    """a DeviceAttitude against the referee's (summary, attitude, status): all three parts, exactly"""
    with r:
        summary, att, status = r.copy_to_host()
    assert summary.dtype == np.int32 and att.dtype == np.float32 and status.dtype == np.uint8, what
    assert summary.shape == want[0].shape and att.shape == want[1].shape and status.shape == want[2].shape, (what, summary.shape, att.shape, status.shape)
    if not np.array_equal(status, want[2]):
        bad = np.argwhere(status != want[2])
        raise AssertionError("%s: the pose statuses differ in %d poses, first (%d, %d): got %d, referee %d" % (
            what, len(bad), bad[0][0], bad[0][1], status[tuple(bad[0])], want[2][tuple(bad[0])]))
    if not np.array_equal(att, want[1], equal_nan=True):
        bad = np.argwhere(~((att == want[1]) | (np.isnan(att) & np.isnan(want[1]))))
        raise AssertionError("%s: the values differ in %d numbers, first (%d, %d, %d): got %r, referee %r" % (
            what, len(bad), bad[0][0], bad[0][1], bad[0][2], att[tuple(bad[0])], want[1][tuple(bad[0])]))
    if not np.array_equal(summary, want[0]):
        bad = np.argwhere((summary != want[0]).any(axis=1))
        raise AssertionError("%s: the summaries differ in %d rollouts, first %d: got %r, referee %r" % (
            what, len(bad), bad[0][0], summary[bad[0][0]].tolist(), want[0][bad[0][0]].tolist()))
    return summary, att, status


def _run(gvom, g, q, dev, device=None):
    """one case through the host or the device route"""
    g.set_footprint(q["table"])
    g.set_chassis(_chassis(gvom, q["chassis"]))
    assert np.array_equal(g.cos_sin, q["cos_sin"])                         # the referee turns with the numbers the library got
    if q["device"] if device is None else device:
        K, T = q["poses"].shape[:2]
        gp = dev.upload(np.asfortranarray(q["g"]).T)                       # cell (x, y) at [y * xy + x]
        return g.score_attitude_of_device(gp, dev.upload(q["poses"]), K, T, origin=q["origin"])
    return g.score_attitude_of(q["g"], q["poses"], origin=q["origin"])


@pytest.mark.parametrize("shape", ar.SHAPES, ids=lambda s: "%dx%d" % s)
def test_synthetic_inputs_match_the_referee_exactly(gvom, handles, shape):
    dev = _Device()
    K, T = shape
    try:
        for q, want in zip(ar.cases(shape), ar.expected(shape)):
            r = _run(gvom, handles[q["xy"]], q, dev)
            assert r.summary.shape == (K, 5) and r.attitude.shape == (K, T, 3) and r.status.shape == shape
            assert r.summary.strides == (5, 1) and r.attitude.strides == (3 * T, 3, 1) and r.status.strides == (T, 1)
            assert r.summary.ptr % 256 == 0 and r.attitude.ptr % 256 == 0 and r.status.ptr % 256 == 0
            _hold(r, want, q["name"])
    finally:
        dev.free()


def test_a_value_one_ulp_above_on_and_below_each_limit(gvom, handles):
    dev = _Device()
    try:
        for q, want in zip(ar.limit_cases(), ar.expected_limits()):
            _hold(_run(gvom, handles[q["xy"]], q, dev), want, q["name"])
    finally:
        dev.free()


def test_host_and_device_routes_agree(gvom, handles):
    """every case of one shape through BOTH routes"""
    dev = _Device()
    shape = (65, 7)
    try:
        for q, want in zip(ar.cases(shape), ar.expected(shape)):
            for device in (False, True):
                _hold(_run(gvom, handles[q["xy"]], q, dev, device), want, "%s, %s route" % (q["name"], "device" if device else "host"))
    finally:
        dev.free()


def test_memory_orders_number_types_and_heights_that_overflow(gvom, handles):
    q = [q for q in ar.cases((257, 33)) if q["pattern"] == "random"][0]
    g = handles[q["xy"]]
    want = ar._score_case(q)
    assert not np.array_equal(np.nan_to_num(q["g"]), np.nan_to_num(q["g"].T))
    g.set_footprint(q["table"])
    g.set_chassis(_chassis(gvom, q["chassis"]))
    for name, gm in (("fortran", np.asfortranarray(q["g"])), ("view", np.ascontiguousarray(q["g"].T).T)):
        _hold(g.score_attitude_of(gm, q["poses"].astype(np.float64), origin=q["origin"]), want, name)
    _hold(g.score_attitude_of(q["g"], np.asfortranarray(q["poses"]), origin=np.array(q["origin"] + (0.0,))), want, "fortran poses, 3-d origin")
    f32 = q["g"].astype(np.float32)                                         # a float32 map is cast as it is
    _hold(g.score_attitude_of(f32, q["poses"], origin=q["origin"]),
          ar.score(f32.astype(np.float64), q["poses"], q["table"], q["chassis"], q["cos_sin"], q["res"], q["origin_cells"]), "float32 map")
    huge = q["g"].copy()                                                    # sums of heights that overflow: infinite and NaN tangents
    rng = np.random.default_rng(8)
    huge[rng.random(huge.shape) < 0.2] = 1.5e308
    huge[rng.random(huge.shape) < 0.1] = -1.7e308
    want = ar.score(huge, q["poses"], q["table"], q["chassis"], q["cos_sin"], q["res"], q["origin_cells"])
    assert np.isnan(want[1]).any() and np.isinf(want[1][..., :2]).any()
    _hold(g.score_attitude_of(huge, q["poses"], origin=q["origin"]), want, "heights that overflow")


def test_1024_cells_with_a_car_at_a_negative_origin(gvom):
    xy = 1024
    g = gvom.Gvom(*_params(xy, rr.RES[xy], zs=1), voxel_statistics=False)
    car = gvom.rectangle_footprint(rr.CAR["front"], rr.CAR["rear"], rr.CAR["half_width"], rr.RES[xy], headings=64)
    q, want = ar.large_case((car[0].tobytes(), car[1].tobytes(), 64))
    assert q["poses"].shape == (1024, 64, 3) and 300 < np.diff(car[0]).mean() < 360
    dev = _Device()
    try:
        summary, att, status = _hold(_run(gvom, g, q, dev, True), want, "xy 1024, device route")
        _hold(_run(gvom, g, q, dev, False), want, "xy 1024, host route")
    finally:
        dev.free()
    assert all((status == s).sum() >= 100 for s in range(6))


def _scene(gvom, name):
    g = gvom.Gvom(*ob.params(name), voxel_statistics=False)
    for pc, ego in ob.scans(name):
        g.process_pointcloud(pc, ego)
    return g, np.array(ob.scans(name)[-1][1][:2])


@pytest.mark.parametrize("name", cf.SCENES)
def test_scenes_through_real_map_sets_with_and_without_the_inferred_ground(gvom, name):
    """combine_maps_device().score_attitude(...) after the ego has moved (the window's origin is not zero), against the referee fed
    with the set's own maps 4 and 5"""
    g, ego = _scene(gvom, name)
    res, xy = g.xy_resolution, g.xy_size
    table = gvom.rectangle_footprint(0.9, 0.5, 0.45, res, headings=16, margin=0.1)
    g.set_footprint(table)
    ch = ar.make_chassis(0.7, -0.3, 0.8, 0.3, max_pitch=np.float32(np.tan(0.3)), max_roll=np.float32(np.tan(0.25)), min_clearance=np.float32(0.05))
    g.set_chassis(_chassis(gvom, ch))
    seen = {}
    dev = _Device()
    try:
        with g.combine_maps_device() as m:
            oc = tuple(int(v) for v in np.round(np.asarray(m.origin)[:2] / res))
            assert oc != (0, 0)
            height, inferred = m.height_map.copy_to_host(), m.inferred_height_map.copy_to_host()
            assert height.shape == (xy, xy) and (height <= -1000).any() and (height > -1000).any() and ((height <= -1000) & (inferred > -1000)).any()
            poses = rr.arc_poses(200, 40, xy, res, oc, 77, spread=6.0, centre=tuple(np.floor(ego / res).astype(int) - oc))
            poses[7, 20] = np.nan
            for use in (True, False):
                ground = ar.ground_of(height, inferred, use)
                want = ar.score(ground, poses, table, ch, g.cos_sin, res, oc)
                seen[use] = _hold(m.score_attitude(poses, inferred_ground=use), want, "%s, inferred_ground=%r" % (name, use))
                # the same ground by pointer, read in place
                by_pointer = g.score_attitude_of_device(dev.upload(np.asfortranarray(ground).T), dev.upload(poses), 200, 40, origin=m.origin)
                _hold(by_pointer, want, "%s, by pointer, inferred_ground=%r" % (name, use))
    finally:
        dev.free()
    for use in (True, False):
        print(name, "inferred" if use else "height only", "status counts", np.bincount(seen[use][2].ravel(), minlength=7).tolist())
    assert (seen[True][2] == ar.OK).any() and (seen[False][2] == ar.UNKNOWN_GROUND).sum() > (seen[True][2] == ar.UNKNOWN_GROUND).sum()
    assert seen[True][0][7, 1] <= 20 and len(np.unique(seen[True][1])) > 10


def test_an_attitude_product_is_a_snapshot(gvom):
    name = "one_round"
    g = gvom.Gvom(*ob.params(name), voxel_statistics=False)
    scans = ob.scans(name)
    res, xy = g.xy_resolution, g.xy_size
    g.set_footprint(gvom.disc_footprint(0.5, res))
    g.set_chassis(gvom.chassis(0.5, -0.3, 0.6, 0.3))
    g.process_pointcloud(*scans[0])
    with g.combine_maps_device() as m:
        oc = tuple(int(v) for v in np.round(np.asarray(m.origin)[:2] / res))
        poses = rr.arc_poses(64, 30, xy, res, oc, 5)
        held = m.score_attitude(poses)
    before = held.copy_to_host()
    assert (before[2] == ar.OK).any() and (before[2] != ar.OK).any()
    for pc, ego in scans[1:]:
        g.process_pointcloud(pc, ego)
        with g.combine_maps_device() as m:
            g.set_footprint(gvom.rectangle_footprint(1.5, 0.5, 0.6, res, headings=8))
            g.set_chassis(gvom.chassis(1.2, -0.2, 0.9, 0.2))
            later = m.score_attitude(poses)
            assert later.summary.ptr != held.summary.ptr
            now = later.copy_to_host()
            later.release()
    after = held.copy_to_host()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert not np.array_equal(now[1], after[1])                    # the map, the footprint and the chassis have moved on; the held product has not


def test_pool_capacity_reuse_and_no_allocation_in_steady_state(gvom):
    xy = 64
    g = gvom.Gvom(*_params(xy, rr.RES[xy]), voxel_statistics=False)
    assert g.get_tuning("attitude") == 1 and g.get_tuning("chassis") == 0 and g.get_tuning("attitude_allocations") == 0
    q = [q for q in ar.cases((65, 7)) if q["xy"] == xy][0]
    want = ar._score_case(q)
    g.set_footprint(q["table"])
    g.set_chassis(_chassis(gvom, q["chassis"]))
    assert g.get_tuning("chassis") == 1
    call = lambda poses=q["poses"]: g.score_attitude_of(q["g"], poses, origin=q["origin"])
    first = call()
    assert g.get_tuning("attitude_allocations") == 2            # the product set and the host staging buffer
    assert g.get_tuning("device_product_sets") == 1
    ptr = first.summary.ptr
    first.release()
    for _ in range(3):                                         # released: everything is reused
        with call() as r:
            assert r.summary.ptr == ptr
            _hold(r, want, "reused set")
    assert g.get_tuning("attitude_allocations") == 2 and g.get_tuning("device_product_sets") == 1
    # replacing the chassis between calls: the next call scores with the new one
    other = ar.make_chassis(1.1 * q["res"], -2.2 * q["res"], 1.4 * q["res"], 0.5 * q["res"], max_roll=np.float32(0.2))
    g.set_chassis(_chassis(gvom, other))
    _hold(call(), ar.score(q["g"], q["poses"], q["table"], other, q["cos_sin"], q["res"], q["origin_cells"]), "after set_chassis")
    g.set_chassis(_chassis(gvom, q["chassis"]))
    assert g.get_tuning("attitude_allocations") == 2
    # a larger shape gives the small set up for one that holds it
    big = np.concatenate([q["poses"]] * 40, axis=0)
    with call(big) as r:
        assert r.summary.shape == (65 * 40, 5)
        _hold(r, tuple(np.concatenate([w] * 40, axis=0) for w in want), "a larger K")
    grown = g.get_tuning("attitude_allocations")
    assert grown > 2 and g.get_tuning("device_product_sets") == 1
    with call() as r:                                           # the smaller shape fits the larger set
        _hold(r, want, "the smaller shape again")
    assert g.get_tuning("attitude_allocations") == grown
    held = [call() for _ in range(4)]
    assert len({r.summary.ptr for r in held}) == 4 and g.get_tuning("device_product_sets") == 4
    with pytest.raises(gvom.GvomBackendError, match="all 4 device product sets of this kind"):
        call()
    held[2].release()
    allocs = g.get_tuning("attitude_allocations")
    with call() as r:
        _hold(r, want, "after a release")
    assert g.get_tuning("device_product_sets") == 4 and g.get_tuning("attitude_allocations") == allocs
    for k in (0, 1, 3):                                        # (the set of held[2] has been handed out again: its id is stale)
        _hold(held[k], want, "held")
    with pytest.raises(gvom.GvomBackendError, match="unknown or stale device product id"):
        held[2].copy_to_host()


def test_errors(gvom):
    xy = 64
    g = gvom.Gvom(*_params(xy), voxel_statistics=False)
    ground = np.zeros((xy, xy))
    poses = np.zeros((2, 3, 3), np.float32)
    with pytest.raises(ValueError, match="no footprint table is set"):
        g.score_attitude_of(ground, poses)
    g.set_footprint(gvom.rectangle_footprint(0.5, 0.5, 0.4, 0.4, headings=8))
    with pytest.raises(ValueError, match="no chassis is set"):
        g.score_attitude_of(ground, poses)
    assert g.get_tuning("attitude_allocations") == 0
    g.set_chassis(gvom.chassis(0.5, -0.3, 0.6, 0.3))
    assert g.cos_sin.shape == (8, 2)
    g.set_footprint(gvom.disc_footprint(0.5, 0.4))              # one heading now: the chassis was set for eight
    with pytest.raises(ValueError, match="another number of headings"):
        g.score_attitude_of(ground, poses)
    g.set_chassis(gvom.chassis(0.5, -0.3, 0.6, 0.3))
    pid = ctypes.c_int64(-1)
    oc = (ctypes.c_int64 * 2)(0, 0)
    gp, pp = ground.ctypes.data_as(ctypes.c_void_p), poses.ctypes.data_as(ctypes.c_void_p)

    def raw(set_id=-1, gr=gp, p=pp, K=2, T=3, flags=0, origin=oc, out=pid):
        return g._check(g._lib.gvom_score_attitude(g._h, set_id, gr, p, K, T, 0, flags, origin, ctypes.byref(out) if out is not None else None))
    assert raw() == 0
    g._check(g._lib.gvom_device_product_export(g._h, pid.value, 0, ctypes.c_void_p(gvom._STREAM_NOSYNC), ctypes.byref(ctypes.c_void_p()),
                                               ctypes.byref(ctypes.c_int32()), (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()))
    g._check(g._lib.gvom_device_product_release(g._h, pid.value, ctypes.c_void_p(gvom._STREAM_NOSYNC)))
    far = (ctypes.c_int64 * 2)(1 << 41, 0)
    for kw, word in ((dict(set_id=10 ** 9, gr=None), "unknown or stale device map set id"), (dict(set_id=1), "not both"),
                     (dict(gr=None), "a map set id or a ground map"), (dict(p=None), "poses"), (dict(origin=None), "origin_cells"),
                     (dict(T=0), "T outside"), (dict(T=4097), "T outside"), (dict(K=0), "K must be"), (dict(flags=2), "unknown flag bits"),
                     (dict(K=(1 << 26) // 3 + 1), "2\\^26 poses"), (dict(origin=far), "2\\^40")):
        with pytest.raises(gvom.GvomBackendError, match=word):
            raw(**kw)
        assert pid.value == -1
    assert g._lib.gvom_score_attitude(g._h, -1, gp, pp, 2, 3, 0, 0, oc, None) == gvom.GVOM_ERR_INVALID            # NULL product_id
    assert g._lib.gvom_score_attitude(g._h, -1, gp, pp, (1 << 26) // 3 + 1, 3, 0, 0, oc, ctypes.byref(pid)) == -4   # GVOM_ERR_CAPACITY
    with pytest.raises(gvom.GvomBackendError, match="gvom_score_attitude"):
        g._device_product(gvom.PRODUCT_ATTITUDE)
    with pytest.raises(gvom.GvomBackendError, match="unknown product kind"):
        g._device_product(13)
    # a stale map set: released and recycled by the next combine
    name = "one_round"
    s = gvom.Gvom(*ob.params(name), voxel_statistics=False)
    s.set_footprint(gvom.disc_footprint(0.5, s.xy_resolution))
    s.set_chassis(gvom.chassis(0.5, -0.3, 0.6, 0.3))
    s.process_pointcloud(*ob.scans(name)[0])
    m = s.combine_maps_device()
    old = m.set_id
    m.score_attitude(poses).release()
    m.release()
    s.process_pointcloud(*ob.scans(name)[1])
    s.combine_maps_device().release()                           # the unheld set was recycled: its id is stale
    with pytest.raises(gvom.GvomBackendError, match="unknown or stale device map set id"):
        s._check(s._lib.gvom_score_attitude(s._h, old, None, pp, 2, 3, 0, 0, oc, ctypes.byref(pid)))
    # bad chassis, as the library itself sees them
    good = gvom.chassis(0.5, -0.3, 0.6, 0.3)
    cs = np.array([[1.0, 0.0]])
    cs_ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    cset = lambda c, H, a: g._lib.gvom_chassis_set(g._h, ctypes.byref(c) if c is not None else None, H, cs_ptr(a) if a is not None else None)
    assert cset(good, 1, cs) == 0

    def variant(**kw):
        c = gvom.chassis(0.5, -0.3, 0.6, 0.3)
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    nan, inf = float("nan"), float("inf")
    for c, H, a in ((None, 1, cs), (good, 1, None), (good, 0, cs), (good, 1025, cs), (variant(front_axle=nan), 1, cs), (variant(track=inf), 1, cs),
                    (variant(belly_height=-inf), 1, cs), (variant(rear_axle=0.5), 1, cs), (variant(rear_axle=0.7), 1, cs), (variant(track=0.0), 1, cs),
                    (variant(track=-1.0), 1, cs), (variant(max_pitch=nan), 1, cs), (variant(max_roll=nan), 1, cs), (variant(min_clearance=nan), 1, cs),
                    (good, 1, np.array([[nan, 0.0]])), (good, 1, np.array([[1.0, inf]])), (good, 1, np.array([[1.0000001, 0.0]])),
                    (good, 2, np.array([[1.0, 0.0], [0.0, -1.5]]))):
        assert cset(c, H, a) == gvom.GVOM_ERR_INVALID
        assert g.get_tuning("chassis") == 1                     # a refused chassis leaves the one that is set
    assert cset(variant(max_pitch=inf, max_roll=0.0, min_clearance=-inf), 1, cs) == 0          # infinite limits are no errors
    sharded = gvom.Gvom(*_params(64), voxel_statistics=False, _shard=(0, 2))
    with pytest.raises(ValueError, match="sharded handles are not supported"):
        sharded.score_attitude_of(ground, poses)


def test_maps_of_more_than_4096_cells_a_side_are_refused(gvom):
    xy = 4100
    g = gvom.Gvom(0.4, 0.2, xy, 1, 1, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1, voxel_statistics=False)
    g.set_footprint(gvom.disc_footprint(0.5, 0.4))
    g.set_chassis(gvom.chassis(0.5, -0.3, 0.6, 0.3))
    with pytest.raises(gvom.GvomBackendError, match="4096"):
        g.score_attitude_of_device(1 << 20, 1 << 21, 1, 1)
    assert g.get_tuning("attitude_allocations") == 0


def _torch_case(name):
    """One case per fresh child process that imports torch BEFORE the library is loaded (one HIP runtime in the process)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_attitude_torch.py"), name],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "CASE OK " + name in r.stdout, r.stdout[-4000:]


def test_a_torch_planner_reads_the_attitude_on_a_side_stream():
    _torch_case("planner")
