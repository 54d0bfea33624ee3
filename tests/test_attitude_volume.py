"""Attitude volumes on the GPU (gvom_attitude_volume: k_volume_attitude_table, k_volume_attitude, k_attitude_ground;
gvom_pose_field_attitude: k_cspace_attitude; DeviceMaps.attitude_volume, Gvom.attitude_volume_of, Gvom.attitude_volume_of_device,
pose_field(attitude=...)) against the referee of tests/attitude_volume_ref.py with tolerance 0: status, tilt and counts of every state
on windows of 16, 31, 33, 64, 65 and 100 cells with 1, 4 and 16 headings, footprints of 1, 63, 64, 65 and 257 cells and the five
grounds of tests/attitude_ref.py, through host and device pointers and through real map sets with and without the inferred ground;
the volume against score_attitude() itself at the cell-centre poses; the masked pose field against its referee; a side slope that is
closed broadside and open nose-first; the identity without a volume; snapshots, the product pool, refusals, a recalled atlas set and
a torch consumer in a child process.  tests/test_attitude_volume_cpu.py holds the referee together and has the census of the inputs."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import atlas_ref
import attitude_ref as ar
import attitude_volume_ref as av
import costfield_ref as cf
import obstacle_scenes as ob
import posefield_ref as pf
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
    assert mod.PRODUCT_ATTITUDE_VOLUME == 30
    return mod


@pytest.fixture(scope="module")
def handles(gvom):
    return {xy: gvom.Gvom(*_params(xy, av.RES[xy]), voxel_statistics=False) for xy in av.SIZES}


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


def _hold(v, want, what, release=True):
    """a DeviceAttitudeVolume against the referee's (status, tilt, counts): all three parts, exactly; counts = the histogram of status"""
    status, tilt, counts = v.copy_to_host()
    H, xy, _ = want[0].shape
    assert status.dtype == np.uint8 and tilt.dtype == np.uint8 and counts.dtype == np.int32, what
    assert status.shape == tilt.shape == want[0].shape == v.status.shape == v.tilt.shape and counts.shape == (8,) == v.counts.shape, what
    assert v.status.strides == v.tilt.strides == (xy * xy, 1, xy) and v.status.ptr % 256 == 0 and v.tilt.ptr % 256 == 0 and v.counts.ptr % 256 == 0, what
    if not np.array_equal(status, want[0]):
        bad = np.argwhere(status != want[0])
        raise AssertionError("%s: the statuses differ in %d states, first (h %d, x %d, y %d): got %d, referee %d" % (
            what, len(bad), bad[0][0], bad[0][1], bad[0][2], status[tuple(bad[0])], want[0][tuple(bad[0])]))
    if not np.array_equal(tilt, want[1]):
        bad = np.argwhere(tilt != want[1])
        raise AssertionError("%s: the tilts differ in %d states, first (h %d, x %d, y %d): got %d, referee %d" % (
            what, len(bad), bad[0][0], bad[0][1], bad[0][2], tilt[tuple(bad[0])], want[1][tuple(bad[0])]))
    assert np.array_equal(counts, want[2]), (what, counts.tolist(), want[2].tolist())
    assert np.array_equal(counts[:7], np.bincount(status.ravel(), minlength=7)) and counts[7] == H, what
    if release:
        v.release()
    return status, tilt, counts


def _run(gvom, g, q, dev, device):
    """one case through the host or the device route"""
    g.set_footprint(q["table"])
    g.set_chassis(_chassis(gvom, q["chassis"]))
    assert np.array_equal(g.cos_sin, q["cos_sin"])                         # the referee turns with the numbers the library got
    if device:
        return g.attitude_volume_of_device(dev.upload(np.asfortranarray(q["g"]).T))      # cell (x, y) at [y * xy + x]
    return g.attitude_volume_of(q["g"])


@pytest.mark.parametrize("xy", av.SIZES)
def test_synthetic_inputs_match_the_referee_exactly(gvom, handles, xy):
    dev = _Device()
    try:
        for q, want in zip(av.cases(xy), av.expected(xy)):
            _hold(_run(gvom, handles[xy], q, dev, q["device"]), want, q["name"])
    finally:
        dev.free()


def test_host_and_device_routes_agree_and_the_limits_reach_every_status(gvom, handles):
    """every case of two sides through BOTH routes; the counts the library itself made say that every status 0 .. 5 occurs"""
    dev = _Device()
    seen = np.zeros(8, np.int64)
    try:
        for xy in (33, 100):
            for q, want in zip(av.cases(xy), av.expected(xy)):
                for device in (False, True):
                    v = _run(gvom, handles[xy], q, dev, device)
                    seen += v.counts.copy_to_host()
                    _hold(v, want, "%s, %s route" % (q["name"], "device" if device else "host"))
    finally:
        dev.free()
    print("states per status", seen[:7].tolist())
    assert (seen[:6] > 0).all() and seen[6] == 0


def _scene(gvom, name):
    g = gvom.Gvom(*ob.params(name), voxel_statistics=False)
    for pc, ego in ob.scans(name):
        g.process_pointcloud(pc, ego)
    return g


@pytest.mark.parametrize("name", cf.SCENES)
def test_scenes_through_real_map_sets_with_and_without_the_inferred_ground(gvom, name):
    """combine_maps_device().attitude_volume(...) after the ego has moved (the window's origin is not zero), against the referee fed
    with the set's own maps 4 and 5"""
    g = _scene(gvom, name)
    res, xy = g.xy_resolution, g.xy_size
    table = gvom.rectangle_footprint(0.9, 0.5, 0.45, res, headings=16, margin=0.1)
    g.set_footprint(table)
    ch = ar.make_chassis(0.7, -0.3, 0.8, 0.3, max_pitch=np.float32(np.tan(0.3)), max_roll=np.float32(np.tan(0.25)), min_clearance=np.float32(0.05))
    g.set_chassis(_chassis(gvom, ch))
    seen = {}
    dev = _Device()
    try:
        with g.combine_maps_device() as m:
            assert tuple(int(v) for v in np.round(np.asarray(m.origin)[:2] / res)) != (0, 0)
            height, inferred = m.height_map.copy_to_host(), m.inferred_height_map.copy_to_host()
            assert (height <= -1000).any() and (height > -1000).any() and ((height <= -1000) & (inferred > -1000)).any()
            for use in (True, False):
                ground = ar.ground_of(height, inferred, use)
                want = av.volume(ground, table, ch, g.cos_sin, res)
                seen[use] = _hold(m.attitude_volume(inferred_ground=use), want, "%s, inferred_ground=%r" % (name, use))
                by_pointer = g.attitude_volume_of_device(dev.upload(np.asfortranarray(ground).T))      # the same ground by pointer, read in place
                _hold(by_pointer, want, "%s, by pointer, inferred_ground=%r" % (name, use))
    finally:
        dev.free()
    for use in (True, False):
        print(name, "inferred" if use else "height only", "states per status", seen[use][2][:7].tolist())
    assert seen[True][2][ar.OK] > 0 and seen[False][2][ar.UNKNOWN_GROUND] > seen[True][2][ar.UNKNOWN_GROUND]


def test_the_volume_is_score_attitude_at_the_cell_centres(gvom):
    """the same GPU, the other kernel: the volume's status equals gvom_score_attitude's pose status on the float32 poses at the cell
    centres, with the car, at a window origin that is not zero"""
    xy, H, res, oc = 33, 16, 0.5, (37, -512)
    g = gvom.Gvom(*_params(xy, res), voxel_statistics=False)
    table = gvom.rectangle_footprint(rr.CAR["front"], rr.CAR["rear"], rr.CAR["half_width"], res, headings=H)
    ch = ar.make_chassis(max_pitch=np.float32(np.tan(0.2)), max_roll=np.float32(np.tan(0.17)), min_clearance=np.float32(0.02), **ar.CAR_CHASSIS)
    g.set_footprint(table)
    g.set_chassis(_chassis(gvom, ch))
    assert av.wheel_rules_agree(ch, g.cos_sin, res, xy, oc) == 0
    rng = np.random.default_rng(12)
    i, j = np.meshgrid(np.arange(xy, dtype=np.float64), np.arange(xy, dtype=np.float64), indexing="ij")
    ground = 0.6 * np.sin(i * 0.31) * np.cos(j * 0.27) + rng.uniform(0.0, 0.06, (xy, xy))
    ground[rng.random((xy, xy)) < 0.02] = np.nan
    assert (av.volume(ground, table, ch, g.cos_sin, res)[2][:6] > 0).all()     # the referee: this ground reaches every status
    poses = av.centre_poses(xy, H, res, oc)
    with g.attitude_volume_of(ground) as v, g.score_attitude_of(ground, poses, origin=(oc[0] * res, oc[1] * res)) as s:
        status, tilt, counts = v.copy_to_host()
        _, att, pose_status = s.copy_to_host()
    assert np.array_equal(status, pose_status.reshape(H, xy, xy))
    att = att.reshape(H, xy, xy, 3)
    assert np.array_equal(tilt, av.tilt_of(att[..., 0], att[..., 1], ch, status))
    assert (counts[:6] > 0).all(), counts.tolist()


# ---- into the pose field ---------------------------------------------------------------------------------------------------------------
def _field_hold(f, want, what):
    """a DevicePoseField against the referee's (C', D, action, seeds, info): the three volumes and the info, exactly"""
    C, D, A, seeds, info = want
    with f:
        cost, action, pose_cost = f.copy_to_host()
        assert np.array_equal(pose_cost, C), "%s: the pose cost volume differs in %d states" % (what, int((pose_cost != C).sum()))
        if not np.array_equal(cost, D):
            bad = np.argwhere(cost != D)
            h, x, y = bad[0]
            raise AssertionError("%s: the field differs in %d states, first at h %d cell (%d, %d): %d, the referee has %d"
                                 % (what, len(bad), h, x, y, cost[h, x, y], D[h, x, y]))
        assert np.array_equal(action, A), "%s: the actions differ in %d states" % (what, int((action != A).sum()))
        assert f.converged and (f.reached, f.goals_seeded) == info, (what, f.converged, f.reached, f.goals_seeded, info)
    return cost, action, pose_cost


def _field_case(gvom, xy):
    """a mapper with 16 headings, a small rectangle and arcs with reverse; a cost map, a rolling ground with holes, goals"""
    H, res = 16, 0.5
    g = gvom.Gvom(*_params(xy, res), voxel_statistics=False)
    footprint = gvom.rectangle_footprint(1.2, 0.6, 0.5, res, headings=H)
    table = gvom.arc_primitives(H, 2.0, res, reach=3, reverse_weight=2.5)
    ch = ar.make_chassis(1.0, -0.4, 0.9, 0.3, max_pitch=np.float32(0.3), max_roll=np.float32(0.25), min_clearance=np.float32(0.12))
    g.set_footprint(footprint)
    g.set_primitives(table)
    g.set_chassis(_chassis(gvom, ch))
    rng = np.random.default_rng(40 + xy)
    i, j = np.meshgrid(np.arange(xy, dtype=np.float64), np.arange(xy, dtype=np.float64), indexing="ij")
    ground = 0.5 * np.sin(i * 0.45) * np.cos(j * 0.4) + rng.uniform(0.0, 0.1, (xy, xy))
    ground[rng.random((xy, xy)) < 0.01] = -1000.0
    c = pf.cost_map(xy, 21, zeros=0.01)
    goals = np.array([(xy // 2, xy // 2, -1), (5, xy - 6, -1), (xy - 5, 4, -1)], np.int32)
    return dict(g=g, H=H, res=res, footprint=footprint, table=table, chassis=ch, ground=ground, c=c, goals=goals)


@pytest.mark.parametrize("xy", [33, 64])
@pytest.mark.parametrize("tilt_weight", [0, 7])
@pytest.mark.parametrize("blocks", [(ar.PITCH, ar.ROLL, ar.BELLY), (1, 2, 3, 4, 5)], ids=["limits", "all"])
def test_the_masked_pose_field_matches_its_referee(gvom, xy, tilt_weight, blocks):
    q = _field_case(gvom, xy)
    g = q["g"]
    status, tilt, counts = av.volume(q["ground"], q["footprint"], q["chassis"], g.cos_sin, q["res"])
    assert (counts[:6] > 0).all(), counts.tolist()
    want = av.field(q["c"], q["footprint"], q["table"], q["goals"], status, tilt, av.mask_of(blocks), tilt_weight)
    assert want[4][0] > 100 and (want[0] != pf.volume(q["c"], q["footprint"])).any()
    with g.attitude_volume_of(q["ground"]) as vol:
        f = g.pose_field_of(q["c"], q["goals"][:, :2], attitude=vol, attitude_blocks=blocks, tilt_weight=tilt_weight)
        _field_hold(f, want, "host cost map")
        with g.cost_to_go_of(q["c"], q["goals"][:1, :2]) as field:          # the same through a cost field's cell costs
            _field_hold(field.pose_field(q["goals"][:, :2], goals_in_cells=True, attitude=vol, attitude_blocks=blocks, tilt_weight=tilt_weight),
                        want, "a cost field")
        dev = _Device()
        try:
            ptr = dev.upload(np.asfortranarray(q["c"].astype(np.int32)).T)
            _field_hold(g.pose_field_of_device(ptr, q["goals"][:, :2], attitude=vol, attitude_blocks=blocks, tilt_weight=tilt_weight), want,
                        "device route")
        finally:
            dev.free()


def test_a_side_slope_is_closed_broadside_and_open_nose_first(gvom):
    """a plane tilted across y, max_roll below its slope and max_pitch above it: heading along x rolls over, heading along y climbs"""
    xy, H, res, slope = 40, 16, 0.5, 0.3
    g = gvom.Gvom(*_params(xy, res), voxel_statistics=False)
    car = gvom.rectangle_footprint(xy_resolution=res, headings=H, **pf.CAR)
    arcs = gvom.arc_primitives(H, 3.0, res, reach=3, reverse_weight=2.5)
    ch = ar.make_chassis(max_pitch=np.float32(0.4), max_roll=np.float32(0.2), min_clearance=np.float32(0.1), **ar.CAR_CHASSIS)
    g.set_footprint(car)
    g.set_primitives(arcs)
    g.set_chassis(_chassis(gvom, ch))
    ground = av.side_slope(xy, res, slope)
    c = np.full((xy, xy), 3, np.uint16)
    goal = (20, 30, 4)                                                      # heading 4 of 16: along +y, up the slope
    vol = g.attitude_volume_of(ground)
    status, tilt, counts = _hold(vol, av.volume(ground, car, ch, g.cos_sin, res), "side slope", release=False)
    for h in (0, 8):                                                        # along x, either way round
        assert np.isin(status[h], (ar.ROLL, ar.LEFT_WINDOW)).all() and (status[h] == ar.ROLL).sum() > 500
        assert (status[h, 8:-8, 8:-8] == ar.ROLL).all()
    for h in (4, 12):                                                       # along y
        assert np.isin(status[h], (ar.OK, ar.LEFT_WINDOW)).all() and (status[h, 8:-8, 8:-8] == ar.OK).all()
    plain = g.pose_field_of(c, [(goal[0], goal[1], np.pi / 2)])
    f = g.pose_field_of(c, [(goal[0], goal[1], np.pi / 2)], attitude=vol, tilt_weight=7)
    want = av.field(c, car, arcs, [goal], status, tilt, av.mask_of((ar.PITCH, ar.ROLL, ar.BELLY)), 7)
    cost, action, pose_cost = _field_hold(f, want, "side slope")
    reached = cost < pf.UNREACHED
    open_headings = {h for h in range(H) if reached[h].any()}
    print("headings with reached states", sorted(open_headings), "states", int(reached.sum()), "without the volume", plain.reached)
    assert 4 in open_headings and not open_headings & {0, 1, 7, 8, 9, 15} and reached.sum() < plain.reached
    assert (status[reached] == ar.OK).all() and (pose_cost[reached] != 0).all()
    assert all((status[h, 8:-8, 8:-8] == ar.OK).all() for h in open_headings)
    plain_cost = plain.copy_to_host()[0]
    assert (plain_cost[0] < pf.UNREACHED).any()                             # the field without the volume does drive broadside
    n = 0
    for x, y, h in ((8, 10, 4), (30, 12, 4), (12, 20, 3), (28, 25, 5), (20, 14, 4)):
        path = f.path_from(x, y, h)
        assert path is not None and path[-1] == goal, (x, y, h)
        for px, py, ph in path:
            assert status[ph, px, py] == ar.OK and pose_cost[ph, px, py] != 0
        assert pf.path_price(path, want[0], arcs) == cost[h, x, y]
        n += len(path)
    assert n > 20
    assert f.path_from(20, 20, 0) is None                                   # broadside: nowhere to go
    plain.release(); f.release(); vol.release()


def test_without_a_volume_and_with_an_idle_one_the_field_is_the_parents(gvom):
    """attitude=None is gvom_pose_field; a volume whose every state is OK, with tilt_weight 0, changes no bit either"""
    i = [k for k, q in enumerate(pf.cases()) if q["name"] == "xy40 H16 car arcs random"][0]
    q = pf.cases()[i]
    g = gvom.Gvom(*_params(q["xy"], 0.5), voxel_statistics=False)
    g.set_footprint(q["footprint"])
    g.set_primitives(q["table"])
    goals = pf.goals_for_binding(q["goals"], q["H"])
    want = pf.expected(i)
    allocs = g.get_tuning("pose_field_allocations")
    _field_hold(g.pose_field_of(q["c"], goals), want, "no keyword")
    _field_hold(g.pose_field_of(q["c"], goals, attitude=None, tilt_weight=0), want, "attitude=None")
    assert g.get_tuning("attitude_volume_allocations") == 0 and g.get_tuning("pose_field_allocations") > allocs
    g.set_chassis(gvom.chassis(ar.CAR_CHASSIS["front_axle"], ar.CAR_CHASSIS["rear_axle"], ar.CAR_CHASSIS["track"], 10.0))      # no limits, a high belly
    ground = np.zeros((q["xy"], q["xy"]))
    with g.attitude_volume_of(ground) as vol:
        status, tilt, counts = vol.copy_to_host()
        assert set(np.unique(status)) == {ar.OK, ar.LEFT_WINDOW} and (tilt == 0).all()
        steady = g.get_tuning("pose_field_allocations")
        # (a state that leaves the window has pose cost 0 already: blocking LEFT_WINDOW too changes nothing)
        for blocks, w in (((ar.PITCH, ar.ROLL, ar.BELLY), 0), ((), 0), ((ar.LEFT_WINDOW,), 0), ((ar.PITCH, ar.ROLL, ar.BELLY), 255)):
            _field_hold(g.pose_field_of(q["c"], goals, attitude=vol, attitude_blocks=blocks, tilt_weight=w), want, "idle volume %r %d" % (blocks, w))
        assert g.get_tuning("pose_field_allocations") == steady


# ---- the product -----------------------------------------------------------------------------------------------------------------------
def test_the_products_are_snapshots(gvom):
    name = "one_round"
    g = gvom.Gvom(*ob.params(name), voxel_statistics=False)
    scans = ob.scans(name)
    res, xy = g.xy_resolution, g.xy_size
    g.set_footprint(gvom.rectangle_footprint(0.9, 0.5, 0.45, res, headings=8))
    g.set_primitives(gvom.arc_primitives(8, 1.0, res, reach=3))
    g.set_chassis(gvom.chassis(0.7, -0.3, 0.8, 0.3, max_pitch=0.3, max_roll=0.25, min_clearance=0.05))
    g.process_pointcloud(*scans[0])
    c = np.full((xy, xy), 2, np.uint16)
    with g.combine_maps_device() as m:
        held = m.attitude_volume()
        field = g.pose_field_of(c, [(xy // 2, xy // 2)], attitude=held, tilt_weight=3)
    before, field_before = held.copy_to_host(), field.copy_to_host()
    assert (before[0] == ar.OK).any() and (before[0] != ar.OK).any() and field.reached > 0
    for pc, ego in scans[1:]:
        g.process_pointcloud(pc, ego)
        with g.combine_maps_device() as m:
            g.set_footprint(gvom.rectangle_footprint(1.5, 0.5, 0.6, res, headings=8))
            g.set_chassis(gvom.chassis(1.2, -0.2, 0.9, 0.2, max_pitch=0.2, max_roll=0.2, min_clearance=0.1))
            later = m.attitude_volume()
            assert later.status.ptr != held.status.ptr
            now = later.copy_to_host()
            later_field = g.pose_field_of(c, [(xy // 2, xy // 2)], attitude=later, tilt_weight=3)
            assert later_field.cost.ptr != field.cost.ptr
            later_field.release()
            later.release()
    after, field_after = held.copy_to_host(), field.copy_to_host()
    assert all(np.array_equal(a, b) for a, b in zip(before, after)) and all(np.array_equal(a, b) for a, b in zip(field_before, field_after))
    assert not np.array_equal(now[0], after[0])                     # the map, the footprint and the chassis have moved on; the held products have not


def test_pool_capacity_reuse_and_no_allocation_in_steady_state(gvom):
    xy = 64
    g = gvom.Gvom(*_params(xy, av.RES[xy]), voxel_statistics=False)
    assert g.get_tuning("attitude_volume") == 1 and g.get_tuning("attitude_volume_allocations") == 0
    q, want = av.cases(xy)[0], av.expected(xy)[0]
    before = [g.get_tuning(n) for n in ("rollout_allocations", "attitude_allocations")]
    g.set_footprint(q["table"])
    g.set_chassis(_chassis(gvom, q["chassis"]))
    assert g.get_tuning("attitude_volume_allocations") == 0         # the two setters build nothing for the volume
    assert [g.get_tuning(n) for n in ("rollout_allocations", "attitude_allocations")] == before
    first = g.attitude_volume_of(q["g"])
    assert g.get_tuning("attitude_volume_allocations") == 3         # the product set, the table and the host staging buffer
    assert g.get_tuning("device_product_sets") == 1
    ptr = first.status.ptr
    first.release()
    for _ in range(3):                                              # released: everything is reused
        v = g.attitude_volume_of(q["g"])
        assert v.status.ptr == ptr
        _hold(v, want, "reused set")
    assert g.get_tuning("attitude_volume_allocations") == 3 and g.get_tuning("device_product_sets") == 1
    # replacing the chassis between calls: the next call rebuilds its table in place and scores with the new one
    other = ar.make_chassis(1.1 * q["res"], -2.2 * q["res"], 1.4 * q["res"], 0.5 * q["res"], max_roll=np.float32(0.2))
    g.set_chassis(_chassis(gvom, other))
    _hold(g.attitude_volume_of(q["g"]), av.volume(q["g"], q["table"], other, q["cos_sin"], q["res"]), "after set_chassis")
    g.set_chassis(_chassis(gvom, q["chassis"]))
    _hold(g.attitude_volume_of(q["g"]), want, "the first chassis again")
    assert g.get_tuning("attitude_volume_allocations") == 3
    assert [g.get_tuning(n) for n in ("rollout_allocations", "attitude_allocations")] == before
    held = [g.attitude_volume_of(q["g"]) for _ in range(4)]
    assert len({v.status.ptr for v in held}) == 4 and g.get_tuning("device_product_sets") == 4
    with pytest.raises(gvom.GvomBackendError, match="all 4 device product sets of this kind"):
        g.attitude_volume_of(q["g"])
    held[2].release()
    allocs = g.get_tuning("attitude_volume_allocations")
    _hold(g.attitude_volume_of(q["g"]), want, "after a release")
    assert g.get_tuning("device_product_sets") == 4 and g.get_tuning("attitude_volume_allocations") == allocs
    for k in (0, 1, 3):                                             # (the set of held[2] has been handed out again: its id is stale)
        _hold(held[k], want, "held")
    with pytest.raises(gvom.GvomBackendError, match="unknown or stale device product id"):
        held[2].copy_to_host()


def test_refusals(gvom):
    xy = 32
    g = gvom.Gvom(*_params(xy), voxel_statistics=False)
    ground = np.zeros((xy, xy))
    with pytest.raises(ValueError, match="no footprint table is set"):
        g.attitude_volume_of(ground)
    g.set_footprint(gvom.rectangle_footprint(0.5, 0.5, 0.4, 0.4, headings=8))
    with pytest.raises(ValueError, match="no chassis is set"):
        g.attitude_volume_of(ground)
    g.set_chassis(gvom.chassis(0.5, -0.3, 0.6, 0.3))
    g.set_footprint(gvom.disc_footprint(0.5, 0.4))                 # one heading now: the chassis was set for eight
    with pytest.raises(ValueError, match="another number of headings"):
        g.attitude_volume_of(ground)
    assert g.get_tuning("attitude_volume_allocations") == 0
    with pytest.raises(ValueError, match="device address"):
        g.attitude_volume_of_device(0)
    with pytest.raises(ValueError):
        g.attitude_volume_of(np.zeros((xy, xy + 1)))
    g.set_footprint(gvom.rectangle_footprint(0.5, 0.5, 0.4, 0.4, headings=8))
    g.set_chassis(gvom.chassis(0.5, -0.3, 0.6, 0.3))
    g.set_primitives(gvom.arc_primitives(8, 1.0, 0.4, reach=3))
    pid = ctypes.c_int64(-1)
    gp = ground.ctypes.data_as(ctypes.c_void_p)

    def raw(set_id=-1, gr=gp, flags=0, out=pid):
        return g._check(g._lib.gvom_attitude_volume(g._h, set_id, gr, 0, flags, ctypes.byref(out) if out is not None else None))
    assert raw() == 0 and pid.value >= 0
    vol_id = pid.value
    for kw, word in ((dict(set_id=10 ** 9, gr=None), "unknown or stale device map set id"), (dict(set_id=1), "not both"),
                     (dict(gr=None), "a map set id or a ground map"), (dict(flags=2), "unknown flag bits")):
        with pytest.raises(gvom.GvomBackendError, match=word):
            raw(**kw)
        assert pid.value == -1
    assert g._lib.gvom_attitude_volume(g._h, -1, gp, 0, 0, None) == gvom.GVOM_ERR_INVALID               # NULL product_id
    with pytest.raises(gvom.GvomBackendError, match="unknown product kind"):
        g._device_product(gvom.PRODUCT_ATTITUDE_VOLUME)
    with pytest.raises(gvom.GvomBackendError, match="unknown product kind"):
        g._device_product(29)
    # the pose field's side: the mask, the weight, and what volume_id may name
    c = np.full((xy, xy), 2, np.int32)
    goals = np.array([[3, 3, -1]], np.int32)
    info = (ctypes.c_int64 * 4)()
    assert raw() == 0
    vol_id = pid.value
    fid = ctypes.c_int64(-1)

    def field(volume=None, mask=0xe, w=0):
        return g._lib.gvom_pose_field_attitude(g._h, -1, c.ctypes.data_as(ctypes.c_void_p), 0, vol_id if volume is None else volume, mask, w,
                                               goals.ctypes.data_as(ctypes.c_void_p), 1, 0, 0, ctypes.byref(fid), info)
    assert field() == 0 and fid.value >= 0
    field_id = fid.value
    for kw, word in ((dict(mask=0x80), "block_mask"), (dict(w=-1), "tilt_weight"), (dict(w=256), "tilt_weight"), (dict(volume=-1), "attitude volume id"),
                     (dict(volume=10 ** 9), "attitude volume id"), (dict(volume=field_id), "attitude volume id")):
        assert field(**kw) == gvom.GVOM_ERR_INVALID and fid.value == -1, kw
        assert word in g._lib.gvom_last_error(g._h).decode() and "gvom_pose_field_attitude" in g._lib.gvom_last_error(g._h).decode(), kw
    assert raw() == 0                                                # the next volume call takes the unexported set back: the old id is stale
    assert pid.value != vol_id and field() == gvom.GVOM_ERR_INVALID and field(volume=pid.value) == 0
    # a volume of another number of headings
    keep = g.attitude_volume_of(ground)
    g.set_footprint(gvom.rectangle_footprint(0.5, 0.5, 0.4, 0.4, headings=4))
    g.set_primitives(gvom.arc_primitives(4, 0.5, 0.4, reach=3))
    with pytest.raises(ValueError, match="another number of headings"):
        g.pose_field_of(c, [(3, 3)], attitude=keep)
    keep.release()
    # another window side
    other = gvom.Gvom(*_params(16), voxel_statistics=False)
    other.set_footprint(gvom.rectangle_footprint(0.5, 0.5, 0.4, 0.4, headings=4))
    other.set_chassis(gvom.chassis(0.5, -0.3, 0.6, 0.3))
    small = other.attitude_volume_of(np.zeros((16, 16)))
    with pytest.raises(ValueError, match="attitude volume id"):      # (ids are per mapper: another mapper's volume is no volume of this one)
        g.pose_field_of(c, [(3, 3)], attitude=small)
    small.release()
    with pytest.raises(TypeError):
        g.pose_field_of(c, [(3, 3)], attitude=ground)
    with pytest.raises(ValueError, match="tilt_weight"):
        g.pose_field_of(c, [(3, 3)], tilt_weight=3)
    # more than 64 headings
    many = gvom.Gvom(*_params(16), voxel_statistics=False)
    many.set_footprint(gvom.rectangle_footprint(0.5, 0.5, 0.4, 0.4, headings=128))
    many.set_chassis(gvom.chassis(0.5, -0.3, 0.6, 0.3))
    with pytest.raises(gvom.GvomBackendError, match="more than 64 headings"):
        many.attitude_volume_of(np.zeros((16, 16)))
    assert many.get_tuning("attitude_volume_allocations") == 0
    sharded = gvom.Gvom(*_params(64), voxel_statistics=False, _shard=(0, 2))
    with pytest.raises(ValueError, match="sharded handles are not supported"):
        sharded.attitude_volume_of(np.zeros((64, 64)))


def test_more_than_4096_cells_a_side_and_more_than_2_to_the_28_states_are_refused(gvom):
    g = gvom.Gvom(0.4, 0.2, 4100, 1, 1, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1, voxel_statistics=False)
    g.set_footprint(gvom.disc_footprint(0.5, 0.4))
    g.set_chassis(gvom.chassis(0.5, -0.3, 0.6, 0.3))
    with pytest.raises(gvom.GvomBackendError, match="4096"):
        g.attitude_volume_of_device(1 << 20)
    assert g.get_tuning("attitude_volume_allocations") == 0
    g = gvom.Gvom(0.4, 0.2, 4096, 1, 1, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1, voxel_statistics=False)
    g.set_footprint(gvom.rectangle_footprint(0.5, 0.5, 0.4, 0.4, headings=32))         # 32 x 4096^2 = 2^29 states
    g.set_chassis(gvom.chassis(0.5, -0.3, 0.6, 0.3))
    with pytest.raises(gvom.GvomBackendError, match="2\\^28 states"):
        g.attitude_volume_of_device(1 << 20)
    assert g.get_tuning("attitude_volume_allocations") == 0


def test_a_recalled_atlas_set_works(gvom):
    """the volume of a set recalled from the atlas equals the volume of its own host copies"""
    xy, res = atlas_ref.DRIVE_XY, atlas_ref.DRIVE_RES
    g = gvom.Gvom(res, atlas_ref.DRIVE_ZRES, xy, 8, 1, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1, voxel_statistics=False)
    a = g.create_atlas(atlas_ref.DRIVE_A)
    first = None
    for pc, ego in atlas_ref.drive_scans()[:4]:
        g.process_pointcloud(pc, ego)
        with g.combine_maps_device() as m:
            a.integrate(m)
            first = first or m.origin_cells[:2]
    table = gvom.rectangle_footprint(0.9, 0.5, 0.45, res, headings=16, margin=0.1)
    ch = ar.make_chassis(0.7, -0.3, 0.8, 0.3, max_pitch=np.float32(0.3), max_roll=np.float32(0.25), min_clearance=np.float32(0.05))
    g.set_footprint(table)
    g.set_chassis(_chassis(gvom, ch))
    with a.recall(origin_cells=first) as m:
        height, inferred = m.height_map.copy_to_host(), m.inferred_height_map.copy_to_host()
        assert (height > -1000).sum() > 500
        for use in (True, False):
            want = av.volume(ar.ground_of(height, inferred, use), table, ch, g.cos_sin, res)
            status, _, counts = _hold(m.attitude_volume(inferred_ground=use), want, "recalled, inferred_ground=%r" % use)
        assert counts[ar.OK] > 0 or (status == ar.UNKNOWN_GROUND).any()


def _torch_case(name):
    """One case per fresh child process that imports torch BEFORE the library is loaded (one HIP runtime in the process)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_attitude_volume_torch.py"), name],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "CASE OK " + name in r.stdout, r.stdout[-4000:]


def test_a_torch_consumer_reads_the_status_through_dlpack():
    _torch_case("consumer")
