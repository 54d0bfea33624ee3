"""Body volumes on the GPU (gvom_body_volume: k_volume_body; gvom_pose_field_volumes: k_cspace_attitude a second time;
DeviceDistanceField.body_volume / body_volume_of, Gvom.body_volume_of / body_volume_of_device, pose_field(body=...)) against the referee
of tests/body_volume_ref.py: status, squeeze, clearance and counts with tolerance 0, floats by bit pattern.

  callers' fields and grounds   the grids of body_ref: 16 x 16 x 8 at 0.4 / 0.4 m, 33 x 33 x 8 at 0.25 and 40 x 40 x 6 at 0.3 / 0.2 m (33 and
                   40 leave partial tiles and partial waves on both axes); H of 1, 7 and 16; S of 1, 2, 64, 65 and 256; field boxes off the
                   window and below zero; the five grounds of attitude_ref; host and device routes; a field with NaN
  other kernels    on the 33-cell grid the volume equals score_body() itself at the cell-centre poses
  the pose field   body only, attitude only (pose_field(attitude=...) bit for bit), both, neither (the parent's pose_field), squeeze_weight 0
                   and 255, masks that block nothing and everything -- against the referee's field()
  real products    the two scenes of tests/body_volume_scenes.py: scan, combine_maps_device(), integrate(), distance_field(),
                   body_volume(), pose_field(body=...), path_from(); the physical statement, and every part against the referee fed from the
                   products' own host copies
  lifecycle        snapshots; the field released right after the call; the pool and "body_volume_allocations"; refusals; a recalled atlas
                   set as the ground; DLPack (a torch child)

tests/test_body_volume_cpu.py holds the census of every input and the two forms of the referee together."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import atlas_ref
import attitude_ref as ar
import attitude_volume_ref as avr
import body_ref as br
import body_scenes as bs
import body_volume_ref as bv
import body_volume_scenes as bvs
import obstacle_scenes
import posefield_ref as pf
import voxel_atlas_ref as va

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = va.DRIVE_TAIL


@pytest.fixture(scope="module")
def gvom():
    import gvom as mod
    rc, info = mod.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    assert mod.PRODUCT_BODY_VOLUME == 46
    return mod


@pytest.fixture(scope="module")
def handles(gvom):
    return {xy: gvom.Gvom(res, zres, xy, zs, 1, *TAIL, voxel_statistics=False) for xy, (res, zres, zs, _, _) in bv.GRIDS.items()}


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
    c = gvom.chassis(ch.front_axle, ch.rear_axle, ch.track, ch.belly_height)
    c.max_pitch, c.max_roll, c.min_clearance = ch.max_pitch, ch.max_roll, ch.min_clearance
    return c


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _hold(v, want, what, release=True):
    """a DeviceBodyVolume against the referee's (status, squeeze, clearance, counts): all four parts, exactly"""
    status, squeeze, clr, counts = v.copy_to_host()
    H, xy, _ = want[0].shape
    assert status.dtype == np.uint8 and squeeze.dtype == np.uint8 and clr.dtype == np.float32 and counts.dtype == np.int32, what
    assert status.shape == squeeze.shape == clr.shape == want[0].shape == v.status.shape == v.squeeze.shape == v.clearance.shape, what
    assert counts.shape == (8,) == v.counts.shape, what
    assert v.status.strides == v.squeeze.strides == v.clearance.strides == (xy * xy, 1, xy), what
    assert all(p.ptr % 256 == 0 for p in (v.status, v.squeeze, v.clearance, v.counts)), what
    for name, got, ref in (("statuses", status, want[0]), ("squeezes", squeeze, want[1]), ("clearances", _bits(clr), _bits(want[2]))):
        if not np.array_equal(got, ref):
            bad = np.argwhere(got != ref)
            h, x, y = bad[0]
            raise AssertionError("%s: the %s differ in %d states, first (h %d, x %d, y %d): got %r, referee %r (status %d / %d, clearance %r / %r)" % (
                what, name, len(bad), h, x, y, got[h, x, y], ref[h, x, y], status[h, x, y], want[0][h, x, y], clr[h, x, y], want[2][h, x, y]))
    assert np.array_equal(counts, want[3]), (what, counts.tolist(), want[3].tolist())
    assert np.array_equal(counts[:6], np.bincount(status.ravel(), minlength=6)) and counts[6] == H, what
    if release:
        v.release()
    return status, squeeze, clr, counts


def _setup(gvom, g, q):
    g.set_footprint(q["table"])
    g.set_chassis(_chassis(gvom, q["chassis"]))
    assert np.array_equal(g.cos_sin, q["cos_sin"])                         # the referee turns with the numbers the library got
    g.set_body(q["body"])


def _run(gvom, g, q, dev, device):
    """one case through the host or the device route"""
    _setup(gvom, g, q)
    B = np.array(q["field_origin"], np.int64)
    kw = dict(origin=q["origin"], min_margin=q["min_margin"], soft_margin=q["soft_margin"])
    if device:
        gp = dev.upload(np.asfortranarray(q["g"]).T)                       # cell (x, y) at [y * xy + x]
        return g.body_volume_of_device(dev.upload(q["field"]), B, gp, **kw)
    return g.body_volume_of(q["field"], B, q["g"], **kw)


@pytest.mark.parametrize("i", range(len(bv.cases())), ids=[q["name"].replace(" ", "-") for q in bv.cases()])
def test_synthetic_inputs_match_the_referee_exactly(gvom, handles, i):
    q, want = bv.cases()[i], bv.expected()[i]
    dev = _Device()
    try:
        _hold(_run(gvom, handles[q["xy"]], q, dev, q["device"]), want, q["name"])
    finally:
        dev.free()


def test_host_and_device_routes_agree_and_soft_margin_defaults_to_min_margin(gvom, handles):
    dev = _Device()
    seen = np.zeros(8, np.int64)
    try:
        for i in (1, 4, 7):                                                 # 33 / H7 / S64, 40 / H16 / S1, the NaN field
            q, want = bv.cases()[i], bv.expected()[i]
            for device in (False, True):
                v = _run(gvom, handles[q["xy"]], q, dev, device)
                seen += v.counts.copy_to_host()
                _hold(v, want, "%s, %s route" % (q["name"], "device" if device else "host"))
        q = bv.cases()[1]
        g = handles[q["xy"]]
        _setup(gvom, g, q)
        same = dict(q, soft_margin=q["min_margin"])
        _hold(g.body_volume_of(q["field"], np.array(q["field_origin"]), q["g"], origin=q["origin"], min_margin=q["min_margin"]), bv.score_case(same),
              "soft_margin=None")
    finally:
        dev.free()
    print("states per status", seen[:6].tolist())
    assert (seen[:5] > 0).all() and seen[5] == 0


def test_the_volume_is_score_body_at_the_cell_centres(gvom, handles):
    """the same GPU, the other kernel: on the 33-cell grid (res 0.25: the centres are float32 numbers, the two wheel rules agree) status,
    clearance bits and the squeeze derived from score_body()'s clearance equal the volume's"""
    dev = _Device()
    try:
        for q in [q for q in bv.cases() if q["xy"] == 33 and len(q["cos_sin"]) == 7]:
            g = handles[33]
            H, xy = 7, 33
            assert avr.wheel_rules_agree(q["chassis"], q["cos_sin"], q["res"], xy, q["origin_cells"]) == 0
            poses = avr.centre_poses(xy, H, q["res"], q["origin_cells"])
            v = _run(gvom, g, q, dev, False)
            status, squeeze, clr, counts = v.copy_to_host()
            v.release()
            with g.score_body_of(q["field"], np.array(q["field_origin"]), q["g"], poses, origin=q["origin"], min_margin=q["min_margin"]) as r:
                _, pose_clr, pairs = r.copy_to_host()
            assert np.array_equal(pairs[..., 0].reshape(H, xy, xy), status), q["name"]
            assert np.array_equal(_bits(pose_clr.reshape(H, xy, xy)), _bits(clr)), q["name"]
            assert np.array_equal(bv.squeeze_of(pose_clr, pairs[..., 0], q["min_margin"], q["soft_margin"]).reshape(H, xy, xy), squeeze), q["name"]
            assert (counts[:3] > 0).all(), counts.tolist()
    finally:
        dev.free()


# ---- into the pose field ---------------------------------------------------------------------------------------------------------------
def _field_hold(f, want, what):
    """a DevicePoseField against the referee's (C'', D, action, seeds, info): the three volumes and the info, exactly"""
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


@pytest.fixture(scope="module")
def field_case(gvom):
    """a mapper with 16 headings, a small rectangle and arcs with reverse on the 33-cell grid; a cost map, a rolling ground with holes, a
    field of distances, a body; the two volumes (on the GPU and from the referees) and the goals"""
    xy, H = 33, 16
    res, zres, zs, oc, fo = bv.GRIDS[xy]
    g = gvom.Gvom(res, zres, xy, zs, 1, *TAIL, voxel_statistics=False)
    footprint = gvom.rectangle_footprint(0.6, 0.3, 0.25, res, headings=H)
    table = gvom.arc_primitives(H, 1.0, res, reach=3, reverse_weight=2.5)
    ch = ar.make_chassis(0.5, -0.2, 0.45, 0.15, max_pitch=np.float32(0.3), max_roll=np.float32(0.25), min_clearance=np.float32(0.06))
    g.set_footprint(footprint)
    g.set_primitives(table)
    g.set_chassis(_chassis(gvom, ch))
    rng = np.random.default_rng(73)
    i, j = np.meshgrid(np.arange(xy, dtype=np.float64), np.arange(xy, dtype=np.float64), indexing="ij")
    ground = 0.25 * np.sin(i * 0.45) * np.cos(j * 0.4) + rng.uniform(0.0, 0.05, (xy, xy))
    ground[rng.random((xy, xy)) < 0.01] = -1000.0
    field = br.random_field(xy, zs, res, zres, 19)
    body = br.random_body(6, res, zres, 3)
    B = (fo[0], fo[1], -1)
    g.set_body(body)
    mm, sm = np.float32(0.1), np.float32(0.9)
    bvol = bv.volume(field, B, ground, body, ch, g.cos_sin, res, zres, oc, mm, sm)
    avol = avr.volume(ground, footprint, ch, g.cos_sin, res)
    assert (bvol[3][:5] > 20).all() and ((bvol[1] > 0) & (bvol[1] < 100)).sum() > 100, bvol[3].tolist()
    c = pf.cost_map(xy, 21, zeros=0.01)
    goals = np.array([(xy // 2, xy // 2, -1), (5, xy - 6, -1), (xy - 5, 4, -1)], np.int32)
    body_dev = g.body_volume_of(field, np.array(B), ground, origin=(oc[0] * res, oc[1] * res), min_margin=mm, soft_margin=sm)
    _hold(body_dev, bvol, "the field case's body volume", release=False)
    att_dev = g.attitude_volume_of(ground)
    yield dict(g=g, footprint=footprint, table=table, c=c, goals=goals, bvol=bvol, avol=avol, body=body_dev, attitude=att_dev)
    body_dev.release()
    att_dev.release()


@pytest.mark.parametrize("weight", [0, 255])
@pytest.mark.parametrize("blocks", [(), (bv.COLLISION, bv.LEFT_BOX), (0, 1, 2, 3, 4, 5)], ids=["nothing", "default", "everything"])
def test_the_body_masked_pose_field_matches_its_referee(gvom, field_case, weight, blocks):
    q = field_case
    g = q["g"]
    want = bv.field(q["c"], q["footprint"], q["table"], q["goals"], None, (q["bvol"][0], q["bvol"][1], avr.mask_of(blocks), weight))
    plain = pf.volume(q["c"], q["footprint"])
    if len(blocks) == 6:
        assert not want[0].any() and want[4] == (0, 0)                      # every status blocked: nothing is left
    elif blocks or weight:
        assert want[4][0] > 100 and (want[0] != plain).any()
    else:
        assert np.array_equal(want[0], plain)                               # nothing blocked, no weight: the parent's cost volume
    f = g.pose_field_of(q["c"], q["goals"][:, :2], body=q["body"], body_blocks=blocks, squeeze_weight=weight)
    _field_hold(f, want, "host cost map")
    if weight == 255 and len(blocks) == 2:
        with g.cost_to_go_of(q["c"], q["goals"][:1, :2]) as field:          # the same through a cost field's cell costs, and by pointer
            _field_hold(field.pose_field(q["goals"][:, :2], goals_in_cells=True, body=q["body"], body_blocks=blocks, squeeze_weight=weight), want,
                        "a cost field")
        dev = _Device()
        try:
            ptr = dev.upload(np.asfortranarray(q["c"].astype(np.int32)).T)
            _field_hold(g.pose_field_of_device(ptr, q["goals"][:, :2], body=q["body"], body_blocks=blocks, squeeze_weight=weight), want, "device route")
        finally:
            dev.free()


def test_both_volumes_one_volume_and_none_compose_as_defined(gvom, field_case):
    q = field_case
    g = q["g"]
    a_blocks, tilt_weight, b_blocks, squeeze_weight = (ar.PITCH, ar.ROLL, ar.BELLY), 7, (bv.COLLISION, bv.LEFT_BOX), 3
    att = (q["avol"][0], q["avol"][1], avr.mask_of(a_blocks), tilt_weight)
    body = (q["bvol"][0], q["bvol"][1], avr.mask_of(b_blocks), squeeze_weight)
    goals = q["goals"][:, :2]
    # both: the attitude volume first, then the body volume
    both = bv.field(q["c"], q["footprint"], q["table"], q["goals"], att, body)
    only_a = bv.field(q["c"], q["footprint"], q["table"], q["goals"], att, None)
    only_b = bv.field(q["c"], q["footprint"], q["table"], q["goals"], None, body)
    assert (both[0] != only_a[0]).any() and (both[0] != only_b[0]).any() and both[4][0] > 100
    _field_hold(g.pose_field_of(q["c"], goals, attitude=q["attitude"], attitude_blocks=a_blocks, tilt_weight=tilt_weight, body=q["body"],
                                body_blocks=b_blocks, squeeze_weight=squeeze_weight), both, "both volumes")
    # attitude only: pose_field(attitude=...) as it was, and gvom_pose_field_volumes with body_volume_id = -1, bit for bit
    parent = _field_hold(g.pose_field_of(q["c"], goals, attitude=q["attitude"], attitude_blocks=a_blocks, tilt_weight=tilt_weight), only_a, "attitude only")
    assert all(np.array_equal(x, y) for x, y in zip(only_a[:4], avr.field(q["c"], q["footprint"], q["table"], q["goals"], *att)[:4]))
    c32 = np.ascontiguousarray(np.asfortranarray(q["c"].astype(np.int32)).T)
    cells = np.ascontiguousarray(q["goals"], np.int32)
    info, pid = (ctypes.c_int64 * 4)(), ctypes.c_int64(-1)

    def raw(a_id, a_mask, a_w, b_id, b_mask, b_w):
        rc = g._lib.gvom_pose_field_volumes(g._h, -1, c32.ctypes.data_as(ctypes.c_void_p), 0, a_id, a_mask, a_w, b_id, b_mask, b_w,
                                            cells.ctypes.data_as(ctypes.c_void_p), len(cells), 0, 0, ctypes.byref(pid), info)
        assert rc == 0, g._lib.gvom_last_error(g._h)
        out = []
        for part, dt in ((0, np.int32), (1, np.uint8), (2, np.uint16)):
            a = np.empty((16, 33, 33), dt)
            g._check(g._lib.gvom_device_product_copy(g._h, pid.value, part, ctypes.c_void_p(a.ctypes.data)))
            out.append(a.transpose(0, 2, 1))
        return out
    got = raw(q["attitude"].product_id, avr.mask_of(a_blocks), tilt_weight, -1, 0, 0)
    assert all(np.array_equal(x, y) for x, y in zip(got, parent)), "gvom_pose_field_volumes without a body volume is gvom_pose_field_attitude"
    # neither: the parent's pose_field
    none = pf.field(q["c"], q["footprint"], q["table"], q["goals"])
    plain = _field_hold(g.pose_field_of(q["c"], goals), none, "no keyword")
    _field_hold(g.pose_field_of(q["c"], goals, body=None, squeeze_weight=0, attitude=None, tilt_weight=0), none, "body=None")
    got = raw(-1, 0, 0, -1, 0, 0)
    assert all(np.array_equal(x, y) for x, y in zip(got, plain)), "gvom_pose_field_volumes without a volume is gvom_pose_field"
    # body only through the raw entry point equals the keyword route
    got = raw(-1, 0, 0, q["body"].product_id, avr.mask_of(b_blocks), squeeze_weight)
    assert np.array_equal(got[2], only_b[0]) and np.array_equal(got[0], only_b[1]) and np.array_equal(got[1], only_b[2])


# ---- real products ------------------------------------------------------------------------------------------------------------------------
def _scene(gvom, bar):
    """one scan of a scene of tests/body_volume_scenes.py through combine_maps_device() and integrate()"""
    S = bvs.SCENE
    g = gvom.Gvom(S["res"], S["zres"], S["xy"], S["zs"], 1, *TAIL, voxel_statistics=False)
    g.process_pointcloud(bvs.cloud(bar), S["ego"])
    m = g.combine_maps_device()
    atlas = g.create_voxel_atlas(64, 16)
    assert atlas.integrate() is True
    footprint, prims = bvs.tables()
    g.set_footprint(footprint)
    g.set_primitives(prims)
    g.set_chassis(_chassis(gvom, bvs.CHASSIS))
    return g, atlas, m


@pytest.mark.parametrize("bar", ["half", "full"])
def test_the_scenes_statement_through_real_products(gvom, bar):
    """the low vehicle drives under the bar, the tall one round its end (half) or nowhere (full): scan, combine, integrate, distance field,
    body volume, pose field, path -- and every product against the referee fed from the products' own host copies"""
    g, atlas, m = _scene(gvom, bar)
    seen = {}
    with m:
        f = atlas.distance_field(bvs.CAP)
        W = tuple(int(v) for v in f.origin_voxels)
        field = f.distance.copy_to_host()
        ground = ar.ground_of(m.height_map.copy_to_host(), m.inferred_height_map.copy_to_host(), True)
        ref = bvs.referee_fields(bar, field, W, ground)
        for name, body in sorted(bs.bodies().items()):
            g.set_body(body)
            want = ref[name]
            vol = f.body_volume(m, min_margin=bvs.MIN_MARGIN, soft_margin=bvs.SOFT_MARGIN)
            _hold(vol, want["volume"], "%s, %s body" % (bar, name), release=False)
            pfield = g.pose_field_of(bvs.cost_map(), [want["goal"][:2]], origin=m.origin, body=vol, body_blocks=bvs.BLOCKS,
                                     squeeze_weight=bvs.SQUEEZE_WEIGHT)
            cost, action, pose_cost = pfield.copy_to_host()
            assert np.array_equal(pose_cost, want["C"]) and np.array_equal(cost, want["D"]) and np.array_equal(action, want["action"]), (bar, name)
            path = pfield.path_from(*want["start"])
            assert path == want["path"]
            seen[name] = dict(want, D=cost, action=action, path=path)
            pfield.release()
            vol.release()
        f.release()
    bvs.hold_statement(bar, seen)
    print(bar, {k: (int(v["D"][v["start"][2], v["start"][0], v["start"][1]]), None if v["path"] is None else len(v["path"])) for k, v in seen.items()})


def test_the_field_may_be_released_as_soon_as_the_call_returns_and_the_volume_is_a_snapshot(gvom):
    """ordering: the field and the set are released right after the call; a scan, a combine, an integrate and another field are enqueued
    behind it; set_body and set_chassis are replaced -- and the volume still equals the referee of the call's moment"""
    S = bvs.SCENE
    res, zres = S["res"], S["zres"]
    g, atlas, m = _scene(gvom, "full")
    body = bs.bodies()["tall"]
    g.set_body(body)
    f = atlas.distance_field(bvs.CAP)
    W = tuple(int(v) for v in f.origin_voxels)
    field = f.distance.copy_to_host()
    ground = ar.ground_of(m.height_map.copy_to_host(), m.inferred_height_map.copy_to_host(), True)
    want = bv.volume(field, W, ground, body, bvs.CHASSIS, g.cos_sin, res, zres, W[:2], bvs.MIN_MARGIN, bvs.SOFT_MARGIN)
    v = f.body_volume(m, min_margin=bvs.MIN_MARGIN, soft_margin=bvs.SOFT_MARGIN)
    f.release()
    m.release()
    ego2 = (S["ego"][0] + 1.3, S["ego"][1] - 0.7, S["ego"][2])
    g.process_pointcloud(obstacle_scenes.post_scene(5, S["xy"], res, zres, ego2, n_posts=30, ground_pts=2000), ego2)
    g.combine_maps_device().release()
    assert atlas.integrate() is True
    atlas.distance_field(0.5).release()                                     # (takes the set the field gave back)
    g.set_body(bs.bodies()["low"])
    g.set_chassis(gvom.chassis(1.2, -0.2, 0.9, 0.2))
    _hold(v, want, "behind a scan, a combine, an integrate, another field, another body and another chassis")


def test_the_pool_reuse_and_no_allocation_in_steady_state(gvom):
    q, want = bv.cases()[1], bv.expected()[1]
    xy = q["xy"]
    res, zres, zs, _, _ = bv.GRIDS[xy]
    g = gvom.Gvom(res, zres, xy, zs, 1, *TAIL, voxel_statistics=False)
    assert g.get_tuning("body_volume") == 1 and g.get_tuning("body_volume_allocations") == 0
    _setup(gvom, g, q)
    assert g.get_tuning("body_volume_allocations") == 0 and g.get_tuning("attitude_volume_allocations") == 0   # the setters build nothing for it
    B = np.array(q["field_origin"])
    call = lambda: g.body_volume_of(q["field"], B, q["g"], origin=q["origin"], min_margin=q["min_margin"], soft_margin=q["soft_margin"])
    first = call()
    assert g.get_tuning("body_volume_allocations") == 2 and g.get_tuning("device_product_sets") == 1     # the product set and the staging buffer
    assert g.get_tuning("attitude_volume_allocations") == 1                 # the wheel-offset table is the attitude volume's: one, shared
    before = first.copy_to_host()
    ptr = first.status.ptr
    other = br.random_body(5, res, zres, 77)
    g.set_body(other)                                                       # replaced between calls: the earlier product is unchanged
    _hold(call(), bv.score_case(dict(q, body=other)), "after set_body")
    ch2 = ar.make_chassis(1.1 * res, -2.2 * res, 1.4 * res, 0.5 * res)
    g.set_chassis(_chassis(gvom, ch2))                                      # the next call rebuilds the shared table in place
    _hold(call(), bv.score_case(dict(q, body=other, chassis=ch2)), "after set_chassis")
    assert all(np.array_equal(a, b) for a, b in zip(before, first.copy_to_host()))
    _hold(first, want, "the earlier product")
    g.set_chassis(_chassis(gvom, q["chassis"]))
    g.set_body(q["body"])
    with g.attitude_volume_of(q["g"]) as av_:                               # the other entry point finds the table ready: no second one
        assert g.get_tuning("attitude_volume_allocations") == 3             # + its own product set and staging buffer
        av_.copy_to_host()
    allocs = g.get_tuning("body_volume_allocations")
    ptrs = set()
    for _ in range(20):
        with call() as r:
            ptrs.add(r.status.ptr)
            _hold(r, want, "steady state", release=False)
    assert g.get_tuning("body_volume_allocations") == allocs and ptrs == {ptr} and g.get_tuning("attitude_volume_allocations") == 3
    held = [call() for _ in range(4)]
    with pytest.raises(gvom.GvomBackendError, match="all 4 device product sets of this kind"):
        call()
    for r in held:
        _hold(r, want, "held")


def test_refusals(gvom):
    xy = 16
    res, zres, zs, _, _ = bv.GRIDS[xy]
    g = gvom.Gvom(res, zres, xy, zs, 1, *TAIL, voxel_statistics=False)
    ground, field = np.zeros((xy, xy)), np.ones((xy, xy, zs), np.float32)
    B = np.array([0, 0, 0])
    with pytest.raises(ValueError, match="no footprint table is set"):
        g.body_volume_of(field, B, ground)
    g.set_footprint(gvom.rectangle_footprint(0.5, 0.5, 0.4, res, headings=8))
    with pytest.raises(ValueError, match="no chassis is set"):
        g.body_volume_of(field, B, ground)
    g.set_chassis(gvom.chassis(0.5, -0.3, 0.6, 0.3))
    with pytest.raises(ValueError, match="no body is set"):
        g.body_volume_of(field, B, ground)
    one = np.array([[0, 0, 0.5, 0.1]], np.float32)
    g.set_body(one)
    g.set_footprint(gvom.rectangle_footprint(0.5, 0.5, 0.4, res, headings=1))   # one heading now: the chassis was set for eight
    with pytest.raises(ValueError, match="another number of headings"):
        g.body_volume_of(field, B, ground)
    assert g.get_tuning("body_volume_allocations") == 0
    g.set_footprint(gvom.rectangle_footprint(0.5, 0.5, 0.4, res, headings=8))
    g.set_primitives(gvom.arc_primitives(8, 1.0, res, reach=3))
    pid = ctypes.c_int64(-1)
    oc = (ctypes.c_int64 * 2)(0, 0)
    fo = (ctypes.c_int64 * 3)(0, 0, 0)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    gp, fp = vp(ground), vp(field)

    def raw(fid=-1, f=fp, forg=fo, set_id=-1, gr=gp, flags=0, origin=oc, mm=0.0, sm=0.5, out=pid):
        return g._check(g._lib.gvom_body_volume(g._h, fid, f, forg, set_id, gr, 0, flags, origin, ctypes.c_float(mm), ctypes.c_float(sm),
                                                ctypes.byref(out) if out is not None else None))
    assert raw() == 0 and pid.value >= 0
    far2, far3 = (ctypes.c_int64 * 2)(1 << 41, 0), (ctypes.c_int64 * 3)(0, 0, -(1 << 41))
    for kw, word in ((dict(set_id=10 ** 9, gr=None), "unknown or stale device map set id"), (dict(set_id=1), "not both"),
                     (dict(gr=None), "a map set id or a ground map"), (dict(fid=10 ** 9, f=None, forg=None), "unknown or stale distance field id"),
                     (dict(fid=1), "not both"), (dict(fid=1, f=None), "not both"), (dict(f=None), "a distance field id or a field pointer"),
                     (dict(forg=None), "field_origin"), (dict(forg=far3), "2\\^40"), (dict(origin=None), "origin_cells"), (dict(flags=2), "unknown flag bits"),
                     (dict(mm=float("nan")), "min_margin"), (dict(mm=float("inf")), "min_margin"), (dict(mm=float("-inf")), "min_margin"),
                     (dict(sm=float("nan")), "soft_margin"), (dict(sm=float("inf")), "soft_margin"), (dict(mm=0.5, sm=0.25), "soft_margin must not be less"),
                     (dict(origin=far2), "2\\^40")):
        with pytest.raises(gvom.GvomBackendError, match=word):
            raw(**kw)
        assert pid.value == -1
    assert g._lib.gvom_body_volume(g._h, -1, fp, fo, -1, gp, 0, 0, oc, ctypes.c_float(0), ctypes.c_float(0), None) == gvom.GVOM_ERR_INVALID   # NULL product_id
    with pytest.raises(gvom.GvomBackendError, match="unknown product kind"):
        g._device_product(gvom.PRODUCT_BODY_VOLUME)
    with pytest.raises(gvom.GvomBackendError, match="unknown product kind"):
        g._device_product(45)
    raw()
    with pytest.raises(gvom.GvomBackendError, match="unknown or stale distance field id"):
        raw(fid=pid.value, f=None, forg=None)                               # (a body volume is no distance field)
    # the pose field's side: the masks, the weights, and what the ids may name
    vol = g.body_volume_of(field, B, ground)
    avol = g.attitude_volume_of(ground)
    c = np.full((xy, xy), 2, np.int32)
    goals = np.array([[3, 3, -1]], np.int32)
    info = (ctypes.c_int64 * 4)()
    fid = ctypes.c_int64(-1)

    def pose(a=-1, am=0, aw=0, b=None, bm=0x6, bw=0):
        return g._lib.gvom_pose_field_volumes(g._h, -1, vp(c), 0, a, am, aw, vol.product_id if b is None else b, bm, bw, vp(goals), 1, 0, 0,
                                              ctypes.byref(fid), info)
    assert pose() == 0 and fid.value >= 0
    field_id = fid.value
    for kw, word in ((dict(bm=0x40), "body_block_mask"), (dict(bw=-1), "squeeze_weight"), (dict(bw=256), "squeeze_weight"),
                     (dict(b=10 ** 9), "body volume id"), (dict(b=field_id), "body volume id"), (dict(b=avol.product_id), "body volume id"),
                     (dict(a=vol.product_id, am=0xe), "attitude volume id"), (dict(a=avol.product_id, am=0x80), "block_mask"),
                     (dict(b=-1), "beside a volume id of -1"), (dict(b=-1, bm=0, bw=1), "beside a volume id of -1"), (dict(am=2), "beside a volume id of -1"),
                     (dict(aw=1), "beside a volume id of -1")):
        assert pose(**kw) == gvom.GVOM_ERR_INVALID and fid.value == -1, kw
        err = g._lib.gvom_last_error(g._h).decode()
        assert word in err and "gvom_pose_field_volumes" in err, (kw, err)
    assert pose(a=avol.product_id, am=0xe, aw=3) == 0 and pose(b=-1, bm=0, bw=0) == 0
    # a volume of another number of headings, another mapper's, something that is no volume
    g.set_footprint(gvom.rectangle_footprint(0.5, 0.5, 0.4, res, headings=4))
    g.set_primitives(gvom.arc_primitives(4, 0.5, res, reach=3))
    with pytest.raises(ValueError, match="another number of headings"):
        g.pose_field_of(c, [(3, 3)], body=vol)
    other = gvom.Gvom(res, zres, xy, zs, 1, *TAIL, voxel_statistics=False)
    other.set_footprint(gvom.rectangle_footprint(0.5, 0.5, 0.4, res, headings=4))
    other.set_primitives(gvom.arc_primitives(4, 0.5, res, reach=3))
    with pytest.raises(ValueError, match="body volume id"):                 # (ids are per mapper)
        other.pose_field_of(c, [(3, 3)], body=vol)
    with pytest.raises(TypeError):
        g.pose_field_of(c, [(3, 3)], body=ground)
    with pytest.raises(ValueError, match="squeeze_weight"):
        g.pose_field_of(c, [(3, 3)], squeeze_weight=3)
    vol.release()
    avol.release()
    many = gvom.Gvom(res, zres, xy, zs, 1, *TAIL, voxel_statistics=False)
    many.set_footprint(gvom.rectangle_footprint(0.5, 0.5, 0.4, res, headings=128))
    many.set_chassis(gvom.chassis(0.5, -0.3, 0.6, 0.3))
    many.set_body(one)
    with pytest.raises(gvom.GvomBackendError, match="more than 64 headings"):
        many.body_volume_of(field, B, ground)
    assert many.get_tuning("body_volume_allocations") == 0
    sharded = gvom.Gvom(res, zres, 64, zs, 1, *TAIL, voxel_statistics=False, _shard=(0, 2))
    with pytest.raises(ValueError, match="sharded handles are not supported"):
        sharded.body_volume_of(np.ones((64, 64, zs), np.float32), B, np.zeros((64, 64)))


def test_more_than_4096_cells_a_side_and_more_than_2_to_the_28_states_are_refused(gvom):
    one = np.array([[0, 0, 0.5, 0.1]], np.float32)
    g = gvom.Gvom(0.4, 0.2, 4100, 1, 1, *TAIL, voxel_statistics=False)
    g.set_footprint(gvom.disc_footprint(0.5, 0.4))
    g.set_chassis(gvom.chassis(0.5, -0.3, 0.6, 0.3))
    g.set_body(one)
    with pytest.raises(gvom.GvomBackendError, match="4096"):
        g.body_volume_of_device(1 << 20, np.array([0, 0, 0]), 1 << 21)
    assert g.get_tuning("body_volume_allocations") == 0
    g = gvom.Gvom(0.4, 0.2, 4096, 1, 1, *TAIL, voxel_statistics=False)
    g.set_footprint(gvom.rectangle_footprint(0.5, 0.5, 0.4, 0.4, headings=32))         # 32 x 4096^2 = 2^29 states
    g.set_chassis(gvom.chassis(0.5, -0.3, 0.6, 0.3))
    g.set_body(one)
    with pytest.raises(gvom.GvomBackendError, match="2\\^28 states"):
        g.body_volume_of_device(1 << 20, np.array([0, 0, 0]), 1 << 21)
    assert g.get_tuning("body_volume_allocations") == 0


def test_a_recalled_atlas_set_works_as_the_ground(gvom):
    """the body volume on a set recalled from the map atlas equals the referee on the set's own host copies"""
    xy, res, zres, zs = atlas_ref.DRIVE_XY, atlas_ref.DRIVE_RES, atlas_ref.DRIVE_ZRES, 8
    g = gvom.Gvom(res, zres, xy, zs, 1, *TAIL, voxel_statistics=False)
    a = g.create_atlas(atlas_ref.DRIVE_A)
    first = None
    for pc, ego in atlas_ref.drive_scans()[:4]:
        g.process_pointcloud(pc, ego)
        with g.combine_maps_device() as m:
            a.integrate(m)
            first = first or m.origin_cells[:2]
    ch = ar.make_chassis(0.7, -0.3, 0.8, 0.3)
    g.set_footprint(gvom.rectangle_footprint(0.9, 0.5, 0.45, res, headings=16, margin=0.1))
    g.set_chassis(_chassis(gvom, ch))
    body = br.random_body(9, res, zres, 5)
    g.set_body(body)
    field = br.random_field(xy, zs, res, zres, 44)
    with a.recall(origin_cells=first) as m:
        height, inferred = m.height_map.copy_to_host(), m.inferred_height_map.copy_to_host()
        assert (height > -1000).sum() > 500
        oc = tuple(int(v) for v in m.origin_cells[:2])
        kn = height[height > -1000]
        B = (oc[0] + 1, oc[1] - 1, int(np.floor(float(np.median(kn)) / zres)) - 1)
        dev = _Device()
        pid = ctypes.c_int64(-1)
        try:
            fptr = dev.upload(field)
            for use in (True, False):
                want = bv.volume(field, B, ar.ground_of(height, inferred, use), body, ch, g.cos_sin, res, zres, oc, np.float32(0.05), np.float32(0.6))
                g._check(g._lib.gvom_body_volume(g._h, -1, ctypes.c_void_p(fptr), (ctypes.c_int64 * 3)(*B), m.set_id, None, 1, 1 if use else 0,
                                                 (ctypes.c_int64 * 2)(*oc), ctypes.c_float(0.05), ctypes.c_float(0.6), ctypes.byref(pid)))
                v = gvom.DeviceBodyVolume(gvom._ProductHold(g, gvom.PRODUCT_BODY_VOLUME, pid.value))
                status, _, _, counts = _hold(v, want, "recalled, inferred_ground=%r" % use)
        finally:
            dev.free()
        assert counts[bv.OK] + counts[bv.COLLISION] + counts[bv.LEFT_BOX] > 0 and (status == bv.UNKNOWN_GROUND).any()


def test_a_torch_consumer_reads_the_status_through_dlpack():
    """One case in a fresh child process that imports torch BEFORE the library is loaded (one HIP runtime in the process)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_body_volume_torch.py"), "consumer"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "CASE OK consumer" in r.stdout, r.stdout[-4000:]
