"""Body clearance scoring on the GPU (gvom_body_set, gvom_score_body: k_body; Gvom.set_body, DeviceDistanceField.score_body /
score_body_of, Gvom.score_body_of / score_body_of_device) against the referee of tests/body_ref.py: the summary, the clearance and the
{status, tightest} pairs with tolerance 0, floats by bit pattern -- every float64 operation is one IEEE operation in the header's order.

  callers' fields and grounds   grids of 16 x 16 x 8 at 0.4 / 0.4 m, 33 x 33 x 8 and 40 x 40 x 6 at 0.3 / 0.2 m; field origins negative
                   and off zero; random fields and one with NaN; the five grounds of attitude_ref; S of 1, 2, 63, 64, 65 and 256;
                   K x T of 1 x 1, 3 x 63, 2 x 64, 2 x 65, 1 x 256, 2 x 257 and 2 x 4096; 1, 7 and 64 headings; host and device routes
  the limit        a clearance one float32 ulp above, on and below min_margin
  edges            a sphere exactly on a box face, at negative coordinates, at |quotient| >= 2^30; a wheel outside the window while every
                   sphere is inside the box, and the reverse
  real products    the 40 x 40 x 6 post scene and the gate scene of tests/body_scenes.py: one scan, combine_maps_device(), integrate(),
                   distance_field(), score_body() with the set's ground, with and without the inferred ground, at the window's box and at
                   a displaced one, against the referee fed from read_dense(), the atlas and distance referees and the set's maps 4 and 5
  ordering         the field released right after the call; a scan, combine and integrate enqueued behind it
  housekeeping     error codes, set_body replaced between calls, the pool and "body_allocations", DLPack (a torch child)

tests/test_body_cpu.py holds the census of every input and the two forms of the referee together.

Wall time on the MI355X (pytest --durations, one run): the torch child 2.4 s, the ordering test 0.25 s, every other test below 0.2 s;
the file 4 s."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import attitude_ref as ar
import body_ref as br
import body_scenes as bs
import obstacle_scenes
import voxel_atlas_ref as va
import voxel_distance_ref as vd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = va.DRIVE_TAIL


@pytest.fixture(scope="module")
def gvom():
    import gvom as mod
    rc, info = mod.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    assert mod.PRODUCT_BODY == 44
    return mod


@pytest.fixture(scope="module")
def handles(gvom):
    return {xy: gvom.Gvom(res, zres, xy, zs, 1, *TAIL, voxel_statistics=False) for xy, (res, zres, zs, _, _) in br.GRIDS.items()}


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
    return gvom.chassis(ch.front_axle, ch.rear_axle, ch.track, ch.belly_height)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _hold(r, want, what):
    """a DeviceBodyClearance against the referee's (summary, clearance, pairs): all three parts, exactly"""
    with r:
        summary, clr, pairs = r.copy_to_host()
    assert summary.dtype == np.int32 and clr.dtype == np.float32 and pairs.dtype == np.uint8, what
    assert summary.shape == want[0].shape and clr.shape == want[1].shape and pairs.shape == want[2].shape, (what, summary.shape, clr.shape, pairs.shape)
    if not np.array_equal(pairs, want[2]):
        bad = np.argwhere((pairs != want[2]).any(axis=2))
        raise AssertionError("%s: {status, tightest} differ in %d poses, first (%d, %d): got %r, referee %r" % (
            what, len(bad), bad[0][0], bad[0][1], pairs[tuple(bad[0])].tolist(), want[2][tuple(bad[0])].tolist()))
    if not np.array_equal(_bits(clr), _bits(want[1])):
        bad = np.argwhere(_bits(clr) != _bits(want[1]))
        raise AssertionError("%s: the clearances differ in %d poses, first (%d, %d): got %r, referee %r" % (
            what, len(bad), bad[0][0], bad[0][1], clr[tuple(bad[0])], want[1][tuple(bad[0])]))
    if not np.array_equal(summary, want[0]):
        bad = np.argwhere((summary != want[0]).any(axis=1))
        raise AssertionError("%s: the summaries differ in %d rollouts, first %d: got %r, referee %r" % (
            what, len(bad), bad[0][0], summary[bad[0][0]].tolist(), want[0][bad[0][0]].tolist()))
    return summary, clr, pairs


def _run(gvom, g, q, dev, device=None):
    """one case through the host or the device route"""
    g.set_footprint(q["table"])
    g.set_chassis(_chassis(gvom, q["chassis"]))
    assert np.array_equal(g.cos_sin, q["cos_sin"])                         # the referee turns with the numbers the library got
    g.set_body(q["body"])
    assert g.get_tuning("body_spheres") == len(q["body"])
    B = np.array(q["field_origin"], np.int64)
    if q["device"] if device is None else device:
        K, T = q["poses"].shape[:2]
        gp = dev.upload(np.asfortranarray(q["g"]).T)                       # cell (x, y) at [y * xy + x]
        return g.score_body_of_device(dev.upload(q["field"]), B, gp, dev.upload(q["poses"]), K, T, origin=q["origin"], min_margin=q["min_margin"])
    return g.score_body_of(q["field"], B, q["g"], q["poses"], origin=q["origin"], min_margin=q["min_margin"])


@pytest.mark.parametrize("shape", br.SHAPES, ids=lambda s: "%dx%d" % s)
def test_synthetic_inputs_match_the_referee_exactly(gvom, handles, shape):
    dev = _Device()
    K, T = shape
    try:
        for q, want in zip(br.cases(shape), br.expected(shape)):
            r = _run(gvom, handles[q["xy"]], q, dev)
            assert r.summary.shape == (K, 4) and r.clearance.shape == shape and r.status.shape == (K, T, 2)
            assert r.summary.strides == (4, 1) and r.clearance.strides == (T, 1) and r.status.strides == (2 * T, 2, 1)
            assert r.summary.ptr % 256 == 0 and r.clearance.ptr % 256 == 0 and r.status.ptr % 256 == 0
            _hold(r, want, q["name"])
    finally:
        dev.free()


def test_a_nan_field_the_limit_and_the_edges_through_both_routes(gvom, handles):
    """a field with NaN entries; a clearance one float32 ulp above, on and below min_margin; spheres on box faces, at negative
    coordinates and beyond 2^30 voxels; a wheel outside the window with the body inside the box, and the reverse -- each through the host
    AND the device route"""
    dev = _Device()
    others = [br.nan_case()] + list(br.limit_cases()) + list(br.edge_cases())
    try:
        for q, want in zip(others, br.expected_other()):
            for device in (False, True):
                got = _hold(_run(gvom, handles[q["xy"]], q, dev, device), want, "%s, %s route" % (q["name"], "device" if device else "host"))
            if "probe" in q:
                assert got[2][q["probe"]][0] == q["expect"], q["name"]
            elif q.get("expect") is not None:
                assert (got[2][..., 0] == q["expect"]).all(), q["name"]
    finally:
        dev.free()
    nan = br.expected_other()[0]
    assert (nan[2][..., 1][nan[2][..., 0] == br.OK] == br.NO_SPHERE).any()  # every margin skipped somewhere: +inf and 255


def test_host_and_device_routes_agree(gvom, handles):
    dev = _Device()
    shape = (2, 65)
    try:
        for q, want in zip(br.cases(shape), br.expected(shape)):
            for device in (False, True):
                _hold(_run(gvom, handles[q["xy"]], q, dev, device), want, "%s, %s route" % (q["name"], "device" if device else "host"))
    finally:
        dev.free()


# ---- real products ------------------------------------------------------------------------------------------------------------------------
def _scene(gvom, name):
    """one scan of a scene of tests/body_scenes.py through combine_maps_device() and integrate(): (mapper, atlas, its referee, the window's
    origin in voxels, the map set)"""
    S = bs.SCENES[name]
    g = gvom.Gvom(S["res"], S["zres"], S["xy"], S["zs"], 1, *TAIL, voxel_statistics=False)
    g.process_pointcloud(bs.cloud(name), S["ego"])
    m = g.combine_maps_device()
    state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
    W = tuple(int(v) for v in origin)
    atlas = g.create_voxel_atlas(64, 16)
    ref = va.VoxelAtlasRef(64, 16, S["xy"], S["zs"])
    assert atlas.integrate() is True
    ref.integrate(state, W)
    g.set_footprint(gvom.rectangle_footprint(0.3, 0.3, 0.3, S["res"], headings=bs.HEADINGS))
    g.set_chassis(_chassis(gvom, bs.CHASSIS))
    return g, atlas, ref, W, m


@pytest.mark.parametrize("name", sorted(bs.SCENES))
def test_scenes_through_real_fields_and_map_sets(gvom, name):
    S = bs.SCENES[name]
    res, zres = S["res"], S["zres"]
    g, atlas, ref, W, m = _scene(gvom, name)
    seen = {}
    with m:
        oc = tuple(int(v) for v in np.round(np.asarray(m.origin)[:2] / res))
        height, inferred = m.height_map.copy_to_host(), m.inferred_height_map.copy_to_host()
        for box in (W, tuple(W[k] + bs.DISPLACED[k] for k in range(3))):
            field_ref = vd.separable(ref, box, bs.CAP, (res, zres))[0]
            f = atlas.distance_field(bs.CAP, origin_voxels=np.array(box))
            assert vd.same_bits(f.distance.copy_to_host(), field_ref)
            for body_name, body in sorted(bs.bodies(name).items()):
                g.set_body(body)
                for use in (True, False):
                    ground = ar.ground_of(height, inferred, use)
                    poses = bs.poses(name)
                    want = br.score(field_ref, box, ground, poses, body, bs.CHASSIS, g.cos_sin, res, zres, oc, bs.MIN_MARGIN)
                    got = _hold(f.score_body(m, poses, min_margin=bs.MIN_MARGIN, inferred_ground=use), want,
                                "%s, box %r, %s body, inferred_ground=%r" % (name, box, body_name, use))
                    _hold(f.score_body_of(ground, poses, origin=m.origin, min_margin=bs.MIN_MARGIN), want, "%s, the same ground by pointer" % name)
                    if box == W and use:
                        seen[body_name] = got
                        if body_name == "low":                               # the untilted frame is the referee's alone: what the tilt changes
                            seen["untilted"] = br.score(field_ref, box, ground, poses, body, bs.CHASSIS, g.cos_sin, res, zres, oc, bs.MIN_MARGIN, tilt=False)
            f.release()
    for body_name, got in sorted(seen.items()):
        print(name, body_name, "status counts", np.bincount(got[2][..., 0].ravel(), minlength=br.N_STATUS).tolist())
    bs.hold_statement(name, seen, seen["untilted"])


def test_the_field_may_be_released_as_soon_as_the_call_returns(gvom):
    """ordering: the field is released right after the call, a scan, a combine and an integrate are enqueued behind it, another field takes
    the released set -- and the result still equals the referee of the call's moment"""
    name = "gate"
    S = bs.SCENES[name]
    g, atlas, ref, W, m = _scene(gvom, name)
    res, zres = S["res"], S["zres"]
    oc = tuple(int(v) for v in np.round(np.asarray(m.origin)[:2] / res))
    ground = ar.ground_of(m.height_map.copy_to_host(), m.inferred_height_map.copy_to_host(), True)
    field_ref = vd.separable(ref, W, bs.CAP, (res, zres))[0]
    body = bs.bodies()["tall"]
    g.set_body(body)
    poses = np.concatenate([bs.poses(name)] * 64, axis=0)
    want = br.score(field_ref, W, ground, poses, body, bs.CHASSIS, g.cos_sin, res, zres, oc, bs.MIN_MARGIN)
    f = atlas.distance_field(bs.CAP, origin_voxels=np.array(W))
    r = f.score_body(m, poses, min_margin=bs.MIN_MARGIN)
    f.release()
    m.release()
    ego2 = (S["ego"][0] + 1.3, S["ego"][1] - 0.7, S["ego"][2])
    g.process_pointcloud(obstacle_scenes.post_scene(5, S["xy"], res, zres, ego2, n_posts=30, ground_pts=2000), ego2)
    g.combine_maps_device().release()
    assert atlas.integrate() is True
    atlas.distance_field(0.5).release()                                     # (takes the set the field gave back)
    g.set_body(bs.bodies()["low"])
    _hold(r, want, "behind a scan, a combine, an integrate, another field and another body")


# ---- housekeeping ---------------------------------------------------------------------------------------------------------------------------
def test_set_body_replaced_the_pool_and_no_allocation_in_steady_state(gvom):
    xy = 33
    res, zres, zs, _, _ = br.GRIDS[xy]
    g = gvom.Gvom(res, zres, xy, zs, 1, *TAIL, voxel_statistics=False)
    assert g.get_tuning("body") == 1 and g.get_tuning("body_spheres") == 0 and g.get_tuning("body_allocations") == 0
    q = [q for q in br.cases((3, 63)) if q["xy"] == xy][0]
    want = br.score_case(q)
    g.set_footprint(q["table"])
    g.set_chassis(_chassis(gvom, q["chassis"]))
    g.set_body(q["body"])
    assert g.get_tuning("body_spheres") == len(q["body"]) and g.get_tuning("body_allocations") == 1       # the table
    B = np.array(q["field_origin"])
    call = lambda: g.score_body_of(q["field"], B, q["g"], q["poses"], origin=q["origin"], min_margin=q["min_margin"])
    first = call()
    assert g.get_tuning("body_allocations") == 3 and g.get_tuning("device_product_sets") == 1            # + the product set and the staging buffer
    before = first.copy_to_host()
    other = br.random_body(5, res, zres, 77)
    g.set_body(other)                                                       # replaced between calls: the earlier product is unchanged
    assert g.get_tuning("body_spheres") == 5
    q2 = dict(q, body=other)
    second = call()
    _hold(second, br.score_case(q2), "after set_body")
    assert all(np.array_equal(a, b) for a, b in zip(before, first.copy_to_host()))
    _hold(first, want, "the earlier product")
    g.set_body(q["body"])
    allocs = g.get_tuning("body_allocations")
    ptrs = set()
    for _ in range(20):
        with call() as r:
            ptrs.add(r.summary.ptr)
            _hold(r, want, "steady state")
    assert g.get_tuning("body_allocations") == allocs and len(ptrs) == 1
    held = [call() for _ in range(4)]
    with pytest.raises(gvom.GvomBackendError, match="all 4 device product sets of this kind"):
        call()
    for r in held:
        _hold(r, want, "held")


def test_errors(gvom):
    xy = 16
    res, zres, zs, _, _ = br.GRIDS[xy]
    g = gvom.Gvom(res, zres, xy, zs, 1, *TAIL, voxel_statistics=False)
    ground, field = np.zeros((xy, xy)), np.ones((xy, xy, zs), np.float32)
    poses = np.zeros((2, 3, 3), np.float32)
    B = np.array([0, 0, 0])
    with pytest.raises(ValueError, match="no footprint table is set"):
        g.score_body_of(field, B, ground, poses)
    g.set_footprint(gvom.rectangle_footprint(0.5, 0.5, 0.4, res, headings=8))
    with pytest.raises(ValueError, match="no chassis is set"):
        g.score_body_of(field, B, ground, poses)
    g.set_chassis(gvom.chassis(0.5, -0.3, 0.6, 0.3))
    with pytest.raises(ValueError, match="no body is set"):
        g.score_body_of(field, B, ground, poses)
    assert g.get_tuning("body_allocations") == 0
    for bad in (np.zeros((0, 4)), np.zeros((257, 4)), np.zeros((3, 3)), [[0, 0, 0, -1.0]], [[np.nan, 0, 0, 1]], [[0, np.inf, 0, 1]]):
        with pytest.raises(ValueError):
            g.set_body(bad)
    one = np.array([[0, 0, 0.5, 0.1]], np.float32)
    raw_set = lambda a, S: g._lib.gvom_body_set(g._h, a.ctypes.data_as(ctypes.c_void_p) if a is not None else None, S)
    for a, S in ((None, 1), (one, 0), (one, 257), (np.array([[0, 0, 0, -0.5]], np.float32), 1), (np.array([[0, np.nan, 0, 0.5]], np.float32), 1),
                 (np.array([[0, 0, 0, np.inf]], np.float32), 1)):
        assert raw_set(a, S) == gvom.GVOM_ERR_INVALID
    assert g.get_tuning("body_spheres") == 0
    g.set_body(one)
    g.set_footprint(gvom.rectangle_footprint(0.5, 0.5, 0.4, res, headings=1))   # one heading now: the chassis was set for eight
    with pytest.raises(ValueError, match="another number of headings"):
        g.score_body_of(field, B, ground, poses)
    g.set_chassis(gvom.chassis(0.5, -0.3, 0.6, 0.3))
    pid = ctypes.c_int64(-1)
    oc = (ctypes.c_int64 * 2)(0, 0)
    fo = (ctypes.c_int64 * 3)(0, 0, 0)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    gp, pp, fp = vp(ground), vp(poses), vp(field)

    def raw(fid=-1, f=fp, forg=fo, set_id=-1, gr=gp, p=pp, K=2, T=3, flags=0, origin=oc, mm=0.0, out=pid):
        return g._check(g._lib.gvom_score_body(g._h, fid, f, forg, set_id, gr, p, K, T, 0, flags, origin, ctypes.c_float(mm),
                                               ctypes.byref(out) if out is not None else None))
    assert raw() == 0 and pid.value >= 0
    far2, far3 = (ctypes.c_int64 * 2)(1 << 41, 0), (ctypes.c_int64 * 3)(0, 0, -(1 << 41))
    for kw, word in ((dict(set_id=10 ** 9, gr=None), "unknown or stale device map set id"), (dict(set_id=1), "not both"),
                     (dict(gr=None), "a map set id or a ground map"), (dict(fid=10 ** 9, f=None, forg=None), "unknown or stale distance field id"),
                     (dict(fid=1), "not both"), (dict(fid=1, f=None), "not both"), (dict(f=None), "a distance field id or a field pointer"),
                     (dict(forg=None), "field_origin"), (dict(forg=far3), "2\\^40"), (dict(p=None), "poses"), (dict(origin=None), "origin_cells"),
                     (dict(T=0), "T outside"), (dict(T=4097), "T outside"), (dict(K=0), "K must be"), (dict(flags=2), "unknown flag bits"),
                     (dict(mm=float("nan")), "min_margin"), (dict(mm=float("inf")), "min_margin"), (dict(mm=float("-inf")), "min_margin"),
                     (dict(K=(1 << 26) // 3 + 1), "2\\^26 poses"), (dict(origin=far2), "2\\^40")):
        with pytest.raises(gvom.GvomBackendError, match=word):
            raw(**kw)
        assert pid.value == -1
    assert g._lib.gvom_score_body(g._h, -1, fp, fo, -1, gp, pp, 2, 3, 0, 0, oc, ctypes.c_float(0), None) == gvom.GVOM_ERR_INVALID      # NULL product_id
    assert g._lib.gvom_score_body(g._h, -1, fp, fo, -1, gp, pp, (1 << 26) // 3 + 1, 3, 0, 0, oc, ctypes.c_float(0), ctypes.byref(pid)) == -4   # GVOM_ERR_CAPACITY
    with pytest.raises(gvom.GvomBackendError, match="unknown product kind"):
        g._device_product(gvom.PRODUCT_BODY)
    with pytest.raises(gvom.GvomBackendError, match="unknown product kind"):
        g._device_product(43)
    # a product of another kind, and a stale field
    raw()
    with pytest.raises(gvom.GvomBackendError, match="unknown or stale distance field id"):
        raw(fid=pid.value, f=None, forg=None)                               # (a body product is no distance field)
    with pytest.raises(ValueError, match="min_margin"):
        g.score_body_of(field, B, ground, poses, min_margin=float("nan"))
    with pytest.raises(ValueError, match="shape"):
        g.score_body_of(field[:, :, :-1], B, ground, poses)
    sharded = gvom.Gvom(res, zres, xy, zs, 1, *TAIL, voxel_statistics=False, _shard=(0, 2))
    with pytest.raises(ValueError, match="sharded handles are not supported"):
        sharded.score_body_of(field, B, ground, poses)


def test_a_stale_field_id_is_refused(gvom):
    g, atlas, ref, W, m = _scene(gvom, "gate")
    g.set_body(bs.bodies()["low"])
    f = atlas.distance_field(bs.CAP)
    old = f.product_id
    f.release()
    atlas.distance_field(0.5).release()                                     # the unheld set was handed out again: the id is stale
    pid = ctypes.c_int64(-1)
    poses = bs.poses("gate")
    with pytest.raises(gvom.GvomBackendError, match="unknown or stale distance field id"):
        g._check(g._lib.gvom_score_body(g._h, old, None, None, m.set_id, None, poses.ctypes.data_as(ctypes.c_void_p), poses.shape[0], poses.shape[1],
                                        0, 1, (ctypes.c_int64 * 2)(0, 0), ctypes.c_float(0), ctypes.byref(pid)))
    m.release()


def test_maps_of_more_than_4096_cells_a_side_are_refused(gvom):
    g = gvom.Gvom(0.4, 0.2, 4100, 1, 1, *TAIL, voxel_statistics=False)
    g.set_footprint(gvom.disc_footprint(0.5, 0.4))
    g.set_chassis(gvom.chassis(0.5, -0.3, 0.6, 0.3))
    g.set_body(np.array([[0, 0, 0.5, 0.1]]))
    with pytest.raises(gvom.GvomBackendError, match="4096"):
        g.score_body_of_device(1 << 20, np.array([0, 0, 0]), 1 << 21, 1 << 22, 1, 1)
    assert g.get_tuning("body_allocations") == 1


def test_a_torch_planner_reads_the_clearance_through_dlpack():
    """One case in a fresh child process that imports torch BEFORE the library is loaded (one HIP runtime in the process)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_body_torch.py"), "planner"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "CASE OK planner" in r.stdout, r.stdout[-4000:]
