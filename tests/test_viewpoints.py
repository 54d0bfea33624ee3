"""Viewpoint scoring on the GPU (gvom_score_viewpoints: k_viewpoints, k_viewpoint_best; Gvom.score_viewpoints,
Gvom.score_viewpoints_device, DeviceViewpoints) against the numpy referee of tests/viewpoint_ref.py, with tolerance 0: every result is
an integer.  The referee walks the dense fused state the SAME handle returns (read_dense(GVOM_WHICH_FUSED)) after four scans of a
moving ego (tests/raycast_ref.py build_map: non-zero storage offsets, stale tiles), on the grids p2, np2, tall, w128, far and the
256 x 256 x 48 grid of tests/viewpoint_ref.py, ring lengths 1 and 2; the cases, sensor models, viewpoints and ranges are
viewpoint_ref.CASES, whose census tests/test_viewpoints_cpu.py holds on the CPU oracle's maps.  Every case runs on the host and the
device route, with one viewpoint per launch ("viewpoint_bitmap_mb" 0) and with all of them in one, and twice in a row; the v256
case also with two per launch (K = 33: a last batch of one).  Then: the cross-check against K raycast() calls (no referee walk),
the float32 square root, snapshots, the pool, the error codes, a torch consumer in a child process, and the chain from
combine_maps_device() to score_viewpoints() on the obstacle scenes.

Wall time on the MI355X (pytest --durations, one run): the first case 0.30 s (it builds its map), the v256 case 0.26 s, every other
case of test_viewpoints_match_the_referee_exactly 0.02 to 0.10 s; the scenes 0.09 and 0.16 s, test_errors 0.14 s, the torch consumer
(a child process) 2.1 s; the file 5 s."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import costfield_ref as cf
import obstacle_scenes as ob
import raycast_ref as rr
import viewpoint_ref as vr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GVOM_ERR_INVALID, GVOM_ERR_CAPACITY, GVOM_NO_DATA = -1, -4, 4


@pytest.fixture(scope="module")
def gvom():
    import gvom as mod
    rc, info = mod.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    return mod


class _Hip(object):
    """device memory for the device-input route, from the HIP runtime the library itself uses"""

    def __init__(self):
        self.rt = ctypes.CDLL("libamdhip64.so")
        self.rt.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.rt.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.rt.hipFree.argtypes = [ctypes.c_void_p]
        self.held = []

    def upload(self, a):
        a = np.ascontiguousarray(a, np.float64)
        p = ctypes.c_void_p()
        assert self.rt.hipMalloc(ctypes.byref(p), a.nbytes) == 0
        assert self.rt.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0           # host to device, blocking
        self.held.append(p)
        return p.value

    def free(self):
        for p in self.held:
            self.rt.hipFree(p)
        self.held = []


@pytest.fixture(scope="module")
def hip():
    h = _Hip()
    yield h
    h.free()


@pytest.fixture(scope="module")
def maps(gvom):
    """(handle, dense fused state, window origin) per (grid, ring slots): built on first use, never changed"""
    built = {}

    def get(grid, bs):
        if (grid, bs) not in built:
            g = rr.build_map(gvom.Gvom, grid, bs, voxel_statistics=False)
            state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
            W = np.asarray(origin, np.float64)
            assert np.array_equal(W, rr.window_origin(grid, rr.ego_of(grid, rr.N_SCANS - 1)))
            xr, zr, xy, zs = rr.GRIDS[grid]
            assert all(int(W[k]) % (xy if k < 2 else zs) != 0 for k in range(3)), W      # non-zero storage offsets on every axis
            built[grid, bs] = (g, state, W)
        return built[grid, bs]
    return get


def _got(v, W, what):
    assert v is not None, what
    with v:
        assert np.array_equal(v.origin, W), what
        rows, best = v.copy_to_host()
    assert rows.dtype == np.int32 and best.dtype == np.int32 and best.shape == (4,), what
    return rows, best


def _hold(v, want, W, what):
    rows, best = _got(v, W, what)
    wr, wb = want
    assert rows.shape == wr.shape, what
    if not np.array_equal(rows, wr):
        bad = np.flatnonzero((rows != wr).any(axis=1))
        raise AssertionError("%s: %d viewpoints differ, first %d: got %r, referee %r" % (what, len(bad), bad[0], rows[bad[0]], wr[bad[0]]))
    assert np.array_equal(best, wb), (what, best, wb)
    return rows, best


@pytest.mark.parametrize("case", vr.CASES, ids=vr.case_id)
def test_viewpoints_match_the_referee_exactly(maps, hip, case):
    grid, bs, name, strides, K, rng, ub = case
    g, state, W = maps(grid, bs)
    d, o, poses, r = vr.case_inputs(case, state, W)
    want = vr.product(state, W, grid, d, o, poses, r, strides, ub)
    print(vr.case_id(case), "best", want[1], "endings", want[0][:, 3:].sum(axis=0), "visits > gain:", int((want[0][:, 2] > want[0][:, 1]).sum()))
    g.set_sensor_model(d, o)
    xr, zr, xy, zs = rr.GRIDS[grid]
    bitmap = (((xy * xy * zs + 31) // 32 + 63) // 64 * 64) * 4
    dev = hip.upload(vr.rows34(poses))
    kw = dict(beam_stride=strides, unknown_blocks=ub)
    assert (256 << 20) // bitmap >= K and (grid != "v256" or (1 << 20) // bitmap == 2)
    batches = [(0, 1), (-1, K)] + ([(1, 2)] if grid == "v256" else [])      # ("viewpoint_bitmap_mb", viewpoints per launch)
    try:
        for mb, B in batches:
            g.set_tuning("viewpoint_bitmap_mb", mb)
            assert g.get_tuning("viewpoint_bitmap_mb") == (256 if mb < 0 else mb)
            what = "%s, %d per launch" % (vr.case_id(case), B)
            # [K, 4, 4], then [K, 3, 4] (one matrix where K = 1): the same call twice in a row -- bits left over would lower the gain
            rows, _ = _hold(g.score_viewpoints(poses, r, **kw), want, W, what + ", host")
            assert g.get_tuning("viewpoint_batch") == B
            _hold(g.score_viewpoints(poses[0] if K == 1 else poses[:, :3], r, **kw), want, W, what + ", host again")
            _hold(g.score_viewpoints_device(dev, K, r, **kw), want, W, what + ", device")
            if K >= 3:
                assert np.array_equal(rows[1], rows[2])         # two identical poses: equal rows, each with its own bitmap
                assert rows[1, 1] > 0 or rng == "short" or grid == "far"
    finally:
        g.set_tuning("viewpoint_bitmap_mb", -1)                # as created: the maps are shared
    if rng == "short":
        assert (want[0][:, 1:4] == 0).all() and (want[0][:, 4] == want[1][3]).all() and (want[0][:, 5:] == 0).all()
    if rng == "long":
        assert want[0][:, 5].sum() > 0 and want[0][:, 4].sum() == 0
    if K == 33:
        assert want[0][16].tolist() == [rr.INVALID, 0, 0, 0, 0, 0, 0, want[1][3]]            # the NaN pose in the middle
        assert want[0][5, 0] == want[0][6, 0] == rr.LEFT_WINDOW and want[0][3, 0] == rr.OCCUPIED
        assert want[0][6, 1] > 0                               # beams that re-enter the window with their first step
        if grid != "far":                                      # (out there a float32 coordinate has a spacing of 2 voxels: the centre of a
            assert want[0][4, 0] == rr.UNKNOWN                 # voxel rounds into a neighbour)


def test_the_rows_agree_with_k_raycast_calls(maps):
    """no referee walk at all: K raycast() calls on the referee's TARGETS give, per viewpoint, the visits as the sum of their
    `unknown` column and columns 3 .. 7 as the histogram of their statuses"""
    for case in (vr.CASES[1], vr.CASES[2]):
        grid, bs, name, strides, K, rng, ub = case
        g, state, W = maps(grid, bs)
        d, o, poses, r = vr.case_inputs(case, state, W)
        g.set_sensor_model(d, o)
        rows, best = _got(g.score_viewpoints(poses, r, beam_stride=strides, unknown_blocks=ub), W, vr.case_id(case))
        for k, p in enumerate(vr.rows34(poses)):
            if not np.isfinite(p).all():
                continue
            a, b = vr.targets(d, o, p, r, strides)
            with g.raycast(a, b, unknown_blocks=ub) as rays:
                res, _ = rays.copy_to_host()
            assert rows[k, 2] == res[:, 3].sum(), (k, rows[k])
            assert rows[k, 3:].tolist() == [int((res[:, 0] == c).sum()) for c in (rr.OCCUPIED, rr.CLEAR, rr.LEFT_WINDOW, rr.UNKNOWN, rr.INVALID)], (k, rows[k])
            assert rows[k, 1] <= rows[k, 2]


def test_numba_cuda_typing_changes_the_step_rule_as_in_the_scan(gvom):
    grid = "p2"
    g = rr.build_map(gvom.Gvom, grid, 1, voxel_statistics=False, numba_cuda_typing=True)
    state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
    W = np.asarray(origin, np.float64)
    d, o = vr.model("m8x64")
    poses, r = vr.viewpoints_of(grid, state, W, 33), vr.max_range_of(grid, "third")
    g.set_sensor_model(d, o)
    for ub in (False, True):
        _hold(g.score_viewpoints(poses, r, unknown_blocks=ub), vr.product(state, W, grid, d, o, poses, r, (1, 1), ub, f32_sqrt=True), W, "f32 sqrt %d" % ub)


def test_a_product_is_a_snapshot(gvom):
    grid = "np2"
    g = rr.build_map(gvom.Gvom, grid, 2, voxel_statistics=False)
    state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
    W = np.asarray(origin, np.float64)
    d, o = vr.model("m5x37")
    poses, r = vr.viewpoints_of(grid, state, W, 33), vr.max_range_of(grid, "third")
    g.set_sensor_model(d, o)
    held = g.score_viewpoints(poses, r)
    before = held.copy_to_host()
    g.process_pointcloud(rr.cloud_of(grid, 9), rr.ego_of(grid, 9))         # a further scan from elsewhere, and its combine
    g.combine_maps()
    g.set_sensor_model(*vr.model("m8x64"))                                 # ... and another sensor
    after = held.copy_to_host()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    with g.score_viewpoints(poses, r) as again:                            # the map itself has moved on
        assert not np.array_equal(again.origin, held.origin)
        assert not np.array_equal(again.rows.copy_to_host(), before[0])
    k, gain, pose = held.best_pose()
    assert (k, gain) == tuple(before[1][:2]) and np.array_equal(pose, vr.rows34(poses)[k])
    held.release()


def test_pool_and_allocations(gvom, maps):
    g, state, W = maps("p2", 2)
    d, o = vr.model("m5x37")
    poses, r = vr.viewpoints_of("p2", state, W, 33), vr.max_range_of("p2", "third")
    g.set_sensor_model(d, o)
    assert g.get_tuning("viewpoints") == 1
    base = g.get_tuning("viewpoint_allocations")
    g.score_viewpoints(poses, r).release()
    first = g.get_tuning("viewpoint_allocations")
    for _ in range(20):                                        # steady state: nothing is allocated
        g.score_viewpoints(poses, r, unknown_blocks=True).release()
        g.score_viewpoints(poses[:3], r).release()
    assert g.get_tuning("viewpoint_allocations") == first >= base
    held = [g.score_viewpoints(poses, r) for _ in range(4)]
    assert len({v.rows.ptr for v in held}) == 4
    with pytest.raises(gvom.GvomBackendError, match="exported"):
        g.score_viewpoints(poses, r)                           # the fifth product of the kind while four are held
    p = vr.rows34(poses)
    assert g._lib.gvom_score_viewpoints(g._h, p.ctypes.data_as(ctypes.c_void_p), 33, 0, r, 1, 1, 0, None, ctypes.byref(ctypes.c_int64())) == GVOM_ERR_CAPACITY
    held.pop().release()
    _hold(g.score_viewpoints(poses, r), vr.product(state, W, "p2", d, o, poses, r), W, "after a release")
    for v in held:
        v.release()
    sets = g.get_tuning("device_product_sets")
    g.score_viewpoints(poses, r).release()
    assert g.get_tuning("device_product_sets") == sets


def test_errors(gvom, maps):
    g, state, W = maps("tall", 1)
    g.set_sensor_model(*vr.model("m5x37"))
    p = vr.rows34(vr.viewpoints_of("tall", state, W, 3))
    pp = p.ctypes.data_as(ctypes.c_void_p)
    pid = ctypes.c_int64(-1)

    def call(h, poses=pp, K=3, r=2.0, sh=1, sw=1, flags=0, out=pid):
        return h._lib.gvom_score_viewpoints(h._h, poses, K, 0, r, sh, sw, flags, None, ctypes.byref(out) if out is not None else None)
    assert call(g) == 0 and pid.value > 0                      # (origin_voxels may be NULL)
    assert call(g, K=0) == GVOM_ERR_INVALID and pid.value == -1
    assert call(g, K=-2) == GVOM_ERR_INVALID
    assert call(g, poses=None) == GVOM_ERR_INVALID and call(g, out=None) == GVOM_ERR_INVALID
    assert call(g, sh=0) == GVOM_ERR_INVALID and call(g, sw=-1) == GVOM_ERR_INVALID and b"strides" in g._lib.gvom_last_error(g._h)
    for r in (0.0, -1.0, float("inf"), float("nan")):
        assert call(g, r=r) == GVOM_ERR_INVALID and b"max_range" in g._lib.gvom_last_error(g._h)
    assert call(g, flags=2) == GVOM_ERR_INVALID and call(g, flags=-1) == GVOM_ERR_INVALID and call(g, flags=1) == 0   # (no CHECK_TARGET)
    assert call(g, K=65537) == GVOM_ERR_CAPACITY               # refused before anything is read
    assert g._lib.gvom_device_product(g._h, gvom.PRODUCT_VIEWPOINTS, 0, ctypes.byref(pid)) == GVOM_ERR_INVALID
    big = np.zeros((2049, 2049, 3))                            # 2049^2 > 2^22 selected beams; with strides (1, 8) 2049 x 257 beams x 49 steps < 2^31
    big[:, :, 0] = 1.0
    g.set_sensor_model(big)
    assert call(g) == GVOM_ERR_CAPACITY and b"2^22" in g._lib.gvom_last_error(g._h)
    assert call(g, sw=8) == 0
    g.set_sensor_model(*vr.model("m5x37"))
    for bad, word in ((dict(max_range=0.0), "max_range"), (dict(max_range="far"), "max_range"), (dict(beam_stride=(0, 1)), "beam_stride"),
                      (dict(beam_stride=3), "beam_stride"), (dict(beam_stride=(1.5, 1)), "beam_stride")):
        with pytest.raises(ValueError, match=word):
            g.score_viewpoints(p, **dict(dict(max_range=2.0), **bad))
    with pytest.raises(TypeError, match="float64"):
        g.score_viewpoints(p.astype(np.float32), 2.0)
    with pytest.raises(ValueError, match="shape"):
        g.score_viewpoints(p[:, :2], 2.0)
    with pytest.raises(ValueError, match="device address"):
        g.score_viewpoints_device(0, 3, 2.0)
    with pytest.raises(ValueError, match="65536"):
        g.score_viewpoints_device(1234, 65537, 2.0)
    # a window so large that nb * (xy + z + 1) reaches 2^31: 2^22 beams need xy + z + 1 >= 512
    wide = gvom.Gvom(0.4, 0.2, 512, 8, 1, *rr.params("p2", 1)[5:], voxel_statistics=False)
    wide.set_sensor_model(big[:2048, :2048])
    wide.process_pointcloud(rr.cloud_of("p2", 0), rr.ego_of("p2", 0))
    wide.combine_maps()
    assert call(wide) == GVOM_ERR_CAPACITY and b"2^31" in wide._lib.gvom_last_error(wide._h)
    fresh = gvom.Gvom(*rr.params("tall", 1), voxel_statistics=False)
    assert call(fresh) == GVOM_ERR_INVALID and b"sensor model" in fresh._lib.gvom_last_error(fresh._h)
    fresh.set_sensor_model(*vr.model("m5x37"))
    assert call(fresh) == GVOM_NO_DATA and fresh.score_viewpoints(p, 2.0) is None
    fresh.process_pointcloud(rr.cloud_of("tall", 0), rr.ego_of("tall", 0))
    assert fresh.score_viewpoints(p, 2.0) is None              # scanned, not combined yet
    fresh.combine_maps()
    assert fresh.score_viewpoints(p, 2.0) is not None
    sharded = gvom.Gvom(*rr.params("tall", 1), voxel_statistics=False, _shard=(0, 1))
    assert call(sharded) == GVOM_ERR_INVALID and b"sharded" in sharded._lib.gvom_last_error(sharded._h)


@pytest.mark.parametrize("name", ("one_round", "two_rounds"))
def test_scenes_end_to_end_from_the_device_maps_to_the_scores(gvom, name):
    """combine_maps_device(), a field seeded at the ego, frontiers(), goals(), viewpoint_poses(), score_viewpoints(): the candidates
    are the cheapest frontier goals at sensor height under four yaws, and the product equals the referee's on the handle's own map"""
    xy, z_res, zs = ob.GRIDS[name][:3]
    grid = "scene_" + name
    rr.GRIDS.setdefault(grid, (ob.XY_RES, z_res, xy, zs))
    g = gvom.Gvom(*ob.params(name), voxel_statistics=False)
    for pc, ego in ob.scans(name):
        g.process_pointcloud(pc, ego)
    d, o = vr.model("m8x64")
    g.set_sensor_model(d, o)
    with g.combine_maps_device() as m:
        with m.cost_to_go([ego[:2]], density_threshold=cf.SCENE_THRESHOLD) as field:
            with field.frontiers(m, min_cells=3) as f:
                best, _, _ = f.goals("cost")
    assert len(best) >= 1
    points = np.column_stack([best[:8], np.full(len(best[:8]), ego[2] + 0.5)])
    mount = vr.pose_of((0.1, 0.0, 0.3), 0.0, 0.05)
    poses = gvom.viewpoint_poses(points, [0.0, 0.8, 1.6, 2.4], sensor_to_body=mount)
    assert poses.shape == (4 * len(points), 4, 4) and np.array_equal(poses[1], vr.pose_of(points[0], 0.8).dot(mount))
    state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
    W = np.asarray(origin, np.float64)
    for ub in (False, True):
        want = vr.product(state, W, grid, d, o, poses, 6.0, (1, 1), ub)
        rows, best_row = _hold(g.score_viewpoints(poses, 6.0, unknown_blocks=ub), want, W, "%s ub %d" % (name, ub))
    print(name, "K", len(poses), "best", best_row, "statuses", np.bincount(rows[:, 0], minlength=5))
    assert (rows[:, 1] > 0).any() and (rows[:, 2] > rows[:, 1]).any()


def test_torch_consumer():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_viewpoints_torch.py"), "consumer_stream"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "CASE OK consumer_stream" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
