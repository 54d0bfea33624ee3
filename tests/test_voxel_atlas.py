"""The voxel atlas on the GPU (gvom_voxel_atlas_*: gvom_voxel_atlas.hip; Gvom.create_voxel_atlas, VoxelAtlas) against the numpy referee of
tests/voxel_atlas_ref.py, which is fed with the dense fused states the SAME handle returns (read_dense(GVOM_WHICH_FUSED)): it referees the
atlas, not the mapper.  Tolerance 0 everywhere; float positions are compared through their bit patterns.

  the drive              17 scans out and back, climbing, rings of 1 and 2 slots, following and fixed: after every integrate counts() and the
                         box at four origins equal the referee at every voxel
  first integrate        on tests/raycast_ref.py's grids a ray that gvom_raycast does not report LEFT_WINDOW has the same answer in the atlas
  remembered space       rays to and between remembered voxels outside the final window; gvom_raycast answers LEFT_WINDOW there
  viewpoints             poses outside and inside the final window; gvom_score_viewpoints' rows after one integrate; the bitmap budget
  cycle, housekeeping    a scan alone changes nothing an integrate merges (the full cycle: tests/test_voxel_atlas_cycle.py); errors, the pool, allocations, clear, free, the largest atlas"""
import ctypes

import numpy as np
import pytest

import raycast_ref as rr
import viewpoint_ref as vr
import voxel_atlas_ref as va

pytestmark = pytest.mark.gpu
FLAGS = [(False, False), (True, False), (False, True), (True, True)]       # (unknown_blocks, check_target)
GVOM_ERR_INVALID, GVOM_ERR_CAPACITY, GVOM_NO_DATA = -1, -4, 4
rr.GRIDS.setdefault("vdrive", va.DRIVE_PARAMS)                             # the drive's grid, for rays_of (a grid of this file's own)


@pytest.fixture(scope="module")
def gvom():
    import gvom as mod
    rc, info = mod.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    return mod


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _hold_rays(rays, want, E, what):
    with rays:
        assert tuple(rays.extent_origin) == tuple(int(v) for v in E), what
        result, position, voxel = rays.copy_to_host()
    wr, wp, wv = want
    assert result.dtype == np.int32 and position.dtype == np.float32 and voxel.dtype == np.int32 and result.shape == wr.shape, what
    if not np.array_equal(result, wr):
        bad = np.flatnonzero((result != wr).any(axis=1))
        raise AssertionError("%s: %d rays differ, first %d: got %r, referee %r" % (what, len(bad), bad[0], result[bad[0]], wr[bad[0]]))
    assert ((_bits(position) == _bits(wp)) | (np.isnan(position) & np.isnan(wp))).all(), what
    assert np.array_equal(np.isnan(position), np.isnan(wp)) and np.array_equal(voxel, wv), what
    return result, position, voxel


def _hold_box(box, want, origin, what):
    with box:
        assert tuple(box.origin_voxels) == tuple(int(v) for v in origin), what
        classes, counts = box.copy_to_host()
    assert classes.dtype == np.uint8 and classes.shape == want[0].shape and np.array_equal(classes, want[0]), what
    assert np.array_equal(counts, want[1]), (what, counts, want[1])


def _drive(gvom, ring, follow, each=None):
    """the climbing drive on a fresh mapper and atlas, the referee beside it; each(k, g, atlas, ref, first W) after every integrate"""
    g = gvom.Gvom(*(va.DRIVE_PARAMS + (ring,) + va.DRIVE_TAIL), voxel_statistics=False)
    kw = dict(follow=True) if follow else dict(follow=False, origin_voxels=np.array(va.fixed_origin()))
    atlas = g.create_voxel_atlas(va.DRIVE_A, va.DRIVE_Z, **kw)
    assert g.get_tuning("voxel_atlas") == va.DRIVE_A and g.get_tuning("voxel_atlas_levels") == va.DRIVE_Z
    ref = va.VoxelAtlasRef(va.DRIVE_A, va.DRIVE_Z, va.DRIVE_XY, va.DRIVE_ZS, follow=follow, origin=(0, 0, 0) if follow else va.fixed_origin())
    first = None
    for k, (pc, ego) in enumerate(va.drive_scans()):
        g.process_pointcloud(pc, ego)
        g.combine_maps()
        state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
        W = tuple(int(v) for v in origin)
        assert W == va.window_origin(ego)
        first = first or W
        assert atlas.integrate() is True
        ref.integrate(state, W)
        assert atlas.extent_origin == ref.E and atlas.seq == ref.seq == k + 1
        if each:
            each(k, g, atlas, ref, first)
    return g, atlas, ref, W, ego, (pc, state)


@pytest.fixture(scope="module")
def driven(gvom):
    """per ring length: the following atlas after the drive -- (mapper, atlas, referee, final W, final ego, (last cloud, last state))"""
    return {ring: _drive(gvom, ring, True) for ring in (1, 2)}


# ---- 3. the drive ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("follow", [True, False])
@pytest.mark.parametrize("ring", [1, 2])
def test_the_drive_counts_and_boxes_equal_the_referee_after_every_integrate(gvom, ring, follow):
    def each(k, g, atlas, ref, first):
        got, want = atlas.counts(), ref.counts()
        assert got == want, (k, got, want)
        assert sum(got[n] for n in va.COUNT_NAMES[:6]) == va.DRIVE_XY ** 2 * va.DRIVE_ZS
        for j, origin in enumerate(va.box_origins(ref, first)):
            _hold_box(atlas.box(None if j == 0 else np.array(origin)), ref.box(origin), origin, "integrate %d, box %d" % (k, j))
    g, atlas, ref, W, ego, _ = _drive(gvom, ring, follow, each)
    print(ring, follow, ref.total, ref.counts())
    need = va.COUNT_NAMES[:5] + (("cleared", "cleared_observed") if follow else ("outside",))
    assert all(ref.total[n] >= 1 for n in need), ref.total
    # the centre route of box(): the window a scan at the final ego would have
    _hold_box(atlas.box(center=ego), ref.box(W), W, "box by centre")
    atlas.release()
    assert g.get_tuning("voxel_atlas") == 0


# ---- 4. first integrate equals the window ----------------------------------------------------------------------------------------------------
def _atlas_sides(xy, zs):
    A = 64
    while A < xy or A < zs:
        A *= 2
    Z = 1
    while Z < zs:
        Z *= 2
    return A, Z


@pytest.mark.parametrize("grid", ["p2", "np2", "tall", "w128", "w192", "far", "v256"])      # (v256: more rows than k_vatlas_merge has waves)
def test_after_one_integrate_the_atlas_answers_as_the_window_does(gvom, grid):
    xr, zr, xy, zs = rr.GRIDS[grid]
    res = (xr, xr, zr)
    g = rr.build_map(gvom.Gvom, grid, 2, voxel_statistics=False)
    state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
    W = np.asarray(origin, np.float64)
    A, Z = _atlas_sides(xy, zs)
    assert A == (256 if grid == "w192" else A)
    room = [(A, A, Z)[k] - (xy, xy, zs)[k] for k in range(3)]                  # the window lies inside the extent, off its middle where there is room
    E = tuple(int(W[k]) - min(room[k], room[k] // 2 + (3, 1, 0)[k]) for k in range(3))
    assert (grid == "far") == all(abs(e) >= 1 << 24 for e in E)               # far: the literal lookup
    atlas = g.create_voxel_atlas(A, Z, follow=False, origin_voxels=np.array(E))
    ref = va.VoxelAtlasRef(A, Z, xy, zs, follow=False, origin=E)
    assert atlas.integrate() and ref.integrate(state, W)["outside"] == 0
    assert atlas.counts() == ref.counts()
    a, b, fam = rr.rays_of(grid, state, W)
    for ub, ct in FLAGS:
        want = va.atlas_walk(ref, res, a, b, unknown_blocks=ub, check_target=ct)
        result, position, voxel = _hold_rays(atlas.raycast(a, b, unknown_blocks=ub, check_target=ct), want, E, "%s flags %d%d" % (grid, ub, ct))
        with g.raycast(a, b, unknown_blocks=ub, check_target=ct) as rays:
            wres, wpos = rays.copy_to_host()
        same = wres[:, 0] != rr.LEFT_WINDOW
        assert same.sum() >= 2048 and np.array_equal(result[same], wres[same][:, [0, 1, 3]]), (grid, ub, ct)
        assert (_bits(position[same]) == _bits(wpos[same])).all()
        v = wres[same, 2].astype(np.int64)
        decoded = np.stack([v % xy, v // xy % xy, v // (xy * xy)], axis=1) + W.astype(np.int64)
        assert np.array_equal(voxel[same], np.where((v >= 0)[:, None], decoded, 0)), (grid, ub, ct)
    # one origin for all rays, and the device route
    want = va.atlas_walk(ref, res, a[:1], b, unknown_blocks=True)
    _hold_rays(atlas.raycast(a[0], b, unknown_blocks=True), want, E, grid + ", one origin")


# ---- 5. remembered space ---------------------------------------------------------------------------------------------------------------------
class _Hip(object):
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


@pytest.fixture(scope="module")
def hip():
    h = _Hip()
    yield h
    h.free()


@pytest.mark.parametrize("ring", [1, 2])
def test_rays_through_remembered_space_equal_the_referee(driven, hip, ring):
    g, atlas, ref, W, ego, (pc, state) = driven[ring]
    a, b = va.drive_rays(ref, W, ego)
    fa, fb, fam = rr.rays_of("vdrive", state, np.array(W, np.float64), last=(ego, np.asarray(pc)))
    a, b = np.concatenate([a, fa]), np.concatenate([b, fb])
    da, db = hip.upload(a), hip.upload(b)
    for ub, ct in FLAGS:
        want = va.atlas_walk(ref, va.DRIVE_RES, a, b, unknown_blocks=ub, check_target=ct, record=(ub, ct) == (True, False))
        result, position, voxel = _hold_rays(atlas.raycast(a, b, unknown_blocks=ub, check_target=ct), want[:3], ref.E, "ring %d flags %d%d" % (ring, ub, ct))
        _hold_rays(atlas.raycast_device(da, len(a), db, len(b), unknown_blocks=ub, check_target=ct), want[:3], ref.E, "device route")
        if (ub, ct) == (True, False):                                       # the census of tests/test_voxel_atlas_cpu.py, on the GPU's own answer
            n = len(a) - len(fa)
            w = voxel[:n].astype(np.int64) - np.array(W)
            outside = ~((w >= 0) & (w < np.array([va.DRIVE_XY, va.DRIVE_XY, va.DRIVE_ZS]))).all(axis=1)
            counted = np.flatnonzero((result[:n, 0] == va.HIT) & outside)
            status = [int((result[:n, 0] == k).sum()) for k in range(5)]
            seams = va.seam_crossers(ref, [v for v in want[3] if v[0] < n], n)
            print(ring, status, len(counted), seams)
            assert len(counted) >= 256 and min(status) >= 32 and min(seams) >= 32
            with g.raycast(a[counted], b[counted]) as rays:                  # the window alone cannot answer them
                assert (rays.result.copy_to_host()[:, 0] == rr.LEFT_WINDOW).all()


# ---- 6. viewpoints ---------------------------------------------------------------------------------------------------------------------------
def _hold_views(v, want, E, what):
    with v:
        assert tuple(v.extent_origin) == tuple(int(e) for e in E), what
        rows, best = v.copy_to_host()
    assert rows.dtype == np.int32 and np.array_equal(rows, want[0]), (what, np.flatnonzero((rows != want[0]).any(axis=1))[:4], rows[:4], want[0][:4])
    assert np.array_equal(best, want[1]), (what, best, want[1])
    return rows, best


@pytest.mark.parametrize("ring", [1, 2])
def test_viewpoints_in_remembered_space_equal_the_referee(driven, hip, ring):
    g, atlas, ref, W, ego, _ = driven[ring]
    d, o = vr.model("m8x64" if ring == 1 else "off5x37")
    g.set_sensor_model(d, o)
    poses = va.drive_poses(ref, W, ego)
    poses[7, 1, 2] = np.nan                                                 # an invalid pose among them
    state = ref.dense_state()
    dev = hip.upload(np.ascontiguousarray(poses[:, :3, :]))
    base = None
    for strides in ((1, 1), (2, 3)):
        for ub in (False, True):
            want = va.viewpoints(state, ref.E, ref.sizes(), va.DRIVE_RES, d, o, poses, 9.0, strides, ub)
            what = "ring %d strides %r ub %d" % (ring, strides, ub)
            rows, best = _hold_views(atlas.score_viewpoints(poses, 9.0, beam_stride=strides, unknown_blocks=ub), want, ref.E, what)
            _hold_views(atlas.score_viewpoints_device(dev, len(poses), 9.0, beam_stride=strides, unknown_blocks=ub), want, ref.E, what + ", device")
            if strides == (1, 1) and not ub:
                base = rows
                assert (rows[:16, 1] > 0).any() and (rows[:, 2] > rows[:, 1]).any() and rows[7, 0] == va.INVALID
                with g.score_viewpoints(poses, 9.0) as win:                  # from outside the window the window form sees nothing
                    wrows = win.rows.copy_to_host()
                assert (wrows[:16][np.arange(16) != 7, 0] == rr.LEFT_WINDOW).all()
                k, gain, pose = atlas.score_viewpoints(poses, 9.0).best_pose()
                assert (k, gain) == (int(want[1][0]), int(want[1][1])) and np.array_equal(pose, poses[k, :3])
    # the bitmap budget changes the batches, never the product
    try:
        g.set_tuning("viewpoint_bitmap_mb", 0)
        with atlas.score_viewpoints(poses, 9.0) as v:
            one = v.copy_to_host()
        assert g.get_tuning("voxel_atlas_viewpoint_batch") == 1
    finally:
        g.set_tuning("viewpoint_bitmap_mb", -1)
    with atlas.score_viewpoints(poses, 9.0) as v:
        many = v.copy_to_host()
    assert g.get_tuning("voxel_atlas_viewpoint_batch") == len(poses)
    assert np.array_equal(one[0], many[0]) and np.array_equal(one[1], many[1]) and np.array_equal(one[0], base)


def test_after_one_integrate_viewpoints_without_a_beam_that_leaves_equal_the_windows(gvom):
    grid = "p2"
    xr, zr, xy, zs = rr.GRIDS[grid]
    g = rr.build_map(gvom.Gvom, grid, 1, voxel_statistics=False)
    state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
    W = np.asarray(origin, np.float64)
    E = tuple(int(W[k]) - (17, 40, 9)[k] for k in range(3))
    atlas = g.create_voxel_atlas(128, 64, follow=False, origin_voxels=np.array(E))
    ref = va.VoxelAtlasRef(128, 64, xy, zs, follow=False, origin=E)
    atlas.integrate(); ref.integrate(state, W)
    d, o = vr.model("m8x64")
    g.set_sensor_model(d, o)
    poses = vr.viewpoints_of(grid, state, W, 33)
    r = 2.0                                                                 # 5 voxels: a third of the poses keep every beam inside the window
    for ub in (False, True):
        want = va.viewpoints(ref.dense_state(), E, ref.sizes(), (xr, xr, zr), d, o, poses, r, (1, 1), ub)
        rows, _ = _hold_views(atlas.score_viewpoints(poses, r, unknown_blocks=ub), want, E, "p2 ub %d" % ub)
        with g.score_viewpoints(poses, r, unknown_blocks=ub) as win:
            wrows = win.rows.copy_to_host()
        stay = (wrows[:, 5] == 0) & (wrows[:, 0] != rr.LEFT_WINDOW)
        assert stay.sum() >= 8 and np.array_equal(rows[stay], wrows[stay]), (ub, int(stay.sum()))


# ---- 7. the scan cycle -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring", [1, 2])
def test_a_scan_changes_what_is_merged_only_after_its_combine(gvom, ring):
    """one scan that has not been combined, with the referee fed from the handle's own read_dense.  The full cycle -- every point of
    tests/query_cycle.py's scripts, the referee fed from the CPU oracle's maps alone -- is tests/test_voxel_atlas_cycle.py"""
    grid = "np2"
    xr, zr, xy, zs = rr.GRIDS[grid]
    g = rr.build_map(gvom.Gvom, grid, ring, voxel_statistics=False)
    state0, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
    W0 = tuple(int(v) for v in origin)
    atlas = g.create_voxel_atlas(64, 32)
    ref = va.VoxelAtlasRef(64, 32, xy, zs)
    g.process_pointcloud(rr.cloud_of(grid, 9), rr.ego_of(grid, 9))         # accepted, not combined: the current fused map is the old one
    atlas.integrate(); ref.integrate(state0, W0)
    assert atlas.counts() == ref.counts()
    _hold_box(atlas.box(), ref.box(), W0, "a scan behind the combine")
    g.combine_maps()
    state1, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
    W1 = tuple(int(v) for v in origin)
    assert W1 != W0
    atlas.integrate(); ref.integrate(state1, W1)
    assert atlas.counts() == ref.counts() and ref.last["cleared"] > 0
    _hold_box(atlas.box(), ref.box(), W1, "after the next combine")
    _hold_box(atlas.box(np.array(W0)), ref.box(W0), W0, "the first window, remembered")


# ---- 8. housekeeping ---------------------------------------------------------------------------------------------------------------------------
def test_errors_and_no_data(gvom):
    g = gvom.Gvom(*rr.params("tall", 1), voxel_statistics=False)               # xy 16, z 32
    L, h = g._lib, g._h
    pid, out3 = ctypes.c_int64(-1), (ctypes.c_int64 * 3)()
    a = np.zeros((8, 3), np.float32); b = np.ones((8, 3), np.float32)
    pa, pb = a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p)
    poses = np.ascontiguousarray(vr.rows34(np.stack([vr.pose_of((0.0, 0.0, 0.0))] * 3)))
    pp = poses.ctypes.data_as(ctypes.c_void_p)

    def err():
        return L.gvom_last_error(h)
    # no voxel atlas configured
    assert g.get_tuning("voxel_atlas") == 0 and g.get_tuning("voxel_atlas_levels") == 0
    for rc in (L.gvom_voxel_atlas_integrate(h), L.gvom_voxel_atlas_clear(h), L.gvom_voxel_atlas_counts(h, (ctypes.c_int64 * 11)()),
               L.gvom_voxel_atlas_box(h, None, ctypes.byref(pid), None), L.gvom_voxel_atlas_raycast(h, pa, 8, pb, 8, 0, 0, None, ctypes.byref(pid)),
               L.gvom_voxel_atlas_score_viewpoints(h, pp, 3, 0, 2.0, 1, 1, 0, None, ctypes.byref(pid))):
        assert rc == GVOM_ERR_INVALID and b"no voxel atlas" in err()
    # sizes, mode, origin
    for cells, levels, mode, org in ((96, 32, 0, None), (32, 32, 0, None), (8192, 32, 0, None), (64, 16, 0, None), (64, 48, 0, None), (64, 128, 0, None),
                                     (4096, 512, 0, None), (64, 32, 2, None), (64, 32, -1, None), (64, 32, 1, (1 << 30, 0, 0)), (64, 32, 0, (0, 0, -(1 << 30)))):
        o = None if org is None else (ctypes.c_int64 * 3)(*org)
        assert L.gvom_voxel_atlas_configure(h, cells, levels, mode, o) == GVOM_ERR_INVALID, (cells, levels, mode, org)
    assert g.get_tuning("voxel_atlas") == 0
    atlas = g.create_voxel_atlas(64, 32)
    # before the first combine
    assert L.gvom_voxel_atlas_integrate(h) == GVOM_NO_DATA and atlas.integrate() is False and atlas.seq == 0
    assert atlas.box() is None and atlas.raycast(a, b) is None
    g.set_sensor_model(*vr.model("m5x37"))
    assert atlas.score_viewpoints(poses, 2.0) is None
    assert atlas.counts() == dict.fromkeys(gvom.VOXEL_ATLAS_COUNTS, 0)
    g.process_pointcloud(rr.cloud_of("tall", 0), rr.ego_of("tall", 0))
    assert atlas.integrate() is False                                          # scanned, not combined yet
    g.combine_maps()
    assert atlas.integrate() is True and atlas.counts()["seq"] == 1

    def ray(frm=pa, K=8, to=pb, n=8, flags=0, out=pid):
        return L.gvom_voxel_atlas_raycast(h, frm, K, to, n, 0, flags, out3, ctypes.byref(out) if out is not None else None)
    assert ray() == 0 and pid.value > 0 and tuple(out3) == atlas.extent_origin
    assert ray(n=0) == GVOM_ERR_INVALID and pid.value == -1
    assert ray(K=2) == GVOM_ERR_INVALID and b"K must be 1 or n" in err()
    assert ray(frm=None) == GVOM_ERR_INVALID and ray(to=None) == GVOM_ERR_INVALID and ray(out=None) == GVOM_ERR_INVALID
    assert ray(flags=4) == GVOM_ERR_INVALID and ray(flags=-1) == GVOM_ERR_INVALID and ray(flags=3) == 0
    assert ray(K=1, n=(1 << 26) + 1) == GVOM_ERR_CAPACITY

    def view(p=pp, K=3, r=2.0, sh=1, sw=1, flags=0, out=pid):
        return L.gvom_voxel_atlas_score_viewpoints(h, p, K, 0, r, sh, sw, flags, None, ctypes.byref(out) if out is not None else None)
    assert view() == 0 and pid.value > 0
    assert view(K=0) == GVOM_ERR_INVALID and view(p=None) == GVOM_ERR_INVALID and view(out=None) == GVOM_ERR_INVALID
    assert view(sh=0) == GVOM_ERR_INVALID and view(sw=-1) == GVOM_ERR_INVALID and view(flags=2) == GVOM_ERR_INVALID
    assert view(r=0.0) == GVOM_ERR_INVALID and view(r=float("inf")) == GVOM_ERR_INVALID and view(r=float("nan")) == GVOM_ERR_INVALID
    assert view(K=65537) == GVOM_ERR_CAPACITY and b"65536" in err()
    big = np.zeros((2049, 2048, 3)); big[:, :, 0] = 1.0
    g.set_sensor_model(big)
    assert view() == GVOM_ERR_CAPACITY and b"2^22" in err()
    g.set_sensor_model(*vr.model("m5x37"))
    assert L.gvom_voxel_atlas_box(h, None, None, None) == GVOM_ERR_INVALID and L.gvom_voxel_atlas_counts(h, None) == GVOM_ERR_INVALID
    for kind in (32, 34, 36):
        assert L.gvom_device_product(h, kind, 0, ctypes.byref(pid)) == GVOM_ERR_INVALID
    for kind in (31, 33, 35):
        assert L.gvom_device_product(h, kind, 0, ctypes.byref(pid)) == GVOM_ERR_INVALID
    # a window at or beyond 2^30 voxels is not integrated (the mapper itself goes there: its literal float64 lookup), and the atlas stays as it was
    xr, zr, xy, zs = rr.GRIDS["tall"]
    seq, E, known = atlas.seq, atlas.extent_origin, atlas.counts()["observed"]
    rng = np.random.default_rng(5)
    for axis, sign in ((0, 1.0), (1, -1.0)):
        ego = [0.0, 0.0, 0.0]
        ego[axis] = sign * ((1 << 30) + 64) * xr
        pc = np.array(ego) + rng.uniform(-0.4, 0.4, (384, 3)) * np.array([xr * xy, xr * xy, zr * zs])       # float64 returns around the ego
        g.process_pointcloud(pc, tuple(ego))
        g.combine_maps()
        W = [int(v) for v in g.read_dense(gvom.GVOM_WHICH_FUSED)[4]]
        assert abs(W[axis]) >= 1 << 30, W
        assert L.gvom_voxel_atlas_integrate(h) == GVOM_ERR_INVALID and b"2^30" in err()
        with pytest.raises(ValueError, match="2\\^30"):
            atlas.integrate()
        assert (atlas.seq, atlas.extent_origin) == (seq, E) and atlas.counts()["seq"] == seq and atlas.counts()["observed"] == known
    g.process_pointcloud(rr.cloud_of("tall", 1), rr.ego_of("tall", 1))
    g.combine_maps()
    assert atlas.integrate() is True and atlas.counts()["seq"] == seq + 1      # back near the origin: merged again
    # box(None) is the last integrated window: there is none right after a configure, whatever the mapper has combined
    atlas = g.create_voxel_atlas(64, 32)
    assert L.gvom_voxel_atlas_box(h, None, ctypes.byref(pid), None) == GVOM_NO_DATA and pid.value == -1 and atlas.box() is None
    with atlas.box(np.array([0, 0, 0])) as box:
        assert not box.classes.copy_to_host().any()
    sharded = gvom.Gvom(*rr.params("tall", 1), voxel_statistics=False, _shard=(0, 1))
    assert sharded._lib.gvom_voxel_atlas_configure(sharded._h, 64, 32, 0, None) == GVOM_ERR_INVALID and b"sharded" in sharded._lib.gvom_last_error(sharded._h)
    assert sharded._lib.gvom_voxel_atlas_integrate(sharded._h) == GVOM_ERR_INVALID and b"sharded" in sharded._lib.gvom_last_error(sharded._h)


def test_the_pool_allocations_clear_and_free(gvom, driven):
    g, atlas, ref, W, ego, (pc, state) = driven[2]
    a, b = va.drive_rays(ref, W, ego)
    a, b = a[:500], b[:500]
    d, o = vr.model("m5x37")
    g.set_sensor_model(d, o)
    poses = va.drive_poses(ref, W, ego)[:8]
    with atlas.raycast(a, b), atlas.box(), atlas.score_viewpoints(poses, 6.0):
        pass
    first = g.get_tuning("voxel_atlas_allocations")
    for k in range(20):                                                     # steady state: scan, combine, integrate and the queries
        g.process_pointcloud(pc, ego)
        g.combine_maps()
        atlas.integrate()
        atlas.raycast(a, b, check_target=True).release()
        atlas.box().release()
        atlas.score_viewpoints(poses, 6.0).release()
    assert g.get_tuning("voxel_atlas_allocations") == first
    held = [atlas.raycast(a, b) for _ in range(4)]
    assert len({r.result.ptr for r in held}) == 4
    with pytest.raises(gvom.GvomBackendError, match="exported"):
        atlas.raycast(a, b)                                                 # the fifth product of the kind while four are held
    held.pop().release()
    atlas.raycast(a, b).release()                                           # export, release, reuse
    for r in held:
        r.release()
    sets = g.get_tuning("device_product_sets")
    atlas.raycast(a, b).release()
    assert g.get_tuning("device_product_sets") == sets
    seq, E = atlas.counts()["seq"], atlas.extent_origin
    assert atlas.counts()["observed"] > 0
    atlas.clear()
    c = atlas.counts()
    assert c["observed"] == c["occupied"] == 0 and c["seq"] == seq and atlas.extent_origin == E
    classes, counts = atlas.box().copy_to_host()
    assert not classes.any() and list(counts) == [0, 0, 0, seq]
    atlas.release()                                                         # configure(0) frees
    assert g.get_tuning("voxel_atlas") == 0
    with pytest.raises(ValueError, match="no voxel atlas"):
        atlas.integrate()


def test_the_largest_atlas(gvom):
    """4096 x 4096 x 128 voxels, 512 MiB: configure, one integrate, counts"""
    grid = "p2"
    xr, zr, xy, zs = rr.GRIDS[grid]
    g = gvom.Gvom(*rr.params(grid, 1), voxel_statistics=False)
    g.process_pointcloud(rr.cloud_of(grid, 0), rr.ego_of(grid, 0))
    g.combine_maps()
    state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
    atlas = g.create_voxel_atlas(4096, 128)
    assert g.get_tuning("voxel_atlas") == 4096 and g.get_tuning("voxel_atlas_levels") == 128
    assert atlas.integrate()
    c = atlas.counts()
    cls = va.classes(state)
    assert c["observed"] == c["first_seen"] == int((cls != va.NEVER).sum()) and c["occupied"] == int((cls == va.OCCUPIED).sum())
    stayed = 1
    for e, size in zip(atlas.extent_origin, (4096, 4096, 128)):              # the extent came from (0, 0, 0)
        stayed *= max(0, size - abs(e))
    assert c["uninformative"] == int((cls == va.NEVER).sum()) and c["outside"] == 0 and c["cleared"] == 4096 * 4096 * 128 - stayed and c["cleared_observed"] == 0
    classes, counts = atlas.box().copy_to_host()
    assert np.array_equal(classes, cls.reshape(zs, xy, xy).transpose(2, 1, 0))
    # the two refusals of the viewpoint call that only an atlas of this size reaches, in the order of the checks: A + Z + 1 = 4225
    L, h = g._lib, g._h
    pid = ctypes.c_int64(-1)
    centre = (np.asarray(origin, np.float64) + 0.5 * np.array([xy, xy, zs])) * np.array([xr, xr, zr])
    poses = np.ascontiguousarray(vr.rows34(np.stack([vr.pose_of(tuple(centre)), vr.pose_of(tuple(centre), yaw=0.7, pitch=0.2)])))
    pp = poses.ctypes.data_as(ctypes.c_void_p)

    def view(r, sh=1, sw=1):
        rc = L.gvom_voxel_atlas_score_viewpoints(h, pp, 2, 0, r, sh, sw, 0, None, ctypes.byref(pid))
        return rc, L.gvom_last_error(h)
    far = 4096 * xr * 8                                                        # beams that end far beyond the extent on every axis
    g.set_sensor_model(np.ones((512, 1024, 3)))                               # 2^19 beams, all along (1, 1, 1)
    assert 512 * 1024 * 4225 >= 1 << 31 and 256 * 1024 * 4225 < 1 << 31 and 4096 * 4096 * 128 == 1 << 31
    rc, text = view(far)
    assert rc == GVOM_ERR_CAPACITY and pid.value == -1 and b"beams x (cells + levels + 1) reaches 2^31" in text, text
    rc, text = view(2.0)
    assert rc == GVOM_ERR_CAPACITY and b"reaches 2^31" in text, text         # whatever the range
    rc, text = view(far, sh=2)                                               # half the beams pass; now the clipped box is the whole extent: 2^31 voxels
    assert rc == GVOM_ERR_CAPACITY and pid.value == -1 and b"the box of a pose holds 2^31 voxels or more" in text, text
    rc, text = view(2.0, sh=2)                                               # the same beams at a range whose box is small
    assert rc == 0 and pid.value > 0, text
    with pytest.raises(gvom.GvomBackendError, match="box of a pose"):
        atlas.score_viewpoints(poses, far, beam_stride=(2, 1))
    v = atlas.score_viewpoints(poses, 2.0, beam_stride=(2, 1))
    assert v.rows.copy_to_host()[:, 7].sum() == 0 and (v.rows.copy_to_host()[:, 3:7].sum(axis=1) == 256 * 1024).all()
    v.release()
    atlas.release()
