"""Scan alignment scoring against the voxel atlas on the GPU (gvom_voxel_atlas_score_alignments: k_vatlas_align_field in front of the
unchanged k_align_score and k_align_best; VoxelAtlas.score_alignments, score_alignments_device) against the referee of
tests/voxel_atlas_align_ref.py, which is fed with the dense fused states the SAME handle returns (read_dense(GVOM_WHICH_FUSED)).
Tolerance 0 everywhere: everything is integer.

  first integrate        on ten grids, after one integrate into a fresh atlas and with a NULL origin, both parts equal
                         gvom_score_alignments' on the same handle bit for bit, dilate 1 included, through both division forms
  every voxel            planted maps under line probes at the window and at two displaced origins (words, pairs and level chunks on other
                         phases, part of the box outside the extent): every voxel of the class grid is held to the referee three times
  remembered space       the climbing drive, rings of 1 and 2 slots: scans 4, 6, 8, 10 and 16 in the box at their own window origin; the six
                         boxes of the halo census under line probes; the centre route; the fixed-mode drive probed after every integrate
  box independence       a cloud inside the intersection of two boxes has the same counts in both
  cycle, housekeeping    a scan and a combine between integrate and query change nothing; routes, the pool, allocations, refusals, clear"""
import ctypes
import re

import numpy as np
import pytest

import align_ref as ar
import raycast_ref as rr
import voxel_atlas_align_ref as vaa
import voxel_atlas_ref as va

pytestmark = pytest.mark.gpu
GVOM_ERR_INVALID, GVOM_ERR_CAPACITY, GVOM_NO_DATA = -1, -4, 4
FIRST_GRIDS = ("p2", "np2", "tall", "w128", "w192", "far", "r72", "r37", "third", "odd")
PLANTED_GRIDS = ("r72", "r37", "w192", "tall")
SHIFT = (-17, 5, -3)                                           # the displaced origin every planted grid is probed at


@pytest.fixture(scope="module")
def gvom():
    import gvom as mod
    rc, info = mod.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    assert mod.PRODUCT_VOXEL_ATLAS_ALIGNMENT == 38
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


def _hold(r, want, what, origin=None):
    """a DeviceAtlasAlignments (or DeviceAlignments) against (counts, best): both parts, exactly"""
    assert r is not None, what
    with r:
        if origin is not None:
            assert tuple(r.origin_voxels) == tuple(int(v) for v in origin), (what, r.origin_voxels)
        counts, best = r.copy_to_host()
    assert counts.dtype == np.int32 and best.dtype == np.int32, what
    assert counts.shape == want[0].shape and best.shape == (4,), (what, counts.shape, best.shape)
    if not np.array_equal(counts, want[0]):
        bad = np.flatnonzero((counts != want[0]).any(axis=1))
        raise AssertionError("%s: the counts differ in %d candidates, first %d: got %r, want %r" % (
            what, len(bad), bad[0], counts[bad[0]].tolist(), want[0][bad[0]].tolist()))
    assert best.tolist() == want[1].tolist(), (what, best.tolist(), want[1].tolist())
    return counts, best


def _atlas_sides(xy, zs):
    A = 64
    while A < xy or A < zs:
        A *= 2
    Z = 1
    while Z < zs:
        Z *= 2
    return A, Z


def _fixed_atlas(g, gvom, grid, low=(5, 1, 0)):
    """a fresh fixed atlas of the smallest legal sides around the current window, the window `low` voxels (where there is room) above the
    extent's corner; its referee after one integrate.  Returns (atlas, referee, state, W)"""
    _, _, xy, zs = ar.GRIDS[grid]
    state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
    W = tuple(int(v) for v in origin)
    A, Z = _atlas_sides(xy, zs)
    room = (A - xy, A - xy, Z - zs)
    E = tuple(W[k] - min(room[k], low[k]) for k in range(3))
    atlas = g.create_voxel_atlas(A, Z, follow=False, origin_voxels=np.array(E))
    ref = va.VoxelAtlasRef(A, Z, xy, zs, follow=False, origin=E)
    assert atlas.integrate() is True and ref.integrate(state, W)["outside"] == 0
    return atlas, ref, state, W


# ---- 1. first integrate equals the window -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", FIRST_GRIDS)
def test_after_one_integrate_the_atlas_scores_as_the_window_does(gvom, grid):
    g = rr.build_map(gvom.Gvom, grid, 2, voxel_statistics=False)
    assert g.get_tuning("voxel_atlas_alignments") == 1
    atlas, ref, state, W = _fixed_atlas(g, gvom, grid)
    assert (grid == "far") == all(abs(e) >= 1 << 24 for e in ref.E)
    cases = [("candidates", ar.cloud_of(grid), ar.candidates(grid), (None,))]
    if grid in ar.EDGE_GRIDS:
        cases.append(("edges", ar.edge_cloud(grid, np.asarray(W, np.float64))[0], ar.edge_candidates(grid, np.asarray(W, np.float64)), (None, 0)))
    try:
        for name, cloud, M, knobs in cases:
            for knob in knobs:
                if knob is not None:
                    g.set_tuning("fastdiv", knob)                          # k_align_score<false>: the IEEE divide
                for dilate in (0, 1):
                    what = "%s %s dilate %d fastdiv %r" % (grid, name, dilate, knob)
                    with g.score_alignments(cloud, M, dilate=dilate) as w:
                        want = w.copy_to_host()
                    counts, best = _hold(atlas.score_alignments(cloud, M, dilate=dilate), want, what, W)      # NULL origin: the last integrated window
                    assert (counts[:, 1:].sum(axis=1) == len(cloud)).all() and best[2] == len(cloud) and best[3] == len(M), what
                    if name == "candidates" and knob is None and grid in ("np2", "r37"):      # and the referee, so that the two cannot be wrong together
                        _hold(atlas.score_alignments(cloud, M, dilate=dilate, origin_voxels=np.array(W)), vaa.score(ref, W, grid, cloud, M, dilate), what + ", referee", W)
    finally:
        g.set_tuning("fastdiv", -1)
    atlas.release()


# ---- 2. every voxel of the class grid -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", PLANTED_GRIDS)
def test_every_voxel_of_the_class_grid_is_held_to_the_referee_at_three_origins(gvom, grid):
    _, _, xy, zs = ar.GRIDS[grid]
    g = ar.planted_map(gvom.Gvom, grid, 2, voxel_statistics=False)
    atlas, ref, state, W = _fixed_atlas(g, gvom, grid)
    ar.planted_census_holds(state, grid)
    E, A, Z = ref.E, ref.A, ref.Z
    origins = [W, tuple(W[k] + SHIFT[k] for k in range(3)), (E[0] + A - xy + 9, E[1] - 6, W[2] + 2)]
    outside = [xy * xy * zs - (0 if ref._overlap(B, (xy, xy, zs)) is None else ref.cls[ref._overlap(B, (xy, xy, zs))[1]].size) for B in origins]
    assert outside[0] == 0 and outside[1] > 0 and outside[2] > 0, outside   # part of either displaced box lies outside the extent
    seen = np.zeros(5, np.int64)
    for B in origins:
        probes = ar.line_probes(grid, np.asarray(B, np.float64))
        for dilate in (0, 1):
            cls = vaa.box_classes(ref, B, dilate)
            for axis, (cloud, M) in enumerate(probes):
                what = "%s box %r dilate %d, lines along axis %d" % (grid, B, dilate, axis)
                want = ar.score(None, B, grid, cloud, M, dilate, cls=cls)
                counts, _ = _hold(atlas.score_alignments(cloud, M, dilate=dilate, origin_voxels=np.array(B)), want, what, B)
                hist = np.bincount(cls.ravel(), minlength=5)
                assert counts[:, 1:].astype(np.int64).sum(axis=0).tolist() == hist.tolist(), what        # every box voxel once
                seen += hist
    assert (seen[:4] > 0).all(), seen
    atlas.release()


# ---- 3. remembered space ------------------------------------------------------------------------------------------------------------------------
def _drive(gvom, ring, follow, each=None):
    """the climbing drive on a fresh mapper and atlas, the referee beside it; each(k, g, atlas, ref, W) after every integrate"""
    g = gvom.Gvom(*(va.DRIVE_PARAMS + (ring,) + va.DRIVE_TAIL), voxel_statistics=False)
    kw = dict(follow=True) if follow else dict(follow=False, origin_voxels=np.array(va.fixed_origin()))
    atlas = g.create_voxel_atlas(va.DRIVE_A, va.DRIVE_Z, **kw)
    ref = va.VoxelAtlasRef(va.DRIVE_A, va.DRIVE_Z, va.DRIVE_XY, va.DRIVE_ZS, follow=follow, origin=(0, 0, 0) if follow else va.fixed_origin())
    Ws = []
    for k, (pc, ego) in enumerate(va.drive_scans()):
        g.process_pointcloud(pc, ego)
        g.combine_maps()
        state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
        W = tuple(int(v) for v in origin)
        Ws.append(W)
        assert atlas.integrate() is True
        ref.integrate(state, W)
        assert atlas.extent_origin == ref.E
        if each:
            each(k, g, atlas, ref, W)
    return g, atlas, ref, tuple(Ws), state


@pytest.fixture(scope="module")
def driven(gvom):
    """per ring length, made on demand and kept: the following atlas after the drive -- (mapper, atlas, referee, window origins, last state)"""
    made = {}

    def get(ring):
        if ring not in made:
            made[ring] = _drive(gvom, ring, True)
        return made[ring]
    yield get
    made.clear()


def _probe(atlas, ref, B, what):
    """the three line probes of the box at B, dilate 0 and 1, against the referee; returns the box's class histogram under dilate 1"""
    probes = ar.line_probes(vaa.GRID, np.asarray(B, np.float64))
    for dilate in (0, 1):
        cls = vaa.box_classes(ref, B, dilate)
        hist = np.bincount(cls.ravel(), minlength=5)
        for axis, (cloud, M) in enumerate(probes):
            want = ar.score(None, B, vaa.GRID, cloud, M, dilate, cls=cls)
            counts, _ = _hold(atlas.score_alignments(cloud, M, dilate=dilate, origin_voxels=np.array(B)), want, "%s dilate %d axis %d" % (what, dilate, axis), B)
            assert counts[:, 1:].astype(np.int64).sum(axis=0).tolist() == hist.tolist(), (what, dilate, axis)
    return hist


@pytest.mark.parametrize("ring", [1, 2])
def test_the_true_pose_wins_on_remembered_space(gvom, driven, ring):
    g, atlas, ref, Ws, state = driven(ring)
    scans = va.drive_scans()
    W = Ws[-1]
    dev = _Device()
    try:
        for k in vaa.SCANS:
            pc, ego = scans[k]
            cloud = np.ascontiguousarray(pc, np.float32)
            M = vaa.drive_candidates(gvom, ego)
            for dilate in (0, 1):
                what = "ring %d scan %d dilate %d" % (ring, k, dilate)
                want = vaa.score(ref, Ws[k], vaa.GRID, cloud, M, dilate)
                counts, best = _hold(atlas.score_alignments(cloud, M, dilate=dilate, origin_voxels=np.array(Ws[k])), want, what, Ws[k])
                assert best[0] == vaa.BEST, (what, best)
                if k == 8:                                                  # host and device routes are equal
                    d = atlas.score_alignments_device(dev.upload(cloud), len(cloud), dev.upload(M[:, :3, :]), len(M), dilate=dilate, origin_voxels=np.array(Ws[k]))
                    _hold(d, want, what + ", device", Ws[k])
                if k in (8, 10):                                            # the window sees nothing of it: held to its referee and to the census
                    with g.score_alignments(cloud, M, dilate=dilate) as w:
                        wcounts, wbest = w.copy_to_host()
                    want_w = ar.score(state, W, vaa.GRID, cloud, M, dilate)
                    assert np.array_equal(wcounts, want_w[0]) and wbest.tolist() == want_w[1].tolist(), what
                    vaa.window_sees_nothing(k, dilate, wcounts, wbest, len(cloud))
                if k == 16:                                                 # the centre route at the final ego is origin_voxels = W
                    assert Ws[k] == W
                    _hold(atlas.score_alignments(cloud, M, dilate=dilate, center=ego), want, what + ", by centre", W)
                    _hold(atlas.score_alignments(cloud, M, dilate=dilate), want, what + ", NULL origin", W)
    finally:
        dev.free()


@pytest.mark.parametrize("ring", [1, 2])
def test_the_six_boxes_of_the_halo_census_under_line_probes(gvom, driven, ring):
    g, atlas, ref, Ws, _ = driven(ring)
    for name, B in vaa.drive_boxes(ref, Ws):
        hist = _probe(atlas, ref, B, "ring %d, %s %r" % (ring, name, B))
        halo = vaa.halo_only(ref, B)
        print(ring, name, B, "classes", hist.tolist(), "halo-only", halo)
        if name == "wholly outside":
            assert hist.tolist() == [0, 0, 0, ref.xy * ref.xy * ref.zs, 0]
        else:
            assert hist[ar.OCCUPIED] > 0 and hist[ar.NEAR] > 0 and halo > 0, (name, hist, halo)


@pytest.mark.parametrize("ring", [1, 2])
def test_the_fixed_drive_probed_after_every_integrate(gvom, ring):
    outside = []

    def each(k, g, atlas, ref, W):
        _probe(atlas, ref, W, "ring %d fixed, integrate %d" % (ring, k))
        outside.append(ref.last["outside"])
    g, atlas, ref, Ws, _ = _drive(gvom, ring, False, each)
    assert min(outside) == 0 and max(outside) > va.DRIVE_XY ** 2 * va.DRIVE_ZS // 2 and len(set(outside)) > 4, outside  # inside the extent, and mostly outside it
    atlas.release()


# ---- 4. box independence ------------------------------------------------------------------------------------------------------------------------
def test_two_boxes_give_a_world_voxel_the_same_class(gvom, driven):
    g, atlas, ref, Ws, _ = driven(1)
    B1 = Ws[-1]
    B2 = tuple(B1[k] + (17, -5, 3)[k] for k in range(3))
    pc, ego = va.drive_scans()[16]
    M = vaa.drive_candidates(gvom, ego)
    cloud = np.ascontiguousarray(pc, np.float32)
    w = ar.world(cloud, M)
    both = ar.voxels(w, vaa.GRID, B1)[1] & ar.voxels(w, vaa.GRID, B2)[1]
    cloud = np.ascontiguousarray(cloud[both.all(axis=0)])                  # the returns that every candidate puts into the intersection
    assert len(cloud) >= 64, len(cloud)
    for dilate in (0, 1):
        want = vaa.score(ref, B1, vaa.GRID, cloud, M, dilate)
        assert np.array_equal(want[0], vaa.score(ref, B2, vaa.GRID, cloud, M, dilate)[0]) and (want[0][:, 5] == 0).all()
        one, _ = _hold(atlas.score_alignments(cloud, M, dilate=dilate, origin_voxels=np.array(B1)), want, "box 1 dilate %d" % dilate, B1)
        two, _ = _hold(atlas.score_alignments(cloud, M, dilate=dilate, origin_voxels=np.array(B2)), want, "box 2 dilate %d" % dilate, B2)
        assert np.array_equal(one, two)
        print("dilate", dilate, len(cloud), "returns, totals", ar.totals(one))
        assert len(np.unique(one[:, 1:], axis=0)) > 1


# ---- 5. cycle and housekeeping ------------------------------------------------------------------------------------------------------------------
def test_a_scan_and_a_combine_between_integrate_and_query_change_nothing(gvom):
    grid = "np2"
    g = rr.build_map(gvom.Gvom, grid, 2, voxel_statistics=False)
    atlas, ref, state, W = _fixed_atlas(g, gvom, grid)
    cloud, M = ar.cloud_of(grid), ar.candidates(grid)
    before = {d: _hold(atlas.score_alignments(cloud, M, dilate=d), vaa.score(ref, W, grid, cloud, M, d), "before, dilate %d" % d, W) for d in (0, 1)}
    held = atlas.score_alignments(cloud, M, dilate=1)
    g.process_pointcloud(rr.cloud_of(grid, 1), rr.ego_of(grid, rr.N_SCANS))
    for d in (0, 1):
        _hold(atlas.score_alignments(cloud, M, dilate=d), before[d], "after a scan, dilate %d" % d, W)
    g.combine_maps()
    now = tuple(int(v) for v in g.read_dense(gvom.GVOM_WHICH_FUSED)[4])
    assert now != W
    for d in (0, 1):                                                        # the window moved on; the atlas and its last integrated window did not
        _hold(atlas.score_alignments(cloud, M, dilate=d), before[d], "after a combine, dilate %d" % d, W)
    _hold(held, before[1], "the held snapshot", W)
    counts_before = atlas.counts()
    atlas.score_alignments(cloud, M, dilate=1).release()
    assert atlas.counts() == counts_before                                  # read-only on the atlas
    atlas.release()


def test_the_pool_allocations_clear_and_refusals(gvom):
    grid = "tall"
    cloud, M = ar.cloud_of(grid), np.ascontiguousarray(ar.candidates(grid)[:, :3, :])
    fresh = gvom.Gvom(*rr.params(grid, 1), voxel_statistics=False)
    pid, out3 = ctypes.c_int64(-1), (ctypes.c_int64 * 3)()
    w5 = (ctypes.c_int32 * 5)(2, 1, -1, 0, 0)
    cp, tp = cloud.ctypes.data_as(ctypes.c_void_p), M.ctypes.data_as(ctypes.c_void_p)

    def raw(h, c=cp, n=len(cloud), t=tp, K=len(M), dilate=0, w=w5, org=None, out=pid):
        return h._lib.gvom_voxel_atlas_score_alignments(h._h, c, n, t, K, 0, dilate, w, org, out3, ctypes.byref(out) if out is not None else None)
    err = lambda h: h._lib.gvom_last_error(h._h).decode()
    assert raw(fresh) == GVOM_ERR_INVALID and "no voxel atlas" in err(fresh)                    # no atlas configured
    a0 = fresh.create_voxel_atlas(64, 32)
    assert a0.score_alignments(cloud, M) is None                                                # before the first combine
    assert a0.score_alignments(cloud, M, origin_voxels=np.array([0, 0, 0])) is None
    fresh.process_pointcloud(cloud, rr.ego_of(grid, 0))
    fresh.combine_maps()
    assert a0.score_alignments(cloud, M) is None                                                # a NULL origin before the first integrate
    with a0.score_alignments(cloud, M, origin_voxels=np.array([0, 0, 0])) as r:                 # an origin of its own: nothing is known yet
        counts, _ = r.copy_to_host()
        assert (counts[:, 1:4] == 0).all() and (counts[:, 4] + counts[:, 5] == len(cloud)).all()
    sharded = gvom.Gvom(*rr.params(grid, 1), voxel_statistics=False, _shard=(0, 1))
    assert raw(sharded) == GVOM_ERR_INVALID and "sharded" in err(sharded)

    g = rr.build_map(gvom.Gvom, grid, 1, voxel_statistics=False)
    atlas, ref, state, W = _fixed_atlas(g, gvom, grid)
    assert raw(g) == 0 and pid.value >= 0 and tuple(out3) == W
    for kw, rc, word in ((dict(dilate=2), GVOM_ERR_INVALID, "dilate"), (dict(dilate=-1), GVOM_ERR_INVALID, "dilate"),
                         (dict(w=(ctypes.c_int32 * 5)(0, 1025, 0, 0, 0)), GVOM_ERR_INVALID, "weight"), (dict(w=(ctypes.c_int32 * 5)(0, 0, 0, 0, -1025)), GVOM_ERR_INVALID, "weight"),
                         (dict(n=0), GVOM_ERR_INVALID, "n must be"), (dict(K=0), GVOM_ERR_INVALID, "K must be"), (dict(c=None), GVOM_ERR_INVALID, "NULL"),
                         (dict(t=None), GVOM_ERR_INVALID, "NULL"), (dict(w=None), GVOM_ERR_INVALID, "NULL"), (dict(n=(1 << 20) + 1, K=1), GVOM_ERR_CAPACITY, "2\\^20"),
                         (dict(K=65537, n=1), GVOM_ERR_CAPACITY, "65536"), (dict(n=1 << 20, K=4097), GVOM_ERR_CAPACITY, "2\\^32")):
        assert raw(g, **kw) == rc, kw
        assert pid.value == -1, kw
        assert re.search(word, err(g)) and "gvom_voxel_atlas_score_alignments" in err(g), (kw, err(g))
    assert raw(g, out=None) == GVOM_ERR_INVALID                                                 # NULL product_id
    for bad in (dict(origin_voxels=np.array([0.5, 0, 0])), dict(origin_voxels=np.array([0, 0])), dict(origin_voxels=np.array(W), center=(0, 0, 0)), dict(center=(0, np.inf, 0))):
        with pytest.raises(ValueError):
            atlas.score_alignments(cloud, M, **bad)
    with pytest.raises(gvom.GvomBackendError, match="unknown product kind"):
        g._device_product(gvom.PRODUCT_VOXEL_ATLAS_ALIGNMENT)
    with pytest.raises(gvom.GvomBackendError, match="unknown product kind"):
        g._device_product(37)

    # the pool: released sets are reused, four can be held, nothing is allocated in steady state
    want = vaa.score(ref, W, grid, cloud, M, 1)
    call = lambda: atlas.score_alignments(cloud, M, dilate=1)
    with call() as r:
        ptr = r.counts.ptr
        _hold(r, want, "first", W)
    va_allocs, al_allocs, grid_bytes = g.get_tuning("voxel_atlas_allocations"), g.get_tuning("alignment_allocations"), g.get_tuning("alignment_grid_bytes")
    assert al_allocs == 1 and grid_bytes > 0                                                    # the class grid alone: sets and staging count with the atlas
    for _ in range(3):
        with call() as r:
            assert r.counts.ptr == ptr
            _hold(r, want, "reused set", W)
    with g.score_alignments(cloud, M, dilate=1) as w:                                           # the window call shares the class grid and rebuilds it
        _hold(atlas.score_alignments(cloud, M, dilate=1), w.copy_to_host(), "after the window call", W)
    al_allocs = g.get_tuning("alignment_allocations")
    hold4 = [call() for _ in range(4)]
    assert len({r.counts.ptr for r in hold4}) == 4
    with pytest.raises(gvom.GvomBackendError, match="all 4 device product sets of this kind"):
        call()
    for r in hold4:
        _hold(r, want, "one of four", W)
    va_allocs = g.get_tuning("voxel_atlas_allocations")
    for _ in range(3):
        with call() as r:
            _hold(r, want, "steady state", W)
        with g.score_alignments(cloud, M, dilate=1):
            pass
    assert g.get_tuning("voxel_atlas_allocations") == va_allocs and g.get_tuning("alignment_allocations") == al_allocs
    assert g.get_tuning("alignment_grid_bytes") == grid_bytes

    # clear(): every pair inside the box is UNKNOWN
    atlas.clear()
    for dilate in (0, 1):
        with atlas.score_alignments(cloud, M, dilate=dilate) as r:
            counts, best = r.copy_to_host()
        assert (counts[:, 1:4] == 0).all() and np.array_equal(counts[:, 5], want[0][:, 5]) and np.array_equal(counts[:, 4], len(cloud) - want[0][:, 5])
        assert best.tolist() == [0, 0, len(cloud), len(M)]
    atlas.release()
    assert raw(g) == GVOM_ERR_INVALID and "no voxel atlas" in err(g)
