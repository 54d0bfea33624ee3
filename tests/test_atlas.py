"""The map atlas on the GPU (gvom_atlas_configure / _integrate / _recall / _extent / _clear / _counts: k_atlas_fill, k_atlas_move,
k_atlas_merge, k_atlas_recall; Gvom.create_atlas and the Atlas it returns) against the referee of tests/atlas_ref.py with tolerance 0
-- everything is copied or counted; f64 maps are compared through their int64 bit patterns.  Synthetic nine-map sets on windows of
16, 33 and 64 cells in atlases of 64 and 128, following and fixed, through host and device pointers; a drive out of the window and
back through combine_maps_device() on rings of one and two slots; a recalled set under clearance, cost-to-go, frontiers and attitude
scoring; the pool, the errors, an atlas of 4096 cells, and a torch consumer in a child process.  tests/test_atlas_cpu.py holds the
census of every input."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import atlas_ref as ar
import attitude_ref as att

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_NAMES = ("written", "kept", "uninformative", "outside", "cleared", "cleared_known", "known", "seq")


def _params(xy, res=0.4, buffer_size=1):
    return (res, 0.2, xy, 8, buffer_size, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)


@pytest.fixture(scope="module")
def gvom():
    import gvom as mod
    rc, info = mod.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    assert (mod.PRODUCT_ATLAS_RECALL, mod.PRODUCT_ATLAS_EXTENT) == (22, 24)
    return mod


@pytest.fixture(scope="module")
def handles(gvom):
    return {xy: gvom.Gvom(*_params(xy), voxel_statistics=False) for xy in (16, 33, 64)}


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


def _same(got, want, what):
    """a binding's [x, y] map against a referee's [y][x] map: int32 as it is, f64 through the bit patterns"""
    assert got.flags.f_contiguous and got.shape == want.shape[::-1], what
    g = got.T if got.dtype == np.int32 else np.ascontiguousarray(got.T).view(np.int64)
    assert g.dtype == want.dtype, (what, g.dtype, want.dtype)
    if not np.array_equal(g, want):
        bad = np.argwhere(g != want)
        raise AssertionError("%s: %d cells differ, first (x %d, y %d): got %r, referee %r" % (
            what, len(bad), bad[0][1], bad[0][0], g[tuple(bad[0])], want[tuple(bad[0])]))


def _hold_recall(gvom, m, want, origin, res, what):
    """a recalled DeviceMaps against the referee's recall: nine maps, stamps, counts, origins"""
    maps, stamp, counts = want
    with m:
        assert m.origin_cells[:2] == tuple(origin) and np.array_equal(m.origin[:2], np.array(origin, np.float64) * res), what
        host = [getattr(m, name).copy_to_host() for name in gvom.DEVICE_MAP_NAMES]
        for k, name in enumerate(gvom.DEVICE_MAP_NAMES):
            assert host[k].dtype == (np.int32 if k < 3 else np.float64), what
            _same(host[k], maps[k], "%s, %s" % (what, name))
        assert m.stamps.dtype == np.int32 and m.stamps.strides == (1, stamp.shape[0]), what
        _same(m.stamps.copy_to_host(), stamp, what + ", stamps")
        got = m.recall_counts.copy_to_host()
        assert got.dtype == np.int32 and np.array_equal(got, counts), (what, got, counts)
        m.stamps.release()
    return host


def _hold_extent(e, want, what):
    parts, E = want
    with e:
        assert e.origin_cells == tuple(E), (what, e.origin_cells, E)
        got = e.copy_to_host()
        assert [a.dtype for a in got] == [np.int32, np.int32, np.int32, np.float64, np.float64, np.int32], what
        for k, name in enumerate(("positive", "negative", "visibility", "roughness", "height", "stamp")):
            assert getattr(e, ("height_map" if name == "height" else name)).strides == (1, parts[k].shape[0]), what
            _same(got[k], parts[k], "%s, extent %s" % (what, name))


def _counts(a, ref, what):
    got, want = a.counts(), ref.counts()
    assert tuple(got) == COUNT_NAMES and got == want, (what, got, want)
    assert a.seq == ref.seq and tuple(a.extent_origin) == ref.E, (what, a.extent_origin, ref.E)


@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("follow", [True, False])
@pytest.mark.parametrize("xy,A", ar.SCENARIOS)
def test_synthetic_sets_match_the_referee_exactly(gvom, handles, xy, A, follow, route):
    """12 integrates along the scenario's walk; after each: the counters, four recalls (the current origin, the first, half outside
    the extent, wholly outside it) and the extent export"""
    g, dev = handles[xy], _Device()
    e0 = (0, 0) if follow else ar.fixed_origin(xy, A)
    a = g.create_atlas(A, follow=follow, origin_cells=None if follow else e0)
    ref = ar.AtlasRef(A, xy, follow, e0)
    origins, sets = ar.walk(xy, A), ar.scenario_sets(xy, A)
    allocs = None
    try:
        for k in range(ar.N_INTEGRATES):
            what = "xy %d, A %d, %s, %s, integrate %d" % (xy, A, "follow" if follow else "fixed", route, k)
            if route == "host":
                a.integrate_of([m.T for m in sets[k]], origins[k])             # [x, y] views of the [y][x] maps
            else:
                a.integrate_of_device([dev.upload(m) for m in sets[k]], origins[k])
            ref.integrate(sets[k], origins[k])
            _counts(a, ref, what)
            for r in ar.recall_origins(xy, A, ref, origins, k):
                _hold_recall(gvom, a.recall(origin_cells=r), ref.recall(r), r, g.xy_resolution, "%s, recall at %r" % (what, (r,)))
            _hold_extent(a.extent_device(), ref.extent(), what)
            if k == 1:
                allocs = (g.get_tuning("atlas_allocations"), g.get_tuning("device_map_sets"), g.get_tuning("device_product_sets"))
            dev.free()
        assert (g.get_tuning("atlas_allocations"), g.get_tuning("device_map_sets"), g.get_tuning("device_product_sets")) == allocs
        census = dict(ref.census)
        if not follow:
            census["cleared_known"] = 1                             # (a fixed extent never moves: nothing to clear)
        assert ar.census_ok(census), census
    finally:
        dev.free()


def _drive(gvom, ring):
    """the drive of tests/atlas_ref.py through a mapper and its atlas, the referee fed with the host copies of the same sets"""
    g = gvom.Gvom(*_params(ar.DRIVE_XY, ar.DRIVE_RES, ring), voxel_statistics=False)
    a = g.create_atlas(ar.DRIVE_A)
    ref = ar.AtlasRef(ar.DRIVE_A, ar.DRIVE_XY)
    first = live = None
    for k, (pc, ego) in enumerate(ar.drive_scans()):
        g.process_pointcloud(pc, ego)
        m = g.combine_maps_device()                                 # combine, integrate, recall: enqueued behind one another, no host wait
        a.integrate(m)
        rec = a.recall()
        centred = a.recall(center=ego[:2])
        org = m.origin_cells[:2]
        assert np.array_equal(np.array(m.origin_cells, np.float64) * (ar.DRIVE_RES, ar.DRIVE_RES, ar.DRIVE_ZRES), m.origin)
        assert centred.origin_cells[:2] == org and rec.origin_cells == m.origin_cells      # the scan's own arithmetic; z is the set's
        centred.release()
        live = [getattr(m, name).copy_to_host() for name in gvom.DEVICE_MAP_NAMES]
        m.release()
        first = first or org
        ref.integrate([x.T for x in live], org)
        what = "ring %d, scan %d" % (ring, k)
        _hold_recall(gvom, rec, ref.recall(), org, ar.DRIVE_RES, what)
        _counts(a, ref, what)
        if k % 4 == 0:
            _hold_recall(gvom, a.recall(origin_cells=first), ref.recall(first), first, ar.DRIVE_RES, what + ", at the first origin")
    return g, a, ref, first, live


@pytest.mark.parametrize("ring", [1, 2])
def test_drive_out_and_back_end_to_end(gvom, ring):
    g, a, ref, first, live = _drive(gvom, ring)
    assert ref.last_origin == first                                 # the drive ends where it began
    want = ref.recall(first)
    back = _hold_recall(gvom, a.recall(origin_cells=first), want, first, ar.DRIVE_RES, "ring %d, after the return leg" % ring)
    remembered = (back[2] > 0) & (live[2] <= 0)
    print("ring", ring, "observed cells: atlas", int((back[2] > 0).sum()), "live", int((live[2] > 0).sum()), "only the atlas", int(remembered.sum()))
    assert remembered.sum() > 100 and not np.array_equal(back[4], live[4])     # ground the live combine no longer has
    _hold_extent(a.extent_device(), ref.extent(), "ring %d" % ring)
    assert ar.census_ok(ref.census), ref.census


def test_a_recalled_set_is_a_map_set(gvom):
    """clearance, cost-to-go, frontiers and attitude scoring of a recalled set equal the same calls on its host copies; export,
    release and copy_to_host work on it"""
    g, a, ref, first, _ = _drive(gvom, 1)
    res, xy = g.xy_resolution, g.xy_size
    m = a.recall(origin_cells=first)
    host = [getattr(m, name).copy_to_host() for name in gvom.DEVICE_MAP_NAMES]
    pos, neg, vis, rough, height, inferred = host[:6]
    assert (vis > 0).sum() > 500 and m.positive.ptr and m.positive.ptr != m.negative.ptr
    # clearance
    for kw in (dict(), dict(density_threshold=10, include_negative=False, max_distance=3.0)):
        c0, c1 = m.clearance(**kw), g.clearance_of(pos, neg, **kw)
        for x, y in zip(c0.copy_to_host(), c1.copy_to_host()):
            assert np.array_equal(x, y)
    # cost to go: the set's field, then the same solve on the field's own cost map
    goals = np.argwhere(vis > 0)[::97][:5].astype(np.int32)
    f0 = m.cost_to_go(goals, goals_in_cells=True, inflation_radius=0.5, soft_weight=2, unknown=5)
    cost, direction, cell_cost = f0.copy_to_host()
    f1 = g.cost_to_go_of(cell_cost, goals)
    assert f0.reached > 500 and f0.converged and f1.converged and (f0.reached, f0.goals_seeded) == (f1.reached, f1.goals_seeded)
    for x, y in zip((cost, direction, cell_cost), f1.copy_to_host()):
        assert np.array_equal(x, y)
    # frontiers of the field over the recalled set's visibility
    fr0, fr1 = f0.frontiers(m, min_cells=2, max_clusters=256), g.frontiers_of(cell_cost, vis, cost, min_cells=2, max_clusters=256)
    assert fr0.n_clusters >= 1 and (fr0.n_clusters, fr0.frontier_cells, fr0.dropped) == (fr1.n_clusters, fr1.frontier_cells, fr1.dropped)
    for x, y in zip(fr0.copy_to_host(), fr1.copy_to_host()):
        assert np.array_equal(x, y)
    # attitude
    g.set_footprint(gvom.rectangle_footprint(0.9, 0.5, 0.45, res, headings=16, margin=0.1))
    g.set_chassis(gvom.chassis(0.7, -0.3, 0.8, 0.3))
    rng = np.random.default_rng(3)
    poses = np.empty((40, 12, 3), np.float32)
    poses[..., 0] = first[0] * res + rng.uniform(2, xy * res - 2, (40, 12))
    poses[..., 1] = first[1] * res + rng.uniform(2, xy * res - 2, (40, 12))
    poses[..., 2] = rng.uniform(-3.2, 3.2, (40, 12))
    for use in (True, False):
        s0 = m.score_attitude(poses, inferred_ground=use)
        s1 = g.score_attitude_of(att.ground_of(height, inferred, use), poses, origin=m.origin)
        got, want = s0.copy_to_host(), s1.copy_to_host()
        for x, y in zip(got, want):
            assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f")
    assert (got[2] == att.OK).any()
    # the set is held while `m` lives, and goes back to the pool afterwards
    sets = g.get_tuning("device_map_sets")
    ptr = m.positive.ptr
    other = a.recall(origin_cells=first)
    assert other.positive.ptr != ptr and other.set_id != m.set_id
    other.release()
    m.release()
    assert np.array_equal(m.positive.copy_to_host(), pos)           # released, not yet reused: the id lives until the next recall
    a.recall().release()
    a.recall().release()
    with pytest.raises(gvom.GvomBackendError, match="stale"):
        m.positive.copy_to_host()
    assert g.get_tuning("device_map_sets") <= sets + 1


def test_pool_capacity_and_no_allocation_in_steady_state(gvom, handles):
    g = handles[33]
    a = g.create_atlas(64)
    sets = ar.scenario_sets(33, 64)
    a.integrate_of([m.T for m in sets[0]], (4, -9))
    held = [a.recall() for _ in range(8)]
    assert g.get_tuning("device_map_sets") == 8 and len({m.set_id for m in held}) == 8
    with pytest.raises(gvom.GvomBackendError, match="all 8 device map sets"):
        a.recall()
    held.pop().release()
    a.recall().release()                                            # works after one release
    for m in held:
        m.release()
    a.recall().release()
    allocs = (g.get_tuning("atlas_allocations"), g.get_tuning("device_map_sets"), g.get_tuning("device_product_sets"))
    ref = ar.AtlasRef(64, 33)
    ref.integrate(sets[0], (4, -9))
    for k in range(50):
        o = (4 + 3 * k, -9 - 2 * k)
        a.integrate_of([m.T for m in sets[k % 12]], o)
        ref.integrate(sets[k % 12], o)
        m = a.recall()
        if k % 10 == 9:
            _hold_recall(gvom, m, ref.recall(), o, g.xy_resolution, "step %d" % k)
            _counts(a, ref, "step %d" % k)
        else:
            m.release()
    assert (g.get_tuning("atlas_allocations"), g.get_tuning("device_map_sets"), g.get_tuning("device_product_sets")) == allocs


def test_clear_reconfigure_and_errors(gvom, handles):
    g = handles[16]
    lib, h = g._lib, g._h
    sets = ar.scenario_sets(16, 64)
    a = g.create_atlas(64)
    assert g.get_tuning("atlas") == 64
    a.integrate_of([m.T for m in sets[0]], (0, 0))
    assert a.counts()["known"] > 0
    a.clear()
    ref = ar.AtlasRef(64, 16)
    ref.integrate(sets[0], (0, 0))
    ref.clear()
    _counts(a, ref, "after clear")
    _hold_recall(gvom, a.recall(), ref.recall(), (0, 0), g.xy_resolution, "after clear")
    a.integrate_of([m.T for m in sets[1]], (3, 3))
    ref.integrate(sets[1], (3, 3))
    _counts(a, ref, "after clear and one integrate")
    _hold_extent(a.extent_device(), ref.extent(), "after clear and one integrate")
    # a reconfiguration: another size, everything UNKNOWN, seq 0, the given corner
    b = g.create_atlas(128, follow=False, origin_cells=(-100, 7))
    ref = ar.AtlasRef(128, 16, False, (-100, 7))
    _counts(b, ref, "reconfigured")
    b.integrate_of([m.T for m in sets[2]], (-90, 10))
    ref.integrate(sets[2], (-90, 10))
    _counts(b, ref, "reconfigured, one integrate")
    _hold_extent(b.extent_device(), ref.extent(), "reconfigured, one integrate")
    # GVOM_ERR_INVALID, every case of the definition
    I64 = ctypes.c_int64
    sid, pid, org = I64(-1), I64(-1), (I64 * 2)(0, 0)
    ptrs = (ctypes.c_void_p * 9)(*[np.ascontiguousarray(m).ctypes.data for m in sets[0]])
    for cells in (63, 96, 32, 8192, 8):                            # not a power of two, outside the bounds, below xy_size
        assert lib.gvom_atlas_configure(h, cells, 0, None) == gvom.GVOM_ERR_INVALID, cells
    assert lib.gvom_atlas_configure(h, 64, 2, None) == gvom.GVOM_ERR_INVALID
    wide = gvom.Gvom(*_params(100), voxel_statistics=False)
    assert wide._lib.gvom_atlas_configure(wide._h, 64, 0, None) == gvom.GVOM_ERR_INVALID and b"xy_size" in wide._lib.gvom_last_error(wide._h)
    assert wide._lib.gvom_atlas_configure(wide._h, 128, 0, None) == 0
    assert g.get_tuning("atlas") == 128                             # a refused configuration leaves the atlas as it is
    assert lib.gvom_atlas_integrate(h, 5, ptrs, 0, org) == gvom.GVOM_ERR_INVALID          # id and pointers mixed
    assert lib.gvom_atlas_integrate(h, -1, None, 0, None) == gvom.GVOM_ERR_INVALID        # neither
    assert lib.gvom_atlas_integrate(h, -1, ptrs, 0, None) == gvom.GVOM_ERR_INVALID        # pointers without their origin
    assert lib.gvom_atlas_integrate(h, 1 << 40, None, 0, None) == gvom.GVOM_ERR_INVALID   # an id nobody has
    m = b.recall()
    stale = m.set_id
    m.release()
    b.recall().release()                                            # the set is recycled: its first id is stale
    assert lib.gvom_atlas_integrate(h, stale, None, 0, None) == gvom.GVOM_ERR_INVALID
    assert b"stale" in lib.gvom_last_error(h)
    assert lib.gvom_atlas_recall(h, org, None, ctypes.byref(pid), None) == gvom.GVOM_ERR_INVALID
    assert lib.gvom_atlas_recall(h, org, ctypes.byref(sid), None, None) == gvom.GVOM_ERR_INVALID
    assert lib.gvom_atlas_extent(h, None, None) == gvom.GVOM_ERR_INVALID
    assert lib.gvom_atlas_counts(h, None) == gvom.GVOM_ERR_INVALID
    _counts(b, ref, "after the refused calls")                     # none of them changed anything
    # no atlas configured
    b.release()
    assert g.get_tuning("atlas") == 0
    out = (I64 * 8)()
    assert lib.gvom_atlas_integrate(h, -1, ptrs, 0, org) == gvom.GVOM_ERR_INVALID
    assert lib.gvom_atlas_recall(h, org, ctypes.byref(sid), ctypes.byref(pid), None) == gvom.GVOM_ERR_INVALID
    assert lib.gvom_atlas_extent(h, ctypes.byref(pid), None) == gvom.GVOM_ERR_INVALID
    assert lib.gvom_atlas_clear(h) == gvom.GVOM_ERR_INVALID and lib.gvom_atlas_counts(h, out) == gvom.GVOM_ERR_INVALID
    assert b"no atlas is configured" in lib.gvom_last_error(h)
    with pytest.raises(ValueError):
        b.recall()
    # a sharded handle
    s = gvom.Gvom(*_params(64), voxel_statistics=False, _shard=(0, 2))
    assert s._lib.gvom_atlas_configure(s._h, 64, 0, None) == gvom.GVOM_ERR_INVALID and b"sharded" in s._lib.gvom_last_error(s._h)
    with pytest.raises(ValueError):
        s.create_atlas(64)


def test_an_atlas_of_4096_cells_integrates_one_set_and_recalls_it(gvom, handles):
    """one set into an empty atlas of 4096 cells (1 GiB), its window across the storage seam in x and in y.  What the referee would
    say follows from the definition without 4096 x 4096 arrays on the host: the merge counters and the recall at the set's origin
    are those of a referee of 128 cells (the window lies inside both extents), the move clears what the two extents do not share,
    and everything else is UNKNOWN"""
    g, A, xy = handles[64], 4096, 64
    a = g.create_atlas(A)
    try:
        small = ar.AtlasRef(128, xy)
        o = (-30, 4090)
        assert (o[0] & (A - 1)) + xy > A and (o[1] & (A - 1)) + xy > A
        s = ar.scenario_sets(64, 128)[0]
        a.integrate_of([m.T for m in s], o)
        small.integrate(s, o)
        E = (o[0] + xy // 2 - A // 2, o[1] + xy // 2 - A // 2)
        want = small.counts()
        want["cleared"], want["cleared_known"] = A * A - (A - abs(E[0])) * (A - abs(E[1])), 0       # the extent came from (0, 0)
        assert a.counts() == want and tuple(a.extent_origin) == E
        _hold_recall(gvom, a.recall(), small.recall(), o, g.xy_resolution, "4096")
        far = (E[0] + A - 10, o[1])                                 # ten columns inside the extent, nothing known there
        i, f, stamp = ar.unknown((xy, xy))
        _hold_recall(gvom, a.recall(origin_cells=far), (i + f, stamp, np.array([0, 0, (xy - 10) * xy, 1], np.int32)), far, g.xy_resolution, "4096, across the edge")
        with a.extent_device() as e:
            assert e.origin_cells == E and e.stamp.shape == (A, A) and e.stamp.strides == (1, A)
            stamps = np.zeros((A, A), np.int32)
            stamps[o[1] - E[1]:o[1] - E[1] + xy, o[0] - E[0]:o[0] - E[0] + xy] = small.recall()[1]
            _same(e.stamp.copy_to_host(), stamps, "4096, extent stamps")
    finally:
        a.release()                                                 # 1 GiB goes back


def test_consumer_reads_a_recalled_map_and_the_stamps_on_its_own_stream():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_atlas_torch.py"), "consumer_stream"], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0 and "CASE OK consumer_stream" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])
