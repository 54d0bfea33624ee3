"""Obstacle clearance on the GPU (gvom_clearance: k_clearance_rows + k_clearance_cols; DeviceMaps.clearance, Gvom.clearance_of,
Gvom.clearance_of_device) against the numpy referee of tests/clearance_ref.py: squared cells with tolerance 0, metres bit for
bit.  Synthetic maps on grids of 16 (less than a wave), 50 (xy % 4 != 0, partial tiles), 64 and 256 cells (several waves per
row, several strips and row tiles), the obstacle scenes end to end through combine_maps_device(), snapshots, the product pool,
errors, and a torch consumer in a child process.

From 300 cells on ("launch regimes" below): 300, 520, 1000, 1024, 2049 and 4096 cells against the row-wise and feature-transform
referees of tests/clearance_ref.py, with the launch shape of every call read back from the handle.  Wall time on the MI355X (pytest
--durations, one run): 0.28 / 1.43 / 0.67 / 1.22 / 3.04 / 9.09 s for the six sizes (the largest existing case, 256 cells, 0.25 s);
at 4096 five patterns run unbounded and under one cap each, of which the feature transform of the random map takes about 3 s.

Census of the scenes at the last combine, threshold 50 (one_round / ragged): 166 / 368 cells with 0 < positive <= 50,
387 / 493 with positive > 50, 5 / 1 with negative > 0 (tests/test_clearance_cpu.py holds the floors on the CPU referee)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import clearance_ref as cr
import obstacle_scenes as ob

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = {16: 0.4, 50: 0.15, 64: 0.4, 256: 0.1}


def _params(xy, res=0.4, buffer_size=1):
    return (res, 0.2, xy, 8, buffer_size, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)


@pytest.fixture(scope="module")
def gvom():
    import gvom as mod
    rc, info = mod.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    return mod


@pytest.fixture(scope="module")
def handles(gvom):
    return {xy: gvom.Gvom(*_params(xy, RES[xy]), voxel_statistics=False) for xy in RES}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _hold(c, want_d2, res, what):
    """a DeviceClearance against the referee's squared cells: exact, and the metres bit for bit (inf included)"""
    with c:
        dist, d2 = c.copy_to_host()
    xy = want_d2.shape[0]
    assert d2.dtype == np.int32 and dist.dtype == np.float32 and d2.shape == dist.shape == (xy, xy), what
    assert d2.flags.f_contiguous and dist.flags.f_contiguous, what
    if not np.array_equal(d2, want_d2):
        bad = np.argwhere(d2 != want_d2)
        raise AssertionError("%s: squared cells differ in %d cells, first (%d, %d): got %d, referee %d" % (
            what, len(bad), bad[0][0], bad[0][1], d2[tuple(bad[0])], want_d2[tuple(bad[0])]))
    want = cr.distance(want_d2, res)
    same = _bits(dist) == _bits(want)
    assert same.all(), "%s: %d distances differ in their bits, first d2 = %d: got %r, referee %r" % (
        what, int((~same).sum()), want_d2[~same][0], dist[~same][0], want[~same][0])
    return dist, d2


def _cap_metres(c, res):
    """a max_distance whose floor((d / res)^2) is exactly c"""
    d = float(np.sqrt(c + 0.5)) * res
    assert cr.max_cells2_of(d, res) == c
    return d


@pytest.mark.parametrize("xy", sorted(RES))
def test_synthetic_maps_match_the_referee_exactly(handles, xy):
    g, res = handles[xy], RES[xy]
    pats = cr.patterns(xy)
    assert ("boundary_same_row" in pats) == (xy > 64)
    for name, (pos, neg) in pats.items():
        for thr in ((49.5, 50) if name == "threshold_edge" else (50,)):
            mask = cr.obstacle_mask(pos, neg, thr)
            full = cr.separable(mask)
            for c in cr.CAPS:
                what = "xy %d, %s, threshold %r, cap %d" % (xy, name, thr, c)
                got = g.clearance_of(pos, neg, density_threshold=thr, max_distance=_cap_metres(c, res) if c else None)
                assert got.distance.shape == got.squared_cells.shape == (xy, xy) and got.distance.strides == (1, xy), what
                _hold(got, cr.cap(full, c), res, what)
    # the threshold pattern has cells on both sides of BOTH thresholds
    pos = pats["threshold_edge"][0]
    assert (pos == 49).any() and (pos == 50).any() and (pos == 51).any()
    assert cr.obstacle_mask(pos, None, 49.5).sum() > cr.obstacle_mask(pos, None, 50).sum() > 0


@pytest.mark.parametrize("xy", [50, 256])
def test_negative_obstacles_flag_memory_orders_and_inf(handles, xy):
    g, res = handles[xy], RES[xy]
    pos, neg = cr.patterns(xy)["negative_only"]
    with_neg = cr.separable(cr.obstacle_mask(pos, neg, 50))
    assert (with_neg == 0).sum() == (neg > 0).sum() > 0
    far = np.full((xy, xy), cr.FAR, np.int32)
    _hold(g.clearance_of(pos, neg), with_neg, res, "negative only")
    _hold(g.clearance_of(pos, neg, include_negative=False), far, res, "negative only, GVOM_CLEARANCE_NO_NEGATIVE")
    dist, _ = _hold(g.clearance_of(pos, None), far, res, "negative=None")
    assert np.isposinf(dist).all()
    _hold(g.clearance_of(pos, neg, max_distance=float("inf")), with_neg, res, "max_distance inf")
    # any memory order and integer type: Fortran order, a transposed view, int64
    for name, p, n in (("fortran", np.asfortranarray(pos), np.asfortranarray(neg)), ("int64", pos.astype(np.int64), neg.astype(np.int64)),
                       ("view", np.ascontiguousarray(pos.T).T, np.ascontiguousarray(neg.T).T)):
        _hold(g.clearance_of(p, n), with_neg, res, name)
    rnd = cr.patterns(xy)["random_1"][0]
    asym = cr.separable(cr.obstacle_mask(rnd, None, 50))
    assert not np.array_equal(asym, asym.T)                    # an [x, y] / [y, x] mix-up would show
    _hold(g.clearance_of(rnd), asym, res, "random_1, positive only")


# ---- launch regimes: maps of 300 to 4096 cells a side ---------------------------------------------------------------------------
# The four sizes above all launch k_clearance_cols with strips of 16 columns (lgw 4) and 16 rows per workgroup, and k_clearance_rows
# with at most 4 chunks per row: one trip of its loop per wave.  The sizes of cr.LARGE run the other strip widths (lgw 3, 5, 6: the
# LDS load indexing, the column stride, the row stride), 32 to 256 rows per workgroup with a ragged last row tile, dynamic LDS of
# exactly 65,536 bytes, and up to 64 chunks per row (the chunk loop's later trips, the search across up to 64 masks, chunk 63).
# Which regime a call ran is read back from the handle (gvom_get_tuning "clearance_lgw" ...: what gvom_launch_clearance used).
LARGE_RES = {300: 0.15, 520: 0.1, 1000: 0.4, 1024: 0.2, 2049: 0.25, 4096: 0.05}
SHAPE = ("clearance_lgw", "clearance_rows_per_tile", "clearance_lds_bytes", "clearance_chunks")
SEEN = {}                                                      # xy -> {(lgw, rows per tile, LDS bytes, chunks)} of the calls made so far


def _large_handle(gvom, xy):
    return gvom.Gvom(LARGE_RES[xy], 0.2, xy, 1, 1, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1, voxel_statistics=False)


def _shape(g):
    return tuple(g.get_tuning(n) for n in SHAPE)


def _hold_sample(c, mask, cap, cells, res, what):
    """_hold on the cells [k, 2] alone, against brute_force_near: for the random maps where the full-map referee is missing"""
    with c:
        dist, d2 = c.copy_to_host()
    want = cr.cap(cr.brute_force_near(mask, cells), cap)
    got, got_dist = d2[cells[:, 0], cells[:, 1]], dist[cells[:, 0], cells[:, 1]]
    assert np.array_equal(got, want), "%s: squared cells differ in %d of %d sampled cells" % (what, int((got != want).sum()), len(cells))
    assert np.array_equal(_bits(got_dist), _bits(cr.distance(want, res))), what


def _large_caps(xy, k):
    """the caps pattern number k runs: all five up to 1024 cells; beyond, unbounded and two (2049) or one (4096) of the capped
    ones in turn -- every cap still runs at every size"""
    caps = cr.large_caps(xy)
    if xy <= 1024:
        return caps
    return (0, caps[1 + k % 4]) + ((caps[1 + (k + 2) % 4],) if xy < 4096 else ())


@pytest.mark.parametrize("xy", cr.LARGE)
def test_large_maps_match_the_referee_exactly_in_every_launch_regime(gvom, xy):
    g, res = _large_handle(gvom, xy), LARGE_RES[xy]
    assert _shape(g) == (0, 0, 0, 0)
    seen, caps_run = SEEN.setdefault(xy, set()), set()
    pats = cr.large_patterns(xy, short=xy == 4096)
    assert {"corner_far", "corner_0n", "boundary_same_row", "boundary_adjacent_rows", "lonely", "random_0.1"} <= set(pats)
    for k, (name, pos) in enumerate(pats.items()):
        mask = cr.obstacle_mask(pos, None, 50)
        full = cr.large_referee(mask)
        assert full is not None or name.startswith("random")        # (None: no scipy here; only the random maps need it)
        pos = np.asfortranarray(pos)
        for c in _large_caps(xy, k):
            what = "xy %d, %s, cap %d" % (xy, name, c)
            got = g.clearance_of(pos, None, max_distance=_cap_metres(c, res) if c else None)
            shape = _shape(g)
            seen.add(shape)
            caps_run.add(c)
            lgw, rows, lds, chunks = shape
            assert 3 <= lgw <= 6 and rows % 16 == 0 and 16 <= rows <= 256 and 0 < lds <= 65536 and chunks == (xy + 63) // 64, (what, shape)
            if full is None or (xy == 300 and name == "random_0.1"):      # (at 300 both, so that this route is itself run everywhere)
                _hold_sample(g.clearance_of(pos, None, max_distance=_cap_metres(c, res) if c else None), mask, c, cr.boundary_sample(xy), res, what + ", sampled")
            if full is not None:
                _hold(got, cr.cap(full, c), res, what + ", launch %r" % (shape,))
            else:
                got.release()
    assert caps_run == set(cr.large_caps(xy))
    print(xy, sorted(seen))
    del g


def test_every_launch_regime_ran(gvom, handles):
    """lgw 3, 4, 5 and 6; 16, 32, 64, 128 and 256 rows per workgroup; dynamic LDS of exactly 65,536 bytes; 64 chunks per row:
    all of them seen through the getters.  A size the test above has not run in this process (a selection of tests) is launched
    here on an empty map, for the shapes alone."""
    pos = cr.patterns(256)["random_1"][0]
    handles[256].clearance_of(pos).release()
    shapes = {_shape(handles[256])}
    for xy in cr.LARGE:
        if xy not in SEEN:
            g = _large_handle(gvom, xy)
            empty = np.zeros((xy, xy), np.int32, order="F")
            for c in cr.large_caps(xy):
                g.clearance_of(empty, None, max_distance=_cap_metres(c, LARGE_RES[xy]) if c else None).release()
                SEEN.setdefault(xy, set()).add(_shape(g))
            del g
        shapes |= SEEN[xy]
    print(sorted(shapes))
    assert {s[0] for s in shapes} == {3, 4, 5, 6}, sorted(shapes)
    assert {s[1] for s in shapes} >= {16, 32, 64, 128, 256}, sorted(shapes)
    assert 65536 in {s[2] for s in shapes}, sorted(shapes)
    assert 64 in {s[3] for s in shapes} and max(s[3] for s in shapes) == 64, sorted(shapes)
    assert len({s[3] for s in shapes if s[3] > 4}) >= 5          # the chunk loop's second trip and beyond, at several widths


def _census_floors(pos, neg, what):
    soft, hard, negative = cr.census(pos, neg, cr.SCENE_THRESHOLD)
    assert soft >= cr.CENSUS_FLOOR and hard >= cr.CENSUS_FLOOR and negative >= 1, (what, soft, hard, negative)


@pytest.mark.parametrize("name", cr.SCENES)
def test_scenes_end_to_end_through_device_map_sets(gvom, name):
    """three scans, a device combine after each: the clearance of the set's own maps, unbounded and capped at 2 m; its zero
    cells are the non-zero cells of the node's hard-obstacle grid on an identical second mapper"""
    thr = cr.SCENE_THRESHOLD
    g, twin = (gvom.Gvom(*ob.params(name), voxel_statistics=False) for _ in range(2))
    res = g.xy_resolution
    for k, (pc, ego) in enumerate(ob.scans(name)):
        what = "%s combine %d" % (name, k)
        g.process_pointcloud(pc, ego)
        twin.process_pointcloud(pc, ego)
        m = g.combine_maps_device()
        c, capped = m.clearance(thr), m.clearance(thr, max_distance=2.0)
        pos, neg = m.positive.copy_to_host(), m.negative.copy_to_host()
        full = cr.separable(cr.obstacle_mask(pos, neg, thr))
        _, d2 = _hold(c, full, res, what)
        _hold(capped, cr.cap(full, cr.max_cells2_of(2.0, res)), res, what + ", capped")
        _hold(m.clearance(thr, include_negative=False), cr.separable(cr.obstacle_mask(pos, None, thr)), res, what + ", no negative")
        hard = np.reshape(twin.combine_maps_occupancy(thr)[1], (g.xy_size, g.xy_size), order="F")
        assert np.array_equal(d2 == 0, hard != 0), what
        assert (d2 == 0).sum() > 0 and (d2 > 0).sum() > 0
        m.release()
    _census_floors(pos, neg, name)


def test_device_pointers_equal_the_map_set_route(gvom):
    name = "one_round"
    g = gvom.Gvom(*ob.params(name), voxel_statistics=False)
    for pc, ego in ob.scans(name):
        g.process_pointcloud(pc, ego)
    with g.combine_maps_device() as m:
        a = m.clearance(cr.SCENE_THRESHOLD)
        b = g.clearance_of_device(m.positive.ptr, m.negative.ptr, cr.SCENE_THRESHOLD)
        c = g.clearance_of_device(m.positive.ptr, None, cr.SCENE_THRESHOLD, max_distance=1.0)
        pos, neg = m.positive.copy_to_host(), m.negative.copy_to_host()
        assert a.product_id != b.product_id and a.distance.ptr != b.distance.ptr
        want = _hold(a, cr.separable(cr.obstacle_mask(pos, neg, cr.SCENE_THRESHOLD)), g.xy_resolution, "map set")
        got = b.copy_to_host()
        assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1])
        _hold(c, cr.separable(cr.obstacle_mask(pos, None, cr.SCENE_THRESHOLD), cr.max_cells2_of(1.0, g.xy_resolution)),
              g.xy_resolution, "device pointers, no negative, capped")
        b.release()


def test_a_clearance_product_is_a_snapshot(gvom):
    name = "one_round"
    g = gvom.Gvom(*ob.params(name), voxel_statistics=False)
    scans = ob.scans(name)
    g.process_pointcloud(*scans[0])
    m = g.combine_maps_device()
    held = m.clearance(cr.SCENE_THRESHOLD)
    m.release()
    before = held.copy_to_host()
    for pc, ego in scans[1:]:
        g.process_pointcloud(pc, ego)
        m = g.combine_maps_device()
        later = m.clearance(cr.SCENE_THRESHOLD)
        assert later.distance.ptr != held.distance.ptr
        now = later.copy_to_host()
        later.release()
        m.release()
    after = held.copy_to_host()
    assert np.array_equal(_bits(before[0]), _bits(after[0])) and np.array_equal(before[1], after[1])
    assert not np.array_equal(now[1], after[1])                # the map has moved on; the held product has not


def test_pool_capacity_reuse_and_no_allocation_after_the_first_call(gvom):
    g = gvom.Gvom(*_params(64), voxel_statistics=False)
    pos = cr.patterns(64)["random_1"][0]
    want = cr.separable(cr.obstacle_mask(pos, None, 50))
    first = g.clearance_of(pos)
    assert g.get_tuning("clearance_allocations") == 3          # the product set, the row-pass scratch, the host staging buffer
    assert g.get_tuning("device_product_sets") == 1 and g.get_tuning("device_map_sets") == 0
    ptr = first.distance.ptr
    first.release()
    for _ in range(3):                                         # released: the set, the scratch and the staging buffer are reused
        with g.clearance_of(pos) as c:
            assert c.distance.ptr == ptr
            _hold(c, want, 0.4, "reused set")
    assert g.get_tuning("clearance_allocations") == 3 and g.get_tuning("device_product_sets") == 1
    held = [g.clearance_of(pos) for _ in range(4)]
    assert len({c.distance.ptr for c in held}) == 4 and g.get_tuning("device_product_sets") == 4
    pid = ctypes.c_int64(-1)
    p = np.asfortranarray(pos)
    rc = g._lib.gvom_clearance(g._h, -1, p.ctypes.data_as(ctypes.c_void_p), None, 0, 50.0, 0, 0, ctypes.byref(pid))
    assert rc == -4 and pid.value == -1                        # GVOM_ERR_CAPACITY
    with pytest.raises(gvom.GvomBackendError, match="all 4 device product sets of this kind"):
        g.clearance_of(pos)
    allocs = g.get_tuning("clearance_allocations")
    assert allocs == 6
    held[2].release()
    with g.clearance_of(pos) as c:
        _hold(c, want, 0.4, "after a release")
    assert g.get_tuning("device_product_sets") == 4 and g.get_tuning("clearance_allocations") == allocs
    assert g.get_tuning("device_map_sets") == 0
    for k in (0, 1, 3):                                        # (the set of held[2] has been handed out again: its id is stale)
        _hold(held[k], want, 0.4, "held")
    with pytest.raises(gvom.GvomBackendError, match="unknown or stale device product id"):
        held[2].copy_to_host()


def test_errors(gvom):
    name = "one_round"
    g = gvom.Gvom(*ob.params(name), voxel_statistics=False)
    xy = g.xy_size
    pos = np.zeros((xy, xy), np.int32, order="F")
    pp = pos.ctypes.data_as(ctypes.c_void_p)
    pid = ctypes.c_int64(-1)

    def raw(set_id, p, n, thr=50.0, cap=0, flags=0):
        return g._check(g._lib.gvom_clearance(g._h, set_id, p, n, 0, thr, cap, flags, ctypes.byref(pid)))
    with pytest.raises(gvom.GvomBackendError, match="unknown or stale device map set id"):
        raw(10 ** 9, None, None)
    with pytest.raises(gvom.GvomBackendError, match="not both"):
        raw(1, pp, None)
    with pytest.raises(gvom.GvomBackendError, match="a map set id or a positive map"):
        raw(-1, None, None)
    with pytest.raises(gvom.GvomBackendError, match="a map set id or a positive map"):
        raw(-1, None, pp)
    with pytest.raises(gvom.GvomBackendError, match="not a number"):
        raw(-1, pp, None, thr=float("nan"))
    with pytest.raises(gvom.GvomBackendError, match="unknown flag bits"):
        raw(-1, pp, None, flags=2)
    assert g._lib.gvom_clearance(g._h, -1, pp, None, 0, float("nan"), 0, 0, ctypes.byref(pid)) == gvom.GVOM_ERR_INVALID
    with pytest.raises(gvom.GvomBackendError, match="gvom_clearance"):
        g._device_product(gvom.PRODUCT_CLEARANCE)
    with pytest.raises(gvom.GvomBackendError, match="unknown product kind"):
        g._device_product(9)
    assert g.get_tuning("device_product_sets") == 0            # nothing above allocated a set
    scans = ob.scans(name)
    g.process_pointcloud(*scans[0])
    m = g.combine_maps_device()
    old = m.set_id
    m.clearance().release()
    m.release()
    g.process_pointcloud(*scans[1])
    g.combine_maps_device().release()                           # the unheld set was recycled: its id is stale
    with pytest.raises(gvom.GvomBackendError, match="unknown or stale device map set id"):
        raw(old, None, None)
    sharded = gvom.Gvom(*_params(64), voxel_statistics=False, _shard=(0, 2))
    with pytest.raises(gvom.GvomBackendError, match="sharded handles are not supported"):
        sharded.clearance_of(np.zeros((64, 64), np.int32))


def _torch_case(name):
    """One case per fresh child process that imports torch BEFORE the library is loaded (one HIP runtime in the process)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_clearance_torch.py"), name],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "CASE OK " + name in r.stdout, r.stdout[-4000:]


def test_dlpack_zero_copy_through_torch():
    _torch_case("zero_copy")


def test_consumer_reduces_on_its_own_stream_and_its_release_frees_the_set():
    _torch_case("consumer_stream")
