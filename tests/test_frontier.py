"""Frontier extraction on the GPU (gvom_frontiers: k_frontier_mark, k_frontier_relax, k_frontier_count, k_frontier_rank,
k_frontier_rows, k_frontier_stats; DeviceCostField.frontiers, Gvom.frontiers_of, Gvom.frontiers_of_device) against the referee of
tests/frontier_ref.py: the four parts and the call's info with tolerance 0 -- everything is integer.  Synthetic maps on grids of 16,
31, 32, 33, 64, 65, 100 and 129 cells, 1024 cells once, the obstacle scenes end to end through combine_maps_device() and
cost_to_go() on rings of one and two slots, snapshots, the product pool, errors, and a torch consumer in a child process.
tests/test_frontier_cpu.py holds the census of every input."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import costfield_ref as cf
import frontier_ref as fr
import obstacle_scenes as ob

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(xy, res=0.4, buffer_size=1):
    return (res, 0.2, xy, 8, buffer_size, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)


@pytest.fixture(scope="module")
def gvom():
    import gvom as mod
    rc, info = mod.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    assert mod.PRODUCT_FRONTIERS == 16
    return mod


@pytest.fixture(scope="module")
def handles(gvom):
    return {xy: gvom.Gvom(*_params(xy), voxel_statistics=False) for xy in fr.SIZES}


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


def _hold(f, want, what):
    """a DeviceFrontiers against the referee's product: the four parts and the info, exactly"""
    rows, sums, cmap, counts, info = want
    with f:
        got = f.copy_to_host()
        seen = (f.n_clusters, f.frontier_cells, f.dropped)
        rounds = f.rounds
    cap, xy = rows.shape[0], cmap.shape[0]
    assert [a.dtype for a in got] == [np.int32, np.int64, np.int32, np.int32], what
    assert got[0].shape == (cap, 8) and got[1].shape == (cap, 2) and got[2].shape == (xy, xy) and got[3].shape == (4,), what
    assert got[2].flags.f_contiguous, what
    print(what, "rounds", rounds, "counts", got[3].tolist())
    assert np.array_equal(got[3], counts), (what, got[3], counts)
    if not np.array_equal(got[2].T, cmap):
        bad = np.argwhere(got[2].T != cmap)
        raise AssertionError("%s: the cluster map differs in %d cells, first (x %d, y %d): got %d, referee %d" % (
            what, len(bad), bad[0][1], bad[0][0], got[2].T[tuple(bad[0])], cmap[tuple(bad[0])]))
    if not np.array_equal(got[0], rows):
        bad = np.argwhere((got[0] != rows).any(axis=1))[:, 0]
        raise AssertionError("%s: %d rows differ, first %d: got %r, referee %r" % (what, len(bad), bad[0], got[0][bad[0]], rows[bad[0]]))
    assert np.array_equal(got[1], sums), (what, np.argwhere(got[1] != sums)[:3])
    assert list(seen) == list(info), (what, seen, info)
    assert rounds >= 1, what
    return rounds


def _call(g, case, **kw):
    c, vis, D, mc, cap = case
    return g.frontiers_of(c.T, vis.T, None if D is None else D.T, min_cells=mc, max_clusters=cap, **kw)


@pytest.mark.parametrize("xy", fr.SIZES)
def test_synthetic_maps_match_the_referee_exactly(handles, xy):
    g = handles[xy]
    rounds = {}
    for name, case in fr.patterns(xy).items():
        f = _call(g, case)
        assert f.cluster_map.shape == (xy, xy) and f.cluster_map.strides == (1, xy) and f.clusters.shape == (case[4], 8), name
        rounds[name] = _hold(f, fr.expected(xy, name), "xy %d, %s" % (xy, name))
        assert g.get_tuning("frontier_rounds") == rounds[name]
    assert rounds["nothing_known"] == 1 and rounds["all_known"] == 1 and rounds["corners"] == 1
    if xy > 64:                                                    # the label of the snake's end travels its whole length
        assert rounds["serpentine"] > rounds["disc"] and rounds["serpentine"] > 4 * (xy // 32)


@pytest.mark.parametrize("xy", [31, 65, 129])
def test_device_maps_are_read_in_place(handles, xy):
    g, dev = handles[xy], _Device()
    try:
        for name in ("cut_ring", "random_m2_c7", "diagonal_pairs", "no_D_random", "serpentine"):
            c, vis, D, mc, cap = fr.patterns(xy)[name]
            f = g.frontiers_of_device(dev.upload(c), dev.upload(vis), None if D is None else dev.upload(D), min_cells=mc, max_clusters=cap)
            _hold(f, fr.expected(xy, name), "device, xy %d, %s" % (xy, name))
    finally:
        dev.free()


@pytest.mark.parametrize("xy", [33, 100])
def test_the_result_does_not_depend_on_inner_bound_or_batch(gvom, xy):
    """a tile that runs out of sweeps flags itself again; a batch may end in the middle of the labelling"""
    g = gvom.Gvom(*_params(xy), voxel_statistics=False)
    for inner, batch in ((1, 1), (3, 16), (256, 5), (3, 1)):
        g.set_tuning("frontier_inner", inner)
        g.set_tuning("frontier_batch", batch)
        assert g.get_tuning("frontier_batch") == batch
        for name in ("serpentine", "spiral", "random_m2_cbig", "u_shape", "diagonal_pairs") if inner > 1 or xy == 33 else ("u_shape", "random_m2_cbig"):
            _hold(_call(g, fr.patterns(xy)[name]), fr.expected(xy, name), "xy %d, %s, inner %d, batch %d" % (xy, name, inner, batch))
    assert g.get_tuning("frontier_tiles") > 0


def test_memory_orders_and_integer_types(handles):
    g, xy = handles[100], 100
    c, vis, D, mc, cap = fr.patterns(xy)["cut_ring"]
    want = fr.expected(xy, "cut_ring")
    assert not np.array_equal(want[2], want[2].T)                  # an [x, y] / [y, x] mix-up would show
    for name, conv in (("fortran", np.asfortranarray), ("c order", np.ascontiguousarray), ("int64", lambda a: a.astype(np.int64)),
                       ("float", lambda a: a.astype(np.float64))):
        _hold(g.frontiers_of(conv(c.T), conv(vis.T), conv(D.T), min_cells=mc, max_clusters=cap), want, name)


def test_1024_cells_random_unknown_and_a_snake_across_all_tiles(gvom):
    xy = 1024
    g = gvom.Gvom(0.4, 0.2, xy, 1, 1, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1, voxel_statistics=False)
    case, want = fr.large_case(xy)
    rounds = _hold(_call(g, case), want, "xy 1024")
    print("tile relaxations", g.get_tuning("frontier_tiles"))
    assert rounds >= 32 and want[3][0] > case[4]                   # the snake crosses every tile of a row; more clusters than rows


def _scene(gvom, name):
    g = gvom.Gvom(*ob.params(name), voxel_statistics=False)
    for pc, ego in ob.scans(name):
        g.process_pointcloud(pc, ego)
    return g, np.array(ob.scans(name)[-1][1][:2])


@pytest.mark.parametrize("name", cf.SCENES)
def test_scenes_end_to_end_through_device_map_sets(gvom, name):
    """combine_maps_device(), a field seeded at the ego's cell, frontiers(maps): the referee is fed the field's own parts and the
    set's own visibility.  min_cells 3 keeps at least one cluster on both scenes (tests/test_frontier_cpu.py holds the census of
    the oracle's maps to that)"""
    g, ego = _scene(gvom, name)
    with g.combine_maps_device() as m:
        vis = m.visibility.copy_to_host()
        for kw in (dict(), dict(inflation_radius=0.8), dict(unknown=30, soft_weight=2)):
            with m.cost_to_go([ego], density_threshold=cf.SCENE_THRESHOLD, **kw) as field:
                D, _, c = field.copy_to_host()
                for mc, cap in ((3, 64), (1, 5), (8, 1024)):
                    want = fr.product(c.T, vis.T, D.T, mc, cap)
                    f = field.frontiers(m, min_cells=mc, max_clusters=cap)
                    assert np.array_equal(f.origin, field.origin)
                    best, centroid, rows = f.goals("cost")
                    n = min(want[3][0], cap)
                    assert best.shape == centroid.shape == (n, 2) and sorted(rows.tolist()) == list(range(n))
                    if n:
                        cells = cf.world_to_cells(best, g.xy_resolution, m.origin)
                        assert np.array_equal(cells[:, 1] * g.xy_size + cells[:, 0], want[0][rows, 6])
                        assert (np.diff(want[0][rows, 7]) >= 0).all()
                        assert (np.diff(want[0][f.goals("size")[2], 1]) <= 0).all()
                    _hold(f, want, "%s %r min_cells %d cap %d" % (name, kw, mc, cap))
                    if mc == 3 and not kw:
                        assert want[3][0] >= 1 and want[3][1] > 20, want[3]
        with pytest.raises(ValueError, match="DeviceMaps"):
            field.frontiers(None)


def test_a_frontier_product_is_a_snapshot(gvom):
    name = "one_round"
    g = gvom.Gvom(*ob.params(name), voxel_statistics=False)
    scans = ob.scans(name)
    g.process_pointcloud(*scans[0])
    m = g.combine_maps_device()
    field = m.cost_to_go([(32, 32)], goals_in_cells=True)
    held = field.frontiers(m, min_cells=1)
    field.release()
    m.release()
    before = held.copy_to_host()
    assert before[3][1] > 0
    for pc, ego in scans[1:]:
        g.process_pointcloud(pc, ego)
        with g.combine_maps_device() as m:
            with m.cost_to_go([(32, 32)], goals_in_cells=True) as field:
                with field.frontiers(m, min_cells=1) as later:
                    assert later.cluster_map.ptr != held.cluster_map.ptr
                    now = later.copy_to_host()
    after = held.copy_to_host()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert not np.array_equal(now[2], after[2])                    # the map has moved on; the held product has not


def test_pool_capacity_reuse_and_no_allocation_in_steady_state(gvom):
    xy = 64
    g = gvom.Gvom(*_params(xy), voxel_statistics=False)
    assert g.get_tuning("frontiers") == 1 and g.get_tuning("frontier_allocations") == 0
    case, want = fr.patterns(xy)["random_m2_c7"], fr.expected(xy, "random_m2_c7")
    first = _call(g, case)
    assert g.get_tuning("frontier_allocations") == 3              # the product set, the work buffer, the host staging buffer
    assert g.get_tuning("device_product_sets") == 1
    ptr = first.clusters.ptr
    first.release()
    for _ in range(20):                                            # released: everything is reused
        with _call(g, case) as f:
            assert f.clusters.ptr == ptr
    assert g.get_tuning("frontier_allocations") == 3 and g.get_tuning("device_product_sets") == 1
    held = [_call(g, case) for _ in range(4)]
    assert len({f.clusters.ptr for f in held}) == 4 and g.get_tuning("device_product_sets") == 4
    with pytest.raises(gvom.GvomBackendError, match="all 4 device product sets of this kind"):
        _call(g, case)
    allocs = g.get_tuning("frontier_allocations")
    assert allocs == 6
    held[2].release()
    _hold(_call(g, case), want, "after a release")
    assert g.get_tuning("device_product_sets") == 4 and g.get_tuning("frontier_allocations") == allocs
    for k in (0, 1, 3):
        _hold(held[k], want, "held")
    with pytest.raises(gvom.GvomBackendError, match="unknown or stale device product id"):
        held[2].copy_to_host()


def test_errors(gvom):
    name = "one_round"
    g = gvom.Gvom(*ob.params(name), voxel_statistics=False)
    xy = g.xy_size
    c, vis, D = np.ones((xy, xy), np.uint16), np.zeros((xy, xy), np.int32), np.ones((xy, xy), np.int32)
    cp, vp, dp = (a.ctypes.data_as(ctypes.c_void_p) for a in (c, vis, D))
    pid = ctypes.c_int64(-1)

    def raw(field=-1, maps=-1, cost=cp, ctg=dp, seen=vp, mc=1, cap=8, out=pid):
        return g._check(g._lib.gvom_frontiers(g._h, field, maps, cost, ctg, seen, 0, mc, cap, ctypes.byref(out) if out is not None else None, None))
    assert raw() == 0 and raw(ctg=None) == 0
    g.process_pointcloud(*ob.scans(name)[0])
    m = g.combine_maps_device()
    field = m.cost_to_go([(32, 32)], goals_in_cells=True)
    ids = dict(field=field.product_id, maps=m.set_id, cost=None, ctg=None, seen=None)
    assert raw(**ids) == 0
    for kw, word in ((dict(ids, cost=cp), "not both"), (dict(ids, seen=vp), "not both"), (dict(ids, ctg=dp), "not both"),
                     (dict(cost=None), "a cell-cost map and a visibility map"), (dict(seen=None), "a cell-cost map and a visibility map"),
                     (dict(cost=None, ctg=None, seen=None), "a cell-cost map and a visibility map"),
                     (dict(ids, maps=-1), "AND a map set id"), (dict(ids, field=-1), "AND a map set id"), (dict(field=field.product_id), "AND a map set id"),
                     (dict(ids, field=10 ** 9), "unknown or stale cost field id"), (dict(ids, maps=10 ** 9), "unknown or stale device map set id"),
                     (dict(mc=0), "min_cells"), (dict(mc=-3), "min_cells"), (dict(cap=0), "max_clusters"), (dict(cap=2 ** 20 + 1), "max_clusters")):
        with pytest.raises(gvom.GvomBackendError, match=word):
            raw(**kw)
    assert raw(cap=2 ** 20) == 0
    assert g._lib.gvom_frontiers(g._h, -1, -1, cp, dp, vp, 0, 1, 8, None, None) == gvom.GVOM_ERR_INVALID          # NULL product_id
    with pytest.raises(gvom.GvomBackendError, match="gvom_frontiers"):
        g._device_product(gvom.PRODUCT_FRONTIERS)
    # the id of another kind of product is no cost field; a recycled set's id is stale
    with g.clearance_of(np.zeros((xy, xy), np.int32)) as clr:
        with pytest.raises(gvom.GvomBackendError, match="unknown or stale cost field id"):
            raw(**dict(ids, field=clr.product_id))
    old_field, old_set = field.product_id, m.set_id
    field.release()
    m.release()
    g.process_pointcloud(*ob.scans(name)[1])
    with g.combine_maps_device() as m2:
        m2.cost_to_go([(32, 32)], goals_in_cells=True).release()
        with pytest.raises(gvom.GvomBackendError, match="stale"):
            raw(**dict(ids, field=old_field, maps=m2.set_id))
    for bad in (dict(min_cells=0), dict(min_cells=1.5), dict(max_clusters=0), dict(max_clusters=2 ** 20 + 1), dict(max_clusters=None)):
        with pytest.raises(ValueError):
            g.frontiers_of(c, vis, **bad)
    sharded = gvom.Gvom(*_params(64), voxel_statistics=False, _shard=(0, 2))
    with pytest.raises(ValueError, match="sharded handles are not supported"):
        sharded.frontiers_of(np.ones((64, 64), np.uint16), np.ones((64, 64), np.int32))
    assert old_set >= 0


def test_maps_of_more_than_4096_cells_a_side_are_refused(gvom):
    xy = 4100
    g = gvom.Gvom(0.4, 0.2, xy, 1, 1, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1, voxel_statistics=False)
    c, vis, pid = np.ones((xy, xy), np.uint16), np.ones((xy, xy), np.int32), ctypes.c_int64(-1)
    rc = g._lib.gvom_frontiers(g._h, -1, -1, c.ctypes.data_as(ctypes.c_void_p), None, vis.ctypes.data_as(ctypes.c_void_p), 0, 1, 8, ctypes.byref(pid), None)
    assert rc == -4 and pid.value == -1 and b"4096" in g._lib.gvom_last_error(g._h)
    assert g.get_tuning("frontier_allocations") == 0


def _torch_case(name):
    """One case per fresh child process that imports torch BEFORE the library is loaded (one HIP runtime in the process)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_frontier_torch.py"), name],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "CASE OK " + name in r.stdout, r.stdout[-4000:]


def test_consumer_picks_goals_on_its_own_stream():
    _torch_case("consumer_stream")
