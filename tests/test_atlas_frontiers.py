"""Atlas frontiers on the GPU (gvom_atlas_frontiers: k_atlas_frontier_mark in front of gvom_frontiers' labelling, ranking and statistics
kernels at the field's side; DeviceAtlasField.frontiers, DeviceAtlasFrontiers) against the referee of tests/atlas_frontier_ref.py with
tolerance 0.  The harness is tests/test_atlas_field.py's: terrain painted with integrate_of() on windows of 16, 33 and 64 cells in
atlases of 64 and 128, following and fixed; then the moved extent and a re-configured atlas, negative visibility, a cleared atlas, a
field stopped early, the snapshot, 512 cells with one cluster through every tile, the drive's outward leg in an atlas of 256, the
per-window frontiers() beside it, the pool and the errors, and an atlas of 4096.  tests/test_atlas_frontiers_cpu.py holds the census
of every input."""
import ctypes

import numpy as np
import pytest

import atlas_field_ref as afr
import atlas_frontier_ref as af
import atlas_ref as ar
import costfield_ref as cf
import frontier_ref as fr

pytestmark = pytest.mark.gpu
U = cf.UNREACHED


def _params(xy, res=afr.RES, buffer_size=1):
    return (res, 0.2, xy, 8, buffer_size, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)


@pytest.fixture(scope="module")
def gvom():
    import gvom as mod
    rc, info = mod.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    assert mod.PRODUCT_ATLAS_FRONTIERS == 28
    return mod


@pytest.fixture(scope="module")
def handles(gvom):
    return {xy: gvom.Gvom(*_params(xy), voxel_statistics=False) for xy in (16, 33, 64)}


def _paint(a, steps):
    for s, o in steps:
        a.integrate_of([m.T for m in s], o)                             # [x, y] views of the [y][x] maps


def _equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d entries differ, first at %r: got %r, referee %r" % (
            what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def _hold(p, want, A, F, what, res=afr.RES):
    """a DeviceAtlasFrontiers against the referee's (clusters, sums, cluster map [x, y], counts, [kept, cells, dropped]); the four
    arrays on the host are returned"""
    cap = want[0].shape[0]
    assert p.origin_cells == tuple(F) and np.array_equal(p.origin, np.array(F, np.float64) * res), (what, p.origin_cells)
    assert p.clusters.shape == (cap, 8) and p.sums.shape == (cap, 2) and p.counts.shape == (4,), what
    assert p.cluster_map.shape == (A, A) and p.cluster_map.strides == (1, A), (what, p.cluster_map.shape, p.cluster_map.strides)
    assert [a.dtype for a in (p.clusters, p.sums, p.cluster_map, p.counts)] == [np.int32, np.int64, np.int32, np.int32], what
    got = p.copy_to_host()
    assert got[2].flags.f_contiguous, what
    for g, w, name in zip(got, want, ("clusters", "sums", "cluster map", "counts")):
        _equal(g, w, "%s, %s" % (what, name))
    assert [p.n_clusters, p.frontier_cells, p.dropped] == list(want[4]) and p.rounds >= 1, (what, p.n_clusters, p.frontier_cells, p.dropped, want[4])
    return got


def _hold_goals(p, rows, A, F, what, res=afr.RES):
    """goal_cells() and goals() against the rows: world cells of the best cells, cheapest first (then by label), and their centres"""
    n = min(p.n_clusters, rows.shape[0])
    r = rows[:n].astype(np.int64)
    order = sorted(range(n), key=lambda k: (r[k, 7], r[k, 0]))
    cells, pick = p.goal_cells()
    assert pick.tolist() == order and cells.dtype == np.int64 and cells.shape == (n, 2), what
    assert np.array_equal(cells, np.stack([r[order, 6] % A + F[0], r[order, 6] // A + F[1]], axis=1)), what
    best, centroid, pick2 = p.goals()
    assert pick2.tolist() == order and np.array_equal(best, (cells + 0.5) * res), what
    assert np.array_equal(centroid, ((p.sums.copy_to_host()[:n] / np.maximum(r[:, 1:2], 1) + np.array(F, np.float64) + 0.5) * res)[order]), what
    by_size = sorted(range(n), key=lambda k: (-r[k, 1], r[k, 0]))
    assert p.goal_cells(order="size")[1].tolist() == by_size == p.goals(order="size")[2].tolist(), what


def _field(a, want, **more):
    return a.cost_to_go(np.array(want["goals_world"]), goals_in_cells=True, max_cost=want["max_cost"] or None, **dict(afr.keywords(want["params"]), **more))


# ---- 1 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("follow", [True, False])
@pytest.mark.parametrize("xy,A", afr.SCENARIOS)
def test_synthetic_scenarios_match_the_referee_exactly(gvom, handles, xy, A, follow):
    """variants 0, 1 and 5 of every scenario under (min_cells, max_clusters) = (4, 1024), (1, 8) and (2, 2^20)"""
    g = handles[xy]
    ref, steps = afr.scenario(xy, A, follow)
    a = g.create_atlas(A, follow=follow, origin_cells=None if follow else ref.E)
    _paint(a, steps)
    for k in af.VARIANTS:
        with _field(a, afr.expected(xy, A, follow, k)) as f:
            for min_cells, cap in af.LIMITS:
                what = "xy %d, A %d, %s, variant %d, min_cells %d, cap %d" % (xy, A, "follow" if follow else "fixed", k, min_cells, cap)
                with f.frontiers(min_cells=min_cells, max_clusters=cap) as p:
                    got = _hold(p, af.expected(xy, A, follow, k, min_cells, cap), A, ref.E, what)
                    assert g.get_tuning("atlas_frontier_rounds") == p.rounds and (g.get_tuning("atlas_frontier_tiles") >= 1) == (p.frontier_cells >= 1), what
                    if cap != 2 ** 20:
                        _hold_goals(p, got[0], A, ref.E, what)


# ---- 2 -----------------------------------------------------------------------------------------------------------------------------------
def test_the_moved_extent_and_a_reconfigured_atlas(gvom, handles):
    """the field is a snapshot in its own frame; the visibility is the atlas's as it is now: after the extent has moved by (20, -5), and
    after create_atlas() with another side"""
    xy, A = 33, 128
    g = handles[xy]
    ref, steps = afr.scenario(xy, A, True)
    a = g.create_atlas(A)
    _paint(a, steps)
    want = afr.expected(xy, A, True, 0)
    with _field(a, want) as f:
        with f.frontiers() as p:
            _hold(p, af.expected(xy, A, True, 0), A, ref.E, "before the move")
        now, (s, o) = af.moved(xy, A, True)
        a.integrate_of([m.T for m in s], o)
        assert tuple(a.extent_origin) == now.E == (ref.E[0] + 20, ref.E[1] - 5)
        with f.frontiers() as p:
            got = _hold(p, af.of_field(want, now, 4, 1024), A, ref.E, "after the move")
            assert (got[2][:20, :] == -1).all() and (got[2][:, A - 5:] == -1).all()
        E2 = (ref.E[0] + 40, ref.E[1] + 50)
        small = ar.AtlasRef(64, xy, False, E2)
        small.integrate(s, (ref.E[0] + 50, ref.E[1] + 60))
        b = g.create_atlas(64, follow=False, origin_cells=E2)
        b.integrate_of([m.T for m in s], (ref.E[0] + 50, ref.E[1] + 60))
        with f.frontiers(min_cells=1) as p:
            got = _hold(p, af.of_field(want, small, 1, 1024), A, ref.E, "an atlas of 64 cells under a field of 128")
            assert p.frontier_cells >= 1 and (got[2][:40, :] == -1).all() and (got[2][:, 114:] == -1).all()


# ---- 3 -----------------------------------------------------------------------------------------------------------------------------------
def test_negative_visibility_a_cleared_atlas_and_a_field_stopped_early(gvom, handles):
    xy, A = 16, 64
    g = handles[xy]
    E = ar.fixed_origin(xy, A)
    a = g.create_atlas(A, follow=False, origin_cells=E)
    ref = ar.AtlasRef(A, xy, False, E)
    s = af.negative_set(xy)
    a.integrate_of([m.T for m in s], (E[0] + 8, E[1] + 8))
    ref.integrate(s, (E[0] + 8, E[1] + 8))
    seed = (E[0] + 9, E[1] + 9)
    want = afr.field(ref, [seed], afr.params())
    with a.cost_to_go([seed], goals_in_cells=True) as f:
        with f.frontiers(min_cells=1, max_clusters=64) as p:
            got = _hold(p, af.of_field(want, ref, 1, 64), A, E, "visibility -3")
            assert got[2][8 + xy // 2 - 1, 9] >= 0                      # a frontier cell only because -3 counts as UNKNOWN
        a.clear()
        with f.frontiers(min_cells=1, max_clusters=64) as p:
            ref.clear()
            _hold(p, af.of_field(want, ref, 1, 64), A, E, "a cleared atlas")
            assert (p.frontier_cells, p.n_clusters, p.dropped) == (0, 0, 0) and g.get_tuning("atlas_frontier_tiles") == 0
    xy, A = 64, 128
    g = handles[xy]
    ref, steps = afr.scenario(xy, A, False)
    a = g.create_atlas(A, follow=False, origin_cells=ref.E)
    _paint(a, steps)
    with _field(a, afr.expected(xy, A, False, 0), max_rounds=1) as f:
        assert not f.converged
        cost, _, cell = f.copy_to_host()
        assert (cost != U).sum() < afr.expected(xy, A, False, 0)["info"][0]
        with f.frontiers() as p:
            _hold(p, af.product(cell, af.visibility(ref, ref.E, A), cost, 4, 1024), A, ref.E, "a field stopped after one round")
            assert p.frontier_cells >= 1


# ---- 4 -----------------------------------------------------------------------------------------------------------------------------------
def test_a_product_is_a_snapshot(gvom, handles):
    xy, A = 33, 64
    g = handles[xy]
    ref, steps = afr.scenario(xy, A, True)
    a = g.create_atlas(A)
    _paint(a, steps)
    with _field(a, afr.expected(xy, A, True, 0)) as f, f.frontiers() as p:
        want = af.expected(xy, A, True, 0)
        _hold(p, want, A, ref.E, "at first")
        a.integrate_of([m.T for m in steps[0][0]], (steps[-1][1][0] + xy + 40, steps[-1][1][1] - xy - 40))
        a.clear()
        f.frontiers().release()                                         # another product of the kind: this one is held
        _hold(p, want, A, ref.E, "after integrates, a clear and another call")


# ---- 5 -----------------------------------------------------------------------------------------------------------------------------------
def test_512_cells_one_cluster_through_every_tile(gvom, handles):
    """A = 512, fixed, painted by 64 integrate_of() calls of 64 cells: never-seen ground but for a one-cell-wide observed free serpentine,
    unknown="free".  One cluster through all 16 x 16 tiles whose label is its first cell; the labels need more than one batch of rounds"""
    xy, A = 64, 512
    g = handles[xy]
    E = (-300, -77)
    a = g.create_atlas(A, follow=False, origin_cells=E)
    seen = np.zeros((A, A), bool)                                       # [y][x]
    for x, y in fr.snake(A, 16):
        seen[y, x] = True
    try:
        for j in range(0, A, xy):
            for i in range(0, A, xy):
                s = afr.seam_set(xy)
                s[2] = np.where(seen[j:j + xy, i:i + xy], 3, 0).astype(np.int32)
                a.integrate_of([m.T for m in s], (E[0] + i, E[1] + j))
        with a.cost_to_go([E], goals_in_cells=True, unknown="free") as f:
            cost, _, cell = f.copy_to_host()
            assert f.reached == A * A
            with f.frontiers() as p:
                vis3 = seen.T.astype(np.int32)
                want = af.product(cell, vis3, cost, 4, 1024)
                got = _hold(p, want, A, E, "A 512")
                # every cell of the serpentine but its first corner (A - 1, 0), whose neighbours are on the path or outside the field
                assert p.n_clusters == 1 and got[0][0, 0] == 0 and got[0][0, 1] == seen.sum() - 1 == p.frontier_cells and got[2][A - 1, 0] == -1
                assert got[0][0, 2:6].tolist() == [0, 0, A - 1, 496] and got[0][0, 6] == 0 and got[0][0, 7] == 0
                assert p.rounds > 8, p.rounds
                print("A 512: rounds", p.rounds, "tile relaxations", g.get_tuning("atlas_frontier_tiles"), "frontier cells", p.frontier_cells)
    finally:
        a.release()


# ---- 6 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring", [1, 2])
def test_the_drive_end_to_end_goals_lie_outside_the_window(gvom, ring):
    """the drive's outward leg through combine_maps_device() + integrate() with an atlas of 256 cells, the field seeded at the free cell
    nearest the vehicle: the product equals the referee computed from the product's own field and the exported extent's visibility, at
    least one cluster's best cell lies outside the live window, and path_from() walks from each best cell back to the seed at best D"""
    g = gvom.Gvom(*_params(ar.DRIVE_XY, ar.DRIVE_RES, ring), voxel_statistics=False)
    a = g.create_atlas(afr.DRIVE_A)
    scans = afr.drive_out()
    m = None
    for pc, ego in scans:
        if m is not None:
            m.release()
        g.process_pointcloud(pc, ego)
        m = g.combine_maps_device()
        a.integrate(m)
    xy, res, A = ar.DRIVE_XY, ar.DRIVE_RES, afr.DRIVE_A
    org = m.origin_cells[:2]
    with a.extent_device() as e:
        E = e.origin_cells
        pos, neg, vis, rough = (getattr(e, n).copy_to_host() for n in ("positive", "negative", "visibility", "roughness"))
    vehicle = tuple(int(v) for v in gvom.cells_of(scans[-1][1][:2], res))
    seed = afr.nearest_free(afr.cell_costs(pos, neg, vis, rough, afr.params()), (vehicle[0] - E[0], vehicle[1] - E[1]))
    seed = (seed[0] + E[0], seed[1] + E[1])
    with a.cost_to_go([seed], goals_in_cells=True) as f, f.frontiers() as p:
        cost, _, cell = f.copy_to_host()
        got = _hold(p, af.product(cell, (vis > 0).astype(np.int32), cost, 4, 1024), A, E, "the drive, ring %d" % ring, res)
        _hold_goals(p, got[0], A, E, "the drive", res)
        cells, rows = p.goal_cells()
        outside = ~((cells[:, 0] >= org[0]) & (cells[:, 0] < org[0] + xy) & (cells[:, 1] >= org[1]) & (cells[:, 1] < org[1] + xy))
        print("ring", ring, "kept", p.n_clusters, "frontier cells", p.frontier_cells, "best cells outside the window", int(outside.sum()))
        assert p.n_clusters >= 1 and outside.sum() >= 1
        for cell_w, r in zip(cells, rows):
            path = f.path_from(cell_w)
            assert path[0] == tuple(cell_w) and path[-1] == seed
            assert cf.path_cost([(x - E[0], y - E[1]) for x, y in path], cell) == got[0][r, 7]
    m.release()


# ---- 7 -----------------------------------------------------------------------------------------------------------------------------------
def test_the_per_window_frontiers_are_untouched(gvom, handles):
    """DeviceCostField.frontiers() on a cropped field gives the same product before and after atlas calls, its work buffer is never
    re-allocated by them, and the atlas route's own allocations are flat over 20 calls"""
    xy, A = 33, 128
    g = handles[xy]
    ref, steps = afr.scenario(xy, A, True)
    a = g.create_atlas(A)
    _paint(a, steps)
    o = steps[-1][1]
    with _field(a, afr.expected(xy, A, True, 0)) as f, a.recall(origin_cells=o) as m, f.window(m) as w:
        with w.frontiers(m, min_cells=2, max_clusters=256) as p:
            before = p.copy_to_host()
            info = (p.rounds, p.n_clusters, p.frontier_cells, p.dropped)
        assert info[2] >= 1
        window_allocs = g.get_tuning("frontier_allocations")
        f.frontiers().release()
        allocs = g.get_tuning("atlas_frontier_allocations")
        assert allocs >= 2                                              # the work buffer at side A and a product set
        for k in range(20):
            with f.frontiers(min_cells=1 + k % 3, max_clusters=1024) as p:
                if k == 19:
                    _hold(p, af.expected(xy, A, True, 0, 2, 1024), A, ref.E, "the twentieth call")
        assert g.get_tuning("atlas_frontier_allocations") == allocs and g.get_tuning("frontier_allocations") == window_allocs
        with w.frontiers(m, min_cells=2, max_clusters=256) as p:
            after = p.copy_to_host()
            assert (p.rounds, p.n_clusters, p.frontier_cells, p.dropped) == info
        for x, y in zip(before, after):
            assert np.array_equal(x, y)
        assert g.get_tuning("frontier_allocations") == window_allocs
        m.stamps.release()


# ---- 8 -----------------------------------------------------------------------------------------------------------------------------------
def test_the_pool_the_capacity_and_the_errors(gvom, handles):
    xy, A = 16, 64
    g = handles[xy]
    lib, h = g._lib, g._h
    ref, steps = afr.scenario(xy, A, True)
    assert g.get_tuning("atlas_frontiers") == 1
    a = g.create_atlas(A)
    _paint(a, steps)
    want = afr.expected(xy, A, True, 0)
    f = _field(a, want)
    held = [f.frontiers() for _ in range(4)]                            # GVOM_MAX_PRODUCT_SETS
    with pytest.raises(gvom.GvomBackendError, match="all 4 device product sets"):
        f.frontiers()
    stale = held.pop()
    stale_id = stale.product_id
    stale.release()
    with f.frontiers() as p:                                            # a release frees one (and recycles it: the old id is stale)
        _hold(p, af.expected(xy, A, True, 0), A, ref.E, "a recycled set")
        assert p.product_id != stale_id
    for x in held:
        x.release()
    I64 = ctypes.c_int64
    pid, info, e = I64(-1), (I64 * 4)(), (I64 * 2)()
    raw = lambda field=f.product_id, min_cells=4, cap=1024, out=ctypes.byref(pid): lib.gvom_atlas_frontiers(h, field, min_cells, cap, out, info, e)
    with f.window(origin_cells=steps[0][1]) as w, f.frontiers() as p:
        for bad, word in ((dict(field=1 << 40), b"atlas field id"), (dict(field=-1), b"atlas field id"), (dict(field=w.product_id), b"atlas field id"),
                          (dict(field=p.product_id), b"atlas field id"), (dict(min_cells=0), b"min_cells"), (dict(min_cells=-3), b"min_cells"),
                          (dict(cap=0), b"max_clusters"), (dict(cap=2 ** 20 + 1), b"max_clusters")):
            assert raw(**bad) == gvom.GVOM_ERR_INVALID and word in lib.gvom_last_error(h), bad
            assert pid.value == -1
    assert raw(out=None) == gvom.GVOM_ERR_INVALID
    assert lib.gvom_atlas_frontiers(h, f.product_id, 4, 1024, ctypes.byref(pid), None, None) == 0 and pid.value >= 0       # info and extent_origin may be NULL
    assert raw() == 0 and (e[0], e[1]) == ref.E and info[2] == af.expected(xy, A, True, 0)[3][1]
    gone = _field(a, want)
    gone_id = gone.product_id
    gone.release()
    _field(a, want).release()                                           # recycles the set: the id is stale
    with pytest.raises(ValueError, match="stale atlas field id"):
        gone.frontiers()
    assert raw(field=gone_id) == gvom.GVOM_ERR_INVALID
    with pytest.raises(gvom.GvomBackendError, match="unknown product kind"):
        g._device_product(gvom.PRODUCT_ATLAS_FRONTIERS)
    # the field outlives the atlas, the visibility does not: without an atlas there is no answer
    a.release()
    assert raw() == gvom.GVOM_ERR_INVALID and b"no atlas is configured" in lib.gvom_last_error(h)
    with pytest.raises(ValueError, match="no atlas is configured"):
        f.frontiers()
    f.release()
    s = gvom.Gvom(*_params(64), voxel_statistics=False, _shard=(0, 2))
    assert s._lib.gvom_atlas_frontiers(s._h, 1, 4, 1024, ctypes.byref(pid), info, e) == gvom.GVOM_ERR_INVALID and b"sharded" in s._lib.gvom_last_error(s._h)


# ---- 9 -----------------------------------------------------------------------------------------------------------------------------------
def test_an_atlas_of_4096_cells(gvom, handles):
    """one integrated set around the storage seam of an atlas of 4096 cells, everything else never seen: rows, counts and the painted part
    of the cluster map equal the referee -- computed on the set and a ring of never-seen cells around it, and moved into the field's frame
    (the embedding keeps the order of the linear indices, hence labels' order and ranks) --, the rest of the map holds no frontier cell,
    and the allocations are the work buffer and one product set, once"""
    g, A, xy = handles[64], 4096, 64
    a = g.create_atlas(A)
    try:
        o = (-30, 4090)                                                  # across the storage seam in x and in y
        s = afr.terrain_set(np.random.default_rng(4096), xy)
        a.integrate_of([m.T for m in s], o)
        E = a.extent_origin
        x, y = afr.well_connected(afr.cell_costs(s[0].T, s[1].T, s[2].T, s[3].T, afr.params()))
        window_allocs, allocs = g.get_tuning("frontier_allocations"), g.get_tuning("atlas_frontier_allocations")
        with a.cost_to_go([(o[0] + x, o[1] + y)], goals_in_cells=True) as f:
            with f.window(origin_cells=o) as w:
                D, _, c = w.copy_to_host()
            n = xy + 2                                                   # (c and D count at known cells only: the ring's stay 0 and unreached)
            cs, Ds, vs = np.zeros((n, n), np.int32), np.full((n, n), U, np.int32), np.zeros((n, n), np.int32)
            cs[1:xy + 1, 1:xy + 1], Ds[1:xy + 1, 1:xy + 1], vs[1:xy + 1, 1:xy + 1] = c, D, s[2].T > 0
            rows, sums, cmap, counts, info = af.product(cs, vs, Ds, 4, 1024)
            ox, oy = o[0] - 1 - E[0], o[1] - 1 - E[1]                    # the padded square's corner in the field's frame
            k = min(int(counts[0]), 1024)
            r = rows.astype(np.int64)
            for col in (0, 6):
                r[:k, col] = (r[:k, col] // n + oy) * A + r[:k, col] % n + ox
            r[:k, 2] += ox; r[:k, 4] += ox; r[:k, 3] += oy; r[:k, 5] += oy
            sums = sums.copy()
            sums[:k, 0] += r[:k, 1] * ox
            sums[:k, 1] += r[:k, 1] * oy
            with f.frontiers() as p:
                assert g.get_tuning("atlas_frontier_allocations") == allocs + 2 and g.get_tuning("frontier_allocations") == window_allocs
                assert p.cluster_map.shape == (A, A) and p.origin_cells == tuple(E)
                got = p.copy_to_host()
                _equal(got[0], r.astype(np.int32), "4096, clusters")
                _equal(got[1], sums, "4096, sums")
                _equal(got[3], counts, "4096, counts")
                _equal(got[2][ox:ox + n, oy:oy + n], cmap, "4096, the painted part of the cluster map")
                assert (got[2] != -1).sum() == counts[1] >= 1 and [p.n_clusters, p.frontier_cells, p.dropped] == list(info)
                print("A 4096: rounds", p.rounds, "tile relaxations", g.get_tuning("atlas_frontier_tiles"), "frontier cells", p.frontier_cells)
            f.frontiers().release()
            assert g.get_tuning("atlas_frontier_allocations") == allocs + 2
    finally:
        a.release()
