"""Atlas fields on the GPU (gvom_atlas_cost_to_go, gvom_atlas_field_window: k_atlas_clearance_rows, k_atlas_travcost,
k_atlas_field_window in front of and behind the 2-D solver; Atlas.cost_to_go, DeviceAtlasField, DeviceAtlasFieldWindow) against the
referee of tests/atlas_field_ref.py with tolerance 0.  Terrain painted with integrate_of() on windows of 16, 33 and 64 cells in atlases
of 64 and 128, following and fixed; the seam; the snapshot; rollouts and frontiers on a cropped field; an early stop; 512 cells; the
drive's outward leg in an atlas of 256; the pool, the errors and an atlas of 4096.  tests/test_atlas_field_cpu.py holds the census of
every input."""
import ctypes

import numpy as np
import pytest

import atlas_field_ref as afr
import atlas_ref as ar
import costfield_ref as cf
import frontier_ref as fr
import rollouts_ref as rr

pytestmark = pytest.mark.gpu
U = cf.UNREACHED


def _params(xy, res=afr.RES, buffer_size=1):
    return (res, 0.2, xy, 8, buffer_size, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)


@pytest.fixture(scope="module")
def gvom():
    import gvom as mod
    rc, info = mod.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    assert mod.PRODUCT_ATLAS_FIELD == 26
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
        raise AssertionError("%s: %d cells differ, first (x %d, y %d): got %r, referee %r" % (
            what, len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])]))


def _hold_field(f, want, what, converged=True):
    """a DeviceAtlasField against the referee's field: the three planes on the whole extent, the info, the origin"""
    A = want["D"].shape[0]
    assert f.origin_cells == tuple(want["E"]) and np.array_equal(f.origin, np.array(want["E"], np.float64) * afr.RES), (what, f.origin_cells)
    for arr, dt in ((f.cost, np.int32), (f.direction, np.uint8), (f.cell_cost, np.uint16)):
        assert arr.shape == (A, A) and arr.strides == (1, A) and arr.dtype == dt, what
    cost, direction, cell = f.copy_to_host()
    assert cost.flags.f_contiguous and [a.dtype for a in (cost, direction, cell)] == [np.int32, np.uint8, np.uint16], what
    _equal(cell, want["c"], what + ", cell_cost")
    _equal(cost, want["D"], what + ", cost")
    _equal(direction, want["dir"], what + ", direction")
    assert (f.converged, f.reached, f.goals_seeded) == (converged,) + tuple(want["info"]) and f.rounds >= 1, (what, f.reached, f.goals_seeded, want["info"])


def _hold_window(w, want, origin, what):
    """a DeviceAtlasFieldWindow against the plain crop"""
    xy = want[0].shape[0]
    with w:
        assert w.origin_cells == tuple(origin) and np.array_equal(np.asarray(w.origin)[:2], np.array(origin, np.float64) * afr.RES), what
        assert w.cost.strides == (1, xy) and w.cost.shape == (xy, xy), what
        got = w.copy_to_host()
        assert [a.dtype for a in got] == [np.int32, np.uint8, np.uint16], what
        for g, r, name in zip(got, want, ("cost", "direction", "cell_cost")):
            _equal(g, r, "%s, window %s" % (what, name))


@pytest.mark.parametrize("follow", [True, False])
@pytest.mark.parametrize("xy,A", afr.SCENARIOS)
def test_synthetic_scenarios_match_the_referee_exactly(gvom, handles, xy, A, follow):
    """every variant of the scenario: the field on the whole extent, and its window() at the current origin, the first origin, half
    outside and wholly outside the extent, through a live set id and through origin_cells"""
    g = handles[xy]
    ref, steps = afr.scenario(xy, A, follow)
    a = g.create_atlas(A, follow=follow, origin_cells=None if follow else ref.E)
    _paint(a, steps)
    assert tuple(a.extent_origin) == ref.E
    for k, v in enumerate(afr.VARIANTS):
        want = afr.expected(xy, A, follow, k)
        what = "xy %d, A %d, %s, variant %d %r" % (xy, A, "follow" if follow else "fixed", k, v)
        f = a.cost_to_go(np.array(want["goals_world"]), goals_in_cells=True, max_cost=want["max_cost"] or None, **afr.keywords(want["params"]))
        with f:
            _hold_field(f, want, what)
            assert (g.get_tuning("atlas_field_tiles") >= 1) == (f.goals_seeded >= 1), what      # (no goal seeded: no tile ran)
            for o in afr.window_origins(xy, A, ref.E, steps):
                crop = afr.window(want, o, xy)
                _hold_window(f.window(origin_cells=o), crop, o, "%s, origin_cells %r" % (what, (o,)))
                with a.recall(origin_cells=o) as m:
                    _hold_window(f.window(m), crop, o, "%s, the set recalled at %r" % (what, (o,)))
                    m.stamps.release()
    metres = a.cost_to_go((np.array(want["goals_world"]) + 0.5) * afr.RES, **afr.keywords(want["params"]))      # the same goals in world metres
    _hold_field(metres, want, "goals in metres")
    metres.release()


def test_the_seam_is_not_an_edge_of_the_graph(gvom, handles):
    """walls along extent column 0 and row A - 1, three cells of inflation: the cells along the far edges stay free and the way from
    column A - 5 to column 4 is the flat one (the census holds that the toroidal twin's differs)"""
    xy, A = 33, 128
    g = handles[xy]
    E = ar.fixed_origin(xy, A)
    a = g.create_atlas(A, follow=False, origin_cells=E)
    ref = ar.AtlasRef(A, xy, False, E)
    steps, goal, start = afr.seam_case(xy, A, E)
    _paint(a, steps)
    for s, o in steps:
        ref.integrate(s, o)
    p = afr.params(inflation_cells=3)
    want = afr.field(ref, [goal], p)
    with a.cost_to_go([goal], goals_in_cells=True, **afr.keywords(p)) as f:
        _hold_field(f, want, "the seam")
        cost, _, cell = f.copy_to_host()
        assert (cell[A - 1, :A - 4] > 0).all() and (cell[4:, 0] > 0).all() and (cell[:4, :] == 0).all() and (cell[:, A - 4:] == 0).all()
        sx, sy = start[0] - E[0], start[1] - E[1]
        assert cost[sx, sy] == 10 * (A - 9) and cf.path_cost([(x - E[0], y - E[1]) for x, y in f.path_from(start)], want["c"]) == cost[sx, sy]


def test_a_field_is_a_snapshot(gvom, handles):
    """a field and its windows are unchanged by an integrate that moves the extent by more than xy_size, by clear() and by a
    re-configure; a window over cells that have since left the ATLAS's extent still reads the field"""
    xy, A = 33, 64
    g = handles[xy]
    ref, steps = afr.scenario(xy, A, True)
    a = g.create_atlas(A)
    _paint(a, steps)
    want = afr.expected(xy, A, True, 2)
    f = a.cost_to_go(np.array(want["goals_world"]), goals_in_cells=True, **afr.keywords(want["params"]))
    origins = afr.window_origins(xy, A, ref.E, steps)
    away = (steps[-1][1][0] + xy + 40, steps[-1][1][1] - xy - 40)
    a.integrate_of([m.T for m in steps[0][0]], away)
    assert abs(a.extent_origin[0] - ref.E[0]) > xy
    for stage in ("moved", "cleared", "re-configured"):
        _hold_field(f, want, "after the extent " + stage)
        for o in origins + [away]:
            _hold_window(f.window(origin_cells=o), afr.window(want, o, xy), o, "%s, window at %r" % (stage, (o,)))
        if stage == "moved":
            a.clear()
        elif stage == "cleared":
            a = g.create_atlas(128, follow=False, origin_cells=(1000, 1000))
    _hold_window(f.window(origin_cells=(1000, 1000)), afr.window(want, (1000, 1000), xy), (1000, 1000), "inside the new atlas, outside the field")
    f.release()


def test_rollouts_and_frontiers_run_on_a_cropped_field_unchanged(gvom, handles):
    """window() is a cost field in every respect: score_rollouts() equals rollouts_ref.score with the cropped c and D (K 64, T 16,
    rollouts_ref's patch table), frontiers(recalled maps) equals frontier_ref on the cropped arrays; the field is seeded at the
    vehicle, and frontier cells are reached by routes that leave the window"""
    xy, A = 33, 128
    g = handles[xy]
    ref, steps = afr.scenario(xy, A, True)
    a = g.create_atlas(A)
    _paint(a, steps)
    o = steps[-1][1]
    p = afr.params(inflation_cells=1, unknown=40, soft_weight=2)
    maps, E = afr.extent_maps(ref)
    vehicle = afr.nearest_free(afr.cell_costs(*maps, p), (o[0] - E[0] + xy // 2, o[1] - E[1] + xy // 2))
    vehicle = (vehicle[0] + E[0], vehicle[1] + E[1])
    want = afr.field(ref, [vehicle], p)
    D, d, c = afr.window(want, o, xy)
    table = rr.patch_table(16, 9)
    g.set_footprint(table)
    poses = rr.arc_poses(64, 16, xy, afr.RES, o, seed=5)
    with a.cost_to_go([vehicle], goals_in_cells=True, **afr.keywords(p)) as f, a.recall(origin_cells=o) as m:
        w = f.window(m)
        _hold_window(f.window(m), (D, d, c), o, "the vehicle's window")
        summary, pose_cost, _ = rr.score(c, poses, table, afr.RES, o, D)
        with w.score_rollouts(poses) as r:
            got = r.copy_to_host()
        assert np.array_equal(got[0], summary) and np.array_equal(got[1], pose_cost)
        assert ((summary[:, 3] != U) & (summary[:, 3] > 0)).sum() >= 8          # terminals taken from the global field
        vis = m.visibility.copy_to_host()
        fwant = fr.product(c.T, vis.T, D.T, 2, 256)
        with w.frontiers(m, min_cells=2, max_clusters=256) as front:
            fgot = front.copy_to_host()
            assert (front.n_clusters, front.frontier_cells, front.dropped) == tuple(fwant[4][-3:]) and front.n_clusters >= 1
        assert np.array_equal(fgot[0], fwant[0]) and np.array_equal(fgot[1], fwant[1]) and np.array_equal(fgot[2].T, fwant[2]) and np.array_equal(fgot[3], fwant[3])
        # frontier cells the window's own graph cannot reach from the vehicle: the global field took a route outside the window
        local = cf.dijkstra(c, [(vehicle[0] - o[0], vehicle[1] - o[1])])
        assert (fr.frontier_mask(c.T, vis.T, D.T) & (local.T == U)).sum() >= 1
        m.stamps.release()
        w.release()


def test_an_early_stop_keeps_the_headers_promises(gvom, handles):
    """max_rounds = 1 at A = 128: not converged; every finite D is at least the referee's and is the cost of a real path"""
    xy, A = 64, 128
    g = handles[xy]
    ref, steps = afr.scenario(xy, A, False)
    a = g.create_atlas(A, follow=False, origin_cells=ref.E)
    _paint(a, steps)
    want = afr.expected(xy, A, False, 0)
    kw = afr.keywords(want["params"])
    with a.cost_to_go(np.array(want["goals_world"]), goals_in_cells=True, max_rounds=1, **kw) as f:
        assert not f.converged and f.rounds == 1 and f.goals_seeded == want["info"][1]
        cost, direction, cell = f.copy_to_host()
    finite = cost != U
    _equal(cell, want["c"], "early stop, cell_cost")
    assert finite.any() and not finite[want["D"] == U].any() and (cost[finite] >= want["D"][finite]).all() and f.reached == int(finite.sum()) < want["info"][0]
    assert np.array_equal(direction == cf.NONE, ~finite) and np.array_equal(direction == cf.GOAL, cost == 0)
    assert ((direction < 8) | np.isin(direction, (cf.GOAL, cf.UNSETTLED, cf.NONE))).all()
    # every finite value is the cost of a real path: some admissible neighbour offered it or less when it was stored, and that
    # neighbour's value has only gone down since -- D[u] >= min over admissible v of D[v] + w(u, v) everywhere but at the goals
    best = np.full(cost.shape, cf.INF, np.int64)
    for _, offer in cf.iter_matches(cost, want["c"]):
        np.minimum(best, offer, out=best)
    inner = finite & (cost != 0)
    assert (cost[inner] >= best[inner]).all()
    with a.cost_to_go(np.array(want["goals_world"]), goals_in_cells=True, max_rounds=10 ** 6, **kw) as done:
        _hold_field(done, want, "a bound that is not reached")


def test_512_cells_sixteen_by_sixteen_tiles(gvom, handles):
    """A = 512, fixed, the extent tiled by 64 integrate_of() calls of 64 cells, one goal, two cells of inflation: the wavefront runs
    over more than one batch of rounds; the referee is heap Dijkstra"""
    xy, A = 64, 512
    g = handles[xy]
    E = (-300, -77)
    a = g.create_atlas(A, follow=False, origin_cells=E)
    ref = ar.AtlasRef(A, xy, False, E)
    rng = np.random.default_rng(512)
    for j in range(0, A, xy):
        for i in range(0, A, xy):
            s = afr.terrain_set(rng, xy)
            a.integrate_of([m.T for m in s], (E[0] + i, E[1] + j))
            ref.integrate(s, (E[0] + i, E[1] + j))
    p = afr.params(inflation_cells=2)
    maps, _ = afr.extent_maps(ref)
    goal = afr.well_connected(afr.cell_costs(*maps, p)[:64, :64])      # (in the extent's first tile: the far corner is 16 tiles away)
    goal = (goal[0] + E[0], goal[1] + E[1])
    want = afr.field(ref, [goal], p)
    assert want["info"][0] > A * A // 4
    try:
        with a.cost_to_go([goal], goals_in_cells=True, **afr.keywords(p)) as f:
            _hold_field(f, want, "A 512")
            assert f.rounds > 8, f.rounds
            print("A 512: rounds", f.rounds, "tile relaxations", g.get_tuning("atlas_field_tiles"), "reached", f.reached)
    finally:
        a.release()


@pytest.mark.parametrize("ring", [1, 2])
def test_the_drive_end_to_end_home_lies_outside_the_window(gvom, ring):
    """the drive's outward leg through combine_maps_device() + integrate() with an atlas of 256 cells: at the far end the live window's
    cost_to_go(home) raises, the atlas's equals the referee on the exported extent, the path from the free cell nearest the vehicle ends
    at home with the field's cost, and window(device_maps).score_rollouts() reads its terminals from the global field"""
    g = gvom.Gvom(*_params(ar.DRIVE_XY, ar.DRIVE_RES, ring), voxel_statistics=False)
    a = g.create_atlas(afr.DRIVE_A)
    ref = ar.AtlasRef(afr.DRIVE_A, ar.DRIVE_XY)
    scans = afr.drive_out()
    home = tuple(int(v) for v in gvom.cells_of(scans[0][1][:2], ar.DRIVE_RES))
    m = None
    for pc, ego in scans:
        if m is not None:
            m.release()
        g.process_pointcloud(pc, ego)
        m = g.combine_maps_device()
        a.integrate(m)
        ref.integrate([getattr(m, name).copy_to_host().T for name in gvom.DEVICE_MAP_NAMES], m.origin_cells[:2])
    xy, res = ar.DRIVE_XY, ar.DRIVE_RES
    org = m.origin_cells[:2]
    assert not (org[0] <= home[0] < org[0] + xy and org[1] <= home[1] < org[1] + xy)
    home_m = np.array(scans[0][1][:2])
    with pytest.raises(ValueError, match="outside the window"):
        m.cost_to_go([home_m])
    with a.extent_device() as e:                                         # the referee was fed the same sets: the export agrees with it
        assert e.origin_cells == ref.E and np.array_equal(e.positive.copy_to_host().T, ref.i[0])
    vehicle = tuple(int(v) for v in gvom.cells_of(scans[-1][1][:2], res))
    for cells, reaches in ((0, True), (1, None)):
        p = afr.params(inflation_cells=cells)
        want = afr.field(ref, [home], p)
        with a.cost_to_go([home_m], **afr.keywords(p, res)) as f:
            _hold_field_drive(f, want, res, "ring %d, %d cells of inflation" % (ring, cells))
            E = want["E"]
            start = afr.nearest_free(want["c"], (vehicle[0] - E[0], vehicle[1] - E[1]))
            Dv = int(want["D"][start])
            path = f.path_from((start[0] + E[0], start[1] + E[1]))
            print("ring", ring, "inflation", cells, "start", start, "D", Dv, "steps", None if path is None else len(path) - 1)
            if reaches:
                assert Dv != U and path[-1] == home and len(path) - 1 > xy
            assert (path is None) == (Dv == U)                           # (held to equality either way)
            if path is not None:
                assert cf.path_cost([(x - E[0], y - E[1]) for x, y in path], want["c"]) == Dv
            if cells == 0:
                g.set_footprint(rr.patch_table(16, 9))
                poses = rr.arc_poses(64, 16, xy, res, org, seed=9)
                D, _, c = afr.window(want, org, xy)
                summary, pose_cost, _ = rr.score(c, poses, rr.patch_table(16, 9), res, org, D)
                with f.window(m) as w, w.score_rollouts(poses) as r:
                    got = r.copy_to_host()
                assert np.array_equal(got[0], summary) and np.array_equal(got[1], pose_cost) and (summary[:, 3] != U).sum() >= 8
    m.release()


def _hold_field_drive(f, want, res, what):
    cost, direction, cell = f.copy_to_host()
    assert f.origin_cells == tuple(want["E"]), what
    _equal(cell, want["c"], what + ", cell_cost")
    _equal(cost, want["D"], what + ", cost")
    _equal(direction, want["dir"], what + ", direction")
    assert (f.converged, f.reached, f.goals_seeded) == (True,) + tuple(want["info"]), what


def test_the_pool_the_capacity_and_the_errors(gvom, handles):
    xy, A = 16, 64
    g = handles[xy]
    lib, h = g._lib, g._h
    ref, steps = afr.scenario(xy, A, True)
    assert g.get_tuning("atlas_cost_to_go") == 1
    a = g.create_atlas(A)
    _paint(a, steps)
    want = afr.expected(xy, A, True, 2)
    goals, kw = np.array(want["goals_world"]), afr.keywords(want["params"])
    a.cost_to_go(goals, goals_in_cells=True, **kw).window(origin_cells=steps[0][1]).release()
    allocs = g.get_tuning("atlas_field_allocations")
    assert allocs >= 3                                                  # a field, the solver's buffers, a window
    for k in range(20):
        with a.cost_to_go(goals, goals_in_cells=True, **kw) as f:
            if k == 19:
                _hold_field(f, want, "the twentieth call")
            f.window(origin_cells=steps[k % len(steps)][1]).release()
    assert g.get_tuning("atlas_field_allocations") == allocs
    held = [a.cost_to_go(goals, goals_in_cells=True, **kw) for _ in range(4)]          # GVOM_MAX_PRODUCT_SETS
    with pytest.raises(gvom.GvomBackendError, match="all 4 device product sets"):
        a.cost_to_go(goals, goals_in_cells=True, **kw)
    stale = held.pop()
    stale.release()
    a.cost_to_go(goals, goals_in_cells=True, **kw).release()            # a release frees one (and recycles it: the old id is stale)
    with pytest.raises(ValueError, match="stale atlas field id"):
        stale.window(origin_cells=(0, 0))
    f = held[0]
    with a.recall() as m:
        I64 = ctypes.c_int64
        pid, org = I64(-1), (I64 * 2)(0, 0)
        assert lib.gvom_atlas_field_window(h, f.product_id, m.set_id, org, ctypes.byref(pid)) == gvom.GVOM_ERR_INVALID and b"not both" in lib.gvom_last_error(h)
        assert lib.gvom_atlas_field_window(h, f.product_id, -1, None, ctypes.byref(pid)) == gvom.GVOM_ERR_INVALID
        assert lib.gvom_atlas_field_window(h, f.product_id, -1, org, None) == gvom.GVOM_ERR_INVALID
        assert lib.gvom_atlas_field_window(h, 1 << 40, -1, org, ctypes.byref(pid)) == gvom.GVOM_ERR_INVALID
        assert lib.gvom_atlas_field_window(h, f.product_id, 1 << 40, None, ctypes.byref(pid)) == gvom.GVOM_ERR_INVALID and b"stale" in lib.gvom_last_error(h)
        far = (I64 * 2)((1 << 40) + 1, 0)
        assert lib.gvom_atlas_field_window(h, f.product_id, -1, far, ctypes.byref(pid)) == gvom.GVOM_ERR_INVALID
        with pytest.raises(ValueError):
            f.window()
        with pytest.raises(ValueError):
            f.window(m, origin_cells=(0, 0))
        m.stamps.release()
    P = gvom.GvomCtgParams(50.0, 0.0, 0.0, 0, 1, 0, 0, 0)
    gw = np.array(goals[:1], np.int64)                                 # (a copy: it is written below)
    gp = gw.ctypes.data_as(ctypes.POINTER(I64))
    info, e = (I64 * 4)(), (I64 * 2)()
    raw = lambda params=ctypes.byref(P), goals=gp, n=1, max_cost=0, max_rounds=0, flags=0, out=ctypes.byref(pid): lib.gvom_atlas_cost_to_go(
        h, params, goals, n, max_cost, max_rounds, flags, out, info, e)
    for bad in (dict(flags=4), dict(params=None), dict(goals=None), dict(n=0), dict(n=65537), dict(max_cost=-1), dict(max_cost=2 ** 30 + 1),
                dict(max_rounds=-1), dict(out=None)):
        assert raw(**bad) == gvom.GVOM_ERR_INVALID, bad
    assert raw(flags=4) == gvom.GVOM_ERR_INVALID and b"unknown flag bits" in lib.gvom_last_error(h)
    for field, value in (("density_threshold", float("nan")), ("base", 0), ("soft_weight", 65536), ("inflation_cells2", -1)):
        badp = gvom.GvomCtgParams(50.0, 0.0, 0.0, 0, 1, 0, 0, 0)
        setattr(badp, field, value)
        assert raw(params=ctypes.byref(badp)) == gvom.GVOM_ERR_INVALID and b"bad cost parameters" in lib.gvom_last_error(h)
    E = a.extent_origin
    for out in ((E[0] - 1, E[1]), (E[0] + A, E[1]), (E[0], E[1] - 1), (E[0], E[1] + A)):
        gw[0] = out
        assert raw() == gvom.GVOM_ERR_INVALID and b"outside the extent" in lib.gvom_last_error(h), out
        with pytest.raises(ValueError, match=r"outside the extent: cell \(%d, %d\), extent" % out):
            a.cost_to_go([out], goals_in_cells=True)
    with pytest.raises(gvom.GvomBackendError, match="unknown product kind"):
        g._device_product(gvom.PRODUCT_ATLAS_FIELD)
    for x in held:
        x.release()
    # a field outlives the atlas; without an atlas there is no new one
    f = a.cost_to_go(goals, goals_in_cells=True, **kw)
    a.release()
    _hold_field(f, want, "after the atlas is gone")
    _hold_window(f.window(origin_cells=steps[0][1]), afr.window(want, steps[0][1], xy), steps[0][1], "after the atlas is gone")
    f.release()
    gw[0] = goals[0]
    assert raw() == gvom.GVOM_ERR_INVALID and b"no atlas is configured" in lib.gvom_last_error(h)
    s = gvom.Gvom(*_params(64), voxel_statistics=False, _shard=(0, 2))
    assert s._lib.gvom_atlas_cost_to_go(s._h, ctypes.byref(P), gp, 1, 0, 0, 0, ctypes.byref(pid), info, e) == gvom.GVOM_ERR_INVALID
    assert b"sharded" in s._lib.gvom_last_error(s._h)
    assert s._lib.gvom_atlas_field_window(s._h, 1, -1, org, ctypes.byref(pid)) == gvom.GVOM_ERR_INVALID


def test_an_atlas_of_4096_cells(gvom, handles):
    """one call on an atlas of 4096 cells that holds one integrated set, a goal inside it, no inflation, unknown="blocked": nothing
    outside the set is reachable, so the crop at the set's origin equals the recalled set's own cost_to_go()"""
    g, A, xy = handles[64], 4096, 64
    a = g.create_atlas(A)
    try:
        o = (-30, 4090)                                                  # across the storage seam in x and in y
        s = afr.terrain_set(np.random.default_rng(4096), xy)
        a.integrate_of([m.T for m in s], o)
        x, y = afr.well_connected(afr.cell_costs(s[0].T, s[1].T, s[2].T, s[3].T, afr.params(unknown="blocked")))
        goal = (o[0] + x, o[1] + y)
        kw = dict(unknown="blocked", soft_weight=3, rough_weight=5, roughness_range=afr.ROUGHNESS_RANGE)
        with a.recall(origin_cells=o) as m, a.cost_to_go([goal], goals_in_cells=True, **kw) as f:
            assert f.cost.shape == (A, A) and f.converged and f.goals_seeded == 1
            with m.cost_to_go([(int(x), int(y))], goals_in_cells=True, **kw) as local:
                want = local.copy_to_host()
                assert (f.reached, f.goals_seeded) == (local.reached, local.goals_seeded) and local.reached > 100
            _hold_window(f.window(m), want, o, "4096")
            outside = (o[0] - xy, o[1])
            _hold_window(f.window(origin_cells=outside), (np.full((xy, xy), U, np.int32), np.full((xy, xy), cf.NONE, np.uint8), np.zeros((xy, xy), np.uint16)),
                         outside, "4096, beside the set")
            print("A 4096: rounds", f.rounds, "tile relaxations", g.get_tuning("atlas_field_tiles"), "reached", f.reached)
            m.stamps.release()
    finally:
        a.release()
