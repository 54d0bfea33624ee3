"""The voxel atlas's change query on the GPU (gvom_voxel_atlas_changes: gvom_voxel_changes.hip; VoxelAtlas.changes, DeviceVoxelChanges)
against the referee of tests/voxel_changes_ref.py, which is fed with the dense fused states the SAME handle returns
(read_dense(GVOM_WHICH_FUSED)): it referees the query, not the mapper.  Tolerance 0: all seven parts, every element.

  the scene          the hand-placed scene of the referee module, every mask, min_cells 1 / 2 / 4, max_clusters 1 / 2 / 1024
  the drive          tests/voxel_atlas_ref.py's climbing drive, rings of 1 and 2, following and fixed: changes() before every integrate,
                     and its totals against the counts of the integrate that follows
  grids              not a multiple of 64, taller than wide, three segments, more rows than waves; the atlas off the pair grid
  read-only          boxes and counts before and after; a scan without a combine
  housekeeping       no data, a fresh atlas, refusals, the pool, allocations, DLPack (a child process with torch)"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import raycast_ref as rr
import viewpoint_ref  # noqa: F401  (registers the grid "v256" with raycast_ref)
import voxel_atlas_ref as va
import voxel_changes_ref as vc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GVOM_ERR_INVALID, GVOM_ERR_CAPACITY, GVOM_NO_DATA = -1, -4, 4


@pytest.fixture(scope="module")
def gvom():
    import gvom as mod
    rc, info = mod.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    return mod


def _dense(gvom):
    def read(g):
        state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
        return state, tuple(int(v) for v in origin)
    return read


def _hold(ch, ref, state, W, mask, min_cells, cap, what):
    """the product `ch` of changes(mask, min_cells, cap) against the referee on (ref, state, W); returns the parts"""
    want, info = vc.product(ref, state, W, mask, min_cells, cap)
    with ch:
        assert tuple(ch.origin_voxels) == tuple(int(v) for v in W), what
        assert (ch.n_clusters, ch.marked_columns, ch.dropped) == tuple(info) and ch.rounds >= 1, (what, ch.n_clusters, ch.marked_columns, ch.dropped, info)
        got = ch.copy_to_host()
    bad = vc.differing_parts(got, want)
    assert not bad, "%s: parts %r differ; part 3 %r, referee %r" % (what, bad, list(got[3]), list(want[3]))
    return got


def _changes(atlas, mask, min_cells, cap):
    return atlas.changes(appeared=bool(mask & 1), vanished=bool(mask & 2), min_cells=min_cells, max_clusters=cap)


# ---- 1. the hand-placed scene --------------------------------------------------------------------------------------------------------------
def test_the_hand_placed_scene_equals_the_referee_in_every_part(gvom):
    g = gvom.Gvom(*vc.scene_params(), voxel_statistics=False)
    atlas = g.create_voxel_atlas(va.DRIVE_A, va.DRIVE_Z)
    ref = va.VoxelAtlasRef(va.DRIVE_A, va.DRIVE_Z, va.DRIVE_XY, va.DRIVE_ZS)

    def between(state, W):
        assert atlas.integrate() is True
        ref.integrate(state, W)
    state, W = vc.run_scene(g, _dense(gvom), between)
    maps = {}
    for mask in (1, 2, 3):
        for min_cells in (1, 2, 4):
            for cap in (1, 2, 1024):
                got = _hold(_changes(atlas, mask, min_cells, cap), ref, state, W, mask, min_cells, cap, "mask %d min_cells %d cap %d" % (mask, min_cells, cap))
                maps[mask, min_cells, cap] = got[2]
    census = vc.census(*vc.product(ref, state, W, 3, 2, 1024))
    print(census)
    assert census["with_appeared"] >= 3 and census["with_vanished"] >= 3 and census["with_both"] >= 1 and census["dropped"] >= 1
    assert census["across_tiles"] >= 1 and census["nearest_is_not_label"] >= 1 and census["kept"] > 2
    assert not np.array_equal(maps[1, 2, 1024], maps[3, 2, 1024]) and not np.array_equal(maps[2, 2, 1024], maps[3, 2, 1024])
    # the clusters on the host, in world metres
    with atlas.changes() as ch:
        c, (rows, sums, _, counts, rows4, _, _) = ch.clusters(), ch.copy_to_host()
    n = int(counts[0])
    res, zres = va.DRIVE_RES[0], va.DRIVE_RES[2]
    assert len(c["label"]) == n and np.array_equal(c["columns"], rows[:n, 1]) and np.array_equal(c["appeared"], rows4[:n, 0])
    assert np.array_equal(c["vanished"], rows4[:n, 1]) and np.array_equal(c["box"], rows[:n, 2:6]) and np.array_equal(c["levels"], rows4[:n, 2:4])
    assert np.allclose(c["centroid"], (sums[:n] / rows[:n, 1:2] + np.array(W[:2]) + 0.5) * res, rtol=0, atol=1e-12)
    near = np.stack([rows[:n, 6] % va.DRIVE_XY, rows[:n, 6] // va.DRIVE_XY], axis=1)
    assert np.allclose(c["nearest"], (near + np.array(W[:2]) + 0.5) * res, rtol=0, atol=1e-12)
    assert np.allclose(c["z_range"], (rows4[:n, 2:4] + W[2] + np.array([0, 1])) * zres, rtol=0, atol=1e-12)


# ---- 2. the climbing drive -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("follow", [True, False])
@pytest.mark.parametrize("ring", [1, 2])
def test_the_drive_changes_equal_the_referee_before_every_integrate(gvom, ring, follow):
    g = gvom.Gvom(*(va.DRIVE_PARAMS + (ring,) + va.DRIVE_TAIL), voxel_statistics=False)
    kw = dict(follow=True) if follow else dict(follow=False, origin_voxels=np.array(va.fixed_origin()))
    atlas = g.create_voxel_atlas(va.DRIVE_A, va.DRIVE_Z, **kw)
    ref = va.VoxelAtlasRef(va.DRIVE_A, va.DRIVE_Z, va.DRIVE_XY, va.DRIVE_ZS, follow=follow, origin=(0, 0, 0) if follow else va.fixed_origin())
    read = _dense(gvom)
    sides = (va.DRIVE_A, va.DRIVE_A, va.DRIVE_Z)
    seams, compared, totals = [0, 0, 0], 0, np.zeros(3, np.int64)
    partly = wholly = 0
    for k, (pc, ego) in enumerate(va.drive_scans()):
        g.process_pointcloud(pc, ego)
        g.combine_maps()
        state, W = read(g)
        mask, min_cells, cap = 1 + k % 3, 1 + k % 2, (1024, 3)[k % 2]
        E_before = ref.E
        got = _hold(_changes(atlas, mask, min_cells, cap), ref, state, W, mask, min_cells, cap, "ring %d follow %d scan %d" % (ring, follow, k))
        part3 = got[3].astype(np.int64)
        totals += part3[4:7]
        for axis in range(3):                                               # the window lies on both sides of the storage seam of this axis
            lo = W[axis] & (sides[axis] - 1)
            seams[axis] += int(lo + (va.DRIVE_XY, va.DRIVE_XY, va.DRIVE_ZS)[axis] > sides[axis])
        voxels = va.DRIVE_XY ** 2 * va.DRIVE_ZS
        partly += int(0 < part3[6] < voxels); wholly += int(part3[6] == voxels)
        assert atlas.integrate() is True
        ref.integrate(state, W)
        counts = atlas.counts()
        assert counts == ref.counts()
        whole_side = any(abs(ref.E[a] - E_before[a]) >= sides[a] for a in range(3))
        if not whole_side:
            assert (part3[4], part3[5]) == (counts["free_to_occupied"], counts["occupied_to_free"]), (k, list(part3), counts)
            compared += 1
        if not follow:
            assert part3[6] == counts["outside"], (k, list(part3), counts)
    if not follow:                                                          # the drive's windows cross the extent's edge; this one lies wholly outside it
        pc, ego = va.drive_scans()[0]
        far = np.array([200 * va.DRIVE_RES[0], 0.0, 0.0], np.float32)
        g.process_pointcloud(np.ascontiguousarray(np.asarray(pc, np.float32) + far), (ego[0] + float(far[0]), ego[1], ego[2]))
        g.combine_maps()
        state, W = read(g)
        got = _hold(_changes(atlas, 3, 1, 1024), ref, state, W, 3, 1, 1024, "ring %d, a window wholly outside the extent" % ring)
        wholly += int(got[3][6] == va.DRIVE_XY ** 2 * va.DRIVE_ZS)
        assert got[3][1] == 0 and not got[5].any()
    print(ring, follow, list(totals), seams, compared, partly, wholly)
    assert compared >= 16 and totals[0] > 0 and totals[1] > 0 and min(seams) >= 1
    if not follow:
        assert totals[2] > 0 and partly >= 1 and wholly == 1


# ---- 3. grids ------------------------------------------------------------------------------------------------------------------------------
def _atlas_sides(xy, zs):
    A = 64
    while A < xy or A < zs:
        A *= 2
    Z = 1
    while Z < zs:
        Z *= 2
    return A, Z


@pytest.mark.parametrize("grid", ["np2", "tall", "w192", "v256"])           # not a multiple of 64; taller than wide; three segments; more rows than waves
def test_grids_off_the_pair_grid_equal_the_referee(gvom, grid):
    xr, zr, xy, zs = rr.GRIDS[grid]
    g = rr.build_map(gvom.Gvom, grid, 2, voxel_statistics=False)
    read = _dense(gvom)
    state, W = read(g)
    A, Z = _atlas_sides(xy, zs)
    room = [(A, A, Z)[k] - (xy, xy, zs)[k] for k in range(3)]                  # the window lies inside the extent, off its middle where there is room
    E = tuple(int(W[k]) - min(room[k], room[k] // 2 + (3, 1, 0)[k]) for k in range(3))
    assert (E[0] - W[0]) % 64 != 0 or room[0] == 0
    atlas = g.create_voxel_atlas(A, Z, follow=False, origin_voxels=np.array(E))
    ref = va.VoxelAtlasRef(A, Z, xy, zs, follow=False, origin=E)
    assert atlas.integrate()
    ref.integrate(state, W)
    g.process_pointcloud(rr.cloud_of(grid, rr.N_SCANS), rr.ego_of(grid, rr.N_SCANS))
    g.combine_maps()
    state, W1 = read(g)
    assert W1 != W
    for mask, min_cells, cap in ((3, 1, 1024), (1, 2, 5), (2, 3, 1024)):
        got = _hold(_changes(atlas, mask, min_cells, cap), ref, state, W1, mask, min_cells, cap, "%s mask %d" % (grid, mask))
    print(grid, list(got[3]))
    assert got[3][4] + got[3][5] > 0


# ---- 4. read-only --------------------------------------------------------------------------------------------------------------------------
def test_changes_reads_and_a_scan_without_a_combine_changes_nothing(gvom):
    grid = "np2"
    xr, zr, xy, zs = rr.GRIDS[grid]
    g = rr.build_map(gvom.Gvom, grid, 2, voxel_statistics=False)
    read = _dense(gvom)
    state0, W0 = read(g)
    atlas = g.create_voxel_atlas(64, 32)
    assert atlas.integrate()
    g.process_pointcloud(rr.cloud_of(grid, rr.N_SCANS), rr.ego_of(grid, rr.N_SCANS))
    g.combine_maps()
    _, W1 = read(g)
    origins = (np.array(W0), np.array([W1[0] - 5, W1[1] + 3, W1[2] + 1]))

    def snapshot():
        out = [atlas.counts()]
        for o in origins:
            with atlas.box(o) as box:
                out += list(box.copy_to_host())
        return out
    before = snapshot()
    with atlas.changes() as ch:
        first = ch.copy_to_host()
    after = snapshot()
    assert before[0] == after[0] and all(np.array_equal(a, b) for a, b in zip(before[1:], after[1:]))
    assert first[3][4] + first[3][5] > 0                                    # there was something to report
    g.process_pointcloud(rr.cloud_of(grid, rr.N_SCANS + 1), rr.ego_of(grid, rr.N_SCANS + 1))     # accepted, not combined
    with atlas.changes() as ch:
        second = ch.copy_to_host()
        assert tuple(ch.origin_voxels) == W1
    assert not vc.differing_parts(second, first)
    assert snapshot()[0] == before[0]


# ---- 5. housekeeping -----------------------------------------------------------------------------------------------------------------------
def test_no_data_a_fresh_atlas_and_the_refusals(gvom):
    g = gvom.Gvom(*rr.params("tall", 1), voxel_statistics=False)               # xy 16, z 32
    L, h = g._lib, g._h
    pid, out3, info = ctypes.c_int64(-1), (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 4)()

    def call(mask=3, min_cells=2, cap=16, out=pid):
        return L.gvom_voxel_atlas_changes(h, mask, min_cells, cap, ctypes.byref(out) if out is not None else None, out3, info)
    assert g.get_tuning("voxel_changes") == 1
    assert call() == GVOM_ERR_INVALID and b"no voxel atlas" in L.gvom_last_error(h)
    atlas = g.create_voxel_atlas(64, 32)
    assert call() == GVOM_NO_DATA and pid.value == -1 and atlas.changes() is None      # before the first combine
    g.process_pointcloud(rr.cloud_of("tall", 0), rr.ego_of("tall", 0))
    assert atlas.changes() is None                                                      # scanned, not combined
    g.combine_maps()
    with atlas.changes(min_cells=1) as ch:                                              # never integrated: valid, no change
        parts = ch.copy_to_host()
        assert (ch.n_clusters, ch.marked_columns, ch.dropped) == (0, 0, 0)
    state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
    xr, zr, xy, zs = rr.GRIDS["tall"]
    fresh = va.VoxelAtlasRef(64, 32, xy, zs)                                            # its extent still at (0, 0, 0): part of the window lies outside
    outside = vc.codes(fresh, state, tuple(int(v) for v in origin))[1]
    assert list(parts[3]) == [0, 0, 0, 1024, 0, 0, outside, 0] and not parts[5].any() and not parts[6].any() and (parts[2] == -1).all()
    assert not parts[0].any() and not parts[1].any() and not parts[4].any()
    assert call() == 0 and pid.value > 0 and tuple(out3) == tuple(int(v) for v in g.read_dense(gvom.GVOM_WHICH_FUSED)[4])
    for kw in (dict(mask=0), dict(mask=4), dict(mask=-1), dict(min_cells=0), dict(cap=0), dict(cap=(1 << 20) + 1), dict(out=None)):
        assert call(**kw) == GVOM_ERR_INVALID, kw
    assert call(mask=0) == GVOM_ERR_INVALID and b"mask" in L.gvom_last_error(h) and pid.value == -1
    assert L.gvom_device_product(h, 48, 0, ctypes.byref(pid)) == GVOM_ERR_INVALID and L.gvom_device_product(h, 47, 0, ctypes.byref(pid)) == GVOM_ERR_INVALID
    with pytest.raises(ValueError):
        atlas.changes(appeared=False, vanished=False)
    with pytest.raises(ValueError):
        atlas.changes(min_cells=0)
    # a window at or beyond 2^30 voxels
    xr, zr, xy, zs = rr.GRIDS["tall"]
    ego = [((1 << 30) + 64) * xr, 0.0, 0.0]
    pc = np.array(ego) + np.random.default_rng(5).uniform(-0.4, 0.4, (384, 3)) * np.array([xr * xy, xr * xy, zr * zs])
    g.process_pointcloud(pc, tuple(ego))
    g.combine_maps()
    assert call() == GVOM_ERR_INVALID and b"2^30" in L.gvom_last_error(h)
    sharded = gvom.Gvom(*rr.params("tall", 1), voxel_statistics=False, _shard=(0, 1))
    assert sharded._lib.gvom_voxel_atlas_changes(sharded._h, 3, 2, 16, ctypes.byref(pid), None, None) == GVOM_ERR_INVALID
    assert b"sharded" in sharded._lib.gvom_last_error(sharded._h)


def test_the_pool_and_steady_allocations(gvom):
    grid = "np2"
    g = rr.build_map(gvom.Gvom, grid, 1, voxel_statistics=False)
    atlas = g.create_voxel_atlas(64, 32)
    assert atlas.integrate()
    pc, ego = rr.cloud_of(grid, rr.N_SCANS), rr.ego_of(grid, rr.N_SCANS)
    g.process_pointcloud(pc, ego)
    g.combine_maps()
    with atlas.changes() as ch:
        ptr, want = ch.codes.ptr, ch.copy_to_host()
    allocs, sets = g.get_tuning("voxel_atlas_allocations"), g.get_tuning("device_product_sets")
    for _ in range(20):                                                     # steady state: an unexported set goes back to the pool
        with atlas.changes() as ch:
            assert ch.codes.ptr == ptr
    assert g.get_tuning("voxel_atlas_allocations") == allocs and g.get_tuning("device_product_sets") == sets
    held = [atlas.changes() for _ in range(4)]
    assert len({c.codes.ptr for c in held}) == 4
    with pytest.raises(gvom.GvomBackendError, match="exported"):
        atlas.changes()                                                     # the fifth product of the kind while four are held
    assert not vc.differing_parts(held[3].copy_to_host(), want)
    held.pop().release()
    atlas.changes().release()
    for c in held:
        c.release()
    sets = g.get_tuning("device_product_sets")
    atlas.changes(max_clusters=7).release()                                 # another cap, a smaller set: reused
    assert g.get_tuning("device_product_sets") == sets


def test_a_torch_consumer_reads_the_codes_through_dlpack():
    """One case in a fresh child process that imports torch BEFORE the library is loaded (one HIP runtime in the process)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_voxel_changes_torch.py"), "consumer"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "CASE OK consumer" in r.stdout, r.stdout[-4000:]
