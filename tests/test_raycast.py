"""Ray queries on the GPU (gvom_raycast: k_raycast; Gvom.raycast, Gvom.raycast_device, DeviceRays) against the numpy referee of
tests/raycast_ref.py: part 0 {status, steps, voxel, unknown} with tolerance 0, part 1 (the stop position) bit for bit, NaNs
included.  The referee walks the dense fused state the SAME handle returns (read_dense(GVOM_WHICH_FUSED)) after four scans of a
moving ego: the three grids of tests/multi_origin_ref.py (power of two, no power of two, taller than wide), buffer_size 1 (the
adopted eager fusion) and 2 (k_fuse); 1, 63, 65 and 4,096 rays, one origin and one per ray, host and device inputs, the four flag
combinations.  Then: self-consistency with the scan that made the map, snapshots, the product pool, errors, and a torch consumer
in a child process.  tests/test_raycast_cpu.py holds the census floors of the inputs on the CPU referee; they are asserted again
here on the GPU's own maps.  Also: two grids of 128 and 192 cells (2 and 3 tile segments per storage row: tests/raycast_ref.py
WIDE), whose dense state is held to the oracle first, and the np2 grid with its window origin beyond 2^24 voxels (FAR).

Wall time on the MI355X (pytest --durations, one run): the six cases of test_rays_match_the_referee_exactly 0.03 to 0.05 s each
(module fixture 0.5 s); the four wide-grid cases 0.15 to 0.19 s each (their fixture, which also builds the far maps, 0.23 s);
the two far cases 0.04 s each, the far self-consistency check 0.02 s.  One case (np2, ring length 1) runs once more with the
"fastdiv" knob at 0, so that k_raycast's IEEE divides are executed too (0.04 s)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import raycast_ref as rr
from multi_origin_ref import GRIDS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = [(False, False), (True, False), (False, True), (True, True)]       # (unknown_blocks, check_target)
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
        a = np.ascontiguousarray(a, np.float32)
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


def _build_maps(gvom, grids):
    out = {}
    for grid in sorted(grids):
        xr, zr, xy, zs = rr.GRIDS[grid]
        for bs in (1, 2):
            g = rr.build_map(gvom.Gvom, grid, bs, voxel_statistics=False)
            assert (g.get_tuning("fuse_kernel") == 6) == (bs == 1)          # 6: an adopted k_encfuse; else k_fuse*
            state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
            W = rr.window_origin(grid, rr.ego_of(grid, rr.N_SCANS - 1))
            assert np.array_equal(np.asarray(origin, np.float64), W)
            assert all(int(W[k]) % (xy if k < 2 else zs) != 0 for k in range(3)), W      # non-zero storage offsets on every axis
            out[grid, bs] = (g, state, W, rr.rays_of(grid, state, W))
    return out


@pytest.fixture(scope="module")
def maps(gvom):
    """per (grid, buffer_size): (handle, dense fused state, window origin, rays) -- built once, never changed"""
    return _build_maps(gvom, GRIDS)


@pytest.fixture(scope="module")
def wide_maps(gvom):
    """the same on the grids of more than one tile segment and on the far-origin grid (tests/raycast_ref.py WIDE, FAR)"""
    return _build_maps(gvom, list(rr.WIDE) + list(rr.FAR))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _hold(rays, want, W, what):
    with rays:
        assert np.array_equal(rays.origin, W), what
        result, position = rays.copy_to_host()
    wr, wp = want
    assert result.dtype == np.int32 and position.dtype == np.float32 and result.shape == wr.shape and position.shape == wp.shape, what
    if not np.array_equal(result, wr):
        bad = np.flatnonzero((result != wr).any(axis=1))
        raise AssertionError("%s: %d rays differ, first %d: got %r, referee %r" % (what, len(bad), bad[0], result[bad[0]], wr[bad[0]]))
    same = (_bits(position) == _bits(wp)) | (np.isnan(position) & np.isnan(wp))
    assert same.all(), "%s: %d positions differ, first ray %d: got %r, referee %r" % (
        what, int((~same).any(axis=1).sum()), np.flatnonzero((~same).any(axis=1))[0], position[~same][:3], wp[~same][:3])
    assert np.array_equal(np.isnan(position), np.isnan(wp)), what
    return result, position


@pytest.mark.parametrize("bs", [1, 2])
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_rays_match_the_referee_exactly(maps, hip, grid, bs):
    _rays_match_the_referee(maps, hip, grid, bs)


def test_rays_match_the_referee_exactly_with_the_ieee_divide(maps, hip):
    """the np2, ring length 1 case once more with the "fastdiv" knob at 0: k_raycast's `P.fastdiv &` branches take the IEEE divide
    instead of the verified reciprocal, and the answers are held to the same referee (which divides)"""
    g = maps["np2", 1][0]
    assert g.get_tuning("fastdiv") == 3
    try:
        g.set_tuning("fastdiv", 0)
        assert g.get_tuning("fastdiv") == 0
        _rays_match_the_referee(maps, hip, "np2", 1)
    finally:
        g.set_tuning("fastdiv", -1)                            # as created: the maps are shared
    assert g.get_tuning("fastdiv") == 3


def _rays_match_the_referee(maps, hip, grid, bs):
    g, state, W, (A, B, fam) = maps[grid, bs]
    # 1, 63, 65 rays: a spread over all families (the 4,096 are the whole input)
    picks = {n: (np.arange(n) * rr.N_RAYS) // n + (7 if n > 1 else 2050) for n in (1, 63, 65)}
    picks[rr.N_RAYS] = np.arange(rr.N_RAYS)
    calls = 0
    for n, pick in picks.items():
        a, b = np.ascontiguousarray(A[pick]), np.ascontiguousarray(B[pick])
        dev = {}
        for ub, ct in FLAGS:
            for one in (True, False):
                o = a[:1] if one else a
                want = rr.walk(state, W, grid, o, b, unknown_blocks=ub, check_target=ct)
                what = "%s, buffer %d, n %d, K %s, flags %d%d" % (grid, bs, n, "1" if one else "n", ub, ct)
                res, _ = _hold(g.raycast(o[0] if (one and ub) else o, b, unknown_blocks=ub, check_target=ct), want, W, what + ", host")
                if n in (65, rr.N_RAYS):
                    if not dev:
                        dev = {"a": hip.upload(a), "b": hip.upload(b)}
                    _hold(g.raycast_device(dev["a"], 1 if one else n, dev["b"], n, unknown_blocks=ub, check_target=ct), want, W, what + ", device")
                calls += 1
                if n == rr.N_RAYS and not one and (ub, ct) == (rr.CENSUS_FLAGS["unknown_blocks"], rr.CENSUS_FLAGS["check_target"]):
                    per_status, at8, at4 = rr.census(res)                    # the census, on the GPU's own map and answer
                    print(grid, bs, per_status, at8, at4)
                    assert min(per_status) >= rr.STATUS_FLOOR, per_status
                    step, floor = rr.STEP_FLOOR[grid]
                    assert (at8 if step == 8 else at4) >= floor, (at8, at4)
                    assert (res[fam == 4, 0] == rr.INVALID).all() and (res[fam == 2, 3] == 0).all()
    assert calls == 32


def _all_routes(g, hip, state, W, grid, A, B, what):
    """the 4,096 rays under the four flag combinations, one origin and one per ray, host and device inputs: every answer equals the
    referee's; returns the answer of the census call"""
    dev = {"a": hip.upload(A), "b": hip.upload(B)}
    census = None
    for ub, ct in FLAGS:
        for one in (True, False):
            o = A[:1] if one else A
            want = rr.walk(state, W, grid, o, B, unknown_blocks=ub, check_target=ct)
            w = "%s, K %s, flags %d%d" % (what, "1" if one else "n", ub, ct)
            res, _ = _hold(g.raycast(o[0] if (one and ub) else o, B, unknown_blocks=ub, check_target=ct), want, W, w + ", host")
            _hold(g.raycast_device(dev["a"], 1 if one else len(B), dev["b"], len(B), unknown_blocks=ub, check_target=ct), want, W, w + ", device")
            if not one and (ub, ct) == (rr.CENSUS_FLAGS["unknown_blocks"], rr.CENSUS_FLAGS["check_target"]):
                census = res
    return census


@pytest.mark.parametrize("bs", [1, 2])
@pytest.mark.parametrize("grid", sorted(rr.WIDE))
def test_rays_on_maps_of_several_tile_segments_match_the_referee_exactly(wide_maps, hip, grid, bs):
    """128 and 192 cells wide: 2 and 3 tile segments per storage row, so that the tile index of k_raycast (row * nseg + (sx >> 6))
    is held for storage columns 64 and up.  The dense state the referee walks comes from the same handle (k_read_dense, which has
    its own tile index); it is first held, class by class, to an oracle mapper fed the same scans, so that an error the two
    kernels share cannot cancel.  Then the census: every status, stops in every storage segment, rays that cross a segment
    boundary -- on the GPU's own map and answer.  (With sx >> 6 replaced by 0 in a scratch build this test fails on both grids
    and both buffer sizes while the three narrow grids and the far grid pass: DESIGN.md 9.5.)"""
    from oracle import oracle
    g, state, W, (A, B, fam) = wide_maps[grid, bs]
    o = rr.build_map(oracle.OracleGvom, grid, bs)
    assert np.array_equal(np.asarray(o.combined_origin, np.float64), W)
    got, want = rr.state_class(state), rr.state_class(np.asarray(o.combined_index_map))
    assert np.array_equal(got, want), "%s, buffer %d: %d voxels differ from the oracle in their class, first %d: %d, oracle %d" % (
        grid, bs, int((got != want).sum()), np.flatnonzero(got != want)[0], got[got != want][0], want[got != want][0])
    assert min(np.bincount(got, minlength=3)) >= 64
    res = _all_routes(g, hip, state, W, grid, A, B, "%s, buffer %d" % (grid, bs))
    per_status, at8, at4 = rr.census(res)
    _, _, visits = rr.walk(state, W, grid, A, B, record=True, **rr.CENSUS_FLAGS)       # (res IS this walk's result: held above)
    stops, crossing = rr.segment_census(res, visits, W, grid)
    print(grid, bs, per_status, at8, at4, stops, crossing)
    assert min(per_status) >= rr.STATUS_FLOOR, per_status
    assert rr.STEP_FLOOR[grid][0] == 8 and at8 >= rr.STEP_FLOOR[grid][1], at8
    assert len(stops) == (rr.GRIDS[grid][2] + 63) // 64 >= 2 and min(stops) >= rr.SEGMENT_STOP_FLOOR, stops
    assert crossing >= rr.SEGMENT_CROSS_FLOOR, crossing
    assert (res[fam == 4, 0] == rr.INVALID).all() and (res[fam == 2, 3] == 0).all()


@pytest.mark.parametrize("bs", [1, 2])
def test_rays_far_from_the_world_origin_match_the_referee_exactly(wide_maps, hip, bs):
    """every axis of the window origin beyond 2^24 voxels (tests/raycast_ref.py FAR): gvom_raycast switches to the literal float64
    lookup (Q.lit) on a grid that otherwise takes the integer one.  Out there a float32 voxel coordinate has a spacing of 2: most
    steps do not move the position at all -- the reference's arithmetic, which the referee and the kernel share bit for bit"""
    g, state, W, (A, B, fam) = wide_maps["far", bs]
    assert (np.abs(W) >= 2.0 ** 24).all() and (W > 0).any() and (W < 0).any(), W
    res = _all_routes(g, hip, state, W, "far", A, B, "far, buffer %d" % bs)
    per_status, _, _ = rr.census(res)
    print("far", bs, per_status)
    assert min(per_status) >= rr.STATUS_FLOOR, per_status


def test_float64_inputs_are_rounded_to_float32_and_lists_are_taken(maps):
    g, state, W, (A, B, fam) = maps["np2", 2]
    a64, b64 = A[:300].astype(np.float64) + 1e-9, B[:300].astype(np.float64) + 1e-9
    want = rr.walk(state, W, "np2", a64.astype(np.float32), b64.astype(np.float32))
    _hold(g.raycast(a64, b64), want, W, "float64 arrays")
    _hold(g.raycast(np.asfortranarray(a64), b64[::1].tolist()), want, W, "Fortran order, nested lists")


def test_numba_cuda_typing_changes_the_step_rule_as_in_the_scan(gvom):
    """GVOM_FLAG_CUDA_F32_SQRT: the ray length is the float32 square root, in the query as in the scan"""
    grid = "p2"
    g = rr.build_map(gvom.Gvom, grid, 1, voxel_statistics=False, numba_cuda_typing=True)
    state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
    W = np.asarray(origin, np.float64)
    A, B, fam = rr.rays_of(grid, state, W)
    for ub, ct in FLAGS:
        _hold(g.raycast(A, B, unknown_blocks=ub, check_target=ct), rr.walk(state, W, grid, A, B, ub, ct, f32_sqrt=True), W, "f32 sqrt %d%d" % (ub, ct))
    p, inc, S32 = rr.setup(grid, A[fam != 4], B[fam != 4], True)
    p, inc, S64 = rr.setup(grid, A[fam != 4], B[fam != 4], False)
    print("rays whose step count depends on the typing:", int((S32 != S64).sum()))


def _scan_and_own_rays(gvom, grid):
    """Independent of the referee: ONE scan with a float32-representable ego into an empty one-slot map, then combine.  The rays
    from the ego to every return that passes min_distance walk exactly the voxels the scan marked: none of them is unknown, and a
    ray whose return lies inside the window ends OCCUPIED or CLEAR -- with the one exception the reference's step rule makes: the
    loop runs while length < ray_length - 1 and adds |1 / slope| >= 1 per step, so its last sample may lie up to one step BEHIND the
    return, and for a return in the outermost voxel layer of the window that sample can be outside (k_trace's ray ends there the
    same way).  Such a ray is LEFT_WINDOW: on the CPU referee 1 of 5,492 in-window returns on np2, none on p2 and tall.  The
    condition is therefore held for the returns at least one voxel away from every face, and the rim may also leave."""
    xr, zr, xy, zs = rr.GRIDS[grid]
    g = gvom.Gvom(*rr.params(grid, 1), voxel_statistics=False)
    ego = rr.ego_of(grid, 1)
    cloud = rr.cloud_of(grid, 1)
    g.process_pointcloud(cloud, ego)
    g.combine_maps()
    rel = cloud.astype(np.float64)                             # (the scan's min_distance test looks at the return itself, gvom.py:1064-1067)
    far = (rel ** 2).sum(axis=1) >= g.min_distance ** 2
    assert far.sum() >= 256
    targets = cloud[far]
    with g.raycast(np.asarray(ego, np.float32), targets) as rays:
        result, position = rays.copy_to_host()
        W = rays.origin
    assert (result[:, 3] == 0).all(), "%d rays passed a voxel the scan's own ray did not mark" % int((result[:, 3] != 0).sum())
    v = np.floor(targets.astype(np.float64) / np.array([xr, xr, zr]) - W)
    inside = ((v >= 0) & (v < np.array([xy, xy, zs]))).all(axis=1)
    core = ((v >= 1) & (v < np.array([xy, xy, zs]) - 1)).all(axis=1)
    assert core.sum() >= 64 and (~inside).sum() >= 64
    assert np.isin(result[core, 0], (rr.OCCUPIED, rr.CLEAR)).all()
    print(grid, "rim returns whose ray leaves the window:", int((result[inside & ~core, 0] == rr.LEFT_WINDOW).sum()), "of", int((inside & ~core).sum()))
    assert np.isin(result[inside, 0], (rr.OCCUPIED, rr.CLEAR, rr.LEFT_WINDOW)).all()
    assert np.isin(result[~inside, 0], (rr.OCCUPIED, rr.CLEAR, rr.LEFT_WINDOW)).all()
    return result, W


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_a_scan_and_its_own_rays_agree(gvom, grid):
    result, _ = _scan_and_own_rays(gvom, grid)
    assert (result[:, 0] == rr.CLEAR).sum() >= 32 and (result[:, 0] == rr.LEFT_WINDOW).sum() >= 32


def test_a_scan_and_its_own_rays_agree_far_from_the_world_origin(gvom):
    """the same check with the window origin beyond 2^24 voxels on every axis.  No ray leaves the window there: the ego's float32
    voxel coordinates have a spacing of 2, a step of at most one voxel moves them at most once, and every sample stays inside (on
    the CPU referee: 2,565 CLEAR, 5,627 OCCUPIED, 0 LEFT_WINDOW of 8,192) -- so the floor is held on OCCUPIED instead"""
    result, W = _scan_and_own_rays(gvom, "far")
    assert (np.abs(W) >= 2.0 ** 24).all(), W
    assert (result[:, 0] == rr.CLEAR).sum() >= 32 and (result[:, 0] == rr.OCCUPIED).sum() >= 32


def test_a_product_is_a_snapshot(gvom):
    grid = "np2"
    g = rr.build_map(gvom.Gvom, grid, 2, voxel_statistics=False)
    state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
    A, B, fam = rr.rays_of(grid, state, np.asarray(origin, np.float64))
    rays = g.raycast(A, B, unknown_blocks=True)

    def raw(part, shape, dtype):
        out = np.empty(shape, dtype)
        g._check(g._lib.gvom_device_product_copy(g._h, rays.product_id, part, ctypes.c_void_p(out.ctypes.data)))
        return out.tobytes()
    before = raw(0, (rr.N_RAYS, 4), np.int32), raw(1, (rr.N_RAYS, 3), np.float32)
    ego = rr.ego_of(grid, 9)                                   # a further scan from elsewhere, and its combine
    g.process_pointcloud(rr.cloud_of(grid, 9), ego)
    g.combine_maps()
    after = raw(0, (rr.N_RAYS, 4), np.int32), raw(1, (rr.N_RAYS, 3), np.float32)
    assert before == after
    with g.raycast(A, B, unknown_blocks=True) as again:        # ... while the map itself has moved on
        assert not np.array_equal(again.origin, rays.origin)
        assert again.result.copy_to_host().tobytes() != before[0]
    rays.release()


def test_pool_and_allocations(maps):
    g, state, W, (A, B, fam) = maps["p2", 2]
    base = g.get_tuning("raycast_allocations")
    assert g.get_tuning("raycast") == 1
    a, b = A[:500], B[:500]
    g.raycast(a, b).release()
    first = g.get_tuning("raycast_allocations")
    for _ in range(20):                                        # steady state at a fixed n: nothing is allocated
        g.raycast(a, b, check_target=True).release()
        g.raycast(a[:1], b).release()
    assert g.get_tuning("raycast_allocations") == first >= base
    held = [g.raycast(a, b) for _ in range(4)]
    assert len({r.result.ptr for r in held}) == 4
    import gvom as mod
    with pytest.raises(mod.GvomBackendError, match="exported"):
        g.raycast(a, b)                                        # the fifth product of the kind while four are held
    assert g._lib.gvom_raycast(g._h, a.ctypes.data_as(ctypes.c_void_p), 500, b.ctypes.data_as(ctypes.c_void_p), 500, 0, 0, None,
                               ctypes.byref(ctypes.c_int64())) == GVOM_ERR_CAPACITY
    held.pop().release()
    want = rr.walk(state, W, "p2", a, b)
    _hold(g.raycast(a, b), want, W, "after a release")
    for r in held:
        r.release()
    sets = g.get_tuning("device_product_sets")
    g.raycast(a, b).release()
    assert g.get_tuning("device_product_sets") == sets


def test_errors(gvom, maps):
    g, state, W, (A, B, fam) = maps["tall", 1]
    a, b = np.ascontiguousarray(A[:8]), np.ascontiguousarray(B[:8])
    pa, pb = a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p)
    pid = ctypes.c_int64(-1)

    def call(h, frm, K, to, n, flags=0, out=pid):
        return h._lib.gvom_raycast(h._h, frm, K, to, n, 0, flags, None, ctypes.byref(out) if out is not None else None)
    assert call(g, pa, 8, pb, 8) == 0 and pid.value > 0        # (origin_voxels may be NULL)
    assert call(g, pa, 1, pb, 8) == 0
    assert call(g, pa, 8, pb, 0) == GVOM_ERR_INVALID and pid.value == -1
    assert call(g, pa, 8, pb, -3) == GVOM_ERR_INVALID
    assert call(g, pa, 2, pb, 8) == GVOM_ERR_INVALID and b"K must be 1 or n" in g._lib.gvom_last_error(g._h)
    assert call(g, pa, 0, pb, 8) == GVOM_ERR_INVALID
    assert call(g, None, 8, pb, 8) == GVOM_ERR_INVALID
    assert call(g, pa, 8, None, 8) == GVOM_ERR_INVALID
    assert call(g, pa, 8, pb, 8, out=None) == GVOM_ERR_INVALID
    assert call(g, pa, 8, pb, 8, flags=4) == GVOM_ERR_INVALID and call(g, pa, 8, pb, 8, flags=-1) == GVOM_ERR_INVALID
    assert call(g, pa, 8, pb, 8, flags=3) == 0
    assert call(g, pa, 1, pb, (1 << 26) + 1) == GVOM_ERR_CAPACITY           # refused before anything is read
    with pytest.raises(ValueError, match="K must be 1 or n"):
        g.raycast_device(1234, 3, 5678, 8)
    assert g._lib.gvom_device_product(g._h, gvom.PRODUCT_RAYCAST, 0, ctypes.byref(pid)) == GVOM_ERR_INVALID
    fresh = gvom.Gvom(*rr.params("tall", 1), voxel_statistics=False)
    assert call(fresh, pa, 8, pb, 8) == GVOM_NO_DATA and fresh.raycast(a, b) is None
    fresh.process_pointcloud(rr.cloud_of("tall", 0), rr.ego_of("tall", 0))
    assert fresh.raycast(a, b) is None                         # scanned, not combined yet
    fresh.combine_maps()
    assert fresh.raycast(a, b) is not None
    sharded = gvom.Gvom(*rr.params("tall", 1), voxel_statistics=False, _shard=(0, 1))
    assert call(sharded, pa, 8, pb, 8) == GVOM_ERR_INVALID and b"sharded" in sharded._lib.gvom_last_error(sharded._h)


@pytest.mark.parametrize("case", ["zero_copy", "consumer_stream"])
def test_torch_consumer(case):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_raycast_torch.py"), case], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "CASE OK " + case in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
