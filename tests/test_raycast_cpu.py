"""CPU side of the ray queries (gvom_raycast): the referee of tests/raycast_ref.py pinned to the oracle's orc_point_2_map -- the
voxels it walks are exactly the voxels the reference's ray adds a ray pass to -- the census floors of the GPU test's inputs on
oracle-built maps, and the header / binding / library agreement.  No GPU.

Census of the 4,096-ray input under GVOM_RAY_UNKNOWN_BLOCKS on the oracle-built maps (buffer_size 1; rays per status CLEAR /
OCCUPIED / UNKNOWN / LEFT_WINDOW / INVALID; rays that stop at a voxel at step >= 8 / >= 4):
    p2     713 / 2619 / 405 / 263 / 96;   1270 / 2020
    np2    514 / 3018 / 219 / 249 / 96;    423 / 1041
    tall   811 / 2165 / 577 / 447 / 96;    367 / 1515
(buffer_size 2 differs by a few rays.)  The tall grid is 16 voxels wide: from its centre a ray leaves after 8 steps in x or y,
so its step floor is 4; the census shows it would hold the floor at 8 too, through the z axis, which is not asserted.

The grids of more than one tile segment (tests/raycast_ref.py WIDE), same call, buffer_size 1 / 2 -- rays per status; stops at
step >= 8; stop voxels per 64-cell STORAGE segment; rays whose examined voxels span two or more segments:
    w128   834 / 2298 / 563 / 305 / 96;  2016;  2313 / 548;        606        840 / 2307 / 549 / 304 / 96;  1993;  2362 / 494;        557
    w192   914 / 2190 / 532 / 364 / 96;  1686;  2187 / 334 / 201;  616        916 / 2230 / 511 / 343 / 96;  1658;  2268 / 341 / 132;  534
Storage offsets (window origin mod size) x / y / z: 83 / 50 / 17 and 125 / 75 / 13.  Floors: 100 stops in every segment, 300
crossing rays.  The far grid (FAR): window origin 17,499,983 / -17,500,029 / 17,499,991 voxels, 2^24 = 16,777,216."""
import ctypes
import os
import re

import numpy as np
import pytest

import raycast_ref as rr
from multi_origin_ref import GRIDS
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def maps():
    """per (grid, buffer_size): (dense fused state, window origin) of the oracle after the shared scans"""
    out = {}
    for grid in GRIDS:
        for bs in (1, 2):
            g = rr.build_map(oracle.OracleGvom, grid, bs)
            W = np.asarray(g.combined_origin, np.float64)
            assert np.array_equal(W, rr.window_origin(grid, rr.ego_of(grid, rr.N_SCANS - 1)))
            out[grid, bs] = (np.asarray(g.combined_index_map).copy(), W)
    oracle.lib().orc_set_cuda_f32_sqrt(0)
    return out


@pytest.fixture(scope="module")
def wide_maps():
    """the same on the ray tests' own grids (tests/raycast_ref.py WIDE, FAR)"""
    out = {}
    for grid in list(rr.WIDE) + list(rr.FAR):
        for bs in (1, 2):
            g = rr.build_map(oracle.OracleGvom, grid, bs)
            W = np.asarray(g.combined_origin, np.float64)
            assert np.array_equal(W, rr.window_origin(grid, rr.ego_of(grid, rr.N_SCANS - 1)))
            out[grid, bs] = (np.asarray(g.combined_index_map).copy(), W)
    return out


def _special_rays(grid, W):
    """rays that start outside the window, end outside it, are shorter than one voxel, axis-parallel, exact diagonals"""
    xr, zr, xy, zs = rr.GRIDS[grid]
    res = np.array([xr, xr, zr])
    lo, size = W * res, np.array([xy, xy, zs]) * res
    c = lo + 0.5 * size
    A, B = [], []
    for k in range(3):
        for sign in (-1.0, 1.0):
            e = np.zeros(3); e[k] = sign
            A.append(c - e * 0.8 * size); B.append(c + e * 0.2 * size)          # starts outside, enters along an axis: axis-parallel
            A.append(c + e * 0.1 * size); B.append(c + e * 0.9 * size)          # ends outside
            A.append(c); B.append(c + e * 0.3 * res)                            # shorter than one voxel
            A.append(c); B.append(c + e * 1.7 * res)                            # one or two steps
    lattice = (np.floor(c / res) + 0.5) * res
    for sx in (-1, 1):
        for sy in (-1, 1):
            for sz in (-1, 1):
                for m in (3, 6):
                    A.append(lattice); B.append(lattice + m * np.array([sx, sy, sz]) * res)       # |dx| = |dy| = |dz|: z wins the tie
                A.append(lattice); B.append(lattice + 5 * np.array([sx, sy, 0]) * res)            # |dx| = |dy|: y wins
    return np.array(A).astype(np.float32), np.array(B).astype(np.float32)


@pytest.mark.parametrize("f32_sqrt", [False, True])
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_referee_walks_the_voxels_the_oracle_marks(maps, grid, f32_sqrt):
    _referee_against_the_oracle(maps, grid, f32_sqrt)


@pytest.mark.parametrize("grid", sorted(rr.WIDE))
def test_referee_walks_the_voxels_the_oracle_marks_on_the_wide_grids(wide_maps, grid):
    _referee_against_the_oracle(wide_maps, grid, False)


def _referee_against_the_oracle(maps, grid, f32_sqrt):
    xr, zr, xy, zs = rr.GRIDS[grid]
    state, W = maps[grid, 1]
    A, B, fam = rr.rays_of(grid, state, W)
    pick = np.flatnonzero(fam != 4)[::11]                     # ~360 finite rays of every family
    sa, sb = _special_rays(grid, W)
    A, B = np.concatenate([A[pick], sa]), np.concatenate([B[pick], sb])
    n = len(A)
    assert n >= 300
    free = np.full(xy * xy * zs, -2, np.int32)                # nothing stops a ray: it walks as far as the mapper's
    result, _, visits = rr.walk(free, W, grid, A, B, f32_sqrt=f32_sqrt, record=True)
    walked = [[] for _ in range(n)]
    for i, v in visits:
        walked[i].append(v)
    p, inc, S = rr.setup(grid, A, B, f32_sqrt)
    ties3 = int(((np.abs(inc) == 1).all(axis=1)).sum())
    ties2 = int(((np.abs(inc[:, :2]) == 1).all(axis=1) & (inc[:, 2] == 0)).sum())
    assert ties3 >= 16 and ties2 >= 8, (ties3, ties2)         # the diagonals are exact ties in float32
    L = oracle.lib()
    L.orc_set_cuda_f32_sqrt(1 if f32_sqrt else 0)
    try:
        some_steps = 0
        for i in range(n):
            hit, total, _ = oracle.point_2_map(xr, zr, xy, zs, 0.0, B[i:i + 1], A[i].astype(np.float64), W)
            passes = total - hit
            want = np.zeros_like(passes)
            np.add.at(want, np.asarray(walked[i], np.int64), 1)
            assert np.array_equal(passes, want), (grid, f32_sqrt, i, A[i], B[i], np.flatnonzero(passes != want)[:8])
            assert int(passes.sum()) == len(walked[i]) and passes.max(initial=0) <= 1
            # the referee's in-window step count: all S steps of a CLEAR ray, the steps before the face otherwise
            assert result[i, 0] in (rr.CLEAR, rr.LEFT_WINDOW) and result[i, 1] == len(walked[i]), (i, result[i])
            some_steps += len(walked[i]) > 0
        assert some_steps >= 200
    finally:
        L.orc_set_cuda_f32_sqrt(0)


def test_referee_known_answers():
    """a hand-made 16 x 16 x 32 map: one occupied voxel and one unknown voxel on the +x axis of the window's centre"""
    grid = "tall"
    xr, zr, xy, zs = GRIDS[grid]
    W = np.array([-8.0, -8.0, -16.0])
    state = np.full(xy * xy * zs, -3, np.int32)
    vox = lambda x, y, z: x + y * xy + z * xy * xy
    state[vox(12, 8, 16)] = 5
    state[vox(10, 8, 16)] = -1
    a = np.array([[0.2, 0.2, 0.1]], np.float32)               # voxel (8, 8, 16), its centre
    b = np.array([[0.2 + 6 * 0.4, 0.2, 0.1]], np.float32)
    r, pos = rr.walk(state, W, grid, a, b)
    assert r.tolist() == [[rr.OCCUPIED, 4, vox(12, 8, 16), 1]] and np.allclose(pos, [[0.2 + 4 * 0.4, 0.2, 0.1]], atol=1e-6)
    r, pos = rr.walk(state, W, grid, a, b, unknown_blocks=True)
    assert r.tolist() == [[rr.UNKNOWN, 2, vox(10, 8, 16), 1]]
    near = np.array([[0.2 + 4 * 0.4, 0.2, 0.1]], np.float32)  # ends IN the occupied voxel: the walk stops one step short of it
    r, pos = rr.walk(state, W, grid, a, near)
    assert r.tolist() == [[rr.CLEAR, 3, -1, 1]] and np.isnan(pos).all()
    r, pos = rr.walk(state, W, grid, a, near, check_target=True)
    assert r.tolist() == [[rr.OCCUPIED, 4, vox(12, 8, 16), 1]] and np.array_equal(pos, near)
    r, pos = rr.walk(state, W, grid, a, a, check_target=True)
    assert r.tolist() == [[rr.CLEAR, 0, -1, 0]]
    r, pos = rr.walk(state, W, grid, a, np.array([[0.2 - 20 * 0.4, 0.2, 0.1]], np.float32))      # leaves through the -x face after 8 steps inside
    assert r.tolist() == [[rr.LEFT_WINDOW, 8, -1, 0]] and np.isnan(pos).all()
    r, pos = rr.walk(state, W, grid, a, np.array([[np.nan, 0, 0]], np.float32), unknown_blocks=True, check_target=True)
    assert r.tolist() == [[rr.INVALID, 0, -1, 0]] and np.isnan(pos).all()
    r, _ = rr.walk(state, W, grid, np.array([[40.0, 0.2, 0.1]], np.float32), a)        # starts outside: the first step is outside
    assert r.tolist() == [[rr.LEFT_WINDOW, 0, -1, 0]]


@pytest.mark.parametrize("bs", [1, 2])
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_census_floors_of_the_gpu_inputs(maps, grid, bs):
    """the inputs of tests/test_raycast.py on the oracle-built map: every status in >= 32 rays of ONE call, >= 32 rays that stop
    at a voxel at step >= 8 (tall: >= 4), and each family's outcome as constructed"""
    state, W = maps[grid, bs]
    assert (state >= 0).sum() >= 64 and (state == -1).sum() >= 64 and (state <= -2).sum() >= 64
    A, B, fam = rr.rays_of(grid, state, W)
    result, position = rr.walk(state, W, grid, A, B, **rr.CENSUS_FLAGS)
    per_status, at8, at4 = rr.census(result)
    print(grid, bs, per_status, at8, at4)
    assert min(per_status) >= rr.STATUS_FLOOR, per_status
    step, floor = rr.STEP_FLOOR[grid]
    assert (at8 if step == 8 else at4) >= floor, (at8, at4)
    st = result[:, 0]
    assert (st[fam == 4] == rr.INVALID).all() and (st[fam != 4] != rr.INVALID).all()
    assert (st[fam == 5] == rr.CLEAR).all() and (result[fam == 5, 1] == 0).all()
    assert (result[fam == 2, 3] == 0).all() and np.isin(st[fam == 2], (rr.LEFT_WINDOW, rr.OCCUPIED, rr.CLEAR)).all()
    plain, _ = rr.walk(state, W, grid, A, B)
    assert ((plain[fam == 3, 3] > 0) | (plain[fam == 3, 0] == rr.OCCUPIED)).all() and np.isin(st[fam == 3], (rr.UNKNOWN, rr.OCCUPIED)).all()
    assert (plain[fam == 3, 3] > 0).sum() >= 32
    target, _ = rr.walk(state, W, grid, A, B, check_target=True)
    through = (fam == 0) & (np.arange(len(fam)) % 2 == 1)
    assert (plain[through, 0] == rr.OCCUPIED).all()           # through an occupied voxel's centre: stopped at or before it
    assert (target[fam == 0, 0] == rr.OCCUPIED).all()         # ends in one: stopped at or before it once the target is examined
    stopped = np.isin(st, (rr.OCCUPIED, rr.UNKNOWN))
    assert np.isfinite(position[stopped]).all() and np.isnan(position[~stopped]).all()


@pytest.mark.parametrize("bs", [1, 2])
@pytest.mark.parametrize("grid", sorted(rr.WIDE))
def test_wide_inputs_stop_in_every_tile_segment_and_cross_between_them(wide_maps, grid, bs):
    """the conditions under which tests/test_raycast.py's wide-grid test exercises k_raycast's tile index beyond segment 0, on
    the referee alone: non-zero storage offsets on every axis, >= 100 stop voxels in every 64-cell storage segment, >= 300 rays
    whose examined voxels span two or more segments, every status in >= 32 rays, >= 32 stops at step >= 8 (figures: module
    docstring)"""
    xr, zr, xy, zs = rr.GRIDS[grid]
    state, W = wide_maps[grid, bs]
    assert xy > 64 and all(int(W[k]) % (xy if k < 2 else zs) != 0 for k in range(3)), W
    assert min(np.bincount(rr.state_class(state), minlength=3)) >= 64
    A, B, fam = rr.rays_of(grid, state, W)
    result, position, visits = rr.walk(state, W, grid, A, B, record=True, **rr.CENSUS_FLAGS)
    per_status, at8, at4 = rr.census(result)
    stops, crossing = rr.segment_census(result, visits, W, grid)
    print(grid, bs, per_status, at8, at4, stops, crossing)
    assert len(stops) == (xy + 63) // 64 >= 2 and min(stops) >= rr.SEGMENT_STOP_FLOOR, stops
    assert crossing >= rr.SEGMENT_CROSS_FLOOR, crossing
    assert min(per_status) >= rr.STATUS_FLOOR, per_status
    assert rr.STEP_FLOOR[grid][0] == 8 and at8 >= rr.STEP_FLOOR[grid][1], at8
    # the segment of a stop is the segment of its STORAGE column: without the offset the counts differ
    unshifted = np.bincount((result[result[:, 2] >= 0, 2] % xy) >> 6, minlength=len(stops))
    assert unshifted.tolist() != stops
    assert (result[fam == 4, 0] == rr.INVALID).all() and (result[fam != 4, 0] != rr.INVALID).all()


@pytest.mark.parametrize("bs", [1, 2])
def test_the_far_grid_lies_beyond_2_to_the_24_voxels_on_every_axis(wide_maps, bs):
    """where gvom_raycast takes the literal lookup for the origin's sake (gvom_product_calls.hip raycast_params: any |origin| >= 2^24);
    the grid itself (np2) takes the integer one.  The egos are float32-representable and still move from scan to scan."""
    xr, zr, xy, zs = rr.GRIDS["far"]
    assert rr.GRIDS["far"] == GRIDS["np2"] and zs <= xy
    state, W = wide_maps["far", bs]
    assert (np.abs(W) >= 2.0 ** 24).all() and (W > 0).any() and (W < 0).any(), W
    egos = [rr.ego_of("far", k) for k in range(rr.N_SCANS)]
    assert all(float(np.float32(v)) == v for e in egos for v in e)
    origins = [rr.window_origin("far", e) for e in egos]
    assert all((np.abs(o) >= 2.0 ** 24).all() for o in origins)
    assert all(not np.array_equal(origins[k], origins[k + 1]) for k in range(rr.N_SCANS - 1))
    assert all(int(W[k]) % (xy if k < 2 else zs) != 0 for k in range(3)), W
    A, B, fam = rr.rays_of("far", state, W)
    result, _ = rr.walk(state, W, "far", A, B, **rr.CENSUS_FLAGS)
    per_status, _, _ = rr.census(result)
    print("far", bs, per_status)
    assert min(per_status) >= rr.STATUS_FLOOR, per_status


def test_header_binding_and_library_agree():
    import gvom
    header = open(os.path.join(ROOT, "include", "gvom_hip.h")).read()
    m = re.search(r"\bint\s+gvom_raycast\s*\(([^;]*)\)\s*;", header)
    assert m, "gvom_raycast is not declared in include/gvom_hip.h"
    assert len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == 9
    bound = {name: (res, args) for name, res, args in gvom.ABI}
    assert bound["gvom_raycast"][0] is ctypes.c_int and len(bound["gvom_raycast"][1]) == 9
    assert hasattr(gvom.load_library(), "gvom_raycast")
    for word, value in (("GVOM_PRODUCT_RAYCAST", gvom.PRODUCT_RAYCAST), ("GVOM_RAY_CLEAR", gvom.RAY_CLEAR),
                        ("GVOM_RAY_OCCUPIED", gvom.RAY_OCCUPIED), ("GVOM_RAY_UNKNOWN", gvom.RAY_UNKNOWN),
                        ("GVOM_RAY_LEFT_WINDOW", gvom.RAY_LEFT_WINDOW), ("GVOM_RAY_INVALID", gvom.RAY_INVALID),
                        ("GVOM_RAY_UNKNOWN_BLOCKS", 1), ("GVOM_RAY_CHECK_TARGET", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (word, value), header), word
    assert (rr.CLEAR, rr.OCCUPIED, rr.UNKNOWN, rr.LEFT_WINDOW, rr.INVALID) == (0, 1, 2, 3, 4) and gvom.PRODUCT_RAYCAST == 6
    for word in ('"raycast"', '"raycast_allocations"', "NOT PROVIDED: sharded handles; sorting or binning"):
        assert word in header, word
    for name in ("raycast", "raycast_device"):
        assert callable(getattr(gvom.Gvom, name))
    for name in ("result", "position", "origin", "copy_to_host", "release", "__enter__", "__exit__"):
        assert name in gvom.DeviceRays.__init__.__code__.co_names or hasattr(gvom.DeviceRays, name), name


def test_binding_checks_shapes_before_the_library_is_called():
    import gvom
    g = gvom.Gvom.__new__(gvom.Gvom)                          # no handle: the checks below run before any library call
    t = np.zeros((5, 3))
    with pytest.raises(ValueError, match="targets"):
        g.raycast(np.zeros(3), np.zeros((5, 2)))
    with pytest.raises(ValueError, match="targets"):
        g.raycast(np.zeros(3), np.zeros((0, 3)))
    with pytest.raises(ValueError, match="origins"):
        g.raycast(np.zeros((4, 3)), t)
    with pytest.raises(ValueError, match="origins"):
        g.raycast(np.zeros(2), t)
    with pytest.raises(ValueError, match="device addresses"):
        g.raycast_device(0, 1, 1234, 5)
