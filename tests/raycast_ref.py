"""Shared by tests/test_raycast.py, tests/test_raycast_cpu.py and tests/_raycast_torch.py: the referee of gvom_raycast and the
inputs of those tests.

The referee (walk) is a plain numpy float32 / float64 restatement of the definition in include/gvom_hip.h "ray queries": the
ray set-up of gvom.py:1097-1126, the literal length loop of gvom.py:1127 / 1150, three float32 additions per step, the literal
float64 window lookup, on a DENSE state array in the reference's voxel order (x + y * xy + z * xy * xy: what
Gvom.read_dense(GVOM_WHICH_FUSED) and the oracle's combined_index_map hold) and a window origin.  All rays advance in lock
step, one numpy operation per reference operation, every one rounded once.  tests/test_raycast_cpu.py pins it to the oracle's
orc_point_2_map, so that it cannot drift from the reference."""
import math

import numpy as np

import multi_origin_ref
import synth

# The ray tests' own grids, next to the three of tests/multi_origin_ref.py (whose parametrisation they must not change).  WIDE: the
# smallest maps with more than one 64-cell tile segment per storage row (k_raycast's tile index is row * nseg + (sx >> 6): at
# xy <= 64 its second term is always 0) -- a power of two with 2 segments, no power of two with 3.  FAR: the np2 grid with every
# ego moved by FAR_OFFSET metres, which puts every axis of the window origin beyond 2^24 voxels (both signs): the query then
# takes the literal float64 lookup whatever the grid (gvom_product_calls.hip raycast_params).
WIDE = {"w128": (0.2, 0.2, 128, 32), "w192": (0.2, 0.2, 192, 24)}
FAR = {"far": multi_origin_ref.GRIDS["np2"]}
FAR_OFFSET = (7.0e6, -7.0e6, 3.5e6)
GRIDS = dict(multi_origin_ref.GRIDS)
GRIDS.update(WIDE)
GRIDS.update(FAR)

CLEAR, OCCUPIED, UNKNOWN, LEFT_WINDOW, INVALID = range(5)
N_RAYS = 4096
N_SCANS = 4
F32 = np.float32


def params(grid, buffer_size):
    return GRIDS[grid] + (buffer_size,) + synth.REF_TAIL


def _res(grid):
    xr, zr, _, _ = GRIDS[grid]
    return np.array([xr, xr, zr], np.float64)


def setup(grid, a, b, f32_sqrt=False):
    """(p, inc, S) of the rays a -> b (float32 [n, 3], metres): start in voxels, per-step increments (float32) and the number of
    steps the reference's loop test admits, capped at xy + z + 1 (no ray takes that many inside the window)."""
    xr, zr, xy, zs = GRIDS[grid]
    res = _res(grid)
    with np.errstate(all="ignore"):
        p = (a.astype(np.float64) / res).astype(F32)                       # gvom.py:1097-1099
        e = (b.astype(np.float64) / res).astype(F32)                       # :1101-1103
        s = e - p                                                          # :1105-1107 (float32)
        ss = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]   # :1110, float32, left to right
        assert ss.dtype == F32
        ray_length = np.sqrt(ss).astype(np.float64) if f32_sqrt else np.sqrt(ss.astype(np.float64))
        s = (s.astype(np.float64) / ray_length[:, None]).astype(F32)       # :1112-1114
        ab = np.abs(s)
        inner = np.where(ab[:, 2] > ab[:, 1], ab[:, 2], ab[:, 1])          # Python's max(a, b): b if b > a else a
        smax = np.where(inner > ab[:, 0], inner, ab[:, 0])                 # :1116
        si = np.zeros(len(a), np.int64)
        si[smax == ab[:, 1]] = 1
        si[smax == ab[:, 2]] = 2                                           # ties: z over y over x
        sd = s[np.arange(len(a)), si]
        inc = s / np.abs(sd)[:, None]                                      # :1126, 1129-1132: float32 / float32
        assert inc.dtype == F32
        step_len = np.abs(1.0 / sd.astype(np.float64))                     # :1150
        lim = ray_length - 1.0
        cap = xy + zs + 1
        S = np.zeros(len(a), np.int64)
        length = np.zeros(len(a), np.float64)
        for _ in range(cap):
            go = length < lim                                              # :1127
            if not go.any():
                break
            S[go] += 1
            length = np.where(go, length + step_len, length)
    return p, inc, S


def walk(state, W, grid, a, b, unknown_blocks=False, check_target=False, f32_sqrt=False, record=False):
    """result int32 [n, 4] {status, steps, voxel, unknown}, position float32 [n, 3] (and, with record, the list of (ray, voxel)
    pairs examined inside the window, in step order) of the rays a[i] -> b[i] through the dense `state` whose window starts at
    world voxel W."""
    xr, zr, xy, zs = GRIDS[grid]
    res = _res(grid)
    a = np.ascontiguousarray(a, F32).reshape(-1, 3)
    b = np.ascontiguousarray(b, F32).reshape(-1, 3)
    n = len(b)
    if len(a) == 1 and n > 1:
        a = np.repeat(a, n, axis=0)
    W = np.asarray(W, np.float64)
    size = np.array([xy, xy, zs], np.float64)
    result = np.zeros((n, 4), np.int32)
    result[:, 2] = -1
    position = np.full((n, 3), np.nan, F32)
    finite = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1)
    result[~finite, 0] = INVALID
    p, inc, S = setup(grid, a, b, f32_sqrt)
    run = finite.copy()
    unknown = np.zeros(n, np.int64)
    visits = []

    def examine(who, v, steps, pos):
        """rays `who` (indices) look at window voxel v (float64 [m, 3], inside) at step count `steps`; returns who stopped"""
        vi = v.astype(np.int64)
        vox = vi[:, 0] + vi[:, 1] * xy + vi[:, 2] * xy * xy
        if record:
            visits.extend(zip(who.tolist(), vox.tolist()))
        s = state[vox]
        unk = s == -1
        unknown[who[unk]] += 1
        stop = (s >= 0) | (unk & bool(unknown_blocks))
        w = who[stop]
        result[w, 0] = np.where(s[stop] >= 0, OCCUPIED, UNKNOWN)
        result[w, 1] = steps[stop]
        result[w, 2] = vox[stop]
        position[w] = pos[stop]
        run[w] = False

    with np.errstate(all="ignore"):
        j = 0
        while (run & (S > j)).any():
            j += 1
            p = p + inc                                                    # every ray: three float32 additions
            assert p.dtype == F32
            who = np.flatnonzero(run & (S >= j))
            v = np.floor(p[who].astype(np.float64) - W)
            inside = ((v >= 0) & (v < size)).all(axis=1)                   # NaN compares false: outside
            out = who[~inside]
            result[out, 0] = LEFT_WINDOW
            result[out, 1] = j - 1
            run[out] = False
            who, v = who[inside], v[inside]
            examine(who, v, np.full(len(who), j), (p[who].astype(np.float64) * res).astype(F32))
        who = np.flatnonzero(run)
        result[who, 0] = CLEAR
        result[who, 1] = S[who]
        if check_target and len(who):
            v = np.floor(b[who].astype(np.float64) / res - W)              # gvom.py:1072-1080
            inside = ((v >= 0) & (v < size)).all(axis=1)
            result[who[~inside], 0] = LEFT_WINDOW
            run[who[~inside]] = False
            who, v = who[inside], v[inside]
            examine(who, v, S[who] + 1, b[who])
    result[:, 3] = np.where(finite, unknown, 0)
    return (result, position, visits) if record else (result, position)


# ---- the shared inputs: maps -----------------------------------------------------------------------------------------------
def ego_of(grid, k):
    """float32-representable egos that move 5 % of the window per scan in x, 3.5 % in -y: the window origin changes with every
    scan (storage offsets != 0, tiles go stale)"""
    xr, zr, xy, zs = GRIDS[grid]
    w = xr * xy
    off = FAR_OFFSET if grid in FAR else (0.0, 0.0, 0.0)
    return tuple(float(F32(v + o)) for v, o in zip((0.05 * w * k + 0.05, -0.035 * w * k, 0.11 * k), off))


def cloud_of(grid, k):
    """float32 returns of scan k in the world frame: a 16 x 512 lidar sweep of a scene of boxes on the even scans of the grids
    wide enough to hold one, else uniformly random returns (8,192; 384 on the tall grid, whose 16 x 16 columns 8,192 returns would
    fill with occupied voxels) in a box 1.2 windows wide whose top is 0.15 window heights above the ego -- the upper part of the
    window is never scanned"""
    xr, zr, xy, zs = GRIDS[grid]
    ego = ego_of(grid, k)
    if grid not in ("tall", "far") and k % 2 == 0:            # (the scene lies around the world's origin: out of the far window's sight)
        scene = synth.make_scene(2, extent=10.0)
        return synth.lidar_scan(scene, 16, 512, ego, 0.0, k, F32, elevations_deg=np.linspace(-24.0, 3.0, 16))
    wx, wz = xr * xy, zr * zs
    pc = synth.uniform_cloud(384 if grid == "tall" else 8192, 300 + k, (ego[0] - 0.6 * wx, ego[0] + 0.6 * wx), (ego[1] - 0.6 * wx, ego[1] + 0.6 * wx),
                             (ego[2] - 0.55 * wz, ego[2] + 0.15 * wz), np.float64)
    return np.ascontiguousarray(pc.astype(F32))


def build_map(cls, grid, buffer_size, **kw):
    """N_SCANS scans with a combine after each on a mapper of class `cls` (gvom.Gvom or the oracle's OracleGvom); returns it"""
    g = cls(*params(grid, buffer_size), **kw)
    for k in range(N_SCANS):
        g.process_pointcloud(cloud_of(grid, k), ego_of(grid, k))
        g.combine_maps()
    return g


def window_origin(grid, ego):
    xr, zr, xy, zs = GRIDS[grid]
    return np.array([math.floor(ego[0] / xr - xy / 2), math.floor(ego[1] / xr - xy / 2), math.floor(ego[2] / zr - zs / 2)], np.float64)


# ---- the shared inputs: rays -----------------------------------------------------------------------------------------------
def _spread(idx, m):
    """m entries of idx, evenly spread (all of them, repeated, if there are fewer)"""
    assert len(idx) > 0
    return idx[(np.arange(m) * len(idx)) // m] if len(idx) >= m else idx[np.arange(m) % len(idx)]


def _centres(vox, W, grid):
    xr, zr, xy, zs = GRIDS[grid]
    v = np.stack([vox % xy, vox // xy % xy, vox // (xy * xy)], axis=1).astype(np.float64)
    return (W + v + 0.5) * _res(grid)


def rays_of(grid, state, W, last=None):
    """(origins [4096, 3], targets [4096, 3], family [4096]) float32: the ray families of tests/test_raycast.py on the map
    (state, W) built by build_map -- the outcome of each is known by construction (last: the (ego, cloud) that stand for "the
    last scan" below, for a map whose last scan is not scan N_SCANS - 1: tests/query_cycle.py):
      0  1024  end in (even rows) or 3 voxels behind (odd rows) the centre of an occupied voxel, from the last ego: stopped at or
               before it (the walk samples the dominant axis once per voxel, so it looks into the voxel around a centre it passes)
      1  1024  returns of scan 2 from that scan's ego, cut to half their range: mostly CLEAR
      2   768  returns of the LAST scan that lie outside the window, from its ego: every voxel on the way was marked by that
               scan's own ray, so never unknown: LEFT_WINDOW or stopped earlier (CLEAR where the return lies less than a step
               beyond the face: the walk ends a voxel short of its end)
      3   768  through the centre of a never-observed voxel (3 voxels behind it), from the last ego: UNKNOWN under the flag unless
               stopped earlier, unknown > 0 without
      4    96  a non-finite component (in the target on even rows, in the origin on odd rows): INVALID
      5    64  origin == target: no step
      6   352  random segments around the window, every fourth axis-parallel, every fourth (offset 1) an exact diagonal; starts
               inside and outside the window"""
    xr, zr, xy, zs = GRIDS[grid]
    res = _res(grid)
    last_ego, last_cloud = last if last is not None else (ego_of(grid, N_SCANS - 1), cloud_of(grid, N_SCANS - 1))
    last = np.array(last_ego, np.float64)
    rng = np.random.default_rng(7)
    A, B, fam = [], [], []

    def add(a, b, f):
        a = np.broadcast_to(np.asarray(a, np.float64), np.shape(b))
        A.append(a); B.append(np.asarray(b, np.float64)); fam.append(np.full(len(b), f))

    def behind(c, k):                                         # k voxels (of the finer axis) behind c, seen from the last ego
        d = c - last
        return c + d / np.linalg.norm(d / res, axis=1)[:, None] * k
    occ = _centres(_spread(np.flatnonzero(state >= 0), 1024), W, grid)
    occ[1::2] = behind(occ[1::2], 3.0)
    add(last, occ, 0)
    ego2 = np.array(ego_of(grid, 2), np.float64)
    ret = cloud_of(grid, 2).astype(np.float64)
    ret = ret[_spread(np.arange(len(ret)), 1024)]
    add(ego2, ego2 + 0.5 * (ret - ego2), 1)
    ret = last_cloud.astype(np.float64)
    v = np.floor(ret / res - W)
    outside = ~((v >= 0) & (v < np.array([xy, xy, zs]))).all(axis=1)
    outside &= ((ret - last) ** 2).sum(axis=1) >= synth.REF_TAIL[0] ** 2           # (the scan drops returns closer than min_distance)
    add(last, ret[_spread(np.flatnonzero(outside), 768)], 2)
    add(last, behind(_centres(_spread(np.flatnonzero(state == -1), 768), W, grid), 3.0), 3)
    bad = np.array([np.nan, np.inf, -np.inf])
    a4 = np.repeat(last[None], 96, axis=0)
    b4 = last + rng.uniform(-3, 3, (96, 3))
    rows = np.arange(96)
    b4[rows[0::2], rows[0::2] % 3] = bad[(rows[0::2] // 6) % 3]
    a4[rows[1::2], rows[1::2] % 3] = bad[(rows[1::2] // 6) % 3]
    add(a4, b4, 4)
    same = np.repeat(last[None], 64, axis=0)
    same[8:] += rng.uniform(-0.7, 0.7, (56, 3)) * np.array([xr * xy, xr * xy, zr * zs])
    add(same, same.copy(), 5)
    lo, size = W * res, np.array([xy, xy, zs]) * res
    a6 = lo + rng.uniform(-0.25, 1.25, (352, 3)) * size
    b6 = lo + rng.uniform(-0.25, 1.25, (352, 3)) * size
    r = np.arange(352)
    ax = r % 4 == 0                                           # axis-parallel: the target differs in one coordinate only
    keep = (r // 4) % 3
    for k in range(3):
        m = ax & (keep != k)
        b6[m, k] = a6[m, k]
    dg = r % 4 == 1                                           # exact diagonals in voxel space: |dx| = |dy| = |dz| voxels, starts on a lattice
    a6[dg] = (np.floor(a6[dg] / res) + 0.5) * res
    steps = rng.integers(2, 12, dg.sum())[:, None] * rng.choice([-1.0, 1.0], (dg.sum(), 3))
    b6[dg] = a6[dg] + steps * res
    add(a6, b6, 6)
    A, B, fam = np.concatenate(A), np.concatenate(B), np.concatenate(fam)
    assert A.shape == B.shape == (N_RAYS, 3)
    A32, B32 = np.ascontiguousarray(A.astype(F32)), np.ascontiguousarray(B.astype(F32))
    B32[fam == 5] = A32[fam == 5]
    return A32, B32, fam


def census(result):
    """(rays per status 0..4, rays that stopped at a voxel at step >= 8, the same at step >= 4)"""
    st = result[:, 0]
    stopped = (st == OCCUPIED) | (st == UNKNOWN)
    return ([int((st == k).sum()) for k in range(5)], int((stopped & (result[:, 1] >= 8)).sum()), int((stopped & (result[:, 1] >= 4)).sum()))


def storage_segment(vox, W, grid):
    """the 64-cell tile segment (sx >> 6 of gvom_query.hip rq_index) of the STORAGE column that holds window voxel `vox`: the
    window column moved by the storage offset W[0] mod xy"""
    xy = GRIDS[grid][2]
    return (((np.asarray(vox, np.int64) % xy) + int(W[0]) % xy) % xy) >> 6


def segment_census(result, visits, W, grid):
    """(stop voxels per storage segment, rays whose examined voxels lie in two or more segments) of a walk's result and its
    recorded (ray, voxel) visits"""
    nseg = (GRIDS[grid][2] + 63) // 64
    stopped = result[:, 2] >= 0
    stops = np.bincount(storage_segment(result[stopped, 2], W, grid), minlength=nseg)
    v = np.asarray(visits, np.int64).reshape(-1, 2)
    seen = np.zeros((len(result), nseg), bool)
    seen[v[:, 0], storage_segment(v[:, 1], W, grid)] = True
    return [int(s) for s in stops], int((seen.sum(axis=1) >= 2).sum())


def state_class(state):
    """0 occupied, 1 never observed, 2 observed free: what a ray query reads of a dense state (the indices themselves differ
    between builders)"""
    state = np.asarray(state)
    return np.where(state >= 0, 0, np.where(state == -1, 1, 2)).astype(np.int8)


CENSUS_FLAGS = dict(unknown_blocks=True, check_target=False)      # the ONE call whose rays must show every status
STATUS_FLOOR = 32
STEP_FLOOR = {"p2": (8, 32), "np2": (8, 32), "tall": (4, 32), "w128": (8, 32), "w192": (8, 32)}     # (step, rays that stop at a voxel at or beyond it)
SEGMENT_STOP_FLOOR = 100                                          # WIDE: stop voxels in every storage segment
SEGMENT_CROSS_FLOOR = 300                                         # WIDE: rays whose examined voxels span >= 2 segments
