"""Shared by tests/test_align.py, tests/test_align_cpu.py and tests/_align_torch.py: the referee of gvom_score_alignments and the inputs
of those tests.

The referee (score) is a plain numpy restatement of the definition in include/gvom_hip.h "scan alignment scoring", one numpy operation
per operation of the definition, every one rounded once: the float64 transform in source order rounded to float32 (world), the literal
float64 endpoint lookup (voxels), the class of a voxel from a DENSE state array in the reference's voxel order (x + y * xy + z * xy *
xy: what Gvom.read_dense(GVOM_WHICH_FUSED) and the CPU referee's combined_index_map hold), the counts, the weighted score and the
lowest index of the best score.  tests/test_align_cpu.py pins world() and voxels() to the CPU referee's transform and scan kernels, so
that they cannot drift from the reference.  The maps are those of tests/raycast_ref.py (build_map); the cloud is the one of their last
scan, in the world frame, so the unperturbed candidate is the identity.  Next to them: planted maps (planted_map: sparse, with single
occupied voxels where the words, chunks and faces of k_align_field's class grid meet) and the line probes that look at every voxel of
the window (line_probes), and the edge inputs of k_align_score (edge_cloud, edge_candidates)."""
import math

import numpy as np

import raycast_ref as rr
import synth

GRIDS = rr.GRIDS
ALL_GRIDS = ("p2", "np2", "tall", "w128", "w192", "far")
# The alignment tests' own grids, under names of their own in the shared table (rr.build_map, rr.ego_of and rr.window_origin look
# grids up there; no test iterates over the table, and the explicit grid tuples of the ray and multi-origin tests stay as they are).
# RAGGED: rows that are no multiple of 16 voxels -- r72 has two tile segments, the second partial, rw = 5 with a half-filled last word
# and a partial last chunk of levels; r37 is odd, with a last word of 5 voxels.  OFF_GRID: the two resolutions of
# tests/test_hip_parity.py that are no multiple of anything, on a window like np2's.
RAGGED = {"r72": (0.4, 0.2, 72, 20), "r37": (0.4, 0.2, 37, 12)}
OFF_GRID = {"third": (1.0 / 3.0, 0.07, 48, 20), "odd": (0.123456789, 0.987654321, 48, 20)}
GRIDS.update(RAGGED)
GRIDS.update(OFF_GRID)
PROBE_GRIDS = ("np2", "tall", "w128", "w192", "r72", "r37")      # planted maps under the exhaustive probe
EDGE_GRIDS = ("p2", "np2", "tall", "w192", "far", "third", "odd")  # the score kernel at its edges, on the shared maps
F32 = np.float32
OCCUPIED, NEAR, FREE, UNKNOWN, OUTSIDE = range(5)             # class c is column 1 + c of the counts
DEFAULT_WEIGHTS = (2, 1, -1, 0, 0)
SCAN = rr.N_SCANS - 1                                         # the cloud held against the map: the last scan fused into it
XY_STEPS, YAW_STEPS, YAW_STEP = 3, 2, 0.02                    # 7 x 7 offsets of one cell, 5 yaws of 0.02 rad about the ego
N_GRID = (2 * XY_STEPS + 1) ** 2 * (2 * YAW_STEPS + 1)        # 245
CENTRE = N_GRID // 2                                          # the unperturbed candidate


def _res(grid):
    xr, zr, _, _ = GRIDS[grid]
    return np.array([xr, xr, zr], np.float64)


def world(cloud, M):
    """float32 [K, n, 3]: the returns `cloud` (float32 [n, 3]) under the candidates M (float64 [K, 3 or 4, 4]) -- gvom.py:1044-1052:
    products and sums in float64, left to right, rounded once to float32"""
    assert cloud.dtype == F32 and M.dtype == np.float64
    x, y, z = (cloud[None, :, k].astype(np.float64) for k in range(3))
    out = np.empty((len(M), len(cloud), 3), F32)
    with np.errstate(all="ignore"):
        for r in range(3):
            m = [M[:, r, k][:, None] for k in range(4)]
            out[:, :, r] = (((x * m[0] + y * m[1]) + z * m[2]) + m[3]).astype(F32)
    return out


def voxels(w, grid, W):
    """(v float64 [..., 3], inside bool [...]) of world positions w (float32 [..., 3]): gvom.py:1072-1080, floor((f64)w / res - W),
    inside iff 0 <= v < size on all three axes (compared in float64: NaN and infinities are outside)"""
    assert w.dtype == F32
    _, _, xy, zs = GRIDS[grid]
    with np.errstate(all="ignore"):
        v = np.floor(w.astype(np.float64) / _res(grid) - np.asarray(W, np.float64))
        inside = ((v >= 0) & (v < np.array([xy, xy, zs], np.float64))).all(axis=-1)
    return v, inside


def classes(state, grid, dilate):
    """uint8 [zs, xy, xy] ([z][y][x]): the class of every window voxel of the dense `state`"""
    _, _, xy, zs = GRIDS[grid]
    s = np.asarray(state).reshape(zs, xy, xy)
    occ = s >= 0
    near = np.zeros_like(occ)
    if dilate:
        pad = np.zeros((zs + 2, xy + 2, xy + 2), bool)             # voxels outside the window never count as neighbours
        pad[1:-1, 1:-1, 1:-1] = occ
        for dz in range(3):
            for dy in range(3):
                for dx in range(3):
                    near |= pad[dz:dz + zs, dy:dy + xy, dx:dx + xy]
    return np.where(occ, OCCUPIED, np.where(near, NEAR, np.where(s <= -2, FREE, UNKNOWN))).astype(np.uint8)


def class_counts(cls, v, inside):
    """int64 [K, 5]: per candidate the pairs of each class -- the class grid `cls` looked up at the voxels (v, inside) [K, n] of
    voxels(); a pair outside the window is OUTSIDE"""
    vi = np.where(inside[..., None], v, 0.0).astype(np.int64)
    c = np.where(inside, cls[vi[..., 2], vi[..., 1], vi[..., 0]], OUTSIDE)
    return np.stack([(c == j).sum(axis=1) for j in range(5)], axis=1).astype(np.int64)


def score(state, W, grid, cloud, M, dilate=0, weights=DEFAULT_WEIGHTS, cls=None):
    """(counts int32 [K, 6] {score, occupied, near, free, unknown, outside}, best int32 [4] {best index, best score, n, K})"""
    assert dilate in (0, 1)
    _, _, xy, zs = GRIDS[grid]
    cloud = np.ascontiguousarray(cloud, F32).reshape(-1, 3)
    M = np.asarray(M, np.float64)
    K, n = len(M), len(cloud)
    cls = classes(state, grid, dilate) if cls is None else cls
    counts = np.zeros((K, 6), np.int64)
    step = max(1, (1 << 21) // n)                                  # candidates per slice: bounded memory
    for k0 in range(0, K, step):
        v, inside = voxels(world(cloud, M[k0:k0 + step]), grid, W)
        counts[k0:k0 + step, 1:] = class_counts(cls, v, inside)
    assert (counts[:, 1:].sum(axis=1) == n).all()
    counts[:, 0] = (counts[:, 1:] * np.asarray(weights, np.int64)).sum(axis=1)
    best = int(np.argmax(counts[:, 0]))                            # numpy's argmax: the first of the maxima
    return counts.astype(np.int32), np.array([best, counts[best, 0], n, K], np.int32)


# ---- the shared inputs --------------------------------------------------------------------------------------------------------
def cloud_of(grid):
    """the float32 cloud held against the map: scan SCAN of tests/raycast_ref.py, in the world frame"""
    return rr.cloud_of(grid, SCAN)


def yaw_about(pivot, yaw, offset):
    """float64 [4, 4]: turn the world by `yaw` about the vertical through `pivot`, then move it by `offset`"""
    D = np.identity(4)
    c, s = math.cos(yaw), math.sin(yaw)
    D[0, 0], D[0, 1], D[1, 0], D[1, 1] = c, -s, s, c
    p = np.asarray(pivot, np.float64)
    D[:3, 3] = p - D[:3, :3].dot(p) + np.asarray(offset, np.float64)
    return D


def grid_candidates(grid):
    """float64 [245, 4, 4]: 7 x 7 offsets of one cell and 5 yaws of 0.02 rad about the last ego, x offset fastest, then y, then yaw;
    candidate CENTRE is the identity.  (gvom.pose_candidates(identity, ...) returns the same: tests/test_align_cpu.py)"""
    xr = GRIDS[grid][0]
    ego = np.array(rr.ego_of(grid, SCAN), np.float64)
    out = []
    for a in range(-YAW_STEPS, YAW_STEPS + 1):
        for j in range(-XY_STEPS, XY_STEPS + 1):
            for i in range(-XY_STEPS, XY_STEPS + 1):
                out.append(np.identity(4) if (a, j, i) == (0, 0, 0) else yaw_about(ego, a * YAW_STEP, (i * xr, j * xr, 0.0)))
    return np.array(out)


SPECIALS = ("the centre again", "every return outside", "a NaN entry", "beyond float32")


def candidates(grid):
    """float64 [249, 4, 4]: the 245 of grid_candidates and four specials -- the centre candidate once more (the lower index wins the
    tie), a translation that puts every return outside the window, a matrix with a NaN entry, a translation that overflows float32"""
    M = grid_candidates(grid)
    xr, zr, xy, zs = GRIDS[grid]
    again = M[CENTRE].copy()
    away = np.identity(4)
    away[:3, 3] = (3.0 * xr * xy, -3.0 * xr * xy, 3.0 * zr * zs)
    nan = M[CENTRE + 1].copy()
    nan[1, 2] = np.nan
    huge = np.identity(4)
    huge[0, 3] = 1e39
    return np.concatenate([M, np.array([again, away, nan, huge])])


def rotations():
    """float64 [.., 4, 4]: rotations about all three axes, combined, with small and large translations (the transform pin)"""
    rng = np.random.default_rng(21)
    out = []
    for k in range(24):
        a = rng.uniform(-np.pi, np.pi, 3) * (np.arange(3) == k % 3 if k < 12 else 1.0)
        cx, cy, cz = np.cos(a)
        sx, sy, sz = np.sin(a)
        R = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]).dot(np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]]))
             .dot(np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])))
        T = np.identity(4)
        T[:3, :3] = R
        T[:3, 3] = rng.uniform(-1, 1, 3) * (10.0 if k % 2 else 7.0e6)
        out.append(T)
    return np.array(out)


def boundary_points(grid, W):
    """float32 [m, 3]: points on exact voxel boundaries ((W_r + j) * res_r rounded to float32), their float32 neighbours on both
    sides, on every face of the window and inside it, and the same around zero on both signs"""
    _, _, xy, zs = GRIDS[grid]
    res, size = _res(grid), np.array([xy, xy, zs])
    W = np.asarray(W, np.float64)
    centre = ((W + size / 2.0 + 0.5) * res).astype(F32)
    pts = []
    for r in range(3):
        js = sorted({-1, 0, 1, 2, int(size[r]) // 2, int(size[r]) - 1, int(size[r]), int(size[r]) + 1} | {int(-W[r]) + d for d in (-1, 0, 1)})
        for j in js:
            b = F32((W[r] + j) * res[r])
            for v in (np.nextafter(b, F32(-np.inf)), b, np.nextafter(b, F32(np.inf))):
                p = centre.copy()
                p[r] = v
                pts.append(p)
        for v in (F32(0.0), F32(-0.0), np.nextafter(F32(0), F32(1)), np.nextafter(F32(0), F32(-1)), F32(res[r]), F32(-res[r])):
            p = centre.copy()
            p[r] = v
            pts.append(p)
    return np.array(pts, F32)


def totals(counts):
    """the five class counts summed over the candidates"""
    return [int(v) for v in counts[:, 1:].astype(np.int64).sum(axis=0)]


# Floors of the census, summed over the 245 grid candidates, per dilate and class: a little under the smallest figure the referee gives
# on any of CENSUS_GRIDS and either ring length, on the CPU referee's maps (tests/test_align_cpu.py prints them all; its docstring
# quotes them).  The smallest are all the tall grid's, with its 384 returns; FLOORS_8192 holds the grids of 8,192 returns to their own.
# The far grid is left out of the census: at 7e6 m a float32 coordinate moves in steps of half a metre, more than a voxel, so
# neighbouring candidates place the cloud identically and no candidate is the unique best.
CENSUS_GRIDS = ("p2", "np2", "tall", "w128", "w192")
FLOORS = {0: {OCCUPIED: 9500, FREE: 29000, UNKNOWN: 20000, OUTSIDE: 33000},
          1: {NEAR: 46000, FREE: 700, UNKNOWN: 1800}}
FLOORS_8192 = {0: {OCCUPIED: 60000, UNKNOWN: 135000}}
DISTINCT_ROWS = 242


def census_holds(grid, dilate, counts):
    """asserts the floors on the counts of the 245 grid candidates; returns the totals"""
    t = totals(counts[:N_GRID])
    for c, floor in FLOORS.get(dilate, {}).items():
        assert t[c] >= floor, (grid, dilate, c, t)
    if GRIDS[grid] != GRIDS["tall"]:
        for c, floor in FLOORS_8192.get(dilate, {}).items():
            assert t[c] >= floor, (grid, dilate, c, t)
    return t


# ---- planted maps: sparse, with single occupied voxels where k_align_field's words, chunks and faces meet -------------------------
PLANT_RETURNS, PLANT_SEED = 64, 500
CARRY_FLOOR = 21      # a lone occupied voxel next to a word boundary makes 3 x 3 NEAR voxels beyond it, 2 x 3 on the bottom and the top
#                       level: 6 + 9 + 6 from the levels {0, zs // 2, zs - 1} that every planted grid has


def planted_voxels(grid):
    """int64 [m, 3] (x, y, z), distinct window voxels: x = 0, xy - 1 and both sides of every multiple of 16, each on the levels
    {0, zs // 2, zs - 1} and, where zs > 16, {15, 16}; rows y = 0 and y = xy - 1 on the same levels; four corners.  The k-th voxel
    lies on row (or, in the second part, column) (4 k + 2) % xy, the level changing slowest: every voxel of the first part has a
    (y, z) line of its own and its neighbours to itself.  The scan drops a return closer than min_distance to the WORLD's origin
    (gvom.py:1064-1067), which lies inside the window: a voxel of the first part whose centre is that close moves two rows on,
    between its neighbours' rows (np2's (15, 30, 10) is the only one)."""
    _, _, xy, zs = GRIDS[grid]
    W, res = rr.window_origin(grid, rr.ego_of(grid, SCAN)), _res(grid)
    levels = sorted({0, zs // 2, zs - 1} | ({15, 16} if zs > 16 else set()))
    xs = sorted({0, xy - 1} | {b - d for b in range(16, xy, 16) for d in (0, 1)})
    out = []
    for z in levels:
        for x in xs:
            y = (4 * len(out) + 2) % xy
            if np.linalg.norm(((W + (x, y, z) + 0.5) * res).astype(F32).astype(np.float64)) < synth.REF_TAIL[0]:
                y = (y + 2) % xy
            out.append((x, y, z))
    assert len({(y, z) for _, y, z in out}) == len(out)
    for z in levels:
        for y in (0, xy - 1):
            out.append(((4 * len(out) + 2) % xy, y, z))
    out += [(0, 0, 0), (xy - 1, 0, zs - 1), (0, xy - 1, zs - 1), (xy - 1, xy - 1, 0)]
    return np.array(list(dict.fromkeys(out)), np.int64)


def planted_cloud(grid, k):
    """float32 returns of scan k of a planted map: PLANT_RETURNS uniform returns over 1.2 windows and the whole window height; on
    the last scan also one return at the float32 centre of every planted voxel of the final window"""
    xr, zr, xy, zs = GRIDS[grid]
    ego = rr.ego_of(grid, k)
    wx, wz = xr * xy, zr * zs
    pc = synth.uniform_cloud(PLANT_RETURNS, PLANT_SEED + k, (ego[0] - 0.6 * wx, ego[0] + 0.6 * wx), (ego[1] - 0.6 * wx, ego[1] + 0.6 * wx),
                                (ego[2] - 0.55 * wz, ego[2] + 0.55 * wz), np.float64).astype(F32)
    if k == SCAN:
        centres = (rr.window_origin(grid, ego) + planted_voxels(grid) + 0.5) * _res(grid)
        pc = np.concatenate([pc, centres.astype(F32)])
    return np.ascontiguousarray(pc)


def planted_map(cls, grid, buffer_size, **kw):
    """as rr.build_map -- the same four scans with a combine after each, the same moving egos (non-zero storage offsets, stale
    tiles) -- with the planted clouds; returns the mapper of class `cls`"""
    g = cls(*rr.params(grid, buffer_size), **kw)
    for k in range(rr.N_SCANS):
        g.process_pointcloud(planted_cloud(grid, k), rr.ego_of(grid, k))
        g.combine_maps()
    return g


def line_probes(grid, W):
    """three (cloud float32 [n, 3], candidates float64 [K, 4, 4]), one per axis: the centres of the voxels of the window line along
    that axis through voxel (0, 0, 0), and the translations by whole cells over the other two axes (the lower axis fastest).  Under
    candidate k the cloud is one whole line of the window: a pair's counts are the class histogram of every such line, and the
    three pairs together look at every window voxel three times.  Asserted here, on the referee: every pair lies inside the window
    and every window voxel is met exactly once per axis."""
    _, _, xy, zs = GRIDS[grid]
    res, size = _res(grid), (xy, xy, zs)
    W = np.asarray(W, np.float64)
    out = []
    for a in range(3):
        b, c = [r for r in range(3) if r != a]
        v = np.zeros((size[a], 3))
        v[:, a] = np.arange(size[a])
        cloud = np.ascontiguousarray(((W + v + 0.5) * res).astype(F32))
        k = np.arange(size[b] * size[c])
        M = np.tile(np.identity(4), (len(k), 1, 1))
        M[:, b, 3] = (k % size[b]) * res[b]
        M[:, c, 3] = (k // size[b]) * res[c]
        at, inside = voxels(world(cloud, M), grid, W)
        assert inside.all(), (grid, a)
        flat = (at[..., 0] + at[..., 1] * xy + at[..., 2] * xy * xy).astype(np.int64).ravel()
        assert len(flat) == xy * xy * zs and (np.bincount(flat, minlength=xy * xy * zs) == 1).all(), (grid, a)
        out.append((cloud, M))
    return out


def carry_census(cls1, state, grid):
    """per multiple b of 16 inside a row: (NEAR voxels at x = b - 1 whose occupied neighbours all lie at x = b, NEAR voxels at
    x = b whose occupied neighbours all lie at x = b - 1) of the dilated class grid cls1 of `state` -- voxels whose class is
    decided by the bit carried across a word boundary of the class grid, in either direction"""
    _, _, xy, zs = GRIDS[grid]
    occ = np.asarray(state).reshape(zs, xy, xy) >= 0
    pad = np.zeros((zs + 2, xy + 2, xy + 4), bool)
    pad[1:-1, 1:-1, 2:-2] = occ
    col = np.zeros_like(pad[1:-1, 1:-1])                         # col[z, y, x + 2]: an occupied voxel at column x within one voxel in y and z
    for dz in range(3):
        for dy in range(3):
            col |= pad[dz:dz + zs, dy:dy + xy]
    near = cls1 == NEAR
    out = {}
    for b in range(16, xy, 16):
        left = near[:, :, b - 1] & col[:, :, b + 2] & ~col[:, :, b + 1] & ~col[:, :, b]
        right = near[:, :, b] & col[:, :, b + 1] & ~col[:, :, b + 2] & ~col[:, :, b + 3]
        out[b] = (int(left.sum()), int(right.sum()))
    return out


def planted_census_holds(state, grid):
    """asserts, on the dense `state` of a planted map: every planted voxel is OCCUPIED; at every multiple of 16 in x at least
    CARRY_FLOOR voxels on either side are NEAR by the carry alone; there are NEAR voxels on the bottom and the top level, on rows 0
    and xy - 1 and, where zs > 16, on levels 15 and 16.  Returns (planted, occupied in total, the smallest carry count)"""
    _, _, xy, zs = GRIDS[grid]
    cls1 = classes(state, grid, 1)
    p = planted_voxels(grid)
    assert (cls1[p[:, 2], p[:, 1], p[:, 0]] == OCCUPIED).all(), (grid, p[cls1[p[:, 2], p[:, 1], p[:, 0]] != OCCUPIED])
    carry = carry_census(cls1, state, grid)
    assert sorted(carry) == list(range(16, xy, 16)) and all(min(v) >= CARRY_FLOOR for v in carry.values()), (grid, carry)
    near = cls1 == NEAR
    for z in (0, zs - 1) + ((15, 16) if zs > 16 else ()):
        assert near[z].any(), (grid, "level", z)
    assert near[:, 0].any() and near[:, xy - 1].any(), grid
    return len(p), int((cls1 == OCCUPIED).sum()), min([min(v) for v in carry.values()] or [0])


# ---- the score kernel at its edges ---------------------------------------------------------------------------------------------------
EDGE_RETURNS = 2048
EDGE_ANGLES = (0.05, -0.05, 0.3, -0.3, np.pi / 2, np.pi)


def edge_cloud(grid, W):
    """(float32 [<= 2048, 3], m): the m boundary_points of the window, then returns of the shared cloud"""
    b = boundary_points(grid, W)
    return np.ascontiguousarray(np.concatenate([b, cloud_of(grid)])[:EDGE_RETURNS]), len(b)


def edge_candidates(grid, W):
    """float64 [49, 4, 4]: the identity; one voxel up and down every axis; rotations about the window centre around each of the three
    axes by EDGE_ANGLES; rotations()"""
    _, _, xy, zs = GRIDS[grid]
    res = _res(grid)
    centre = (np.asarray(W, np.float64) + np.array([xy, xy, zs]) / 2.0) * res
    out = [np.identity(4)]
    for r in range(3):
        for sign in (1.0, -1.0):
            T = np.identity(4)
            T[r, 3] = sign * res[r]
            out.append(T)
    for r in range(3):
        i, j = [k for k in range(3) if k != r]
        for a in EDGE_ANGLES:
            T = np.identity(4)
            T[i, i], T[i, j], T[j, i], T[j, j] = math.cos(a), -math.sin(a), math.sin(a), math.cos(a)
            T[:3, 3] = centre - T[:3, :3].dot(centre)
            out.append(T)
    return np.concatenate([np.array(out), rotations()])


def upper_pairs(grid, W, cloud, M):
    """the pairs that land in the upper 30 % of the window"""
    v, inside = voxels(world(cloud, M), grid, W)
    return int((inside & (v[..., 2] >= 0.7 * GRIDS[grid][3])).sum())


# Floors of the edge census, summed over the 49 candidates, per dilate and class: a little under the smallest figure the referee gives
# on the CPU referee's maps over the grids and both ring lengths (tests/test_align_cpu.py prints them all; its docstring quotes
# them).  The smallest of EDGE_FLOORS are the tall grid's (498 returns) but for FREE under dilate 1 (np2's 72).  The far
# grid has floors of its own: all four of its scans are uniform clouds, and only 5 pairs in all end in a FREE voxel (floor 1).
EDGE_FLOORS = {0: {OCCUPIED: 2100, FREE: 3900, UNKNOWN: 2700, OUTSIDE: 15000},
               1: {OCCUPIED: 2100, NEAR: 5900, FREE: 65, UNKNOWN: 690, OUTSIDE: 15000}}
EDGE_FLOORS_FAR = {0: {OCCUPIED: 19000, FREE: 1, UNKNOWN: 10500, OUTSIDE: 70000},
                   1: {OCCUPIED: 19000, NEAR: 7900, UNKNOWN: 2750, OUTSIDE: 70000}}
UPPER_FLOOR, UPPER_FLOOR_TALL = 2200, 500                     # (odd 2,268; tall 526)
BOUNDARY_FLOOR = 20                                           # boundary points inside and outside the window under the identity


def edge_census_holds(grid, W, dilate, cloud, m, M, counts):
    """asserts the floors on the counts of the edge candidates, the pairs in the upper 30 % of the window and the boundary points on
    either side of the window's faces; returns (totals, upper pairs, boundary points inside, outside)"""
    t = totals(counts)
    for c, floor in (EDGE_FLOORS_FAR if grid == "far" else EDGE_FLOORS)[dilate].items():
        assert t[c] >= floor, (grid, dilate, c, t)
    up = upper_pairs(grid, W, cloud, M)
    assert up >= (UPPER_FLOOR_TALL if GRIDS[grid] == GRIDS["tall"] else UPPER_FLOOR), (grid, up)
    _, inside = voxels(world(cloud[:m], M[:1]), grid, W)
    assert np.array_equal(M[0], np.identity(4)) and inside.sum() >= BOUNDARY_FLOOR and (~inside).sum() >= BOUNDARY_FLOOR, (grid, inside.sum())
    return t, up, int(inside.sum()), int((~inside).sum())
