"""Shared by tests/test_align.py, tests/test_align_cpu.py and tests/_align_torch.py: the referee of gvom_score_alignments and the inputs
of those tests.

The referee (score) is a plain numpy restatement of the definition in include/gvom_hip.h "scan alignment scoring", one numpy operation
per operation of the definition, every one rounded once: the float64 transform in source order rounded to float32 (world), the literal
float64 endpoint lookup (voxels), the class of a voxel from a DENSE state array in the reference's voxel order (x + y * xy + z * xy *
xy: what Gvom.read_dense(GVOM_WHICH_FUSED) and the CPU referee's combined_index_map hold), the counts, the weighted score and the
lowest index of the best score.  tests/test_align_cpu.py pins world() and voxels() to the CPU referee's transform and scan kernels, so
that they cannot drift from the reference.  The maps are those of tests/raycast_ref.py (build_map); the cloud is the one of their last
scan, in the world frame, so the unperturbed candidate is the identity."""
import math

import numpy as np

import raycast_ref as rr

GRIDS = rr.GRIDS
ALL_GRIDS = ("p2", "np2", "tall", "w128", "w192", "far")
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
        vi = np.where(inside[..., None], v, 0.0).astype(np.int64)
        c = np.where(inside, cls[vi[..., 2], vi[..., 1], vi[..., 0]], OUTSIDE)
        for j in range(5):
            counts[k0:k0 + step, 1 + j] = (c == j).sum(axis=1)
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
