"""Shared by tests/test_viewpoints.py, tests/test_viewpoints_cpu.py and tests/_viewpoints_torch.py: the referee of
gvom_score_viewpoints and the inputs of those tests.

The referee (product) is plain numpy: the beam targets in the operation order of include/gvom_hip.h "viewpoint scoring" (numpy does
not fuse a multiply and an add), raycast_ref.walk(..., record=True) per viewpoint -- the referee of gvom_raycast, which
tests/test_raycast_cpu.py pins to the oracle --, a histogram of the statuses, the sum of the `unknown` column, and np.unique over the
recorded voxels whose class is never-observed.  product_sets is a second, independent form of the counting: one Python set of
(x, y, z) tuples per viewpoint, fed voxel by voxel from the same recorded visits."""
import math

import numpy as np

import raycast_ref as rr

F32 = np.float32
# a grid of this file's own, next to those of tests/raycast_ref.py (whose parametrisations it does not change: they iterate over WIDE,
# FAR and tests/multi_origin_ref.py GRIDS): 256 x 256 x 48 voxels, a bitmap of 393,216 bytes -- with "viewpoint_bitmap_mb" = 1 a
# launch holds exactly TWO viewpoints
rr.GRIDS.setdefault("v256", (0.2, 0.2, 256, 48))
GRID_NAMES = ("p2", "np2", "tall", "w128", "far", "v256")


# ---- sensor models ------------------------------------------------------------------------------------------------------------------
def lidar_model(H, W, el_lo=-40.0, el_hi=40.0):
    """directions float64 [H, W, 3]: H beams between two elevations, W columns around the vertical"""
    el = np.radians(np.linspace(el_lo, el_hi, H))[:, None]
    az = (np.arange(W) * (2.0 * math.pi / W))[None, :]
    return np.ascontiguousarray(np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) * np.ones_like(az)], axis=2))


def model(name):
    """(directions [H, W, 3], offsets [H, W, 3] or None) of the tests' sensor models:
      m8x64    one full wave per row
      m5x37    a partial wave; rows that do not fill one
      m16x256  four waves per row (with strides (3, 5): 6 rows of 52 beams)
      nan8x64  m8x64 with a NaN component in three pixels (rows 0, 3 and 7) and an infinite one in a fourth
      off5x37  m5x37 with offsets of up to 6 cm"""
    if name == "m8x64":
        return lidar_model(8, 64), None
    if name == "m5x37":
        return lidar_model(5, 37), None
    if name == "m16x256":
        return lidar_model(16, 256), None
    if name == "nan8x64":
        d = lidar_model(8, 64)
        d[0, 5, 1] = np.nan
        d[3, 63, 0] = np.nan
        d[7, 0, 2] = np.nan
        d[4, 17, 0] = np.inf
        return d, None
    if name == "off5x37":
        d = lidar_model(5, 37)
        return d, np.ascontiguousarray(np.random.default_rng(11).uniform(-0.06, 0.06, d.shape))
    raise KeyError(name)


def selected(H, W, strides):
    """pixel indices h * W + w of the selected beams, row by row, and their rows h"""
    hs, ws = np.arange(0, H, strides[0]), np.arange(0, W, strides[1])
    return (hs[:, None] * W + ws[None, :]).reshape(-1), np.repeat(hs, len(ws))


# ---- the definition -----------------------------------------------------------------------------------------------------------------
def rows34(poses):
    a = np.asarray(poses, np.float64)
    if a.ndim == 2:
        a = a[None]
    return np.ascontiguousarray(a[:, :3, :])


def targets(directions, offsets, pose, max_range, strides=(1, 1)):
    """(a float32 [3], b float32 [nb, 3]) of one pose (float64 [3, 4]): float64, one rounding per operation, in the header's order"""
    d = np.asarray(directions, np.float64)
    H, W = d.shape[:2]
    pick, _ = selected(H, W, strides)
    d = d.reshape(-1, 3)[pick]
    o = np.zeros_like(d) if offsets is None else np.asarray(offsets, np.float64).reshape(-1, 3)[pick]
    C = np.asarray(pose, np.float64).reshape(12)
    with np.errstate(all="ignore"):
        p = np.float64(max_range) * d
        p = p + o
        q = np.empty_like(p)
        for c in range(3):
            m0, m1, m2 = p[:, 0] * C[4 * c], p[:, 1] * C[4 * c + 1], p[:, 2] * C[4 * c + 2]
            q[:, c] = ((m0 + m1) + m2) + C[4 * c + 3]
        return C[[3, 7, 11]].astype(F32), q.astype(F32)


def origin_status(state, W, grid, a):
    xr, zr, xy, zs = rr.GRIDS[grid]
    with np.errstate(all="ignore"):
        v = np.floor(a.astype(np.float64) / np.array([xr, xr, zr]) - np.asarray(W, np.float64))
    if not ((v >= 0) & (v < np.array([xy, xy, zs]))).all():
        return rr.LEFT_WINDOW
    s = state[int(v[0]) + int(v[1]) * xy + int(v[2]) * xy * xy]
    return rr.OCCUPIED if s >= 0 else (rr.UNKNOWN if s == -1 else rr.CLEAR)


def viewpoint(state, W, grid, directions, offsets, pose, max_range, strides=(1, 1), unknown_blocks=False, f32_sqrt=False):
    """(row int32 [8], the walk's result [nb, 4], its recorded (beam, voxel) visits) of ONE pose [3, 4]"""
    H, Wm = np.asarray(directions).shape[:2]
    nb = len(selected(H, Wm, strides)[0])
    row = np.zeros(8, np.int64)
    if not np.isfinite(pose).all():
        row[0], row[7] = rr.INVALID, nb
        return row.astype(np.int32), None, []
    a, b = targets(directions, offsets, pose, max_range, strides)
    result, _, visits = rr.walk(state, W, grid, a[None], b, unknown_blocks=unknown_blocks, f32_sqrt=f32_sqrt, record=True)
    row[0] = origin_status(state, W, grid, a)
    v = np.asarray(visits, np.int64).reshape(-1, 2)
    unknown = v[rr.state_class(state[v[:, 1]]) == 1, 1]
    row[1] = len(np.unique(unknown))
    row[2] = result[:, 3].sum()
    for col, code in ((3, rr.OCCUPIED), (4, rr.CLEAR), (5, rr.LEFT_WINDOW), (6, rr.UNKNOWN), (7, rr.INVALID)):
        row[col] = (result[:, 0] == code).sum()
    assert row[3:].sum() == nb and row[2] == len(unknown)
    return row.astype(np.int32), result, visits


def best_of(rows, nb):
    rows = np.asarray(rows)
    ok = np.flatnonzero(rows[:, 0] == rr.CLEAR)
    if not len(ok):
        return np.array([-1, 0, len(rows), nb], np.int32)
    k = ok[np.argmax(rows[ok, 1])]                                       # (argmax: the first of the largest)
    return np.array([k, rows[k, 1], len(rows), nb], np.int32)


def product(state, W, grid, directions, offsets, poses, max_range, strides=(1, 1), unknown_blocks=False, f32_sqrt=False):
    """(rows int32 [K, 8], best int32 [4]): parts 0 and 1 of the product"""
    P = rows34(poses)
    rows = np.stack([viewpoint(state, W, grid, directions, offsets, p, max_range, strides, unknown_blocks, f32_sqrt)[0] for p in P])
    H, Wm = np.asarray(directions).shape[:2]
    return rows, best_of(rows, len(selected(H, Wm, strides)[0]))


def product_sets(state, W, grid, directions, offsets, poses, max_range, strides=(1, 1), unknown_blocks=False):
    """the second form: gain as the size of a Python set of (x, y, z) tuples, visits as a plain count, voxel by voxel"""
    xr, zr, xy, zs = rr.GRIDS[grid]
    rows = []
    for p in rows34(poses):
        row, result, visits = viewpoint(state, W, grid, directions, offsets, p, max_range, strides, unknown_blocks)
        seen, count = set(), 0
        for _, vox in visits:
            if state[vox] == -1:
                seen.add((vox % xy, vox // xy % xy, vox // (xy * xy)))
                count += 1
        rows.append([int(row[0]), len(seen), count] + [int(v) for v in row[3:]])
    rows = np.array(rows, np.int32)
    H, Wm = np.asarray(directions).shape[:2]
    return rows, best_of(rows, len(selected(H, Wm, strides)[0]))


# ---- the shared inputs: viewpoints ----------------------------------------------------------------------------------------------------
def pose_of(xyz, yaw=0.0, pitch=0.0):
    """float64 [4, 4]: a yaw about z applied after a pitch about y, at xyz"""
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    T = np.identity(4)
    T[:3, :3] = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]]).dot(np.array([[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]]))
    T[:3, 3] = xyz
    return T


def _frontier_voxels(state, grid):
    """window voxels that are observed free and have a never-observed 6-neighbour, in index order"""
    xr, zr, xy, zs = rr.GRIDS[grid]
    cls = rr.state_class(state).reshape(zs, xy, xy)
    unk = cls == 1
    near = np.zeros_like(unk)
    near[1:] |= unk[:-1]; near[:-1] |= unk[1:]
    near[:, 1:] |= unk[:, :-1]; near[:, :-1] |= unk[:, 1:]
    near[:, :, 1:] |= unk[:, :, :-1]; near[:, :, :-1] |= unk[:, :, 1:]
    return np.flatnonzero(((cls == 2) & near).reshape(-1))


def viewpoints_of(grid, state, W, K):
    """float64 [K, 4, 4], K in (1, 3, 33).  1: the last ego.  3: the ego, and TWICE the same pose in an observed-free voxel next to
    a never-observed one.  33: those three, then the centre of an occupied voxel [3], of a never-observed one [4], a pose 3 voxels
    outside the window [5], one a quarter voxel outside its -x face, whose beams towards +x re-enter with their first step [6], the
    ego pitched by 0.4 rad [7]; [16] is NaN in one entry; every other pose sits in an observed-free voxel next to a never-observed one
    (spread over the window), yawed by 0.37 k and pitched by 0.11 (k mod 5 - 2) rad."""
    assert K in (1, 3, 33)
    xr, zr, xy, zs = rr.GRIDS[grid]
    res = np.array([xr, xr, zr])
    W = np.asarray(W, np.float64)
    ego = np.array(rr.ego_of(grid, rr.N_SCANS - 1), np.float64)
    free = rr._centres(rr._spread(_frontier_voxels(state, grid), 33), W, grid)
    out = [pose_of(ego)]
    if K >= 3:
        out += [pose_of(free[1], 0.6, -0.1)] * 2
    if K == 33:
        occ = rr._centres(rr._spread(np.flatnonzero(state >= 0), 3), W, grid)[1]
        unk = rr._centres(rr._spread(np.flatnonzero(state == -1), 3), W, grid)[1]
        mid = (W + np.array([xy, xy, zs]) / 2.0) * res
        outside = mid + np.array([(xy / 2.0 + 3.0) * xr, 0.0, 0.0])
        edge = mid - np.array([(xy / 2.0 + 0.25) * xr, 0.0, 0.0])
        out += [pose_of(occ), pose_of(unk, 1.0), pose_of(outside), pose_of(edge), pose_of(ego, 0.0, 0.4)]
        for k in range(8, 33):
            out.append(pose_of(free[k], 0.37 * k, 0.11 * (k % 5 - 2)))
        out[16] = out[16].copy()
        out[16][1, 2] = np.nan
    return np.stack(out)


def max_range_of(grid, which):
    """"short": less than one step (S = 0: every beam CLEAR, no voxel examined); "third": about a third of the window; "long":
    one and a half windows (beams that meet nothing leave the window)"""
    xr, zr, xy, zs = rr.GRIDS[grid]
    return {"short": 0.4 * min(xr, zr), "third": xr * xy / 3.0, "long": 1.5 * xr * xy}[which]


# (grid, ring slots, model, strides, K, range, unknown_blocks): what tests/test_viewpoints.py holds to the referee and
# tests/test_viewpoints_cpu.py takes the census of
CASES = (
    ("p2", 1, "m8x64", (1, 1), 33, "third", False),
    ("p2", 2, "m8x64", (1, 1), 33, "third", True),
    ("np2", 1, "m5x37", (1, 1), 33, "third", False),
    ("np2", 2, "nan8x64", (1, 1), 33, "third", True),
    ("tall", 1, "m8x64", (1, 1), 33, "third", True),
    ("tall", 2, "off5x37", (1, 1), 33, "third", False),
    ("w128", 1, "m16x256", (1, 1), 3, "third", False),
    ("w128", 2, "m16x256", (3, 5), 33, "third", True),
    ("far", 1, "m5x37", (1, 1), 33, "third", False),
    ("far", 2, "m8x64", (1, 1), 33, "third", True),
    ("v256", 1, "m8x64", (1, 1), 33, "third", False),
    # the other ranges and K = 1: conditions of their own (has_floors)
    ("p2", 1, "m5x37", (1, 1), 1, "short", False),
    ("p2", 2, "off5x37", (1, 1), 3, "short", True),
    ("np2", 2, "off5x37", (1, 1), 3, "long", True),
    ("tall", 2, "nan8x64", (1, 1), 3, "long", False),
    ("w128", 1, "m8x64", (1, 1), 1, "long", False),
)


def has_floors(case):
    """the census floors of tests/test_viewpoints_cpu.py hold for the cases at a third of the window; "short" admits no step
    (every beam CLEAR, gain 0) and "long" lets no beam end CLEAR"""
    return case[5] == "third"


def case_id(case):
    grid, bs, name, strides, K, rng, ub = case
    return "%s-b%d-%s-s%dx%d-K%d-%s-%s" % (grid, bs, name, strides[0], strides[1], K, rng, "ub" if ub else "count")


def case_inputs(case, state, W):
    """(directions, offsets, poses [K, 4, 4], max_range) of a case on the map (state, W)"""
    grid, bs, name, strides, K, rng, ub = case
    d, o = model(name)
    return d, o, viewpoints_of(grid, state, W, K), max_range_of(grid, rng)


def census(case, state, W):
    """what the referee alone shows of a case: rows, best, beam endings summed over the viewpoints, viewpoints with visits > gain,
    never-observed voxels examined by beams of at least two different model rows (in any one viewpoint)"""
    grid, bs, name, strides, K, rng, ub = case
    d, o, poses, r = case_inputs(case, state, W)
    H, Wm = d.shape[:2]
    _, beam_row = selected(H, Wm, strides)
    rows, shared = [], 0
    for p in rows34(poses):
        row, result, visits = viewpoint(state, W, grid, d, o, p, r, strides, ub)
        rows.append(row)
        v = np.asarray(visits, np.int64).reshape(-1, 2)
        v = v[state[v[:, 1]] == -1] if len(v) else v
        if len(v):
            pairs = np.unique(np.stack([v[:, 1], beam_row[v[:, 0]]], axis=1), axis=0)      # (voxel, model row), distinct
            shared += int((np.bincount(np.unique(pairs[:, 0], return_inverse=True)[1]) >= 2).sum())
    rows = np.stack(rows)
    return dict(rows=rows, best=best_of(rows, len(beam_row)), endings=rows[:, 3:].sum(axis=0), dedup=int((rows[:, 2] > rows[:, 1]).sum()),
                gainful=int((rows[:, 1] > 0).sum()), shared_across_rows=shared, statuses=sorted(set(rows[:, 0].tolist())))
