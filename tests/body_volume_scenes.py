"""The physical statement of body volumes, held on the GPU's result (tests/test_body_volume.py) and on the CPU oracle's maps
(tests/test_body_volume_cpu.py) alike: one scan, combine, integrate, distance field, body volume, pose field, path.

  half   the gate scene's grid (tests/body_scenes.py: 48 x 48 x 16 at 0.25 / 0.2 m), FLAT ground at 0.1 m everywhere, and the bar at
         x = 2 m and z = 2.1 m spanning only y < 1 m.  The drive goes from (-3, -2, heading 0) to the cell of (4, -2) at any heading: beyond the bar
         in the same lane (a goal that fixed heading 0 there leaves the tall body no room to swing back into the lane between the
         bar and the window's edge, so it is the cell that is the goal).
         With the low body the path crosses x = 2 m under the bar (y < 1 m); with the tall body it crosses at y >= 1 m, round the bar's
         end, and the drive is dearer: D_tall > D_low.
  full   body_scenes' own gate: the bar over every y.  The tall body's start state is unreached, the low body's is reached.

The 2-D cost is 1 everywhere: the pose field alone cannot tell the bar from free space.  Every status but OK blocks (body_blocks =
BLOCKS): a state on unknown ground or at the window's edge is no way round the bar.  The bodies are body_scenes.bodies()."""
import functools

import numpy as np

import attitude_ref as ar
import body_ref as br
import body_scenes as bs
import body_volume_ref as bv
import posefield_ref as pf
import voxel_atlas_ref as va
import voxel_distance_ref as vd

SCENE = bs.SCENES["gate"]
HEADINGS, CHASSIS, CAP, MIN_MARGIN = bs.HEADINGS, bs.CHASSIS, bs.CAP, bs.MIN_MARGIN
SOFT_MARGIN = np.float32(0.4)
SQUEEZE_WEIGHT = 1
BLOCKS = (br.COLLISION, br.LEFT_BOX, br.UNKNOWN_GROUND, br.LEFT_WINDOW)
BAR_END_Y = 1.0
START, GOAL = (-3.0, -2.0, 0), (4.0, -2.0, -1)              # (x, y in metres, heading index; -1: the goal cell at any heading)


@functools.lru_cache(maxsize=None)
def cloud(bar):
    """the scene's one scan, float32 [N, 3]; shared, read-only"""
    if bar == "full":
        return bs.cloud("gate")
    gx, gy = bs._grid(-5.6, 5.6, -5.6, 5.6, 0.06)
    bx, by = bs._grid(bs.BAR_X + 0.02, bs.BAR_X + 0.25, -5.6, BAR_END_Y, 0.04)
    pts = np.concatenate([np.stack([gx, gy, np.full(gx.shape, 0.1)], 1), np.stack([bx, by, np.full(bx.shape, bs.BAR_Z)], 1)], 0)
    return np.ascontiguousarray(pts.astype(np.float32))


@functools.lru_cache(maxsize=None)
def tables():
    """(footprint table, primitive table): a small rectangle and forward arcs, 16 headings"""
    import gvom
    res = SCENE["res"]
    return gvom.rectangle_footprint(0.9, 0.5, 0.35, res, headings=HEADINGS), gvom.arc_primitives(HEADINGS, 1.0, res, reach=3)


def cost_map():
    return np.ones((SCENE["xy"], SCENE["xy"]), np.uint16)


def cell_of(W, x, y):
    """the window cell of a world point, W the window's origin in cells"""
    res = SCENE["res"]
    return int(np.floor(x / res)) - int(W[0]), int(np.floor(y / res)) - int(W[1])


def follow(action, table, x, y, h):
    """DevicePoseField.path_from() on host arrays: the states to a goal, None where unreached"""
    import gvom
    start, prims = table
    path = [(x, y, h)]
    for _ in range(action.size):
        k = int(action[h, x, y])
        if k == gvom.POSE_GOAL:
            return path
        if k == gvom.CTG_NONE:
            return None
        assert k < start[h + 1] - start[h]
        dx, dy, ht, _w = (int(v) for v in prims[start[h] + k])
        x, y, h = x + dx, y + dy, ht
        path.append((x, y, h))
    raise AssertionError("the actions do not lead to a goal")


@functools.lru_cache(maxsize=None)
def oracle_maps(bar):
    """(field float32 [x, y, z], W the window's origin in voxels, ground float64 [x, y]) from the CPU oracle's maps alone: a
    VoxelAtlasRef fed from the oracle, then voxel_distance_ref"""
    from oracle import oracle
    res, zres, xy, zs = SCENE["res"], SCENE["zres"], SCENE["xy"], SCENE["zs"]
    o = oracle.OracleGvom(res, zres, xy, zs, 1, *va.DRIVE_TAIL)
    o.process_pointcloud(cloud(bar), SCENE["ego"])
    o.combine_maps()
    W = tuple(int(v) for v in np.asarray(o.combined_origin))
    ref = va.VoxelAtlasRef(64, 16, xy, zs)
    assert ref.integrate(np.asarray(o.combined_index_map), W)["outside"] == 0
    height, inferred = np.asarray(o.height_map).reshape(xy, xy), np.asarray(o.inferred_height_map).reshape(xy, xy)
    return vd.separable(ref, W, CAP, (res, zres))[0], W, ar.ground_of(height, inferred, True)


def referee_fields(bar, field, W, ground):
    """{"low", "tall"} -> dict(volume, C, D, action, start, goal, path): the referee's chain on the given field and ground"""
    import gvom
    footprint, prims = tables()
    cs = gvom.heading_cos_sin(HEADINGS)
    assert np.array_equal(cs, ar.cos_sin(HEADINGS))
    sx, sy = cell_of(W, *START[:2])
    gx, gy = cell_of(W, *GOAL[:2])
    out = {}
    for name, body in bs.bodies().items():
        vol = bv.volume(field, W, ground, body, CHASSIS, cs, SCENE["res"], SCENE["zres"], W[:2], MIN_MARGIN, SOFT_MARGIN)
        C, D, A, seeds, info = bv.field(cost_map(), footprint, prims, [(gx, gy, GOAL[2])], None, (vol[0], vol[1], ar_mask(BLOCKS), SQUEEZE_WEIGHT))
        out[name] = dict(volume=vol, C=C, D=D, action=A, info=info, start=(sx, sy, START[2]), goal=(gx, gy, GOAL[2]), W=W,
                         path=follow(A, prims, sx, sy, START[2]))
    return out


def ar_mask(blocks):
    m = 0
    for b in blocks:
        m |= 1 << int(b)
    return m


def crossing(q):
    """the world y of the two states of the path on either side of x = BAR_X: (y before, y behind)"""
    res, W = SCENE["res"], q["W"]
    world = [((W[0] + x + 0.5) * res, (W[1] + y + 0.5) * res) for x, y, _ in q["path"]]
    k = next(i for i, (x, _) in enumerate(world) if x >= bs.BAR_X)
    assert k > 0
    return world[k - 1][1], world[k][1]


def hold_statement(bar, seen):
    """seen = {"low": ..., "tall": ...} as referee_fields() returns them (the GPU test fills D, action and path from its products)"""
    low, tall = seen["low"], seen["tall"]
    d_low, d_tall = int(low["D"][low["start"][2], low["start"][0], low["start"][1]]), int(tall["D"][tall["start"][2], tall["start"][0], tall["start"][1]])
    if bar == "full":                                       # the bar over every y: only the low body gets through
        assert d_low < pf.UNREACHED and low["path"] is not None and low["path"][-1][:2] == low["goal"][:2], d_low
        assert d_tall == pf.UNREACHED and tall["path"] is None, d_tall
        return
    assert low["path"] is not None and low["path"][-1][:2] == low["goal"][:2] and tall["path"] is not None and tall["path"][-1][:2] == tall["goal"][:2]
    assert all(y < BAR_END_Y for y in crossing(low)), crossing(low)            # under the bar
    assert all(y >= BAR_END_Y for y in crossing(tall)), crossing(tall)         # round its end
    assert d_low < d_tall < pf.UNREACHED, (d_low, d_tall)
