"""Referee of the voxel atlas's change query (include/gvom_hip.h "voxel atlas changes"; gvom_voxel_atlas_changes): pure numpy and scipy on
tests/voxel_atlas_ref.py's VoxelAtlasRef (classes, extent, world_class).  It applies the definition literally: the code of every window
voxel from the class of its fused state and the atlas's class of the same world voxel, the columns' counts, the marked columns, their
8-connected components (scipy.ndimage.label), labels as least member index, kept / rank / cap, the rows, sums, cluster map, part 3 and
part 4.  Like the atlas's referee it is fed with dense fused states in the reference's voxel order and their window origins: it referees
the query, not the mapper.

Also here: the hand-placed scene that tests/test_voxel_changes_cpu.py holds to its census and tests/test_voxel_changes.py runs on the GPU."""
import functools

import numpy as np
from scipy import ndimage

import voxel_atlas_ref as va

APPEARED, VANISHED = 1, 2
NONE, SMALL = -1, -2
PART_DTYPES = (np.int32, np.int64, np.int32, np.int32, np.int32, np.uint8, np.uint16)


def codes(ref, state, W):
    """(codes uint8 [z, y, x], window voxels outside the extent) of the window at W whose dense fused state is `state`"""
    xy, zs = ref.xy, ref.zs
    c = va.classes(state).reshape(zs, xy, xy)
    z, y, x = np.indices(c.shape)
    world = np.stack([x + int(W[0]), y + int(W[1]), z + int(W[2])], axis=-1).reshape(-1, 3).astype(np.int64)
    e = world - np.array(ref.E, np.int64)
    inside = ((e >= 0) & (e < np.array(ref.sizes()))).all(axis=1).reshape(c.shape)
    a = ref.world_class(world).reshape(c.shape)
    out = np.zeros(c.shape, np.uint8)
    out[inside & (c == va.OCCUPIED) & (a == va.FREE)] = APPEARED
    out[inside & (c == va.FREE) & (a == va.OCCUPIED)] = VANISHED
    return out, int((~inside).sum())


def labels(mask):
    """int64 [y, x]: the least linear index y * xy + x of the column's 8-connected component, -1 outside the mask"""
    comp, n = ndimage.label(mask, structure=np.ones((3, 3), int))
    out = np.full(mask.shape, -1, np.int64)
    if n:
        idx = np.arange(mask.size, dtype=np.int64).reshape(mask.shape)
        least = np.asarray(ndimage.minimum(idx, comp, index=np.arange(1, n + 1))).astype(np.int64)
        out[mask] = least[comp[mask] - 1]
    return out


def distance_plane(xy):
    """d2 int64 [y, x] = (x - xy // 2)^2 + (y - xy // 2)^2"""
    d = np.arange(xy, dtype=np.int64) - xy // 2
    return d[None, :] ** 2 + d[:, None] ** 2


def product(ref, state, W, mask=3, min_cells=2, cap=1024):
    """(the seven parts of the product as the binding returns them, info [4] without the rounds {kept, marked columns, dropped}):
    part 2 [x, y]-indexed, part 5 [x, y, z], part 6 [k, x, y]"""
    assert mask in (1, 2, 3) and min_cells >= 1 and cap >= 1
    xy = ref.xy
    code, outside = codes(ref, state, W)
    app, van = (code == APPEARED), (code == VANISHED)
    in_mask = (app if mask & 1 else False) | (van if mask & 2 else False)
    marked = in_mask.any(axis=0)                                            # [y, x]
    lab = labels(marked)
    roots, sizes = np.unique(lab[marked], return_counts=True)
    kept = sizes >= min_cells
    rank_of_root = np.where(kept, np.cumsum(kept) - 1, SMALL)
    cmap = np.full(marked.shape, NONE, np.int32)
    ranks = rank_of_root[np.searchsorted(roots, lab[marked])]
    cmap[marked] = ranks
    n_kept = int(kept.sum())
    n = min(n_kept, cap)
    rows, sums, rows4 = np.zeros((cap, 8), np.int64), np.zeros((cap, 2), np.int64), np.zeros((cap, 4), np.int64)
    D = distance_plane(xy)
    level = np.arange(ref.zs, dtype=np.int64)[:, None, None]
    lowest = np.where(in_mask, level, 1 << 30).min(axis=0)                  # per column, over the voxels whose code is in mask
    highest = np.where(in_mask, level, -1).max(axis=0)
    for r in range(n):                                                     # the literal form: one cluster at a time
        ys, xs = np.nonzero(cmap == r)
        idx = ys * xy + xs
        d = D[ys, xs]
        best = np.lexsort((idx, d))[0]
        rows[r] = [idx.min(), len(idx), xs.min(), ys.min(), xs.max(), ys.max(), idx[best], d[best]]
        sums[r] = [xs.sum(), ys.sum()]
        rows4[r] = [app[:, ys, xs].sum(), van[:, ys, xs].sum(), lowest[ys, xs].min(), highest[ys, xs].max()]
        assert rows[r, 0] == roots[kept][r]
    counts = np.array([n_kept, marked.sum(), (ranks >= 0).sum(), cap, app.sum(), van.sum(), outside, ref.seq], np.int64)
    columns = np.stack([app.sum(axis=0).T, van.sum(axis=0).T])
    parts = (rows, sums, cmap.T, counts, rows4, code.transpose(2, 1, 0), columns)
    parts = tuple(np.ascontiguousarray(p.astype(t)) for p, t in zip(parts, PART_DTYPES))
    return parts, [n_kept, int(marked.sum()), int((~kept).sum())]


def differing_parts(got, want):
    """the numbers of the parts of `got` that are not `want`'s, in dtype, shape or content"""
    return [k for k, (g, w) in enumerate(zip(got, want)) if g.dtype != w.dtype or g.shape != w.shape or not np.array_equal(g, w)]


# ---- the hand-placed scene ---------------------------------------------------------------------------------------------------------------
# Window 64 x 64 x 8 at the drive's resolutions around an ego that does not move: flat ground two levels below the sensor, a ceiling of
# returns three levels above it (so that the levels above the sensor are observed free where nothing stands), and boxes given by the
# corner column of their footprint (window columns), its size in columns and how far the box moves in x between the two halves of the
# scene.  A box fills levels SCENE_BOX_LEVELS with returns at every voxel centre.  BEFORE: the boxes where they are given, scanned twice
# (a ring of two slots holds both) and integrated.  AFTER: every box moved, scanned twice, combined -- and asked for its changes.
SCENE_EGO = (0.13, 0.07, -0.6)
SCENE_RING = 2
SCENE_GROUND_LEVEL, SCENE_CEILING_LEVEL, SCENE_BOX_LEVELS = 2, 7, (3, 4, 5, 6)
SCENE_BOXES = (                                                            # (x, y, nx, ny, move in x)
    (8, 8, 3, 3, 5), (44, 10, 3, 3, 5), (10, 46, 3, 3, 5), (46, 48, 3, 3, 5),      # one per quadrant: a vanished and an appeared cluster each
    (24, 30, 3, 3, 5),                                                     # across the tile border y = 32 before and after the move
    (40, 22, 3, 3, 3),                                                     # moves by its own width: old and new place touch -- one cluster, both codes
    (20, 54, 1, 1, 5),                                                     # a post of one column: clusters below min_cells
    (52, 34, 2, 1, 5),                                                     # two columns: below min_cells 4
)


def scene_origin():
    return va.window_origin(SCENE_EGO)


def scene_cloud(after, jitter=0.0):
    """float32 [n, 3]: ground, ceiling and boxes of the scene, the boxes moved where `after`; `jitter` metres moves every return inside
    its voxel (the second scan of a pair)"""
    res, zres = va.DRIVE_RES[0], va.DRIVE_RES[2]
    W = np.array(scene_origin(), np.float64)
    xy = va.DRIVE_XY
    cx, cy = np.meshgrid(np.arange(xy), np.arange(xy), indexing="ij")
    cols = np.stack([cx.reshape(-1), cy.reshape(-1)], axis=1).astype(np.float64)
    pts = []
    for level in (SCENE_GROUND_LEVEL, SCENE_CEILING_LEVEL):
        pts.append(np.concatenate([cols, np.full((len(cols), 1), float(level))], axis=1))
    for x, y, nx, ny, move in SCENE_BOXES:
        x0 = x + (move if after else 0)
        bx, by, bz = np.meshgrid(np.arange(x0, x0 + nx), np.arange(y, y + ny), np.array(SCENE_BOX_LEVELS), indexing="ij")
        pts.append(np.stack([bx.reshape(-1), by.reshape(-1), bz.reshape(-1)], axis=1).astype(np.float64))
    v = np.concatenate(pts)
    centres = (v + W + 0.5) * np.array([res, res, zres]) + jitter
    return np.ascontiguousarray(centres.astype(np.float32))


def scene_scans():
    """((cloud, ego), ...) x 4: BEFORE twice, AFTER twice"""
    return tuple((scene_cloud(after, jitter), SCENE_EGO) for after in (False, True) for jitter in (0.0, 0.03))


def run_scene(mapper, dense_state, between):
    """the scene on `mapper` (process_pointcloud / combine_maps): BEFORE, between(state BEFORE, W) -- the integrates --, AFTER; returns
    (state AFTER, W).  dense_state(mapper) returns the dense fused state and its window origin"""
    scans = scene_scans()
    state = None
    for k, half in enumerate((scans[:2], scans[2:])):
        for pc, ego in half:
            mapper.process_pointcloud(pc, ego)
        mapper.combine_maps()
        state, W = dense_state(mapper)
        state = np.array(state).copy()
        assert tuple(int(v) for v in W) == scene_origin()
        if k == 0:
            between(state, scene_origin())
    return state, scene_origin()


def scene_params():
    return va.DRIVE_PARAMS + (SCENE_RING,) + va.DRIVE_TAIL


@functools.lru_cache(maxsize=None)
def oracle_scene():
    """(referee atlas with BEFORE integrated, state AFTER, W) from the C oracle"""
    from oracle import oracle
    o = oracle.OracleGvom(*scene_params())
    ref = va.VoxelAtlasRef(va.DRIVE_A, va.DRIVE_Z, va.DRIVE_XY, va.DRIVE_ZS)
    after, W = run_scene(o, lambda m: (np.asarray(m.combined_index_map), np.asarray(m.combined_origin)), ref.integrate)
    return ref, after, W


def census(parts, info, xy=va.DRIVE_XY):
    """what tests/test_voxel_changes_cpu.py asks of a product of the scene: a dict of counts"""
    rows, sums, cmap, counts, rows4, code, columns = parts
    n = min(int(counts[0]), int(counts[3]))
    r, v = rows[:n].astype(np.int64), rows4[:n].astype(np.int64)
    tile = 32
    return {"kept": int(counts[0]), "with_appeared": int((v[:, 0] > 0).sum()), "with_vanished": int((v[:, 1] > 0).sum()),
            "with_both": int(((v[:, 0] > 0) & (v[:, 1] > 0)).sum()), "dropped": int(info[2]),
            "across_tiles": int(((r[:, 2] // tile != r[:, 4] // tile) | (r[:, 3] // tile != r[:, 5] // tile)).sum()),
            "nearest_is_not_label": int((r[:, 6] != r[:, 0]).sum())}
