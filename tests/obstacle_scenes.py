"""Shared by tests/test_obstacle_density.py and tests/test_obstacle_density_cpu.py: scenes on which the positive-obstacle map
carries DENSITIES (gvom.py:502-521; k_map2d role B, k_posdens), and the census that counts which branches of that code the
cells of a combine take.

On uniform random clouds no voxel collects more than ten hits (the map is 100 where the slope is steep and 0 elsewhere), on
the lidar scenes a few dozen cells carry a density, and with the reference's thresholds at z_res 0.2 a window is 7-8 levels:
the second round of the kernels' eight-level loop never sees a countable voxel.  The scenes here are built for that code:

  ground   ~6,000 returns over 92 % of the window at z = -1 + 0.05 sin(0.7 x), 1 cm of noise;
  posts    at 2 m or more from the ego, each centred on its voxel column: from the ground to a random top every level draws
           k in {0, 1, 9, 10, 11, 12, 25, 40} returns inside the middle 60 % of the voxel -- the voxel's hit count of that scan
           is k (plus the ground's in a post's lowest voxel), on both sides of the `> 10` test;
  behind   with an occupied level, m in {0, 0, 3, 15, 60} returns 15-50 % further along the ray from the ego through that
           voxel: rays pass through it, total > hit, the density lies strictly between 0 and 1;
  scans    three, the ego moving (0.9, -0.5, 0.1) k, one combine after each; float32 clouds.

The census is numpy on the attributes of an oracle.OracleGvom (or on bare arrays: census_arrays) and never calls the oracle's
positive-obstacle code: its own arithmetic is held to the reference's known answers and to the oracle's map by the CPU test."""
import functools

import numpy as np

from oracle import oracle

XY_RES = 0.4
STEP = (0.9, -0.5, 0.1)
N_SCANS = 3
LEVEL_RETURNS = (0, 1, 9, 10, 11, 12, 25, 40)
BEHIND_RETURNS = (0, 0, 3, 15, 60)

# name: (xy_size, z_resolution, z_size, robot_height, ring slots, posts per scan)
GRIDS = {
    "one_round": (64, 0.2, 32, 2.0, 1, 60),        # the reference's window length (7-8 levels), on a scene that has densities
    "two_rounds": (64, 0.1, 64, 2.0, 2, 60),       # 15-level windows; the map is fused from two slots
    "four_rounds": (64, 0.05, 128, 2.0, 1, 60),    # 30-level windows
    "gate": (64, 0.1, 40, 3.0, 1, 60),             # fmax >= z_size: the gate rejects valid cells
    "ragged": (50, 0.1, 64, 2.0, 3, 60),           # partial 8 x 32 / 32 x 8 tiles, xy_size % 4 != 0
    "tall": (32, 0.05, 300, 2.0, 2, 60),           # 19-level fusion chunks (the generic k_fuse); a quarter of the cells
}
# what a census of the LAST combine must reach (tests/test_obstacle_density_cpu.py); "tall": halved
FLOORS = {"density_cells": 100, "fractional": 50, "full": 3, "mixed": 50, "small_only": 100}


def floors(name):
    if name != "tall":
        return dict(FLOORS)
    return {k: (v + 1) // 2 for k, v in FLOORS.items()}


def params(name):
    xy, z_res, zs, robot_height, ring, _ = GRIDS[name]
    return (XY_RES, z_res, xy, zs, ring, 0.8, 0.5, 0.5, 0.3, robot_height, 2.0, 1.0, 1, 1)


def ego_of(k):
    return (STEP[0] * k, STEP[1] * k, STEP[2] * k)


def post_scene(seed, xy, xy_res, z_res, ego, n_posts=60, ground_pts=6000):
    """one scan's cloud, float32 [N, 3]"""
    rng = np.random.default_rng(seed)
    ego = np.asarray(ego, np.float64)
    half = 0.5 * xy * xy_res * 0.92
    gx = rng.uniform(-half, half, ground_pts) + ego[0]
    gy = rng.uniform(-half, half, ground_pts) + ego[1]
    gz = -1.0 + 0.05 * np.sin(0.7 * gx) + rng.normal(0, 0.01, ground_pts)
    parts = [np.stack([gx, gy, gz], 1)]
    size = np.array([xy_res, xy_res, z_res])
    for _ in range(n_posts):
        a, r = rng.uniform(0, 2 * np.pi), rng.uniform(2.0, half * 0.95)
        # the centre of the voxel column the post stands in
        px = (np.floor((ego[0] + r * np.cos(a)) / xy_res) + 0.5) * xy_res
        py = (np.floor((ego[1] + r * np.sin(a)) / xy_res) + 0.5) * xy_res
        top = rng.uniform(-0.6, 1.4)
        zc = (np.floor(-1.0 / z_res) + 0.5) * z_res
        while zc < top:
            k = int(rng.choice(LEVEL_RETURNS))
            if k:
                centre = np.array([px, py, zc])
                parts.append(centre + rng.uniform(-0.3, 0.3, (k, 3)) * size)
                m = int(rng.choice(BEHIND_RETURNS))
                if m:
                    t = 1.0 + rng.uniform(0.15, 0.5, m)
                    parts.append(ego + t[:, None] * (centre - ego) + rng.uniform(-0.1, 0.1, (m, 3)) * size)
            zc += z_res
    return np.ascontiguousarray(np.concatenate(parts, 0).astype(np.float32))


@functools.lru_cache(maxsize=None)
def scans(name):
    """((cloud, ego), ...) of the grid's three scans; built once, shared, read-only"""
    xy, z_res, _, _, _, n_posts = GRIDS[name]
    out = []
    for k in range(N_SCANS):
        pc = post_scene(10 + k, xy, XY_RES, z_res, ego_of(k), n_posts)
        pc.setflags(write=False)
        out.append((pc, ego_of(k)))
    return tuple(out)


# ---- the census -----------------------------------------------------------------------------------------------------------------

def census_arrays(index_map, height, hit, total, origin_z, xy, zs, z_res, pos_thr, robot_height, x_slope, y_slope, slope_thr):
    """Which branch of the positive-obstacle code every cell takes, and what it yields.  index_map: x + y xy + z xy xy -> compact
    row or < 0; height / slopes indexed [x, y]; hit / total compact.  Returns a dict of [x, y] arrays, the dense [z, y, x]
    counts, and the counts the tests assert (see the keys below)."""
    xy, zs = int(xy), int(zs)
    H = np.asarray(height, np.float64).reshape(xy, xy)
    sx, sy = np.asarray(x_slope, np.float64).reshape(xy, xy), np.asarray(y_slope, np.float64).reshape(xy, xy)
    steep = np.sqrt(sx * sx + sy * sy) >= slope_thr                                            # gvom.py:498
    fmin = np.floor((H + pos_thr) / z_res - origin_z) + 1.0                                    # :503
    fmax = np.floor((H + robot_height) / z_res - origin_z)                                     # :505
    fmin_ok = (fmin >= 0) & (fmin < zs)
    fmax_ok = (fmax >= 0) & (fmax < zs)
    gate = fmin_ok & fmax_ok                                                                   # :506-509
    zmin = np.where(gate, fmin, 0).astype(np.int64)
    zmax = np.where(gate, fmax, -1).astype(np.int64)
    idx = np.asarray(index_map).reshape(zs, xy, xy)                                            # [z][y][x]
    occ = idx >= 0
    rows = np.where(occ, idx, 0)
    h3 = np.where(occ, np.asarray(hit)[rows], 0).astype(np.int64)
    t3 = np.where(occ, np.asarray(total)[rows], 0).astype(np.int64)
    z = np.arange(zs)[:, None, None]
    win = gate.T[None] & (z >= zmin.T[None]) & (z <= zmax.T[None])                             # :513
    big = win & occ & (h3 > 10)                                                                # :515
    small = win & occ & (h3 >= 1) & (h3 <= 10)
    n = (t3 * big).sum(0).T.astype(np.float64)                                                 # integers: any order of summation
    density = (h3 * big).sum(0).T.astype(np.float64)
    density = np.where(n > 0.0, density / np.where(n > 0.0, n, 1.0), density)                  # :519
    value = np.where(gate, (density * 100).astype(np.int32), 0).astype(np.int32)               # :521, truncation
    positive = np.where(steep, 100, value).astype(np.int32)
    has_big, has_small = big.any(0).T, small.any(0).T
    seen = gate & ~steep                                  # the cells whose density reaches the map
    valid = H > -1000
    open_win = win & seen.T[None]
    c = {
        "steep": steep, "gate": gate, "seen": seen, "valid": valid, "zmin": zmin, "zmax": zmax, "value": value, "positive": positive,
        "has_big": has_big, "has_small": has_small, "hit3": h3, "total3": t3, "occupied3": occ, "xy": xy, "zs": zs,
        # the counts
        "density_cells": int((seen & has_big).sum()),
        "fractional": int((seen & has_big & (value > 0) & (value < 100)).sum()),
        "full": int((seen & has_big & (value >= 100)).sum()),
        "mixed": int((seen & has_big & has_small).sum()),
        "small_only": int((seen & ~has_big & has_small).sum()),
        "gate_passed": int(gate.sum()),
        "shortest_window": int((zmax - zmin + 1)[gate].min()) if gate.any() else 0,
        "longest_window": int((zmax - zmin + 1)[gate].max()) if gate.any() else 0,
        "rejected_above": int((valid & ~steep & fmin_ok & (fmax >= zs)).sum()),               # valid cells the `fmax < zs` test rejects
        "hits_10": int((open_win & occ & (h3 == 10)).sum()),
        "hits_11": int((open_win & occ & (h3 == 11)).sum()),
    }
    return c


def census(o):
    """census_arrays of an oracle.OracleGvom that has just combined"""
    return census_arrays(o.combined_index_map, o.height_map, o.combined_hit_count, o.combined_total_count,
                         float(o.combined_origin[2]), o.xy_size, o.z_size, o.z_resolution, o.positive_obstacle_threshold,
                         o.robot_height, o.x_slope_map, o.y_slope_map, o.slope_obstacle_threshold)


def density_mask(c, lo=0, hi=100):
    """[x, y]: cells whose map value is a density in (lo, hi] -- not the slope override"""
    return c["seen"] & c["has_big"] & (c["value"] > lo) & (c["value"] <= hi)


def cells_per_slab(c, origin_y, world):
    """density cells in every rank's slab of a map sharded `world` ways: rank r owns the STORAGE rows
    [r xy / world, (r + 1) xy / world), storage row = (y + origin_y) mod xy"""
    xy = c["xy"]
    y = np.nonzero(c["seen"] & c["has_big"])[1]
    sy = (y + int(origin_y)) % xy
    return np.bincount(sy * world // xy, minlength=world)


def explain(c, x, y):
    """one cell in words: its window and the hit / total counts the referee summed"""
    x, y = int(x), int(y)
    if not c["gate"][x, y]:
        return "cell (%d, %d): no window (the gate rejects it)%s" % (x, y, ", steep" if c["steep"][x, y] else "")
    z0, z1 = int(c["zmin"][x, y]), int(c["zmax"][x, y])
    h, t, occ = c["hit3"][z0:z1 + 1, y, x], c["total3"][z0:z1 + 1, y, x], c["occupied3"][z0:z1 + 1, y, x]
    levels = " ".join("%d:%d/%d" % (z0 + i, h[i], t[i]) for i in range(len(h)) if occ[i])
    big = h > 10
    return "cell (%d, %d): window z %d..%d (%d levels)%s, value %d, summed hit %d / total %d over %d voxels; occupied levels z:hit/total %s" % (
        x, y, z0, z1, z1 - z0 + 1, ", steep" if c["steep"][x, y] else "", int(c["value"][x, y]), int(h[big].sum()), int(t[big].sum()),
        int(big.sum()), levels or "none")


def explain_mismatch(c, got, want, limit=6):
    """the first cells at which a positive map `got` ([x, y]) differs from the referee's `want`"""
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    lines = ["positive map differs from the referee in %d cells" % len(bad)]
    for x, y in bad[:limit]:
        lines.append("  got %d, referee %d -- %s" % (int(np.asarray(got)[x, y]), int(np.asarray(want)[x, y]), explain(c, x, y)))
    return "\n".join(lines)


# ---- the referee ----------------------------------------------------------------------------------------------------------------

OCCUPANCY_SETTINGS = ((50, -10, 0), (12.5, -6.0, 1.5))     # (density threshold, min roughness, max roughness): the node's defaults, and
#                                                          a threshold that no integer density equals


@functools.lru_cache(maxsize=None)
def referee(name):
    """The unmodified CPU oracle over the grid's three scans: one record per combine -- what combine_maps() returned, every 2-D
    map, the debug rows, the occupancy grids of both OCCUPANCY_SETTINGS, the census; the last one also the fused map densely.
    Computed once per grid and shared: read, never written."""
    o = oracle.OracleGvom(*params(name))
    out = []
    for k, (pc, ego) in enumerate(scans(name)):
        o.process_pointcloud(pc, ego)
        maps = o.combine_maps()
        rec = {
            "maps": maps, "cell_count": o.combined_cell_count_cpu, "combined_origin": o.combined_origin.copy(),
            "census": census(o),
            "height_map": o.height_map.copy(), "inferred_height_map": o.inferred_height_map.copy(),
            "x_slope_map": o.x_slope_map.copy(), "y_slope_map": o.y_slope_map.copy(),
            "guessed_height_delta": o.guessed_height_delta.copy(), "roughness_map": o.roughness_map.copy(),
            "debug_height_map": o.make_debug_height_map(), "debug_inferred_height_map": o.make_debug_inferred_height_map(),
            "occupancy": {s: oracle.ros_occupancy_grids(maps, *s) for s in OCCUPANCY_SETTINGS},
        }
        if k == N_SCANS - 1:
            rec["fused_dense"] = oracle.dense_from_compact(o.combined_index_map, o.combined_hit_count, o.combined_total_count,
                                                           o.combined_min_height)
        for v in list(rec.values()) + list(maps):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(rec)
    return tuple(out)
