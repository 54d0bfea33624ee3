"""Shared by tests/test_map2d_chain.py and tests/test_map2d_chain_cpu.py: scenes that drive k_map2d through every step of its
chain -- the ring search of __guess_height (gvom.py:558-661) to every depth and across every window edge, density windows of
two load rounds, slope-only positives, and store runs that change between default and non-default while the window moves --
and the census that shows, on the CPU oracle's maps alone, that the scenes reach them.

Grids: 64 x 64 x 32 (2 x 8 of the [y][x] form's 32 x 8 tiles: seams, four window edges, the corner workgroup) and 96 x 96 x 32
(3 tag segments per row: no power of two), both at the bench's 0.2 m resolutions.  robot_height 2.4 makes a density window
9-10 levels long (two rounds of eight).

A scan is tests/obstacle_scenes.py's ground with posts, changed in three ways:
  holes      the returns inside two world-fixed rectangles are dropped: a wide one (22 x 40 cells: cells whose search
             finds nothing to one side within 15 rings) and a small one (3 x 3: ring 1 or 2);
  platform   the ground inside a third rectangle is raised by 0.5 m: steep slopes along its rim, no tall returns there;
  far sweep  2,048 rays that end 60 m out, slightly below the sensor: every column they cross has a free voxel, so the cells
             without ground -- the holes, and the margin the ground leaves at the window's edges -- have an INFERRED height.
Six scans, a combine after each: the ego moves one cell in +x per scan for three scans, jumps back three cells, and goes on."""
import functools

import numpy as np

import obstacle_scenes as ob
from oracle import oracle

RES = 0.2
EGO_CELLS = (0, 1, 2, 3, 0, 1)                            # window position in x, cells: one per scan, one jump back
HOLE_WIDE = (-5.4, -1.0, -4.0, 4.0)                       # x0, x1, y0, y1 in metres (world)
HOLE_SMALL = (2.0, 2.6, 2.0, 2.6)
PLATFORM = (1.4, 3.0, -3.0, -1.0)
GRIDS = {"g64": 64, "g96": 96}
MAPS = (("positive", 0), ("negative", 0), ("roughness", -1.0), ("visibility", 0))     # combine_maps()[1 + i], its default
ATTRIBUTES = ("height_map", "inferred_height_map", "x_slope_map", "y_slope_map", "guessed_height_delta")


def params(name, ring=1):
    return (RES, RES, GRIDS[name], 32, ring, 0.8, 0.5, 0.5, 0.3, 2.4, 1.0, 1.0, 1, 1)


def ego_of(k):
    return (RES * EGO_CELLS[k] + 0.05, 0.07, 0.0)


def _inside(p, box):
    return (p[:, 0] >= box[0]) & (p[:, 0] < box[1]) & (p[:, 1] >= box[2]) & (p[:, 1] < box[3])


def scan(name, k):
    xy, ego = GRIDS[name], ego_of(k)
    pc = ob.post_scene(40 + k, xy, RES, RES, ego, n_posts=40, ground_pts=6000 * (xy // 64) ** 2).astype(np.float64)
    pc = pc[~(_inside(pc, HOLE_WIDE) | _inside(pc, HOLE_SMALL))]      # (ground and posts: no return ends in a hole)
    pc[(pc[:, 2] < -0.9) & _inside(pc, PLATFORM), 2] += 0.5
    a = 2 * np.pi * np.arange(2048) / 2048
    far = np.stack([ego[0] + 60 * np.cos(a), ego[1] + 60 * np.sin(a), ego[2] - 2.0 + 0 * a], axis=1)
    return np.ascontiguousarray(np.concatenate([pc, far], 0).astype(np.float32))


@functools.lru_cache(maxsize=None)
def scans(name):
    out = []
    for k in range(len(EGO_CELLS)):
        pc = scan(name, k)
        pc.setflags(write=False)
        out.append((pc, ego_of(k)))
    return tuple(out)


# ---- the census -----------------------------------------------------------------------------------------------------------------

def ring_census(height, inferred):
    """The ring search of every cell without height but with inferred height, on [x, y] maps.  Returns (searched, end): end is the
    ring after which the reference's loop stops (its exit test names x_n twice and x_p never: reproduced), 16 where it runs
    through ring 15 without its exit test ever holding."""
    xy = height.shape[0]
    valid = height > -1000
    searched = ~valid & (inferred != -1000.0)
    pad = np.zeros((xy + 32, xy + 32), bool)
    pad[16:16 + xy, 16:16 + xy] = valid
    X, Y = np.meshgrid(np.arange(xy), np.arange(xy), indexing="ij")
    xn = np.zeros((xy, xy), bool); yp = xn.copy(); yn = xn.copy()
    end = np.full((xy, xy), 16)
    active = np.ones((xy, xy), bool)
    for i in range(1, 16):
        f_xn = np.zeros((xy, xy), bool); f_yp = f_xn.copy(); f_yn = f_xn.copy()
        for d in range(-i + 1, i + 1):
            f_xn |= pad[16 + X - i, 16 + Y + d]             # column x - i, dy in [-i + 1, i]
            f_yp |= pad[16 + X + d, 16 + Y + i]             # row y + i, dx in [-i + 1, i]
        for d in range(-i, i):
            f_yn |= pad[16 + X + d, 16 + Y - i]             # row y - i, dx in [-i, i)
        xn |= f_xn | (X - i < 0)
        yp |= f_yp | (Y + i >= xy)
        yn |= f_yn | (Y - i < 0)
        stop = active & xn & yp & yn
        end[stop] = i
        active &= ~stop
    return searched, end


def default_runs(a, default):
    """a[x, y] -> bool[ceil(xy / 32), xy]: run (x // 32, y) of the [y][x] form holds only the default"""
    xy = a.shape[0]
    return np.stack([(a[x0:x0 + 32] == default).all(axis=0) for x0 in range(0, xy, 32)])


def census(rec):
    height, inferred = rec["height_map"], rec["inferred_height_map"]
    xy = height.shape[0]
    searched, end = ring_census(height, inferred)
    X, Y = np.meshgrid(np.arange(xy), np.arange(xy), indexing="ij")
    c = rec["density_census"]
    length = c["zmax"] - c["zmin"] + 1
    return {
        "searched": int(searched.sum()),
        "ring_1": int((searched & (end == 1)).sum()),
        "ring_8_to_15": int((searched & (end >= 8) & (end <= 15)).sum()),
        "ring_never": int((searched & (end == 16)).sum()),
        "edge_x_lo": int((searched & (X < 15)).sum()), "edge_x_hi": int((searched & (X >= xy - 15)).sum()),
        "edge_y_lo": int((searched & (Y < 15)).sum()), "edge_y_hi": int((searched & (Y >= xy - 15)).sum()),
        "negative_cells": int((rec["maps"][2] != 0).sum()),
        "two_rounds": int((c["gate"] & (length > 8)).sum()),
        "two_rounds_with_density": int((c["seen"] & c["has_big"] & (length > 8)).sum()),
        "slope_alone": int((c["steep"] & (c["value"] == 0)).sum()),
    }


@functools.lru_cache(maxsize=None)
def referee(name):
    """The CPU oracle over the grid's six scans: one record per combine -- the returned maps, the five attributes, the occupancy
    grids, the census, which runs hold only defaults.  Computed once per grid, shared, read-only."""
    o = oracle.OracleGvom(*params(name))
    out = []
    for pc, ego in scans(name):
        o.process_pointcloud(pc, ego)
        maps = o.combine_maps()
        rec = {"maps": maps, "cell_count": o.combined_cell_count_cpu, "density_census": ob.census(o),
               "roughness_map": o.roughness_map.copy(),
               "occupancy": oracle.ros_occupancy_grids(maps, *ob.OCCUPANCY_SETTINGS[1])}
        for a in ATTRIBUTES:
            rec[a] = getattr(o, a).copy()
        rec["census"] = census(rec)
        rec["default_runs"] = [default_runs(maps[1 + i], d) for i, (_, d) in enumerate(MAPS)]
        for v in list(rec.values()) + list(maps):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(rec)
    return tuple(out)


def run_changes(name):
    """(gone, come): runs default now and non-default one combine earlier at the same memory position, and the reverse, summed
    over the maps, per combine from the second on"""
    recs = referee(name)
    gone = [sum(int((~p & r).sum()) for p, r in zip(a["default_runs"], b["default_runs"])) for a, b in zip(recs, recs[1:])]
    come = [sum(int((p & ~r).sum()) for p, r in zip(a["default_runs"], b["default_runs"])) for a, b in zip(recs, recs[1:])]
    return gone, come


def stored_runs(name, k):
    """per map, the runs the delta form stores at combine k >= 1 into a buffer it wrote at combine k - 1: non-default now or then"""
    recs = referee(name)
    return {m: int((~recs[k]["default_runs"][i] | ~recs[k - 1]["default_runs"][i]).sum()) for i, (m, _) in enumerate(MAPS)}
