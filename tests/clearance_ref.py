"""The referee of the obstacle clearance map (gvom_clearance, include/gvom_hip.h "obstacle clearance"): plain numpy, two
independent forms of the squared distance transform and the distance formula of the definition.

  obstacle_mask   (double)positive > density_threshold, or (include_negative and) negative > 0
  brute_force     min over the LIST of obstacle cells of (x - ox)^2 + (y - oy)^2, int64, in chunks of cells (all cells, or a sample)
  separable       nearest obstacle of the same column along y by two running scans, then min over columns of g^2 + (x - i)^2
                  (the OTHER axis order than the kernels', which scan along x first)
  distance        (float32)(sqrt((float64)d2) * xy_resolution), +inf where d2 is FAR

All maps are [x, y]-indexed, as everywhere at the Python boundary."""
import numpy as np

FAR = 2147483647          # GVOM_CLEARANCE_FAR


def obstacle_mask(positive, negative=None, density_threshold=50, include_negative=True):
    mask = np.asarray(positive).astype(np.float64) > float(density_threshold)
    if include_negative and negative is not None:
        mask = mask | (np.asarray(negative) > 0)
    return mask


def cap(d2, max_cells2):
    """an unbounded d2 map under the cap max_cells2 (<= 0: unbounded)"""
    d2 = np.asarray(d2, np.int64)
    if max_cells2 is not None and max_cells2 > 0:
        d2 = np.where(d2 > max_cells2, FAR, d2)
    assert d2.max(initial=0) <= FAR
    return d2.astype(np.int32)


def brute_force(mask, max_cells2=0, cells=None):
    """cells: None = every cell (the [x, y] map comes back), or an int array [k, 2] of (x, y): the k values"""
    mask = np.asarray(mask, bool)
    n, m = mask.shape
    ox, oy = np.nonzero(mask)
    if cells is None:
        cx, cy = (a.reshape(-1) for a in np.meshgrid(np.arange(n), np.arange(m), indexing="ij"))
    else:
        cx, cy = np.asarray(cells)[:, 0], np.asarray(cells)[:, 1]
    shape = (n, m) if cells is None else (len(cx),)
    if ox.size == 0:
        return np.full(shape, FAR, np.int32)
    ox, oy, cx, cy = (a.astype(np.int64) for a in (ox, oy, cx, cy))
    out = np.empty(len(cx), np.int64)
    chunk = max(1, (1 << 22) // ox.size)
    for i in range(0, len(cx), chunk):
        dx = cx[i:i + chunk, None] - ox[None, :]
        dy = cy[i:i + chunk, None] - oy[None, :]
        out[i:i + chunk] = (dx * dx + dy * dy).min(axis=1)
    return cap(out.reshape(shape), max_cells2)


def separable(mask, max_cells2=0):
    mask = np.asarray(mask, bool)
    n, m = mask.shape
    big = np.int64(1) << 40
    # along y: distance to the nearest obstacle of the same x, from below and from above
    g = np.full((n, m), big, np.int64)
    last = np.full(n, -big, np.int64)
    for y in range(m):
        last = np.where(mask[:, y], y, last)
        g[:, y] = np.minimum(g[:, y], y - last)
    last = np.full(n, big, np.int64)
    for y in range(m - 1, -1, -1):
        last = np.where(mask[:, y], y, last)
        g[:, y] = np.minimum(g[:, y], last - y)
    g2 = np.where(g >= big // 2, big, g * g)
    # along x: min over i of g[i, y]^2 + (x - i)^2
    xs = np.arange(n, dtype=np.int64)
    out = np.full((n, m), big, np.int64)
    for i in range(n):
        out = np.minimum(out, g2[i][None, :] + ((xs - i) ** 2)[:, None])
    out = np.where(out >= big // 2, FAR, out)
    return cap(out, max_cells2)


def distance(d2, xy_resolution):
    d2 = np.asarray(d2)
    with np.errstate(over="ignore"):
        d = (np.sqrt(d2.astype(np.float64)) * np.float64(xy_resolution)).astype(np.float32)
    return np.where(d2 == FAR, np.float32(np.inf), d).astype(np.float32)


def census(positive, negative, threshold):
    """(cells with 0 < positive <= threshold, cells with positive > threshold, cells with negative > 0)"""
    positive, negative = np.asarray(positive), np.asarray(negative)
    return (int(np.sum((positive > 0) & (positive <= threshold))), int(np.sum(positive > threshold)), int(np.sum(negative > 0)))


SCENES, SCENE_THRESHOLD, CENSUS_FLOOR = ("one_round", "ragged"), 50, 20      # the scenes (tests/obstacle_scenes.py) run end to end
CAPS = (0, 1, 2, 24, 25, 100)                                                # max_cells2: 25 separates 5^2 and 3^2 + 4^2 from 24


def max_cells2_of(max_distance, xy_resolution):
    """what the binding passes for max_distance (metres); None / inf: 0 = unbounded"""
    import math
    if max_distance is None or max_distance == float("inf"):
        return 0
    return int(math.floor((float(max_distance) / float(xy_resolution)) ** 2))


# ---- the synthetic patterns of the tests (name -> (positive, negative or None)), [x, y] int32 --------------------------------
def patterns(xy, seed=0):
    rng = np.random.default_rng(1000 * xy + seed)
    z = lambda: np.zeros((xy, xy), np.int32)                                  # noqa: E731
    out = {"none": (z(), z()), "all": (np.full((xy, xy), 100, np.int32), z())}
    for name, (x, y) in (("corner00", (0, 0)), ("corner0n", (0, xy - 1)), ("cornern0", (xy - 1, 0)), ("cornernn", (xy - 1, xy - 1))):
        p = z()
        p[x, y] = 100
        out[name] = (p, None)
    if xy > 64:                                                               # the wave / strip boundary at x = 63 | 64
        p = z()
        p[63, 5] = p[64, 5] = 100
        out["boundary_same_row"] = (p, None)
        p = z()
        p[63, xy // 2] = p[64, xy // 2 + 1] = 100
        out["boundary_adjacent_rows"] = (p, None)
        p = z()
        p[64, 16] = 100                                                       # alone in its chunk; its left neighbours look across
        p[xy - 1, 15] = 100
        out["boundary_lonely"] = (p, None)
    p = z()
    p[:, xy // 3] = 100
    out["full_row"] = (p, None)                                               # one y: a full row of the [y][x] storage
    p = z()
    p[xy // 3, :] = 100
    out["full_column"] = (p, None)
    for name, frac in (("random_0.1", 0.001), ("random_1", 0.01), ("random_30", 0.3)):
        p = np.where(rng.random((xy, xy)) < frac, 100, 0).astype(np.int32)
        if not p.any():
            p[rng.integers(xy), rng.integers(xy)] = 100
        out[name] = (p, z())
    p = rng.integers(48, 52, (xy, xy)).astype(np.int32)                       # 48..51 around the fractional threshold 49.5
    p[rng.random((xy, xy)) < 0.9] = 49
    out["threshold_edge"] = (p, None)
    n = np.where(rng.random((xy, xy)) < 0.02, 100, 0).astype(np.int32)
    n[1, 2] = 100
    out["negative_only"] = (np.full((xy, xy), 10, np.int32), n)
    return out


# ---- maps of 300 to 4096 cells a side: every launch regime of the two kernels (tests/test_clearance.py "launch regimes") ------------
# separable() is O(n^3) -- 3.8 s per mask at 1000 cells -- so the large maps have two further exact referees, both pinned to
# separable / brute_force by tests/test_clearance_cpu.py:
#   by_rows             min over the map rows (fixed y) that hold an obstacle of (distance along x within that row)^2 + dy^2:
#                       O(rows * n^2), for the patterns whose obstacles lie in a handful of rows
#   feature_transform   scipy's Euclidean feature transform (the INDEX of a nearest obstacle per cell), then the squared distance
#                       to that obstacle in integer arithmetic: nothing of scipy's floating point reaches the result
LARGE = (300, 520, 1000, 1024, 2049, 4096)


def large_caps(xy):
    """max_cells2 at the large sizes: unbounded, 1, 25, 2500 (a halo of 50 rows) and a cap whose radius is xy itself -- not
    below xy, so the column pass loads every row as when unbounded, but cuts at the cap"""
    return (0, 1, 25, 2500, xy * xy)


def by_rows(mask, max_cells2=0):
    mask = np.asarray(mask, bool)
    n, m = mask.shape
    big = np.int64(1) << 40
    out = np.full((n, m), big, np.int64)
    xs, ys = np.arange(n, dtype=np.int64), np.arange(m, dtype=np.int64)
    for y in np.flatnonzero(mask.any(axis=0)):
        ox = np.flatnonzero(mask[:, y]).astype(np.int64)
        k = np.searchsorted(ox, xs)                                          # ox[k - 1] < x <= ox[k]
        left = np.where(k > 0, xs - ox[np.maximum(k, 1) - 1], big)
        right = np.where(k < len(ox), ox[np.minimum(k, len(ox) - 1)] - xs, big)
        g = np.minimum(left, right)
        np.minimum(out, (g * g)[:, None] + ((ys - y) ** 2)[None, :], out=out)
    return cap(np.where(out >= big // 2, FAR, out), max_cells2)


def have_scipy():
    try:
        import scipy.ndimage                                                 # noqa: F401
        return True
    except ImportError:
        return False


def feature_transform(mask, max_cells2=0):
    from scipy import ndimage
    mask = np.asarray(mask, bool)
    n, m = mask.shape
    if not mask.any():
        return np.full((n, m), FAR, np.int32)
    idx = ndimage.distance_transform_edt(~mask, return_distances=False, return_indices=True)
    assert mask[idx[0], idx[1]].all()                                        # every index names an obstacle cell
    dx = idx[0].astype(np.int64) - np.arange(n, dtype=np.int64)[:, None]
    dy = idx[1].astype(np.int64) - np.arange(m, dtype=np.int64)[None, :]
    return cap(dx * dx + dy * dy, max_cells2)


def brute_force_near(mask, cells, r=48):
    """brute_force at `cells` ([k, 2] of (x, y)) without the full obstacle list where it is not needed: the minimum over the
    obstacles within r cells in x and in y IS the global minimum once it is <= r^2 (every obstacle outside that square is
    further than r); the cells it does not settle go to brute_force itself"""
    mask = np.asarray(mask, bool)
    n, m = mask.shape
    cells = np.asarray(cells, np.int64)
    out = np.full(len(cells), -1, np.int64)
    for k, (x, y) in enumerate(cells):
        x0, y0 = max(0, x - r), max(0, y - r)
        ox, oy = np.nonzero(mask[x0:x + r + 1, y0:y + r + 1])
        if ox.size:
            d = int(((ox + x0 - x) ** 2 + (oy + y0 - y) ** 2).min())
            if d <= r * r:
                out[k] = d
    rest = np.flatnonzero(out < 0)
    if rest.size:
        out[rest] = brute_force(mask, 0, cells[rest])
    return out.astype(np.int32)


def row_tile(xy):
    """output rows per workgroup of k_clearance_cols as gvom_launch_clearance chooses them today; the sample below needs no more
    of it than that it is a multiple of 16"""
    return max(16, (xy // 16 + 15) & ~15)


def boundary_sample(xy, seed=0):
    """[k, 2] (x, y): cells either side of every boundary the kernels have -- x = 8 j (every strip width 8 .. 64 of the column
    pass, and the 64-cell chunks of the row pass), y = 16 j (every row tile: row_tile() is a multiple of 16) -- each x boundary at
    a y next to a row-tile boundary and the other way round, and 2,048 random cells"""
    assert row_tile(xy) % 16 == 0
    xb = np.array([b + e for b in range(8, xy, 8) for e in (-1, 0)], np.int64)
    yb = np.array([t + e for t in range(16, xy, 16) for e in (-1, 0)], np.int64)
    a = np.stack([xb, yb[(np.arange(len(xb)) * 7) % len(yb)]], axis=1)
    b = np.stack([xb[(np.arange(len(yb)) * 5) % len(xb)], yb], axis=1)
    rnd = np.random.default_rng(9000 + xy + seed).integers(0, xy, (2048, 2))
    return np.concatenate([a, b, rnd])


def large_patterns(xy, short=False):
    """name -> positive map [x, y] int32 (no negative map), for xy > 256.  short: the list of the largest size"""
    rng = np.random.default_rng(77 * xy)
    z = lambda: np.zeros((xy, xy), np.int32)                                  # noqa: E731
    out = {}
    p = z()
    p[xy - 1, 0] = 100
    out["corner_far"] = p                                                     # (0, xy - 1) lies 2 (xy - 1)^2 away: the largest d2 there is;
    p = z()                                                                   # its row's other cells look RIGHT across every chunk
    p[0, xy - 1] = 100
    out["corner_0n"] = p                                                      # ... and this one's LEFT
    p = z()
    for b in range(64, xy, 64):                                               # x = b - 1 | b: the last lane of a chunk and the first of the next
        p[b - 1, 5] = p[b, 5] = 100
    out["boundary_same_row"] = p
    p = z()
    for b in range(64, xy, 64):
        p[b - 1, xy // 2] = p[b, xy // 2 + 1] = 100
    out["boundary_adjacent_rows"] = p
    p = z()
    p[0, 16] = p[xy - 1, 16] = 100                                            # chunk 0 and the last chunk, every chunk between empty
    out["lonely"] = p
    out["random_0.1"] = np.where(rng.random((xy, xy)) < 0.001, 100, 0).astype(np.int32)
    if short:
        return out
    out["none"] = z()
    out["all"] = np.full((xy, xy), 100, np.int32)
    p = z()
    p[0, 0] = p[0, xy - 1] = p[xy - 1, 0] = p[xy - 1, xy - 1] = 100
    out["corners"] = p
    p = z()
    p[:, xy // 3] = 100
    out["full_row"] = p                                                       # one y: a full row of the [y][x] storage
    p = z()
    p[xy // 3, :] = 100
    out["full_column"] = p
    out["random_30"] = np.where(rng.random((xy, xy)) < 0.3, 100, 0).astype(np.int32)
    return out


def large_referee(mask):
    """the unbounded d2 of a large map by the cheapest exact referee that fits it; None where that is the feature transform and
    scipy is missing (the random patterns: the caller then holds cr.boundary_sample to brute_force_near)"""
    mask = np.asarray(mask, bool)
    if int(mask.any(axis=0).sum()) <= 8:
        return by_rows(mask)
    if np.array_equal(mask, np.broadcast_to(mask.all(axis=1)[:, None], mask.shape)):      # whole columns x only (or every cell):
        return np.ascontiguousarray(np.broadcast_to(by_rows(mask[:, :1]), mask.shape))    # the distance along x, whatever y
    return feature_transform(mask) if have_scipy() else None
