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
