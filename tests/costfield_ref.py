"""The referee of the cost-to-go field (gvom_cost_to_go; include/gvom_hip.h "cost-to-go fields"), straight from the definition and
shared by tests/test_costfield_cpu.py, tests/test_costfield.py and tools/costfield_bench.py.  Two independent forms that must agree
bit for bit: a heap Dijkstra from the goals, and a vectorised numpy relaxation swept to its fixed point.  Every array is indexed
[x, y].  Also: the direction rule, the cost map of a map set (travcost), the patterns the GPU tests run, and their census."""
import functools
import heapq

import numpy as np

UNREACHED = 2 ** 31 - 1
MAX_COST = 2 ** 30
GOAL, UNSETTLED, NONE = 8, 254, 255
STEPS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))
TILE = 32                                     # the solver's tile: the census counts tile crossings with it
SIZES = (16, 31, 32, 33, 50, 64, 65, 100, 129)     # one partial tile; each side of 16, 32, 64; ragged last tiles; 2 x 2 tiles; >= 3 tiles; 5 x 5 with a last tile one cell wide
LARGE = (1024, 4096)                          # 32 x 32 and 128 x 128 tiles (the largest map the call accepts): large_patterns() below
INF = 2 ** 60                                 # (INF + INF fits int64)


def iter_weights(c, corner_rule=True):
    """w[k][x, y], k = 0 .. 7 in turn: the weight of the step from (x, y) in direction k, INF where it is not admissible"""
    c = np.asarray(c, np.int64)
    n = c.shape[0]
    pad = np.zeros((n + 2, n + 2), np.int64)
    pad[1:-1, 1:-1] = c
    at = lambda dx, dy: pad[1 + dx:n + 1 + dx, 1 + dy:n + 1 + dy]
    for k, (dx, dy) in enumerate(STEPS):
        ok = (c > 0) & (at(dx, dy) > 0)
        if k & 1 and corner_rule:
            ok &= (at(dx, 0) > 0) & (at(0, dy) > 0)
        yield np.where(ok, (7 if k & 1 else 5) * (c + at(dx, dy)), INF)


def weights(c, corner_rule=True):
    """the eight of them as a list (a map of 4096 cells a side is better served one direction at a time: 128 MB each)"""
    return list(iter_weights(c, corner_rule))


def _seed(c, goals):
    c = np.asarray(c)
    return [(int(x), int(y)) for x, y in np.asarray(goals).reshape(-1, 2) if c[int(x), int(y)] > 0]


def dijkstra(c, goals, max_cost=0, corner_rule=True):
    """D int32 [x, y]: a binary heap from the seeded goals; a candidate is accepted only if it is <= max_cost (0: 2^30)"""
    c = np.asarray(c, np.int64)
    n = c.shape[0]
    cap = max_cost or MAX_COST
    cl = c.tolist()
    D = [[UNREACHED] * n for _ in range(n)]
    heap = []
    for x, y in _seed(c, goals):
        D[x][y] = 0
        heap.append((0, x, y))
    heapq.heapify(heap)
    while heap:
        d, x, y = heapq.heappop(heap)
        if d > D[x][y]:
            continue
        cu = cl[x][y]
        for k, (dx, dy) in enumerate(STEPS):
            vx, vy = x + dx, y + dy
            if not (0 <= vx < n and 0 <= vy < n) or cl[vx][vy] <= 0:
                continue
            if k & 1 and corner_rule and (cl[vx][y] <= 0 or cl[x][vy] <= 0):
                continue
            nd = d + (7 if k & 1 else 5) * (cu + cl[vx][vy])
            if nd <= cap and nd < D[vx][vy]:
                D[vx][vy] = nd
                heapq.heappush(heap, (nd, vx, vy))
    return np.array(D, np.int32).reshape(n, n)


def relax(c, goals, max_cost=0, corner_rule=True, sweeps=None):
    """D int32 [x, y]: whole-map Jacobi sweeps of D[u] = min(D[u], D[v] + w(u, v)) to the fixed point (or `sweeps` of them)"""
    c = np.asarray(c, np.int64)
    n = c.shape[0]
    cap = max_cost or MAX_COST
    w = weights(c, corner_rule)
    D = np.full((n + 2, n + 2), INF, np.int64)
    for x, y in _seed(c, goals):
        D[1 + x, 1 + y] = 0
    k = 0
    while sweeps is None or k < sweeps:
        k += 1
        best = np.full((n, n), INF, np.int64)
        for wk, (dx, dy) in zip(w, STEPS):
            np.minimum(best, D[1 + dx:n + 1 + dx, 1 + dy:n + 1 + dy] + wk, out=best)
        inner = D[1:-1, 1:-1]
        take = (best <= cap) & (best < inner)
        if not take.any():
            break
        inner[take] = best[take]
    return np.where(D[1:-1, 1:-1] >= INF, UNREACHED, D[1:-1, 1:-1]).astype(np.int32)


def tiled(c, goals, max_cost=0, inner=256, max_rounds=0, tile=TILE):
    """The solver's own schedule on the CPU, to show that it reaches the same fixed point: rounds in which every ACTIVE tile loads
    itself and a one-cell halo, sweeps to its local fixed point (at most `inner` sweeps; one that runs out marks itself again),
    stores what went down, and marks the up to eight neighbours whose halo holds a lowered rim cell; a goal marks its tile and
    the tiles that see it in their halo.  Returns (D int32 [x, y], rounds run, tile relaxations, converged)."""
    c = np.asarray(c, np.int64)
    n = c.shape[0]
    cap = max_cost or MAX_COST
    nt = (n + tile - 1) // tile
    w = [np.pad(wk, 1, constant_values=INF) for wk in weights(c)]
    D = np.full((n + 2, n + 2), INF, np.int64)
    active = set()
    for x, y in _seed(c, goals):
        D[1 + x, 1 + y] = 0
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                if 0 <= x + dx < n and 0 <= y + dy < n:
                    active.add(((x + dx) // tile, (y + dy) // tile))
    rounds = relaxations = 0
    while True:
        rounds += 1
        nxt, stores = set(), []
        for tx, ty in sorted(active):
            relaxations += 1
            x0, y0 = tx * tile, ty * tile
            x1, y1 = min(n, x0 + tile), min(n, y0 + tile)
            L = D[x0:x1 + 2, y0:y1 + 2].copy()                    # the tile and its halo, as the round found them
            before = L[1:-1, 1:-1].copy()
            more = True
            for _ in range(inner):
                best = np.full(before.shape, INF, np.int64)
                for wk, (dx, dy) in zip(w, STEPS):
                    np.minimum(best, L[1 + dx:L.shape[0] - 1 + dx, 1 + dy:L.shape[1] - 1 + dy] + wk[1 + x0:1 + x1, 1 + y0:1 + y1], out=best)
                take = (best <= cap) & (best < L[1:-1, 1:-1])
                if not take.any():
                    more = False
                    break
                L[1:-1, 1:-1][take] = best[take]
            low = L[1:-1, 1:-1] < before
            stores.append((x0, x1, y0, y1, L[1:-1, 1:-1]))
            if more:
                nxt.add((tx, ty))
            for x, y in np.argwhere(low):
                ex = -1 if x == 0 else (1 if x == tile - 1 else 0)
                ey = -1 if y == 0 else (1 if y == tile - 1 else 0)
                for ax, ay in ((ex, 0), (0, ey), (ex, ey)):
                    if (ax or ay) and (ax == ex or not ax) and 0 <= tx + ax < nt and 0 <= ty + ay < nt:
                        nxt.add((tx + ax, ty + ay))
        for x0, x1, y0, y1, v in stores:                          # (every tile read what EARLIER rounds wrote: the harder case)
            D[1 + x0:1 + x1, 1 + y0:1 + y1] = v
        active = nxt
        if not active or rounds == max_rounds:
            break
    out = np.where(D[1:-1, 1:-1] >= INF, UNREACHED, D[1:-1, 1:-1]).astype(np.int32)
    return out, rounds, relaxations, not active


def iter_matches(D, c, corner_rule=True):
    """(match, offer) of neighbour k = 0 .. 7 in turn.  match [x, y] bool: the neighbour is admissible with D[v] + w(u, v) == D[u]
    (only where D[u] is finite and not 0); offer [x, y] int64: D[v] + w(u, v), >= INF where the step is not admissible or v is
    unreached"""
    D = np.asarray(D, np.int64)
    n = D.shape[0]
    pad = np.full((n + 2, n + 2), INF, np.int64)
    pad[1:-1, 1:-1] = np.where(D == UNREACHED, INF, D)
    live = (D != UNREACHED) & (D != 0)
    for wk, (dx, dy) in zip(iter_weights(c, corner_rule), STEPS):
        offer = pad[1 + dx:n + 1 + dx, 1 + dy:n + 1 + dy] + wk
        yield live & (wk < INF) & (offer == D), offer


def matches(D, c, corner_rule=True):
    """[8][x, y] bool: the matches of iter_matches"""
    return [m for m, _ in iter_matches(D, c, corner_rule)]


def directions(D, c):
    """uint8 [x, y]: the smallest matching k; GOAL where D == 0, NONE where unreached, UNSETTLED where nothing matches"""
    D = np.asarray(D)
    out = np.full(D.shape, UNSETTLED, np.uint8)
    for k, (m, _) in enumerate(iter_matches(D, c)):
        out[m & (out == UNSETTLED)] = k
    out[D == 0] = GOAL
    out[D == UNREACHED] = NONE
    return out


def bellman(D, c, goals, max_cost=0):
    """What makes D THE cost-to-go field of (c, goals, max_cost), checked cell by cell without solving anything -- for the maps a
    heap Dijkstra in Python is too slow for.  Returns ({violation: number of cells}, the directions of D), in one pass over
    iter_matches.  The conditions:
      goal         the cells with D == 0 are exactly the goals that lie on free cells
      blocked      no blocked cell is reached
      above_cap    no reached cell lies above the cap
      no_match     every other reached cell has a neighbour with D[v] + w(u, v) == D[u] ...
      offers_less  ... and no admissible neighbour offers less
      left_out     no unreached free cell has a reached admissible neighbour whose offer is at or below the cap
    Weights are positive, so the matches of a reached cell lead down a chain of strictly smaller values that can only end in a
    goal: D[u] is the cost of a path, hence no less than the true value; offers_less (by induction along a shortest path) makes it
    no more; left_out does the same for the cells Dijkstra would have accepted.  tests/test_costfield_cpu.py pins the check to
    Dijkstra and shows it rejects single-cell errors."""
    D, c = np.asarray(D), np.asarray(c)
    cap = max_cost or MAX_COST
    reached = D != UNREACHED
    seeded = np.zeros(D.shape, bool)
    for x, y in _seed(c, goals):
        seeded[x, y] = True
    any_match = np.zeros(D.shape, bool)
    best = np.full(D.shape, INF, np.int64)
    d = np.full(D.shape, UNSETTLED, np.uint8)
    for k, (m, offer) in enumerate(iter_matches(D, c)):
        d[m & ~any_match] = k
        any_match |= m
        np.minimum(best, offer, out=best)
    d[D == 0] = GOAL
    d[~reached] = NONE
    inner = reached & (D != 0)
    bad = {"goal": int(((D == 0) != seeded).sum()), "blocked": int((reached & (c <= 0)).sum()),
           "above_cap": int((reached & (D > cap)).sum()), "no_match": int((inner & ~any_match).sum()),
           "offers_less": int((inner & (best < D)).sum()), "left_out": int((~reached & (c > 0) & (best <= cap)).sum())}
    return {k: v for k, v in bad.items() if v}, d


def info(D, c, goals):
    """what the call reports besides convergence and rounds: (reached cells, goals seeded)"""
    return int((np.asarray(D) != UNREACHED).sum()), len(_seed(c, goals))


def path_cost(path, c):
    """the sum of the step weights along a list of cells; AssertionError on a step that is not admissible"""
    c = np.asarray(c, np.int64)
    n, total = c.shape[0], 0
    for (x, y), (vx, vy) in zip(path[:-1], path[1:]):
        dx, dy = vx - x, vy - y
        assert (dx, dy) in STEPS and 0 <= vx < n and 0 <= vy < n and c[x, y] > 0 and c[vx, vy] > 0, ((x, y), (vx, vy))
        if dx and dy:
            assert c[vx, y] > 0 and c[x, vy] > 0, ("corner cut", (x, y), (vx, vy))
        total += (7 if dx and dy else 5) * int(c[x, y] + c[vx, vy])
    return total


def roughness_q(r, rough_weight, rmin, rmax):
    r = np.asarray(r, np.float64)
    if rough_weight == 0:
        return np.zeros(r.shape, np.int64)
    with np.errstate(invalid="ignore"):
        on = r > rmin
        q = np.floor(((np.where(on, np.minimum(r, rmax), rmin) - rmin) / (rmax - rmin)) * 100.0)
    return np.where(on, q, 0).astype(np.int64)


def travcost(positive, negative, visibility, roughness, d2, params):
    """The cost map of a map set, [x, y] int32.  params: dict with density_threshold, include_negative, inflation_cells2,
    unknown_blocks, base, soft_weight, unknown_cost, rough_weight, min_roughness, max_roughness.  d2: the clearance's squared
    cells for the same threshold and negative flag (read only when inflation_cells2 > 0)."""
    p = dict(inflation_cells2=0, include_negative=True, unknown_blocks=False, base=1, soft_weight=0, unknown_cost=0, rough_weight=0,
             min_roughness=0.0, max_roughness=1.0, density_threshold=50)
    p.update(params)
    pos, vis = np.asarray(positive, np.int64), np.asarray(visibility, np.int64)
    blocked = pos.astype(np.float64) > float(p["density_threshold"])
    if p["include_negative"]:
        blocked |= np.asarray(negative) > 0
    if p["inflation_cells2"] > 0:
        blocked |= np.asarray(d2, np.int64) <= p["inflation_cells2"]
    if p["unknown_blocks"]:
        blocked |= vis == 0
    q = roughness_q(roughness, p["rough_weight"], p["min_roughness"], p["max_roughness"])
    cost = p["base"] + p["soft_weight"] * pos + np.where(vis == 0, p["unknown_cost"], 0) + p["rough_weight"] * q
    return np.where(blocked, 0, np.minimum(65535, cost)).astype(np.int32)


# ---- the patterns of the GPU tests ------------------------------------------------------------------------------------------------

def _free_near(c, x, y):
    """the free cell nearest (x, y) in the order of a growing square"""
    n = c.shape[0]
    for r in range(n):
        for vx in range(max(0, x - r), min(n, x + r + 1)):
            for vy in range(max(0, y - r), min(n, y + r + 1)):
                if c[vx, vy] > 0:
                    return vx, vy
    raise ValueError("no free cell")


def _random_costs(xy, seed):
    rng = np.random.default_rng(seed)
    c = rng.integers(1, 65536, (xy, xy)).astype(np.int32)
    c[rng.random((xy, xy)) < 0.25] = 0
    return c


@functools.lru_cache(maxsize=None)
def patterns(xy):
    """{name: (cost map int32 [x, y], goals int32 (G, 2), max_cost)}; built once per size, read-only.  The max_cost of the *_cut
    patterns is the median of the finite values of the uncut field: about half of the reachable cells are cut off."""
    out = {}
    one = np.ones((xy, xy), np.int32)
    out["open"] = (one, [(0, 0)], 0)
    rnd = _random_costs(xy, 100 + xy)
    g0 = _free_near(rnd, xy // 2, xy // 3)
    out["random"] = (rnd, [g0], 0)
    walls = one.copy()
    for k, x in enumerate(range(3, xy, 5)):
        walls[x, :] = 0
        walls[x, (7 * k + 2) % xy] = 3
    out["walls"] = (walls, [(0, xy - 1)], 0)
    serp = one.copy()
    for k, x in enumerate(range(1, xy, 2)):
        serp[x, :] = 0
        serp[x, xy - 1 if k % 2 == 0 else 0] = 1
    out["serpentine"] = (serp, [(0, 0)], 0)
    pocket = one.copy()
    a, b = xy // 3, min(xy - 1, xy // 3 + max(4, xy // 4))
    pocket[a:b + 1, a] = pocket[a:b + 1, b] = 0
    pocket[a, a:b + 1] = pocket[b, a:b + 1] = 0
    out["pocket"] = (pocket, [(xy - 1, 0)], 0)
    diag = np.full((xy, xy), 2, np.int32)
    for i in range(xy):
        if i % 16 != 13:
            diag[i, i] = 0                                  # one blocked cell per step: only the corner rule keeps the sides apart
    q = xy // 2
    for x in range(q, min(xy, q + 7)):
        for y in range(0, min(xy // 4, 6)):
            if (x + y) % 2 == 0:
                diag[x, y] = 0                              # a checkerboard: its free cells touch at corners only
    out["diagonal_wall"] = (diag, [(xy - 1, 0)], 0)
    out["all_blocked"] = (np.zeros((xy, xy), np.int32), [(0, 0), (xy - 1, xy - 1)], 0)
    single = np.zeros((xy, xy), np.int32)
    single[xy - 1, xy // 2] = 40000
    out["single_free_goal"] = (single, [(xy - 1, xy // 2)], 0)
    blocked = np.argwhere(rnd == 0)
    free = np.argwhere(rnd > 0)
    rng = np.random.default_rng(7 + xy)
    out["two_goals"] = (rnd, [_free_near(rnd, xy - 1, xy - 1), tuple(blocked[0])], 0)
    pick = [tuple(free[i]) for i in rng.choice(len(free), 12, replace=False)] + [tuple(blocked[i]) for i in rng.choice(len(blocked), 4, replace=False)]
    out["seventeen_goals"] = (rnd, pick + [pick[0]], 0)     # (one goal twice, four on blocked cells)
    for name in ("open", "random", "walls"):
        c, goals, _ = out[name]
        full = dijkstra(c, goals)
        out[name + "_cut"] = (c, goals, int(np.median(full[full != UNREACHED])))
    final = {}
    for name, (c, goals, cap) in out.items():
        c = np.array(c, np.int32)
        c.setflags(write=False)
        final[name] = (c, np.array(goals, np.int32).reshape(-1, 2), cap)
    return final


@functools.lru_cache(maxsize=None)
def large_patterns(xy):
    """the patterns of the LARGE sizes, as patterns() builds them (same seeds and rules): open, random, seventeen_goals, and at
    1024 random_cut.  No serpentine: its rounds grow with corridors x tiles.  The cap of random_cut is the median of random's own
    field (large_expected), so it is filled in there."""
    one = np.ones((xy, xy), np.int32)
    rnd = _random_costs(xy, 100 + xy)
    blocked, free = np.argwhere(rnd == 0), np.argwhere(rnd > 0)
    rng = np.random.default_rng(7 + xy)
    pick = [tuple(free[i]) for i in rng.choice(len(free), 12, replace=False)] + [tuple(blocked[i]) for i in rng.choice(len(blocked), 4, replace=False)]
    out = {"open": (one, [(0, 0)]), "random": (rnd, [_free_near(rnd, xy // 2, xy // 3)]), "seventeen_goals": (rnd, pick + [pick[0]])}
    final = {}
    for name, (c, goals) in out.items():
        c = np.array(c, np.int32)
        c.setflags(write=False)
        final[name] = (c, np.array(goals, np.int32).reshape(-1, 2))
    return final


def open_field(xy, goal=(0, 0)):
    """the field of an all-ones map with one goal, in closed form: min(dx, dy) diagonal steps of 7 (1 + 1) and |dx - dy| straight
    ones of 5 (1 + 1) -- no cheaper mix exists, since a diagonal step (14) costs less than the two straight ones it replaces (20)"""
    dx = np.abs(np.arange(xy, dtype=np.int64) - goal[0])[:, None]
    dy = np.abs(np.arange(xy, dtype=np.int64) - goal[1])[None, :]
    return (14 * np.minimum(dx, dy) + 10 * np.abs(dx - dy)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def large_expected(xy, name):
    """(c, goals, max_cost, D, dir, (reached, seeded)) at 1024 cells by heap Dijkstra -- about 4 s a pattern, computed once"""
    cut = name == "random_cut"
    c, goals = large_patterns(xy)["random" if cut else name]
    cap = 0
    if cut:
        full = large_expected(xy, "random")[3]
        cap = int(np.median(full[full != UNREACHED]))
    D = dijkstra(c, goals, cap)
    d = directions(D, c)
    D.setflags(write=False)
    d.setflags(write=False)
    return c, goals, cap, D, d, info(D, c, goals)


@functools.lru_cache(maxsize=None)
def expected(xy, name):
    """(D, dir, (reached, seeded)) of a pattern by Dijkstra; computed once, shared, read-only"""
    c, goals, cap = patterns(xy)[name]
    D = dijkstra(c, goals, cap)
    d = directions(D, c)
    D.setflags(write=False)
    d.setflags(write=False)
    return D, d, info(D, c, goals)


# ---- the census ---------------------------------------------------------------------------------------------------------------------

def tile_crossings(D, d, tile=TILE):
    """[x, y] int: how many tile boundaries the path that follows the directions from each reached cell crosses (-1: unreached)"""
    D, d = np.asarray(D), np.asarray(d)
    out = np.full(D.shape, -1, np.int64)
    order = np.argsort(np.where(D == UNREACHED, INF, D.astype(np.int64)), axis=None, kind="stable")
    for flat in order:
        x, y = divmod(int(flat), D.shape[1])
        k = int(d[x, y])
        if k == GOAL:
            out[x, y] = 0
        elif k < 8:
            vx, vy = x + STEPS[k][0], y + STEPS[k][1]
            out[x, y] = out[vx, vy] + ((vx // tile, vy // tile) != (x // tile, y // tile))
    return out


def census(c, goals, cap):
    """the counts tests/test_costfield_cpu.py holds floors on, for one pattern"""
    c = np.asarray(c)
    D = dijkstra(c, goals, cap)
    full = dijkstra(c, goals) if cap else D
    loose = dijkstra(c, goals, cap, corner_rule=False)
    d = directions(D, c)
    ties = np.sum(matches(D, c), axis=0)
    return {
        "blocked": int((c == 0).sum()), "reached": int((D != UNREACHED).sum()),
        "pocket": int(((c > 0) & (full == UNREACHED)).sum()),
        "cut": int(((full != UNREACHED) & (D == UNREACHED)).sum()),
        "corner_rule": int((D != loose).sum()), "ties": int((ties >= 2).sum()),
        "crossings3": int((tile_crossings(D, d) >= 3).sum()),
    }


# ---- the map-set scenes (tests/obstacle_scenes.py) ------------------------------------------------------------------------------

SCENES = ("one_round", "two_rounds")          # ring slots (buffer_size) 1 and 2
SCENE_THRESHOLD = 50
ROUGHNESS_RANGE = (-10.0, -4.0)               # (the scenes' roughness runs from -30 to -1: tests/test_costfield_cpu.py counts 0 < q < 100)
# parameter variants of the map-set route: no inflation, one cell, a radius of several cells; each with the unknown flag on and off
VARIANTS = tuple(
    dict(inflation_radius=r, unknown=u, base=b, soft_weight=s, rough_weight=w, include_negative=n)
    for r, b, s, w, n in ((None, 1, 0, 0, True), (0.4, 3, 20, 7, True), (1.0, 2, 5, 600, False))
    for u in ("free", "blocked", 250)
)


def variant_params(v, xy_resolution, max_cells2_of):
    """a VARIANTS entry -> the dict travcost() reads"""
    return dict(density_threshold=SCENE_THRESHOLD, include_negative=v["include_negative"],
                inflation_cells2=max_cells2_of(v["inflation_radius"], xy_resolution), unknown_blocks=v["unknown"] == "blocked",
                base=v["base"], soft_weight=v["soft_weight"], unknown_cost=v["unknown"] if isinstance(v["unknown"], int) else 0,
                rough_weight=v["rough_weight"], min_roughness=ROUGHNESS_RANGE[0], max_roughness=ROUGHNESS_RANGE[1])


def world_to_cells(points, xy_resolution, origin):
    p = np.asarray(points, np.float64)
    return (np.floor(p / xy_resolution) - np.round(np.asarray(origin, np.float64)[:2] / xy_resolution)).astype(np.int64)
