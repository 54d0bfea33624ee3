"""Referee of the atlas fields (include/gvom_hip.h "atlas fields"): pure numpy, composed of what exists -- AtlasRef.extent() (already
unwrapped, NOT toroidal), clearance_ref's obstacle mask and separable transform, costfield_ref's travcost (with the two clarifications
an atlas needs applied here), dijkstra, directions and path_cost, and a plain crop for the window.  Every array here is indexed [x, y]
like costfield_ref's (AtlasRef's are [y][x]: they are transposed on the way in).  Also here: the TOROIDAL TWIN -- the same pipeline
with wrap-around adjacency for the inflation and for the steps, which exists only so that tests/test_atlas_field_cpu.py can prove the
inputs would expose a kernel that forgot the seam --, the generator of terrain-like sets, the scenarios, parameter variants and
windows tests/test_atlas_field.py runs on the GPU, and the 256-cell drive."""
import functools
import heapq

import numpy as np

import atlas_ref as ar
import clearance_ref as cr
import costfield_ref as cf

THRESHOLD = 50
ROUGHNESS_RANGE = (-10.0, -4.0)
RES = 0.4                                                          # xy_resolution of every synthetic scenario


def params(inflation_cells=0, unknown="free", soft_weight=0, rough_weight=0, base=1, include_negative=True, density_threshold=THRESHOLD):
    """the dict costfield_ref.travcost reads; inflation in whole cells (inflation_cells2 = its square)"""
    return dict(density_threshold=density_threshold, include_negative=include_negative, inflation_cells2=inflation_cells * inflation_cells,
                unknown_blocks=unknown == "blocked", base=base, soft_weight=soft_weight, unknown_cost=unknown if isinstance(unknown, int) else 0,
                rough_weight=rough_weight, min_roughness=ROUGHNESS_RANGE[0], max_roughness=ROUGHNESS_RANGE[1])


def keywords(p, res=RES):
    """the same parameters as the keywords of Atlas.cost_to_go (the radius a hair above the whole cells: floor((r / res)^2) is their square)"""
    r = int(round(p["inflation_cells2"] ** 0.5))
    return dict(inflation_radius=(r + 0.01) * res if r else None, density_threshold=p["density_threshold"], include_negative=p["include_negative"],
                unknown="blocked" if p["unknown_blocks"] else (p["unknown_cost"] or "free"), base=p["base"], soft_weight=p["soft_weight"],
                rough_weight=p["rough_weight"], roughness_range=ROUGHNESS_RANGE if p["rough_weight"] else None)


def inflation(mask, cells2, wrap=False):
    """gvom_clearance's squared cells of `mask` capped at cells2, on the flat grid -- or, wrap, on the torus (the twin)"""
    if not wrap:
        return cr.separable(mask, cells2)
    n = mask.shape[0]
    return cr.separable(np.tile(mask, (3, 3)), cells2)[n:2 * n, n:2 * n]


def cell_costs(positive, negative, visibility, roughness, p, wrap=False):
    """the uint16 cost map of the extent, as int32 [x, y].  k_travcost's rule through costfield_ref.travcost, with the clarifications
    of "atlas fields": never observed is visibility <= 0, and an unblocked cost is max(1, .)"""
    vis = np.where(np.asarray(visibility) <= 0, 0, visibility)
    d2 = None
    if p["inflation_cells2"] > 0:
        d2 = inflation(cr.obstacle_mask(positive, negative, p["density_threshold"], p["include_negative"]), p["inflation_cells2"], wrap)
    # blocked: travcost's own rule (at cost 1 everywhere).  The sum is taken in int64 here: travcost's leaves int32 where `positive` is
    # far below zero, which a map set never is and an atlas may be
    free = cf.travcost(positive, negative, vis, roughness, d2, dict(p, base=1, soft_weight=0, unknown_cost=0, rough_weight=0)) > 0
    q = cf.roughness_q(roughness, p["rough_weight"], p["min_roughness"], p["max_roughness"])
    cost = p["base"] + p["soft_weight"] * np.asarray(positive, np.int64) + np.where(vis == 0, p["unknown_cost"], 0) + p["rough_weight"] * q
    return np.where(free, np.clip(cost, 1, 65535), 0).astype(np.int32)


def torus_dijkstra(c, goals, max_cost=0):
    """costfield_ref.dijkstra with wrap-around steps (the twin only)"""
    c = np.asarray(c, np.int64)
    n, cap, cl = c.shape[0], max_cost or cf.MAX_COST, c.tolist()
    D = [[cf.UNREACHED] * n for _ in range(n)]
    heap = []
    for x, y in cf._seed(c, goals):
        D[x][y] = 0
        heap.append((0, x, y))
    heapq.heapify(heap)
    while heap:
        d, x, y = heapq.heappop(heap)
        if d > D[x][y]:
            continue
        for k, (dx, dy) in enumerate(cf.STEPS):
            vx, vy = (x + dx) % n, (y + dy) % n
            if cl[vx][vy] <= 0 or (k & 1 and (cl[vx][y] <= 0 or cl[x][vy] <= 0)):
                continue
            nd = d + (7 if k & 1 else 5) * (cl[x][y] + cl[vx][vy])
            if nd <= cap and nd < D[vx][vy]:
                D[vx][vy] = nd
                heapq.heappush(heap, (nd, vx, vy))
    return np.array(D, np.int32).reshape(n, n)


def extent_maps(ref):
    """(positive, negative, visibility, roughness) of an AtlasRef's extent as [x, y] arrays, and the extent's origin"""
    (pos, neg, vis, rough, _, _), E = ref.extent()
    return (pos.T, neg.T, vis.T, rough.view(np.float64).T), tuple(E)


def field(ref, goals, p, max_cost=0, wrap=False):
    """what gvom_atlas_cost_to_go must give for an AtlasRef: dict(E, c, D, dir, info = (reached, seeded)); goals are WORLD cells
    inside the extent.  wrap: the toroidal twin's answer instead"""
    maps, E = extent_maps(ref)
    c = cell_costs(*maps, p, wrap=wrap)
    g = np.asarray(goals, np.int64).reshape(-1, 2) - np.array(E, np.int64)
    assert ((g >= 0) & (g < ref.A)).all()
    D = torus_dijkstra(c, g, max_cost) if wrap else cf.dijkstra(c, g, max_cost)
    out = dict(E=E, c=c, D=D, info=cf.info(D, c, g), goals=g)
    if not wrap:
        out["dir"] = cf.directions(D, c)
    return out


def window(f, origin, xy):
    """the plain crop: (D, dir, c) [x, y] of the xy x xy window at world cell `origin`; outside the field's extent UNREACHED, NONE, 0"""
    A = f["D"].shape[0]
    D, d, c = np.full((xy, xy), cf.UNREACHED, np.int32), np.full((xy, xy), cf.NONE, np.uint8), np.zeros((xy, xy), np.uint16)
    x0, y0 = origin[0] - f["E"][0], origin[1] - f["E"][1]
    lx, hx, ly, hy = max(x0, 0), min(x0 + xy, A), max(y0, 0), min(y0 + xy, A)
    if lx < hx and ly < hy:
        w, e = (slice(lx - x0, hx - x0), slice(ly - y0, hy - y0)), (slice(lx, hx), slice(ly, hy))
        D[w], d[w], c[w] = f["D"][e], f["dir"][e], f["c"][e]
    return D, d, c


# ---- sets that look like maps ---------------------------------------------------------------------------------------------------------
def terrain_set(rng, xy, ring=True):
    """nine [y][x] maps in set order: positive 0 .. 100 with clumps above the threshold (and, ring, one closed ring of obstacles around
    observed free ground: a pocket), sparse negative > 0, visibility 0 or > 0, roughness in -30 .. -1 or -1.0, a few cells of rank 1"""
    n = (xy, xy)
    pos = rng.integers(0, 41, n).astype(np.int32)
    for _ in range(max(2, xy * xy // 90)):
        x, y, r = rng.integers(0, xy), rng.integers(0, xy), rng.integers(1, 3)
        pos[max(0, y - r):y + r, max(0, x - r):x + r] = rng.integers(60, 101)
    vis = np.where(rng.random(n) < 0.8, rng.integers(1, 10, n), 0).astype(np.int32)
    if ring and xy >= 12:
        x, y = rng.integers(1, xy - 7, 2)
        pos[y:y + 6, x:x + 6] = 100
        pos[y + 1:y + 5, x + 1:x + 5] = rng.integers(0, 30, (4, 4))
        vis[y:y + 6, x:x + 6] = 5
    neg = np.where(rng.random(n) < 0.02, rng.integers(1, 4, n), 0).astype(np.int32)
    if ring and xy >= 12:
        neg[y + 1:y + 5, x + 1:x + 5] = 0
    rough = np.where(rng.random(n) < 0.3, -1.0, -rng.uniform(1.0, 30.0, n))
    inferred = np.full(n, -1000.0)
    r1 = (vis == 0) & (rng.random(n) < 0.2)                          # rank 1: seen by nobody, known by inference
    inferred[r1] = -1.25
    height = np.where(vis > 0, rng.uniform(-1.5, -0.5, n), -1000.0)
    maps = [pos, neg, vis, rough, height, inferred, rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), np.zeros(n)]
    return [np.ascontiguousarray(m, np.int32 if k < 3 else np.float64) for k, m in enumerate(maps)]


# ---- the synthetic scenarios ---------------------------------------------------------------------------------------------------------------
SCENARIOS = ((16, 64), (33, 64), (33, 128), (64, 128))


def _grid(lo, hi, step):
    return sorted(set(list(range(lo, hi, step)) + [hi]))


def scenario_origins(xy, A, follow):
    """the origins of a scenario's integrate_of() calls and the extent they leave.  Follow: a short walk through negative coordinates
    and across the storage seam that ends with the extent at E; every origin lies in [E, last] per axis, so nothing painted leaves
    the extent again.  Fixed: the extent of atlas_ref.fixed_origin tiled"""
    if follow:
        last = (-5 - xy // 2, 9 - xy // 2)
        E = (last[0] + xy // 2 - A // 2, last[1] + xy // 2 - A // 2)
        side = A // 2 - xy // 2
        step = max(xy * 3 // 4, side // 2)
        return [(E[0] + i, E[1] + j) for j in _grid(0, side, step) for i in _grid(0, side, step)], E
    E = ar.fixed_origin(xy, A)
    return [(E[0] + i, E[1] + j) for j in range(0, A, xy) for i in range(0, A, xy)], E


@functools.lru_cache(maxsize=None)
def scenario(xy, A, follow):
    """(AtlasRef after the scenario's integrates, ((set, origin), ...)); built once, shared, read-only"""
    rng = np.random.default_rng(7000 * xy + A + int(follow))
    origins, E = scenario_origins(xy, A, follow)
    ref = ar.AtlasRef(A, xy, follow, (0, 0) if follow else E)
    steps = []
    for o in origins:
        s = terrain_set(rng, xy)
        for m in s:
            m.setflags(write=False)
        ref.integrate(s, o)
        steps.append((tuple(s), o))
    assert ref.E == E and (E[0] & (A - 1)) and (E[1] & (A - 1)) and E[0] < 0 and E[1] < 0
    return ref, tuple(steps)


# (inflation cells, unknown, soft_weight, rough_weight, 17 goals, max_cost cut): every inflation with every `unknown`, the rest alternating
VARIANTS = ((0, "free", 0, 0, False, False), (1, "blocked", 20, 7, True, False), (5, 250, 5, 0, True, False),
            (0, 250, 0, 600, False, True), (1, "free", 0, 0, True, True), (5, "blocked", 0, 7, False, False),
            (0, "blocked", 20, 0, True, False), (5, "free", 3, 40, False, True), (1, 250, 2, 0, False, False))


def variant_params(v):
    return params(inflation_cells=v[0], unknown=v[1], soft_weight=v[2], rough_weight=v[3], base=1 + (v[2] > 0))


@functools.lru_cache(maxsize=None)
def scenario_goals(xy, A, follow, many):
    """WORLD cells.  One goal: the free cell nearest the last set's centre.  Seventeen: twelve free cells, four on hard obstacles, the
    first one twice.  Free means free without inflation; hard obstacles are blocked under every variant"""
    ref, steps = scenario(xy, A, follow)
    maps, E = extent_maps(ref)
    c = cell_costs(*maps, params())
    o = steps[-1][1]
    if not many:                                                   # (not in a pocket: it stays free and connected under five cells of inflation)
        c5 = cell_costs(*maps, params(inflation_cells=5))
        cx, cy = o[0] - E[0] + xy // 2, o[1] - E[1] + xy // 2
        near = sorted((tuple(u) for u in np.argwhere(c5 > 0)), key=lambda u: (max(abs(u[0] - cx), abs(u[1] - cy)), u))
        x, y = max(near[::7][:24] or near[:1] or [cf._free_near(c, cx, cy)], key=lambda u: (c5[u] > 0) and cf.info(cf.dijkstra(c5, [u]), c5, [u])[0])
        return ((int(x) + E[0], int(y) + E[1]),)
    rng = np.random.default_rng(11 * xy + A)
    free, hard = np.argwhere(c > 0), np.argwhere(cr.obstacle_mask(maps[0], maps[1], THRESHOLD))
    pick = [tuple(free[i]) for i in rng.choice(len(free), 12, replace=False)] + [tuple(hard[i]) for i in rng.choice(len(hard), 4, replace=False)]
    return tuple((int(x) + E[0], int(y) + E[1]) for x, y in pick + [pick[0]])


@functools.lru_cache(maxsize=None)
def expected(xy, A, follow, k):
    """the referee's field of variant k of a scenario (the cut: the median of the uncut field's finite values), read-only"""
    ref, _ = scenario(xy, A, follow)
    v = VARIANTS[k]
    p, goals = variant_params(v), scenario_goals(xy, A, follow, v[4])
    cap = 0
    if v[5]:
        full = field(ref, goals, p)["D"]
        cap = int(np.median(full[full != cf.UNREACHED]))
    f = field(ref, goals, p, cap)
    f["max_cost"], f["params"], f["goals_world"] = cap, p, goals
    for a in (f["c"], f["D"], f["dir"]):
        a.setflags(write=False)
    return f


def window_origins(xy, A, E, steps):
    """where the tests crop: the current (last) origin, the first origin, half outside the extent, wholly outside it"""
    return [steps[-1][1], steps[0][1], (E[0] + A - xy // 2, E[1] - xy // 2), (E[0] + A + 7, E[1] - 2 * xy)]


def census(xy, A, follow):
    """what tests/test_atlas_field_cpu.py holds floors on, summed over the scenario's variants and windows"""
    ref, steps = scenario(xy, A, follow)
    maps, E = extent_maps(ref)
    out = dict.fromkeys(("inflation_differs_from_twin", "D_differs_from_twin", "blocked_from_outside_the_window", "blocked_goals",
                         "pocket", "ties", "window_cells_outside", "windows_wholly_outside", "cut", "rank1"), 0)
    out["rank1"] = int((ar.rank(ref.i[2], ref.i[1], ref.f[2]) == 1).sum())
    for k, v in enumerate(VARIANTS):
        f = expected(xy, A, follow, k)
        p = f["params"]
        twin = field(ref, f["goals_world"], p, f["max_cost"], wrap=True)
        out["inflation_differs_from_twin"] += int(((f["c"] > 0) != (twin["c"] > 0)).sum())
        out["D_differs_from_twin"] += int((f["D"] != twin["D"]).sum())
        out["blocked_goals"] += len(f["goals"]) - f["info"][1]
        uncut = field(ref, f["goals_world"], p)["D"] if f["max_cost"] else f["D"]
        out["pocket"] += int(((f["c"] > 0) & (uncut == cf.UNREACHED)).sum())
        out["cut"] += int(((uncut != cf.UNREACHED) & (f["D"] == cf.UNREACHED)).sum())
        out["ties"] += int((np.sum(cf.matches(f["D"], f["c"]), axis=0) >= 2).sum())
        for o in window_origins(xy, A, E, steps):
            lo = (o[0] - E[0], o[1] - E[1])
            inside = (slice(max(lo[0], 0), max(min(lo[0] + xy, A), 0)), slice(max(lo[1], 0), max(min(lo[1] + xy, A), 0)))
            n_in = f["c"][inside].size
            out["window_cells_outside"] += xy * xy - n_in if n_in else 0
            out["windows_wholly_outside"] += n_in == 0
            if n_in and p["inflation_cells2"]:
                local = cell_costs(*[m[inside] for m in maps], p)
                out["blocked_from_outside_the_window"] += int(((local > 0) & (f["c"][inside] == 0)).sum())
    return out


# ---- the seam --------------------------------------------------------------------------------------------------------------------------------
def seam_set(xy):
    """an observed, empty, flat set ([y][x]); seam_walls() says which of its cells become walls"""
    n = (xy, xy)
    return [np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, 3, np.int32), np.full(n, -1.0), np.full(n, -1.0), np.full(n, -1000.0),
            np.zeros(n), np.zeros(n), np.zeros(n)]


def seam_case(xy, A, E):
    """the open map with a wall along extent column 0 and along extent row A - 1: ((set, origin), ...) tiling the extent, the goal in
    column 4 and the start in column A - 5 (world cells), inflation three cells.  On the torus the walls would be neighbours of column
    A - 1 and of row 0"""
    steps = []
    for j in range(0, A, xy):
        for i in range(0, A, xy):
            s = seam_set(xy)
            x = np.arange(i, i + xy)[None, :] + np.zeros((xy, 1), np.int64)
            y = np.arange(j, j + xy)[:, None] + np.zeros((1, xy), np.int64)
            s[0][(x == 0) | (y == A - 1)] = 100
            steps.append((s, (E[0] + i, E[1] + j)))
    return steps, (E[0] + 4, E[1] + A // 2), (E[0] + A - 5, E[1] + A // 2)


# ---- the drive, with an atlas of 256 cells ---------------------------------------------------------------------------------------------------
DRIVE_A = 256


def drive_out():
    """the outward leg of atlas_ref's drive: ((cloud, ego), ...), nine scans"""
    return ar.drive_scans()[:ar.DRIVE_LEGS + 1]


def well_connected(c):
    """a free cell (x, y) of the [x, y] cost map that is in no pocket: of a sample of the free cells, the one that reaches most"""
    free = [tuple(int(v) for v in u) for u in np.argwhere(np.asarray(c) > 0)]
    return max(free[::max(1, len(free) // 16)], key=lambda u: cf.info(cf.dijkstra(c, [u]), c, [u])[0])


def nearest_free(c, cell):
    """the free cell of the [x, y] cost map nearest `cell` in the order of a growing square (costfield_ref._free_near)"""
    return cf._free_near(c, int(cell[0]), int(cell[1]))
