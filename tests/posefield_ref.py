"""The numpy referee of pose fields (include/gvom_hip.h "pose fields"; gvom_pose_field, gvom_posefield.hip) and the inputs of
tests/test_posefield.py and tests/test_posefield_cpu.py.

The definition, said four ways that the CPU test holds together:
  volume()            the pose cost volume C[h, x, y], by shifting the cost map once per footprint cell; volume_by_rollouts() is the
                      pose cost of tests/rollouts_ref.py at the cell centres, the same number by the rollout definition
  dijkstra()          a heap Dijkstra over Python integers on the REVERSED graph, from the seeded states
  relax()             whole-volume relaxation in numpy, one primitive at a time, to the fixed point: bit for bit dijkstra()
  bellman_violations() the state-by-state conditions that make a volume THE field (0 violations), for cases too large for the two:
                      D = 0 exactly at the seeds; a finite D equals the minimum over the admissible primitives of price + D[v] and
                      is at most the cap; an unreached state has no admissible primitive with price + D[v] <= cap.  Prices are
                      positive, so a finite D descends to a seed along real primitives (D >= the field) and no primitive
                      undercuts it (D <= the field along a cheapest drive, by induction from the seed).
actions() is the first primitive in table order that attains D.  Everything is integer: tolerance 0.

cases() are the GPU test's inputs; census() counts what they reach."""
import functools
import heapq
import math

import numpy as np

import rollouts_ref

UNREACHED = 2 ** 31 - 1
MAX_COST = 1 << 30
GOAL, UNSETTLED, NONE = 253, 254, 255
TILE = 8                                            # the solver's tile edge (gvom_posefield.hip PF_T): the grid sizes below straddle it
CTG_STEPS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))


def shifted(A, dx, dy, fill):
    """B[..., x, y] = A[..., x + dx, y + dy]; `fill` where that lies outside"""
    n = A.shape[-1]
    B = np.full_like(A, fill)
    x0, x1, y0, y1 = max(0, -dx), min(n, n - dx), max(0, -dy), min(n, n - dy)
    if x0 < x1 and y0 < y1:
        B[..., x0:x1, y0:y1] = A[..., x0 + dx:x1 + dx, y0 + dy:y1 + dy]
    return B


def volume(c, table):
    """C uint16 [H, x, y] of a cost map c [x, y] under the footprint table (start, offsets)"""
    c = np.asarray(c).astype(np.int64)
    start, offsets = np.asarray(table[0], np.int64), np.asarray(table[1], np.int64)
    H = len(start) - 1
    C = np.zeros((H,) + c.shape, np.uint16)
    for h in range(H):
        bad = np.zeros(c.shape, bool)
        mx = np.zeros(c.shape, np.int64)
        for dx, dy in offsets[start[h]:start[h + 1]]:
            s = shifted(c, int(dx), int(dy), 0)
            bad |= s == 0
            np.maximum(mx, s, out=mx)
        C[h] = np.where(bad, 0, mx)
    return C


def centre_poses(xy, H, res=1.0):
    """float32 [H * xy, xy, 3]: the pose at the centre of every cell with yaw 2 pi h / H; rollout h * xy + x, pose y"""
    x, y = np.meshgrid(np.arange(xy), np.arange(xy), indexing="ij")
    p = np.zeros((H, xy, xy, 3), np.float32)
    p[..., 0] = ((x + 0.5) * res)[None]
    p[..., 1] = ((y + 0.5) * res)[None]
    p[..., 2] = (2.0 * np.pi * np.arange(H) / H).astype(np.float32)[:, None, None]
    return p.reshape(H * xy, xy, 3)


def volume_by_rollouts(c, table):
    """the same through rollouts_ref.score(): the pose cost of "rollout scoring" at the cell centres"""
    xy = np.asarray(c).shape[0]
    H = len(table[0]) - 1
    _, cost, _ = rollouts_ref.score(np.asarray(c, np.uint16), centre_poses(xy, H), table, 1.0, (0, 0))
    return cost.reshape(H, xy, xy)


def seed_mask(C, goals):
    """bool [H, x, y]: the states the goals (G, 3) = (x, y, h; h < 0: every heading) seed -- those with C != 0"""
    m = np.zeros(C.shape, bool)
    for x, y, h in np.asarray(goals, np.int64).reshape(-1, 3):
        if h < 0:
            m[:, x, y] = True
        else:
            m[h, x, y] = True
    return m & (C != 0)


def _prims(table):
    start, prims = np.asarray(table[0], np.int64), np.asarray(table[1], np.int64).reshape(-1, 4)
    return [[tuple(int(v) for v in prims[p]) for p in range(start[h], start[h + 1])] for h in range(len(start) - 1)]


def dijkstra(C, table, seeds, max_cost=None):
    """D int32 [H, x, y] by a heap over Python integers on the reversed graph"""
    H, n, _ = C.shape
    cap = MAX_COST if max_cost is None else int(max_cost)
    Cl = C.astype(np.int64).tolist()
    rev = [[] for _ in range(H)]                     # rev[h_to] = (h, dx, dy, w)
    for h, lst in enumerate(_prims(table)):
        for dx, dy, ht, w in lst:
            rev[ht].append((h, dx, dy, w))
    D = [[[UNREACHED] * n for _ in range(n)] for _ in range(H)]
    heap = []
    for h, x, y in zip(*np.nonzero(seeds)):
        D[h][x][y] = 0
        heap.append((0, int(h), int(x), int(y)))
    heapq.heapify(heap)
    while heap:
        d, ht, x, y = heapq.heappop(heap)
        if d != D[ht][x][y]:
            continue
        cv = Cl[ht][x][y]
        for h, dx, dy, w in rev[ht]:
            ux, uy = x - dx, y - dy
            if not (0 <= ux < n and 0 <= uy < n):
                continue
            cu = Cl[h][ux][uy]
            if cu == 0 or cv == 0:
                continue
            nd = d + w * (cu + cv)
            if nd <= cap and nd < D[h][ux][uy]:
                D[h][ux][uy] = nd
                heapq.heappush(heap, (nd, h, ux, uy))
    return np.array(D, np.int64).astype(np.int32)


def _candidates(C, D, h, prim):
    """price + D[v] of primitive `prim` at every state of heading h (int64; UNREACHED where it is not admissible or v is unreached)"""
    dx, dy, ht, w = prim
    Cu = C[h].astype(np.int64)
    Cv = shifted(C[ht], dx, dy, 0).astype(np.int64)
    Dv = shifted(D[ht], dx, dy, UNREACHED)
    ok = (Cu != 0) & (Cv != 0) & (Dv < UNREACHED)
    return np.where(ok, Dv + w * (Cu + Cv), UNREACHED)


def relax(C, table, seeds, max_cost=None):
    """D int32 [H, x, y] by whole-volume relaxation to the fixed point"""
    cap = MAX_COST if max_cost is None else int(max_cost)
    lists = _prims(table)
    D = np.where(seeds, 0, UNREACHED).astype(np.int64)
    for _ in range(D.size + 1):
        changed = False
        for h, lst in enumerate(lists):
            for prim in lst:
                cand = _candidates(C, D, h, prim)
                better = (cand <= cap) & (cand < D[h])
                if better.any():
                    D[h][better] = cand[better]
                    changed = True
        if not changed:
            return D.astype(np.int32)
    raise AssertionError("relax() did not settle")


def _best(C, D, table):
    lists = _prims(table)
    best = np.full(D.shape, UNREACHED, np.int64)
    attain = np.zeros(D.shape, np.int64)
    for h, lst in enumerate(lists):
        for prim in lst:
            np.minimum(best[h], _candidates(C, D, h, prim), out=best[h])
        for prim in lst:
            attain[h] += _candidates(C, D, h, prim) == best[h]
    return best, attain


def bellman_violations(C, table, D, seeds, max_cost=None):
    """the number of states at which D breaks a condition of the field (0: D is the field)"""
    cap = MAX_COST if max_cost is None else int(max_cost)
    D = np.asarray(D).astype(np.int64)
    best, _ = _best(C, D, table)
    finite = D < UNREACHED
    bad = (seeds & (D != 0)) | (~seeds & (D == 0))
    bad |= finite & ~seeds & (D != best)
    bad |= finite & (D > cap)
    bad |= ~finite & (best <= cap)
    bad |= (D < 0) | (D > UNREACHED)
    return int(bad.sum())


def actions(C, table, D, seeds):
    """uint8 [H, x, y]: the first primitive in table order that attains D; GOAL at seeds, NONE where unreached, UNSETTLED without a match"""
    D = np.asarray(D).astype(np.int64)
    out = np.where(D < UNREACHED, UNSETTLED, NONE).astype(np.uint8)
    for h, lst in enumerate(_prims(table)):
        for k in range(len(lst) - 1, -1, -1):
            cand = _candidates(C, D, h, lst[k])
            m = (D[h] < UNREACHED) & (cand == D[h])
            out[h][m] = k
    out[D == 0] = GOAL
    return out


def field(c, footprint, table, goals, max_cost=None):
    """(C, D, action, seeds, info) of one case: info = (reached states, seeded states)"""
    C = volume(c, footprint)
    seeds = seed_mask(C, goals)
    D = relax(C, table, seeds, max_cost)
    return C, D, actions(C, table, D, seeds), seeds, (int((D < UNREACHED).sum()), int(seeds.sum()))


def path_price(path, C, table):
    """the summed prices of a path [(x, y, h), ...]; AssertionError where a step is no admissible primitive of the table"""
    lists = _prims(table)
    total = 0
    for (x, y, h), (vx, vy, vh) in zip(path[:-1], path[1:]):
        ws = [w for dx, dy, ht, w in lists[h] if (x + dx, y + dy, ht) == (vx, vy, vh)]
        assert ws and C[h, x, y] != 0 and C[vh, vx, vy] != 0, ((x, y, h), (vx, vy, vh))
        total += min(ws) * (int(C[h, x, y]) + int(C[vh, vx, vy]))
    return total


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def cost_map(xy, seed, zeros=0.12, high=False):
    """uint16 [x, y]: about `zeros` blocked cells; costs 1 .. 40, or (high) up to 65535 so that the cap of 2^30 cuts the field"""
    rng = np.random.default_rng(7000 + 13 * xy + seed)
    c = rng.integers(1, 41, (xy, xy)).astype(np.uint16)
    if high:
        m = rng.random((xy, xy)) < 0.3
        c[m] = rng.integers(20000, 65536, int(m.sum())).astype(np.uint16)
    c[rng.random((xy, xy)) < zeros] = 0
    return c


def point_footprint(H):
    return np.arange(H + 1, dtype=np.int32), np.zeros((H, 2), np.int16)


def random_table(H, reach, seed, most=64):
    """1 .. `most` random primitives per heading within the limits; the largest |dx| or |dy| of the table is exactly `reach`"""
    rng = np.random.default_rng(300 + 100 * H + 10 * reach + seed)
    start, rows = [0], []
    for h in range(H):
        m = int(rng.integers(1, most + 1))
        got = []
        while len(got) < m:
            dx, dy, ht, w = int(rng.integers(-reach, reach + 1)), int(rng.integers(-reach, reach + 1)), int(rng.integers(0, H)), int(rng.integers(1, 256))
            if (dx, dy, ht) != (0, 0, h):
                got.append((dx, dy, ht, w if rng.random() < 0.8 else int(rng.integers(1, 4))))
        rows += got
        start.append(len(rows))
    rows[0] = (reach, -reach, rows[0][2], rows[0][3]) if (reach, -reach, rows[0][2]) != (0, 0, 0) else rows[0]
    return np.array(start, np.int32), np.array(rows, np.int16)


def steps_table():
    """H = 1: the eight steps of the 2-D solver in CTG_STEPS order, w = 5 straight and 7 diagonal"""
    rows = [(dx, dy, 0, 7 if dx and dy else 5) for dx, dy in CTG_STEPS]
    return np.array([0, 8], np.int32), np.array(rows, np.int16)


def random_goals(xy, H, seed, with_heading, n=3):
    """(n + 2, 3) = (x, y, h): n random goals -- every one with a heading, or every one without (h = -1) --, the first named twice, and
    cell (0, 0), which the caller blocks"""
    rng = np.random.default_rng(900 + seed)
    g = [(int(rng.integers(0, xy)), int(rng.integers(0, xy)), int(rng.integers(0, H)) if with_heading else -1) for k in range(n)]
    return np.array(g + [g[0], (0, 0, 0 if with_heading else -1)], np.int32)


def goals_for_binding(goals, H):
    """the (x, y, h) goals as the Python binding takes them in cells: (G, 2), or (G, 3) with the yaw of heading h"""
    g = np.asarray(goals)
    if (g[:, 2] < 0).all():
        return g[:, :2]
    return np.concatenate([g[:, :2].astype(np.float64), (2.0 * np.pi * g[:, 2:3] / H)], axis=1)


CAR = dict(front=3.6, rear=1.0, half_width=1.1)     # metres
CAR_RES = 0.5


def gap_scene(footprint, xy=40):
    """a wall across the map at x = xy / 2 with one gap a cell wider than the footprint of heading 0 is wide -- and narrower than it is long:
    (c, gap rows y0 .. y1)"""
    start, offs = np.asarray(footprint[0]), np.asarray(footprint[1], np.int64)
    o = offs[start[0]:start[1]]
    wide, long_ = int(o[:, 1].max() - o[:, 1].min() + 1), int(o[:, 0].max() - o[:, 0].min() + 1)
    assert long_ > wide + 1, (long_, wide)
    c = np.full((xy, xy), 3, np.uint16)
    y0 = xy // 2 - (wide + 1) // 2
    c[xy // 2, :] = 0
    c[xy // 2, y0:y0 + wide + 1] = 5
    return c, (y0, y0 + wide + 1)


def _case(name, c, footprint, table, goals, max_cost=None, inner=0, batch=0):
    c = np.array(c, np.uint16)
    c[0, 0] = 0                                     # the goal at (0, 0) seeds nothing
    return dict(name=name, xy=c.shape[0], H=len(table[0]) - 1, c=c, footprint=footprint, table=table, goals=np.asarray(goals, np.int32),
                max_cost=max_cost, inner=inner, batch=batch)


@functools.lru_cache(maxsize=None)
def cases():
    """the GPU test's inputs.  Grid sizes one below, at and one above the tile edge, a ragged last tile (20), a last tile one cell
    wide (17, 33); H = 1, 4, 8, 16 and 64; halos 1, 3 and 4; footprints of 1 cell, 65 cells and a car; random tables of up to 64
    primitives per heading and arc tables with and without reverse; inner bounds 1 and 3, batches of 1 and 5 rounds; a cap."""
    import gvom
    car = gvom.rectangle_footprint(xy_resolution=CAR_RES, headings=16, **CAR)
    arcs = gvom.arc_primitives(16, 3.0, CAR_RES, reach=3)
    arcs_rev = gvom.arc_primitives(16, 3.0, CAR_RES, reach=3, reverse_weight=2.5)
    gap, rows = gap_scene(car)
    mid = (rows[0] + rows[1]) // 2
    out = [
        _case("xy7 H1 point random r1", cost_map(7, 1), point_footprint(1), random_table(1, 1, 1), random_goals(7, 1, 1, False)),
        _case("xy8 H4 point random r3", cost_map(8, 2), point_footprint(4), random_table(4, 3, 2), random_goals(8, 4, 2, True)),
        _case("xy9 H8 point random r4 inner1", cost_map(9, 3), point_footprint(8), random_table(8, 4, 3, most=12), random_goals(9, 8, 3, False), inner=1),
        _case("xy17 H4 point random r4 batch1", cost_map(17, 4), point_footprint(4), random_table(4, 4, 4), random_goals(17, 4, 4, True), batch=1),
        _case("xy20 H16 point arcs inner3 batch5", cost_map(20, 5), point_footprint(16), arcs, random_goals(20, 16, 5, False), inner=3, batch=5),
        _case("xy33 H8 patch65 random r3", cost_map(33, 6, zeros=0.01), rollouts_ref.patch_table(8, 65), random_table(8, 3, 6, most=8), random_goals(33, 8, 6, False)),
        _case("xy40 H16 car arcs+reverse gap", gap, car, arcs_rev, [(28, mid, 0), (28, mid, 0), (0, 0, 0)]),
        _case("xy40 H16 car arcs gap", gap, car, arcs, [(28, mid, 0), (28, mid, 0), (0, 0, 0)]),
        _case("xy40 H16 car arcs random", cost_map(40, 8, zeros=0.01), car, arcs, random_goals(40, 16, 8, False, n=6)),
        _case("xy12 H64 point random r4", cost_map(12, 9), point_footprint(64), random_table(64, 4, 9, most=6), random_goals(12, 64, 9, True)),
        _case("xy20 H8 point random r3 high costs", cost_map(20, 10, high=True), point_footprint(8), random_table(8, 3, 10, most=10), random_goals(20, 8, 10, False)),
        _case("xy20 H8 point random r3 max_cost", cost_map(20, 11), point_footprint(8), random_table(8, 3, 11, most=10), random_goals(20, 8, 11, False), max_cost=4000),
    ]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(i):
    """field() of case i, computed once"""
    q = cases()[i]
    return field(q["c"], q["footprint"], q["table"], q["goals"], q["max_cost"])


def census(C, c, D, table, seeds, goals):
    """what one solved case reaches, as counters"""
    _, attain = _best(C, np.asarray(D).astype(np.int64), table)
    finite = np.asarray(D) < UNREACHED
    some = finite.any(axis=0) & ((C != 0) & ~finite).any(axis=0)
    named = np.zeros(C.shape, bool)
    for x, y, h in np.asarray(goals, np.int64).reshape(-1, 3):
        named[(slice(None) if h < 0 else h), x, y] = True
    return dict(footprint_blocked=int(((C == 0) & (np.asarray(c) != 0)[None]).sum()), some_headings=int(some.sum()),
                dead_goals=int((named & (C == 0)).sum()), ties=int((finite & ~seeds & (attain > 1)).sum()),
                reached=int(finite.sum()), unreached_free=int(((C != 0) & ~finite).sum()))
