"""Referee of frontier extraction (gvom_frontiers; include/gvom_hip.h "frontier extraction"), numpy and scipy on the host.  Arrays in
here are in DEVICE ORDER, A[y, x] with cell (x, y) at linear index y * xy + x; the binding takes and returns [x, y] arrays, which are
their transposes (`.T`).  Two independent forms of the product: product() labels with scipy.ndimage.label under the 3 x 3 structure
and reduces with numpy, product_loops() runs a plain union-find and plain loops.  tiled() simulates the round schedule of the GPU
labelling on the CPU (32 x 32 tiles, a one-cell halo read as it was at the start of the round) and yields round counts.  The frontier
predicate is the definition's, written down here a second time, not the kernel's."""
import functools

import numpy as np
from scipy import ndimage

UNREACHED = 2 ** 31 - 1
NONE, SMALL = -1, -2
TILE = 32
# one partial tile; each side of the tile edges 32 and 64; exactly 2 x 2 tiles; ragged rims; a last tile one cell wide (the reasoning
# of costfield_ref.SIZES; 50 adds no path of its own here)
SIZES = (16, 31, 32, 33, 64, 65, 100, 129)


def frontier_mask(c, vis, D=None):
    """the FRONTIER CELLS: drivable, known, beside an unknown cell INSIDE the window, and reachable where D is given"""
    c, vis = np.asarray(c), np.asarray(vis)
    unknown = vis == 0
    beside = np.zeros(vis.shape, bool)
    beside[:, 1:] |= unknown[:, :-1]
    beside[:, :-1] |= unknown[:, 1:]
    beside[1:, :] |= unknown[:-1, :]
    beside[:-1, :] |= unknown[1:, :]
    m = (c > 0) & (vis > 0) & beside
    if D is not None:
        m &= np.asarray(D).astype(np.int64) < UNREACHED
    return m


def labels_scipy(mask):
    """int64 [y, x]: the least linear index of the cell's 8-connected component, -1 outside the mask"""
    comp, n = ndimage.label(mask, structure=np.ones((3, 3), int))
    out = np.full(mask.shape, -1, np.int64)
    if n:
        idx = np.arange(mask.size, dtype=np.int64).reshape(mask.shape)
        least = np.asarray(ndimage.minimum(idx, comp, index=np.arange(1, n + 1))).astype(np.int64)
        out[mask] = least[comp[mask] - 1]
    return out


def labels_union_find(mask):
    """the same from a plain union-find over the four backward neighbours of every cell, in pure Python"""
    h, w = mask.shape
    m = mask.tolist()
    parent = {}

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for y in range(h):
        for x in range(w):
            if not m[y][x]:
                continue
            u = y * w + x
            parent[u] = u
            for dx, dy in ((-1, 0), (-1, -1), (0, -1), (1, -1)):
                vx, vy = x + dx, y + dy
                if 0 <= vx < w and 0 <= vy < h and m[vy][vx]:
                    a, b = find(u), find(vy * w + vx)
                    if a != b:
                        parent[max(a, b)] = min(a, b)              # the root is the least index
    out = np.full(mask.shape, -1, np.int64)
    for u in parent:
        out[u // w, u % w] = find(u)
    return out


def product(c, vis, D, min_cells, cap, labels=labels_scipy):
    """(clusters int32 [cap, 8], sums int64 [cap, 2], cluster map int32 [y, x], counts int32 [4], info [4] without the rounds)"""
    mask = frontier_mask(c, vis, D)
    xy = mask.shape[0]
    lab = labels(mask)
    roots, sizes = np.unique(lab[mask], return_counts=True)
    kept = sizes >= min_cells
    rank_of_root = np.where(kept, np.cumsum(kept) - 1, SMALL)
    cmap = np.full(mask.shape, NONE, np.int32)
    ranks = rank_of_root[np.searchsorted(roots, lab[mask])]
    cmap[mask] = ranks
    n_kept = int(kept.sum())
    rows, sums = np.zeros((cap, 8), np.int64), np.zeros((cap, 2), np.int64)
    ys, xs = np.nonzero(mask)
    take = (ranks >= 0) & (ranks < cap)
    r, x, y = ranks[take], xs[take], ys[take]
    n = min(n_kept, cap)
    if n:
        idx = (y * xy + x).astype(np.uint64)
        d = (np.asarray(D)[y, x].astype(np.uint32) if D is not None else np.full(len(r), UNREACHED, np.uint32)).astype(np.uint64)
        key = np.full(n, 2 ** 64 - 1, np.uint64)
        np.minimum.at(key, r, (d << np.uint64(32)) | idx)
        lo, hi = np.full((n, 2), 2 ** 31 - 1, np.int64), np.full((n, 2), -1, np.int64)
        np.minimum.at(lo[:, 0], r, x); np.minimum.at(lo[:, 1], r, y); np.maximum.at(hi[:, 0], r, x); np.maximum.at(hi[:, 1], r, y)
        rows[:n, 0] = roots[kept][:n]
        rows[:n, 1] = np.bincount(r, minlength=n)
        rows[:n, 2:4], rows[:n, 4:6] = lo, hi
        rows[:n, 6] = (key & np.uint64(0xffffffff)).astype(np.int64)
        rows[:n, 7] = (key >> np.uint64(32)).astype(np.uint32).view(np.int32) if n else 0
        sums[:n, 0], sums[:n, 1] = np.bincount(r, weights=x, minlength=n), np.bincount(r, weights=y, minlength=n)
    counts = np.array([n_kept, int(mask.sum()), int((ranks >= 0).sum()), cap], np.int32)
    return rows.astype(np.int32), sums, cmap, counts, [n_kept, int(mask.sum()), int((~kept).sum())]


def product_loops(c, vis, D, min_cells, cap):
    """product() again: union-find labels, and every statistic from plain Python loops over the cells"""
    mask = frontier_mask(c, vis, D)
    xy = mask.shape[0]
    lab = labels_union_find(mask).tolist()
    members = {}
    for y in range(xy):
        for x in range(xy):
            if lab[y][x] >= 0:
                members.setdefault(lab[y][x], []).append((x, y))
    kept = [root for root in sorted(members) if len(members[root]) >= min_cells]
    rank = {root: k for k, root in enumerate(kept)}
    cmap = np.full((xy, xy), NONE, np.int32)
    rows, sums = np.zeros((cap, 8), np.int32), np.zeros((cap, 2), np.int64)
    in_kept = 0
    for root, cells in members.items():
        r = rank.get(root, SMALL)
        for x, y in cells:
            cmap[y, x] = r
        if r < 0:
            continue
        in_kept += len(cells)
        if r >= cap:
            continue
        best = min((((int(D[y][x]) & 0xffffffff) if D is not None else UNREACHED) << 32) | (y * xy + x) for x, y in cells)
        bd = best >> 32
        rows[r] = (root, len(cells), min(x for x, _ in cells), min(y for _, y in cells), max(x for x, _ in cells), max(y for _, y in cells),
                   best & 0xffffffff, bd - 2 ** 32 if bd >= 2 ** 31 else bd)
        sums[r] = (sum(x for x, _ in cells), sum(y for _, y in cells))
    n_front = sum(len(v) for v in members.values())
    counts = np.array([len(kept), n_front, in_kept, cap], np.int32)
    return rows, sums, cmap, counts, [len(kept), n_front, len(members) - len(kept)]


def tiled(mask):
    """(labels as labels_scipy gives them, rounds, tile relaxations) of the GPU's round schedule, simulated: every flagged 32 x 32
    tile takes its one-cell halo as it was at the START of the round, lowers its own labels to the local fixed point, and flags
    the neighbours whose halo holds a rim cell that went down; the first round that flags no tile is the last.  A tile's local
    fixed point gives each of its 8-connected pieces the least of its own labels and of the halo labels that touch it."""
    xy = mask.shape[0]
    nt = (xy + TILE - 1) // TILE
    BIG = np.int64(2 ** 62)
    L = np.where(mask, np.arange(mask.size, dtype=np.int64).reshape(mask.shape), BIG)
    flags = {(ty, tx) for ty in range(nt) for tx in range(nt) if mask[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE].any()}
    rounds = relaxed = 0
    eight = np.ones((3, 3), int)
    while True:
        rounds += 1
        old = np.full((xy + 2, xy + 2), BIG)
        old[1:-1, 1:-1] = L
        nxt = set()
        for ty, tx in sorted(flags):
            relaxed += 1
            y0, x0 = ty * TILE, tx * TILE
            y1, x1 = min(y0 + TILE, xy), min(x0 + TILE, xy)
            win = old[y0:y1 + 2, x0:x1 + 2].copy()                 # the tile with its halo
            inner = win[1:-1, 1:-1]
            comp, n = ndimage.label(inner < BIG, structure=eight)
            if not n:
                continue
            least = np.asarray(ndimage.minimum(inner, comp, index=np.arange(1, n + 1))).astype(np.int64).reshape(-1)
            padded = np.zeros(win.shape, np.int64)
            padded[1:-1, 1:-1] = comp
            halo = np.ones(win.shape, bool)
            halo[1:-1, 1:-1] = False
            for hy, hx in np.argwhere(halo & (win < BIG)):
                for k in np.unique(padded[max(hy - 1, 0):hy + 2, max(hx - 1, 0):hx + 2]):
                    if k:
                        least[k - 1] = min(least[k - 1], win[hy, hx])
            new = np.where(comp > 0, least[np.maximum(comp, 1) - 1], BIG)
            down = new < inner
            L[y0:y1, x0:x1] = new
            h, w = down.shape
            for dy, dx, part in ((-1, 0, down[0, :]), (1, 0, down[TILE - 1:TILE, :]), (0, -1, down[:, 0]), (0, 1, down[:, TILE - 1:TILE]),
                                 (-1, -1, down[0, 0]), (-1, 1, down[0, TILE - 1:TILE]), (1, -1, down[TILE - 1:TILE, 0]),
                                 (1, 1, down[TILE - 1:TILE, TILE - 1:TILE])):
                if np.any(part) and 0 <= ty + dy < nt and 0 <= tx + dx < nt:
                    nxt.add((ty + dy, tx + dx))
        if not nxt:
            break
        flags = nxt
    return np.where(mask, L, -1), rounds, relaxed


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def _from_cells(xy, cells):
    """the maps whose frontier cells are exactly `cells` (a one-cell-wide set): they are known, everything else is not"""
    vis = np.zeros((xy, xy), np.int32)
    for x, y in cells:
        vis[y, x] = 3
    return vis


def snake(xy, pitch=2):
    """a path one cell wide, row after row `pitch` rows apart, joined at alternating ends: it starts at cell (0, 0), its least index"""
    cells = []
    rows = list(range(0, xy, pitch))
    for k, y in enumerate(rows):
        xs = range(xy) if k % 2 == 0 else range(xy - 1, -1, -1)
        cells += [(x, y) for x in xs]
        if k + 1 < len(rows):
            cells += [(xy - 1 if k % 2 == 0 else 0, yy) for yy in range(y + 1, rows[k + 1])]
    return cells


def spiral(xy):
    """a square spiral one cell wide, arms two cells apart, from the bottom left corner inwards: along the bottom, up the right side,
    back along the top and down the left.  Its least index, cell (0, 0), lies inside the path, far from both ends"""
    cells, pos = [(0, xy - 1)], [0, xy - 1]

    def go(tx, ty):
        while (pos[0], pos[1]) != (tx, ty):
            pos[0] += (tx > pos[0]) - (tx < pos[0])
            pos[1] += (ty > pos[1]) - (ty < pos[1])
            cells.append((pos[0], pos[1]))
    lo, hi = 0, xy - 1
    while True:                                                    # at (lo, hi), the bottom left corner of the square lo .. hi
        go(hi, hi), go(hi, lo), go(lo, lo)
        if hi - lo < 4:
            return cells
        go(lo, hi - 2), go(lo + 2, hi - 2)                         # down the left side, and in to the next square
        lo, hi = lo + 2, hi - 2


def default_D(xy):
    """a cost to go with many ties and no symmetry: the best cell of a cluster is rarely its label"""
    y, x = np.mgrid[0:xy, 0:xy]
    return ((x * 7 + y * 13) % 50 + (xy - 1 - x) // 3 + 1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def patterns(xy):
    """{name: (c uint16, vis int32, D int32 or None, min_cells, cap)} in device order"""
    rng = np.random.default_rng(1000 + xy)
    ones = np.ones((xy, xy), np.uint16)
    y, x = np.mgrid[0:xy, 0:xy]
    D = default_D(xy)
    out = {}
    out["nothing_known"] = (ones, np.zeros((xy, xy), np.int32), D, 1, 8)
    out["all_known"] = (ones, np.full((xy, xy), 2, np.int32), D, 1, 8)
    out["corners"] = (ones, _from_cells(xy, [(0, 0), (xy - 1, 0), (0, xy - 1), (xy - 1, xy - 1)]), D, 1, 8)
    disc = ((x - xy // 2) ** 2 + (y - xy // 2) ** 2 <= (0.37 * xy) ** 2).astype(np.int32)
    out["disc"] = (ones, disc, D, 1, 8)
    out["serpentine"] = (ones, _from_cells(xy, snake(xy)), D, 1, 4)
    out["spiral"] = (ones, _from_cells(xy, spiral(xy)), D, 1, 4)
    a, b, bottom = 2, xy - 4, xy - 2
    out["u_shape"] = (ones, _from_cells(xy, [(a, yy) for yy in range(1, bottom + 1)] + [(b, yy) for yy in range(1, bottom + 1)] +
                                        [(xx, bottom) for xx in range(a, b + 1)]), D, 1, 4)
    # two arcs that touch only diagonally, and a third close by that touches neither
    cells = [(xx, 5) for xx in range(2, 8)] + [(xx, 6) for xx in range(8, 13)] + [(xx, 9) for xx in range(2, 13)]
    if xy >= 48:                                                   # ... across the corner of four tiles: (31, 31) and (32, 32)
        cells += [(xx, 31) for xx in range(20, 32)] + [(xx, 32) for xx in range(32, 45)]
    if xy >= 80:                                                   # ... and the other diagonal of a tile corner: (64, 63) and (63, 64)
        cells += [(xx, 63) for xx in range(64, 72)] + [(xx, 64) for xx in range(55, 64)]
    out["diagonal_pairs"] = (ones, _from_cells(xy, cells), D, 2, 8)
    # a ring cut into pieces by blocked cells and by unreached cells
    c = ones.copy()
    Dc = D.copy()
    c[:, xy // 2 - 1:xy // 2 + 1] = 0
    Dc[xy // 2 - 1:xy // 2 + 1, :] = UNREACHED
    c[(x + y) % 11 == 0] = 0
    out["cut_ring"] = (c, disc, Dc, 2, 64)
    # thousands of one-cell clusters
    vis_r = (rng.random((xy, xy)) < 0.5).astype(np.int32) * rng.integers(1, 9, (xy, xy)).astype(np.int32)
    c_r = np.where(rng.random((xy, xy)) < 0.1, 0, rng.integers(1, 65536, (xy, xy))).astype(np.uint16)
    D_r = np.where(rng.random((xy, xy)) < 0.1, UNREACHED, rng.integers(0, 40, (xy, xy))).astype(np.int32)
    big = xy * xy
    for mc, cap in ((1, 1), (1, 7), (1, big), (2, 7), (2, big), (5, 1), (5, big)):
        out["random_m%d_c%s" % (mc, "big" if cap == big else cap)] = (c_r, vis_r, D_r, mc, cap)
    out["tie"] = (ones, disc, np.full((xy, xy), 77, np.int32), 1, 8)
    out["no_D_disc"] = (ones, disc, None, 1, 8)
    out["no_D_random"] = (c_r, vis_r, None, 3, 16)
    return out


@functools.lru_cache(maxsize=None)
def expected(xy, name):
    c, vis, D, mc, cap = patterns(xy)[name]
    return product(c, vis, D, mc, cap)


@functools.lru_cache(maxsize=None)
def large_case(xy=1024):
    """25 % unknown at random plus one snake, 16 rows apart, across all 32 x 32 tiles"""
    rng = np.random.default_rng(77)
    vis = (rng.random((xy, xy)) >= 0.25).astype(np.int32)
    band = np.zeros((xy, xy), bool)
    for x, y in snake(xy, 16):
        band[max(y - 2, 0):y + 3, max(x - 2, 0):x + 3] = True
    vis[band] = 0
    for x, y in snake(xy, 16):
        vis[y, x] = 1
    c = np.where(rng.random((xy, xy)) < 0.05, 0, 7).astype(np.uint16)
    for x, y in snake(xy, 16):
        c[y, x] = 9
    D = rng.integers(0, 1 << 20, (xy, xy)).astype(np.int32)
    return (c, vis, D, 3, 64), product(c, vis, D, 3, 64)


def census(xy, name):
    """what a case holds, from the referee alone"""
    c, vis, D, mc, cap = patterns(xy)[name]
    rows, sums, cmap, counts, info = expected(xy, name)
    mask = frontier_mask(c, vis, D)
    n = min(int(counts[0]), cap)
    tie = 0
    for r in range(n):
        if D is not None:
            member = cmap == r
            tie += int((np.asarray(D)[member] == rows[r, 7]).sum() > 1)
    return dict(frontier=int(mask.sum()), kept=int(counts[0]), dropped=info[2], rows=n, beyond_cap=max(int(counts[0]) - cap, 0),
                largest=int(rows[:n, 1].max()) if n else 0, best_ties=tie, best_is_not_label=int((rows[:n, 6] != rows[:n, 0]).sum()),
                blocked_beside_unknown=int(((np.asarray(c) == 0) & (np.asarray(vis) > 0)).sum()),
                unreached=0 if D is None else int((np.asarray(D) == UNREACHED).sum()))
