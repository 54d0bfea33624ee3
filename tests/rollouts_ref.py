"""The numpy referee of rollout scoring (include/gvom_hip.h "rollout scoring"; gvom_score_rollouts, k_rollouts) and the inputs of
tests/test_rollouts.py and tests/test_rollouts_cpu.py.

score() is the definition, vectorised: centre cell = floor((double)x / res) - o per axis (|x / res| >= 2^30: outside, however far),
heading = rint(float32(yaw) * float32(H / 2 pi)) mod H, a pose invalid where a coordinate is not finite or |yaw * s| < 2^24 fails;
pose cost = 0 where the pose is invalid, a footprint cell lies outside the window or one inside has c == 0, else the maximum of c
under the footprint; per rollout the first blocked pose, its reason (invalid before collision before left-window), the sum in
front of it and the cost-to-go under the last free pose's centre (UNREACHED without one, and where that centre lies outside the
window).  score_loops() says the same a second time as plain Python loops over Python integers; the CPU test holds the two
together on tiny inputs.  Everything is integer but one float32 product and two float64 quotients: tolerance 0.

cases() are the GPU test's synthetic inputs (every one also scored here, once, by expected()); census() counts what they reach."""
import functools
import math

import numpy as np

CLEAR, COLLISION, LEFT_WINDOW, INVALID = 0, 1, 2, 3
UNREACHED = 2 ** 31 - 1
MAX_T = 4096
_OUT = -(1 << 40)                                  # a centre "outside, however far"

SIZES = (16, 33, 64, 100)
RES = {16: 0.4, 33: 0.25, 64: 0.4, 100: 0.1, 1024: 0.2, 4096: 0.4}
ORIGIN_CELLS = {16: (-5, 3), 33: (7, -40), 64: (-100, -31), 100: (12, 9), 1024: (-700, -333), 4096: (-2048, 1000)}
PATTERNS = ("random", "free", "blocked", "one_blocked")
CELLS = (1, 63, 64, 65, 128, 129, 1000)            # footprint cells per heading: each side of the 64-lane and the 256-cell boundaries
HEADINGS = (1, 7, 64)
SHAPES = ((1, 1), (1, 65), (3, 64), (65, 7), (257, 33), (2, 4096))


def heading_scale(H):
    return np.float32(H / (2.0 * np.pi))


def pose_frame(poses, res, origin_cells, H):
    """(cx, cy, heading, valid) of float32 poses [..., 3]; cx, cy int64 (_OUT where the coordinate is outside however far)"""
    p = np.asarray(poses, np.float32)
    x, y, yaw = p[..., 0], p[..., 1], p[..., 2]
    with np.errstate(all="ignore"):
        a = yaw * heading_scale(H)                                       # one float32 multiply
        valid = np.isfinite(x) & np.isfinite(y) & np.isfinite(yaw) & (np.abs(a) < np.float32(2 ** 24))
        h = np.where(valid, np.rint(a), np.float32(0)).astype(np.int64) % H
        cells = []
        for v, o in ((x, origin_cells[0]), (y, origin_cells[1])):
            q = v.astype(np.float64) / float(res)
            near = np.abs(q) < 2.0 ** 30                                 # (False for NaN)
            cells.append(np.where(near, np.floor(np.where(near, q, 0.0)).astype(np.int64) - int(o), _OUT))
    return cells[0], cells[1], h, valid


def score(c, poses, table, res, origin_cells, D=None):
    """c uint16 [x, y]; poses float32 [K, T, 3]; table = (start, offsets); D int32 [x, y] or None -> (summary int32 [K, 4],
    pose_cost uint16 [K, T], pose_status uint8 [K, T])"""
    c = np.asarray(c)
    xy = c.shape[0]
    start, offsets = np.asarray(table[0], np.int64), np.asarray(table[1], np.int64)
    H = len(start) - 1
    poses = np.asarray(poses, np.float32)
    K, T = poses.shape[:2]
    cx, cy, h, valid = pose_frame(poses, res, origin_cells, H)
    cost = np.zeros((K, T), np.uint16)
    status = np.full((K, T), INVALID, np.uint8)
    for hh in np.unique(h[valid]):
        offs = offsets[start[hh]:start[hh + 1]]
        ks, ts = np.nonzero(valid & (h == hh))
        step = max(1, (1 << 22) // len(offs))
        for b in range(0, len(ks), step):
            k, t = ks[b:b + step], ts[b:b + step]
            X = cx[k, t][:, None] + offs[None, :, 0]
            Y = cy[k, t][:, None] + offs[None, :, 1]
            inside = (X >= 0) & (X < xy) & (Y >= 0) & (Y < xy)
            v = np.where(inside, c[np.clip(X, 0, xy - 1), np.clip(Y, 0, xy - 1)], 0).astype(np.int64)
            zero = (inside & (v == 0)).any(axis=1)
            out = (~inside).any(axis=1)
            st = np.where(zero, COLLISION, np.where(out, LEFT_WINDOW, CLEAR))
            status[k, t] = st
            cost[k, t] = np.where(st == CLEAR, v.max(axis=1), 0)
    summary = np.zeros((K, 4), np.int32)
    blocked = cost == 0
    first = np.where(blocked.any(axis=1), blocked.argmax(axis=1), T)
    summary[:, 1] = first
    rows = np.arange(K)
    summary[:, 0] = np.where(first < T, status[rows, np.minimum(first, T - 1)], CLEAR)
    csum = np.concatenate([np.zeros((K, 1), np.int64), np.cumsum(cost.astype(np.int64), axis=1)], axis=1)
    summary[:, 2] = csum[rows, first]
    term = np.full(K, UNREACHED, np.int64)
    if D is not None:
        last = np.maximum(first - 1, 0)
        lx, ly = cx[rows, last], cy[rows, last]
        ok = (first > 0) & (lx >= 0) & (lx < xy) & (ly >= 0) & (ly < xy)
        term[ok] = np.asarray(D)[lx[ok], ly[ok]]
    summary[:, 3] = term
    return summary, cost, status


def score_loops(c, poses, table, res, origin_cells, D=None):
    """the same, pose by pose and cell by cell over Python numbers (tiny inputs only)"""
    xy = len(c)
    start, offsets = [int(v) for v in table[0]], [(int(a), int(b)) for a, b in table[1]]
    H = len(start) - 1
    s = np.float32(H / (2.0 * math.pi))
    K, T = len(poses), len(poses[0])
    summary, costs = [], []
    for k in range(K):
        row, reason, centres = [], [], []
        for t in range(T):
            x, y, yaw = (np.float32(v) for v in poses[k][t])
            with np.errstate(all="ignore"):
                a = np.float32(yaw * s)
            centre = []
            for v, o in ((x, origin_cells[0]), (y, origin_cells[1])):
                q = float(v) / float(res) if math.isfinite(float(v)) else float("nan")
                centre.append(None if not abs(q) < 2.0 ** 30 else math.floor(q) - int(o))
            centres.append(centre)
            if not (math.isfinite(float(x)) and math.isfinite(float(y)) and math.isfinite(float(yaw)) and abs(float(a)) < 2.0 ** 24):
                row.append(0)
                reason.append(INVALID)
                continue
            r = float(a)
            n = math.floor(r)
            if r - n > 0.5 or (r - n == 0.5 and n % 2 == 1):               # round half to even
                n += 1
            h = n % H
            worst, any_zero, any_out = 0, False, False
            for dx, dy in offsets[start[h]:start[h + 1]]:
                if centre[0] is None or centre[1] is None or not (0 <= centre[0] + dx < xy and 0 <= centre[1] + dy < xy):
                    any_out = True
                    continue
                v = int(c[centre[0] + dx][centre[1] + dy])
                any_zero = any_zero or v == 0
                worst = max(worst, v)
            blocked = any_zero or any_out
            row.append(0 if blocked else worst)
            reason.append(COLLISION if any_zero else (LEFT_WINDOW if any_out else CLEAR))
        first = next((t for t in range(T) if row[t] == 0), T)
        terminal = UNREACHED
        if D is not None and first > 0:
            lx, ly = centres[first - 1]
            if lx is not None and ly is not None and 0 <= lx < xy and 0 <= ly < xy:
                terminal = int(D[lx][ly])
        summary.append([reason[first] if first < T else CLEAR, first, sum(row[:first]), terminal])
        costs.append(row)
    return np.array(summary, np.int32), np.array(costs, np.uint16)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def cost_map(xy, pattern, seed=0, zeros=0.1):
    """uint16 [x, y]: random = about `zeros` blocked cells and values up to 65535 (a third of them >= 32768, some exactly 65535)"""
    rng = np.random.default_rng(1000 + 7 * xy + seed)
    if pattern == "free":
        return np.full((xy, xy), 7, np.uint16)
    if pattern == "blocked":
        return np.zeros((xy, xy), np.uint16)
    if pattern == "one_blocked":
        c = np.full((xy, xy), 3, np.uint16)
        c[xy // 2, xy // 3] = 0
        return c
    c = rng.integers(1, 200, (xy, xy)).astype(np.uint16)
    high = rng.random((xy, xy))
    c[high < 0.3] = rng.integers(32768, 65536, int((high < 0.3).sum())).astype(np.uint16)
    c[high < 0.02] = 65535
    c[rng.random((xy, xy)) < zeros] = 0
    return c


def field_of(c):
    """an int32 [x, y] field to gather terminals from: different along x and y, UNREACHED on blocked cells and on a stripe"""
    xy = c.shape[0]
    x, y = np.meshgrid(np.arange(xy, dtype=np.int64), np.arange(xy, dtype=np.int64), indexing="ij")
    D = (x * 7919 + y * 104729) % 1000003
    D[(c == 0) | ((x + 2 * y) % 11 == 0)] = UNREACHED
    return D.astype(np.int32)


def patch_table(H, M, seed=0):
    """a synthetic footprint table: per heading M distinct offsets out of a compact patch whose place depends on the heading"""
    rng = np.random.default_rng(50 + 1000 * H + M + seed)
    side = int(math.ceil(math.sqrt(M))) + 1
    start, offs = [0], []
    for h in range(H):
        pick = np.sort(rng.choice(side * side, M, replace=False))
        ox, oy = -side // 2 + (h % 3) - 1, -side // 2 - (h % 2)
        offs.append(np.stack([pick % side + ox, pick // side + oy], axis=1))
        start.append(start[-1] + M)
    return np.array(start, np.int32), np.concatenate(offs).astype(np.int16)


def asymmetric_table(H=7):
    """cells only at +x, dx and dy extents different, every heading another shape: a swapped axis, a sign error or a wrong heading shows"""
    start, offs = [0], []
    for h in range(H):
        cells = [(dx, dy) for dx in range(1, 4 + h) for dy in range(-1, 1 + (h % 2))]
        offs.append(np.array(cells))
        start.append(start[-1] + len(cells))
    return np.array(start, np.int32), np.concatenate(offs).astype(np.int16)


def _tie_yaw(H, target):
    """a float32 yaw whose float32 product with the heading scale is exactly `target` (None where there is none nearby)"""
    s = heading_scale(H)
    y = np.float32(target / float(s))
    lo = hi = y
    for _ in range(16):
        for cand in (lo, hi):
            if np.float32(cand * s) == np.float32(target):
                return cand
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
    return None


def special_poses(xy, res, origin_cells, H):
    """poses [n, 3] that sit on what the census asks for, all float32: cell borders, negative coordinates, the four sides, rounding
    ties of the heading, the wrap to heading 0, and the invalid ones"""
    ox, oy = origin_cells
    mid = xy // 2
    cell = lambda i, j, yaw=0.0: (np.float32((ox + i + 0.5) * res), np.float32((oy + j + 0.5) * res), np.float32(yaw))
    out = [cell(mid, mid)]
    out += [(np.float32((ox + i) * res), np.float32((oy + j) * res), np.float32(0.3)) for i, j in ((mid, mid), (1, 2), (xy - 1, 0), (0, xy - 1))]   # borders
    out += [cell(0, mid), cell(xy - 1, mid), cell(mid, 0), cell(mid, xy - 1), cell(-1, mid), cell(mid, xy)]              # the four sides
    for target in (0.5, 1.5, 2.5, -0.5):
        y = _tie_yaw(H, target)
        if y is not None:
            out.append(cell(mid, mid, y))
    two_pi = np.float32(2.0 * np.pi)
    out += [cell(mid, mid, np.float32(np.pi)), cell(mid, mid, np.float32(-np.pi)), cell(mid, mid, np.nextafter(two_pi, np.float32(0)))]
    out += [(np.float32(np.nan), out[0][1], np.float32(0)), (out[0][0], np.float32(np.inf), np.float32(0)), (out[0][0], np.float32(-np.inf), np.float32(1)),
            (out[0][0], out[0][1], np.float32(np.nan)), (out[0][0], out[0][1], np.float32(3.0e9)), (np.float32(3.0e38), out[0][1], np.float32(0.1)),
            (np.float32(-1.0e12), out[0][1], np.float32(0.1))]
    return np.array(out, np.float32)


def arc_poses(K, T, xy, res, origin_cells, seed, spread=1.0, centre=None):
    """K arcs of T poses, about a cell apart, from random starts in (and a little around) the window: float32 [K, T, 3]"""
    rng = np.random.default_rng(seed)
    ox, oy = origin_cells
    if centre is None:
        x0 = (ox + rng.uniform(-0.05 * xy, 1.05 * xy, K)) * res
        y0 = (oy + rng.uniform(-0.05 * xy, 1.05 * xy, K)) * res
    else:
        x0 = (ox + centre[0] + rng.uniform(-spread, spread, K)) * res
        y0 = (oy + centre[1] + rng.uniform(-spread, spread, K)) * res
    th0 = rng.uniform(-2 * np.pi, 4 * np.pi, K)
    curv = rng.uniform(-0.15, 0.15, K)
    step = rng.uniform(0.3, 1.4, K) * res
    t = np.arange(T)
    th = th0[:, None] + curv[:, None] * t[None, :]
    x = x0[:, None] + np.cumsum(step[:, None] * np.cos(th), axis=1)
    y = y0[:, None] + np.cumsum(step[:, None] * np.sin(th), axis=1)
    return np.stack([x, y, th], axis=2).astype(np.float32)


def make_poses(K, T, xy, res, origin_cells, H, seed):
    """arcs with the special poses written over the ends (and, where there is room, the middles) of some rollouts; rollout 0 stays
    at the map's centre where a small footprint is clear"""
    p = arc_poses(K, T, xy, res, origin_cells, seed)
    sp = special_poses(xy, res, origin_cells, H)
    mid = xy // 2
    p[0, :, 0], p[0, :, 1] = np.float32((origin_cells[0] + mid + 0.5) * res), np.float32((origin_cells[1] + mid + 0.5) * res)
    rng = np.random.default_rng(seed + 1)
    n = 0
    for k in range(1, K):                                                # the last pose of rollout k, then its first, then one in between
        for t in ((T - 1, 0, T // 2) if T > 2 else (T - 1,)):
            if n < len(sp) and rng.random() < 0.6:
                p[k, t] = sp[n]
                n += 1
    if K == 1 and T > 1:                                                 # one rollout: a special pose in its second half
        p[0, T - 1] = sp[(seed * 5) % len(sp)]
    if K == 1 and T == 1:
        p[0, 0] = sp[(seed * 3) % len(sp)]
    return p


@functools.lru_cache(maxsize=None)
def cases(shape):
    """the synthetic inputs of one (K, T): a tuple of dicts {name, xy, res, origin_cells, origin, c, D, table, poses, device}"""
    K, T = shape
    i = SHAPES.index(shape)
    out = []
    for j, M in enumerate(CELLS):
        xy = SIZES[(i + j) % 4] if M < 1000 else (64, 100)[i % 2]
        pattern = ("random", "random", "free", "one_blocked", "random", "blocked", "random")[(i + 2 * j) % 7]
        H = HEADINGS[(i + j) % 3]
        table = patch_table(H, M, seed=i)
        out.append(_case("%dx%d M%d H%d xy%d %s" % (K, T, M, H, xy, pattern), xy, pattern, table, K, T, seed=100 * i + j,
                         with_field=(i + j) % 2 == 0, device=(i + j) % 3 == 0))
    for j, xy in enumerate(SIZES):
        if (i + j) % 2 == 0:
            out.append(_case("%dx%d asymmetric xy%d" % (K, T, xy), xy, ("free", "one_blocked", "random")[(i + j) % 3], asymmetric_table(7), K, T,
                             seed=900 + 10 * i + j, with_field=True, device=j % 2 == 1))
    return tuple(out)


def _case(name, xy, pattern, table, K, T, seed, with_field, device, zeros=0.1, poses=None):
    res, oc = RES[xy], ORIGIN_CELLS[xy]
    c = cost_map(xy, pattern, seed, zeros)
    H = len(table[0]) - 1
    return dict(name=name, xy=xy, res=res, origin_cells=oc, origin=(oc[0] * res, oc[1] * res), c=c, D=field_of(c) if with_field else None,
                table=table, poses=make_poses(K, T, xy, res, oc, H, seed) if poses is None else poses, device=device)


def all_cases():
    return [case for shape in SHAPES for case in cases(shape)]


@functools.lru_cache(maxsize=None)
def expected(shape):
    """score() of every case of cases(shape), computed once"""
    return tuple(score(q["c"], q["poses"], q["table"], q["res"], q["origin_cells"], q["D"]) for q in cases(shape))


CAR = dict(front=3.6, rear=1.0, half_width=1.1)     # metres: at 0.2 m cells about 325 cells per heading


@functools.lru_cache(maxsize=None)
def large_case(xy, footprint):
    """xy 1024: K = 1024 rollouts of T = 64 poses spread over the map with a car footprint (the caller's rectangle_footprint table:
    `footprint` = (start bytes, offsets bytes, H) so that the cache can hold it), at a negative origin; xy 4096: K = 64, T = 16
    near the far corner.  One blocked cell in a thousand: most poses of a 325-cell footprint are clear."""
    start = np.frombuffer(footprint[0], np.int32)
    table = (start, np.frombuffer(footprint[1], np.int16).reshape(-1, 2))
    res, oc = RES[xy], ORIGIN_CELLS[xy]
    if xy == 1024:
        K, T = 1024, 64
        poses = arc_poses(K, T, xy, res, oc, 4242)
    else:
        K, T = 64, 16
        poses = arc_poses(K, T, xy, res, oc, 4343, spread=40.0, centre=(xy - 30, xy - 25))
    q = _case("large xy%d" % xy, xy, "random", table, K, T, seed=5, with_field=True, device=True, zeros=0.001, poses=poses)
    return q, score(q["c"], q["poses"], q["table"], q["res"], q["origin_cells"], q["D"])


def census(inputs):
    """what a list of (case, (summary, pose_cost, pose_status)) reaches, as counters"""
    n = dict(clear=0, collision=0, left_window=0, invalid=0, first_0=0, first_last=0, first_T=0, clear_after_blocked=0, high_cost=0, cost_65535=0,
             terminal_finite=0, terminal_unreached_with_field=0, on_border=0, negative=0, west=0, east=0, south=0, north=0,
             ties=set(), wrap_to_0=0, pi=0, nan=0, inf=0, yaw_bound=0, far=0)
    for q, (summary, cost, status) in inputs:
        K, T = cost.shape
        for name, code in (("clear", CLEAR), ("collision", COLLISION), ("left_window", LEFT_WINDOW), ("invalid", INVALID)):
            n[name] += int((summary[:, 0] == code).sum())
        first = summary[:, 1]
        n["first_0"] += int((first == 0).sum())
        n["first_last"] += int((first == T - 1).sum())
        n["first_T"] += int((first == T).sum())
        later_clear = np.array([(cost[k, first[k] + 1:] > 0).any() if first[k] < T else False for k in range(K)])
        n["clear_after_blocked"] += int(later_clear.sum())
        n["high_cost"] += int((cost >= 32768).sum())
        n["cost_65535"] += int((cost == 65535).sum())
        if q["D"] is not None:
            n["terminal_finite"] += int((summary[:, 3] != UNREACHED).sum())
            n["terminal_unreached_with_field"] += int((summary[:, 3] == UNREACHED).sum())
        p, xy, res = q["poses"], q["xy"], q["res"]
        start, offsets = q["table"]
        H = len(start) - 1
        cx, cy, h, valid = pose_frame(p, res, q["origin_cells"], H)
        with np.errstate(all="ignore"):
            qx, qy = p[..., 0].astype(np.float64) / res, p[..., 1].astype(np.float64) / res
            a = p[..., 2] * heading_scale(H)
            n["on_border"] += int((valid & ((qx == np.floor(qx)) | (qy == np.floor(qy)))).sum())
            n["negative"] += int((valid & ((p[..., 0] < 0) | (p[..., 1] < 0))).sum())
            frac = a - np.floor(a)
            for target in (0.5, 1.5, 2.5, -0.5):
                if (valid & (a == np.float32(target))).any():
                    n["ties"].add(target)
            n["wrap_to_0"] += int((valid & (np.rint(a) == H) & (frac != 0)).sum())
            n["pi"] += int((np.abs(p[..., 2]) == np.float32(np.pi)).sum())
            n["nan"] += int(np.isnan(p).any(axis=-1).sum())
            n["inf"] += int(np.isinf(p).any(axis=-1).sum())
            n["yaw_bound"] += int((np.isfinite(p).all(axis=-1) & ~(np.abs(a) < np.float32(2 ** 24))).sum())
            n["far"] += int((np.isfinite(p).all(axis=-1) & ((np.abs(qx) >= 2.0 ** 30) | (np.abs(qy) >= 2.0 ** 30))).sum())
        # footprints partly outside: some cell of the pose's footprint inside the window and some beyond the given side
        lo = np.array([offsets[start[k]:start[k + 1]].min(axis=0) for k in range(H)], np.int64)
        hi = np.array([offsets[start[k]:start[k + 1]].max(axis=0) for k in range(H)], np.int64)
        inside = valid & (cx >= 0) & (cx < xy) & (cy >= 0) & (cy < xy)
        n["west"] += int((inside & (cx + lo[h, 0] < 0)).sum())
        n["east"] += int((inside & (cx + hi[h, 0] >= xy)).sum())
        n["south"] += int((inside & (cy + lo[h, 1] < 0)).sum())
        n["north"] += int((inside & (cy + hi[h, 1] >= xy)).sum())
    return n
