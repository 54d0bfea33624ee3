"""The numpy referee of terrain attitude scoring (include/gvom_hip.h "terrain attitude scoring"; gvom_score_attitude, k_attitude) and
the inputs of tests/test_attitude.py and tests/test_attitude_cpu.py.

score() is the definition, vectorised, every float64 operation one numpy operation in the header's order: the pose frame is
rollout scoring's (tests/rollouts_ref.py pose_frame), fx = q - floor(q); the four wheels stand at floor(((double)x + wx) / res) - o;
pitch and roll tangents from the four heights, the belly the least of (plane + belly_height) - g over the footprint's known cells
inside the window; the status the first of INVALID, LEFT_WINDOW, UNKNOWN_GROUND, PITCH, ROLL, BELLY, OK, decided on the float32
values that are stored; per rollout the first bad pose and the three arg-extremes in front of it.  score_loops() says the same a
second time as plain Python loops over Python numbers; the CPU test holds the two together on tiny inputs.  Tolerance 0.

cases() are the GPU test's synthetic inputs (every one also scored here, once, by expected()); census() counts what they reach."""
import collections
import functools
import math

import numpy as np

import rollouts_ref as rr

OK, PITCH, ROLL, BELLY, UNKNOWN_GROUND, LEFT_WINDOW, INVALID = range(7)
_OUT = -(1 << 40)

CELLS = (1, 63, 64, 65, 256, 257, 1000)            # footprint cells per heading: each side of the 64-lane and the 256-cell boundaries
HEADINGS = rr.HEADINGS
SHAPES = rr.SHAPES
SIZES = rr.SIZES
GROUNDS = ("flat", "plane", "steps", "random", "unknown")

# front_axle, rear_axle, track, belly_height in metres; max_pitch, max_roll (tangents) and min_clearance (metres) as float32
Chassis = collections.namedtuple("Chassis", "front_axle rear_axle track belly_height max_pitch max_roll min_clearance")
INF32 = np.float32(np.inf)


def make_chassis(front_axle, rear_axle, track, belly_height, max_pitch=INF32, max_roll=INF32, min_clearance=-INF32):
    return Chassis(float(front_axle), float(rear_axle), float(track), float(belly_height), np.float32(max_pitch), np.float32(max_roll),
                   np.float32(min_clearance))


def cos_sin(H):
    """(cos, sin) of 2 pi k / H as float64 [H, 2], exact at quarter turns (what the binding hands the library)"""
    a = 2.0 * np.pi * np.arange(H, dtype=np.float64) / H
    cs = np.stack([np.cos(a), np.sin(a)], axis=1)
    for k in range(H):
        if (4 * k) % H == 0:
            cs[k] = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[(4 * k) // H]
    return cs


def wheel_table(ch, cs):
    """float64 [H, 4, 2]: FL, FR, RL, RR turned to every heading"""
    half = ch.track / 2
    ab = ((ch.front_axle, half), (ch.front_axle, -half), (ch.rear_axle, half), (ch.rear_axle, -half))
    W = np.zeros((len(cs), 4, 2))
    for k, (c, s) in enumerate(np.asarray(cs, np.float64).tolist()):
        for i, (a, b) in enumerate(ab):
            W[k, i] = (a * c - b * s, a * s + b * c)
    return W


def known(g):
    with np.errstate(invalid="ignore"):
        return (g > -1000.0) & (g < np.inf)


def ground_of(height, inferred, use_inferred):
    """the ground map of a map set's maps 4 and 5"""
    with np.errstate(invalid="ignore"):
        return np.where(height > -1000.0, height, inferred if use_inferred else -1000.0)


def _keys(att):
    """the three keys an arg-extreme is the first maximum of: fabsf(pitch), fabsf(roll) (NaN ranks below every number), -belly"""
    p, r = np.abs(att[..., 0]), np.abs(att[..., 1])
    return np.where(np.isnan(p), np.float32(-1), p), np.where(np.isnan(r), np.float32(-1), r), -att[..., 2]


def summarise(att, status):
    K, T = status.shape
    summary = np.zeros((K, 5), np.int32)
    bad = status != OK
    first = np.where(bad.any(axis=1), bad.argmax(axis=1), T)
    rows = np.arange(K)
    summary[:, 0] = np.where(first < T, status[rows, np.minimum(first, T - 1)], OK)
    summary[:, 1] = first
    keys = _keys(att)
    for k in range(K):
        for j in range(3):
            summary[k, 2 + j] = -1 if first[k] == 0 else int(np.argmax(keys[j][k, :first[k]]))
    return summary


def score(g, poses, table, ch, cs, res, origin_cells):
    """g float64 [x, y]; poses float32 [K, T, 3]; table = (start, offsets); ch a Chassis; cs float64 [H, 2] -> (summary int32 [K, 5],
    attitude float32 [K, T, 3], status uint8 [K, T])"""
    g = np.asarray(g, np.float64)
    xy = g.shape[0]
    start, offsets = np.asarray(table[0], np.int64), np.asarray(table[1], np.int64)
    H = len(start) - 1
    cs = np.asarray(cs, np.float64)
    assert cs.shape == (H, 2)
    poses = np.asarray(poses, np.float32)
    K, T = poses.shape[:2]
    res = float(res)
    cx, cy, h, valid = rr.pose_frame(poses, res, origin_cells, H)
    W = wheel_table(ch, cs)
    wb, am = ch.front_axle - ch.rear_axle, 0.5 * (ch.front_axle + ch.rear_axle)
    with np.errstate(all="ignore"):
        x, y = poses[..., 0].astype(np.float64), poses[..., 1].astype(np.float64)
        x, y = np.where(valid, x, 0.0), np.where(valid, y, 0.0)
        qx, qy = x / res, y / res
        fx, fy = qx - np.floor(qx), qy - np.floor(qy)
        wheel_in = valid.copy()
        wc = []
        for i in range(4):
            cells = []
            for v, j in ((x, 0), (y, 1)):
                q = (v + W[h, i, j]) / res
                near = np.abs(q) < 2.0 ** 30
                c = np.where(near, np.floor(np.where(near, q, 0.0)).astype(np.int64) - int(origin_cells[j]), _OUT)
                wheel_in &= (c >= 0) & (c < xy)
                cells.append(c)
            wc.append(cells)
        z = [np.where(wheel_in, g[np.clip(c[0], 0, xy - 1), np.clip(c[1], 0, xy - 1)], np.nan) for c in wc]
        wheels_known = wheel_in & known(z[0]) & known(z[1]) & known(z[2]) & known(z[3])
        z = [np.where(wheels_known, v, 0.0) for v in z]
        zF, zR, zL, zT = 0.5 * (z[0] + z[1]), 0.5 * (z[2] + z[3]), 0.5 * (z[0] + z[2]), 0.5 * (z[1] + z[3])
        sp = (zF - zR) / wb
        sr = (zL - zT) / ch.track
        z0 = 0.25 * ((z[0] + z[1]) + (z[2] + z[3]))
        belly = np.full((K, T), np.inf)
        out = np.zeros((K, T), bool)
        for hh in np.unique(h[valid]):
            offs = offsets[start[hh]:start[hh + 1]]
            c, s = cs[hh]
            ks, ts = np.nonzero(valid & (h == hh))
            step = max(1, (1 << 21) // len(offs))
            for b in range(0, len(ks), step):
                k, t = ks[b:b + step], ts[b:b + step]
                X = cx[k, t][:, None] + offs[None, :, 0]
                Y = cy[k, t][:, None] + offs[None, :, 1]
                inside = (X >= 0) & (X < xy) & (Y >= 0) & (Y < xy)
                out[k, t] = (~inside).any(axis=1)
                gg = g[np.clip(X, 0, xy - 1), np.clip(Y, 0, xy - 1)]
                use = inside & known(gg) & wheels_known[k, t][:, None]
                gg = np.where(use, gg, 0.0)
                du = ((offs[None, :, 0].astype(np.float64) + 0.5) - fx[k, t][:, None]) * res
                dv = ((offs[None, :, 1].astype(np.float64) + 0.5) - fy[k, t][:, None]) * res
                u = du * c + dv * s
                v = dv * c - du * s
                plane = (z0[k, t][:, None] + sp[k, t][:, None] * (u - am)) + sr[k, t][:, None] * v
                clr = (plane + ch.belly_height) - gg
                belly[k, t] = np.where(use & ~np.isnan(clr), clr, np.inf).min(axis=1)
        att = np.stack([sp, sr, belly], axis=2).astype(np.float32)
        status = np.full((K, T), OK, np.uint8)
        status[att[..., 2] < ch.min_clearance] = BELLY
        status[np.abs(att[..., 1]) > ch.max_roll] = ROLL
        status[np.abs(att[..., 0]) > ch.max_pitch] = PITCH
        status[~wheels_known] = UNKNOWN_GROUND
        status[~wheel_in | out] = LEFT_WINDOW
        status[~valid] = INVALID
        att[status >= UNKNOWN_GROUND] = 0
    return summarise(att, status), att, status


def score_loops(g, poses, table, ch, cs, res, origin_cells):
    """the same, pose by pose and cell by cell over Python numbers (tiny inputs only); g a list of lists [x][y]"""
    xy = len(g)
    start, offsets = [int(v) for v in table[0]], [(int(a), int(b)) for a, b in table[1]]
    H = len(start) - 1
    s32 = np.float32(H / (2.0 * math.pi))
    res = float(res)
    K, T = len(poses), len(poses[0])
    half = ch.track / 2
    ab = ((ch.front_axle, half), (ch.front_axle, -half), (ch.rear_axle, half), (ch.rear_axle, -half))
    is_known = lambda v: v > -1000.0 and v < math.inf
    f32 = lambda v: np.float32(v)

    def cell(v, o):
        q = v / res
        return None if not abs(q) < 2.0 ** 30 else math.floor(q) - int(o)
    inside = lambda c: c is not None and 0 <= c < xy
    att, status = [], []
    for k in range(K):
        arow, srow = [], []
        for t in range(T):
            x, y, yaw = (np.float32(v) for v in poses[k][t])
            with np.errstate(all="ignore"):
                a = np.float32(yaw * s32)
            if not (math.isfinite(float(x)) and math.isfinite(float(y)) and math.isfinite(float(yaw)) and abs(float(a)) < 2.0 ** 24):
                arow.append((0.0, 0.0, 0.0))
                srow.append(INVALID)
                continue
            r = float(a)
            n = math.floor(r)
            if r - n > 0.5 or (r - n == 0.5 and n % 2 == 1):               # round half to even
                n += 1
            h = n % H
            x, y = float(x), float(y)
            c, s = float(cs[h][0]), float(cs[h][1])
            cxy = (cell(x, origin_cells[0]), cell(y, origin_cells[1]))
            left = False
            zs = []
            for a_, b_ in ab:
                wx, wy = a_ * c - b_ * s, a_ * s + b_ * c
                wcx, wcy = cell(x + wx, origin_cells[0]), cell(y + wy, origin_cells[1])
                if inside(wcx) and inside(wcy):
                    zs.append(float(g[wcx][wcy]))
                else:
                    left = True
            cells = []
            for dx, dy in offsets[start[h]:start[h + 1]]:
                if cxy[0] is None or cxy[1] is None or not (inside(cxy[0] + dx) and inside(cxy[1] + dy)):
                    left = True
                else:
                    cells.append((dx, dy, float(g[cxy[0] + dx][cxy[1] + dy])))
            if left:
                arow.append((0.0, 0.0, 0.0))
                srow.append(LEFT_WINDOW)
                continue
            if not all(is_known(v) for v in zs):
                arow.append((0.0, 0.0, 0.0))
                srow.append(UNKNOWN_GROUND)
                continue
            zFL, zFR, zRL, zRR = zs
            with np.errstate(all="ignore"):
                zF, zR, zL, zT = 0.5 * (zFL + zFR), 0.5 * (zRL + zRR), 0.5 * (zFL + zRL), 0.5 * (zFR + zRR)
                sp = float(np.float64(zF - zR) / np.float64(ch.front_axle - ch.rear_axle))
                sr = float(np.float64(zL - zT) / np.float64(ch.track))
                z0 = 0.25 * ((zFL + zFR) + (zRL + zRR))
                am = 0.5 * (ch.front_axle + ch.rear_axle)
                qx, qy = x / res, y / res
                fx, fy = qx - math.floor(qx), qy - math.floor(qy)
                belly = math.inf
                for dx, dy, gg in cells:
                    if not is_known(gg):
                        continue
                    du = ((dx + 0.5) - fx) * res
                    dv = ((dy + 0.5) - fy) * res
                    u = du * c + dv * s
                    v = dv * c - du * s
                    plane = (z0 + sp * (u - am)) + sr * v
                    clr = (plane + ch.belly_height) - gg
                    if clr < belly:
                        belly = clr
                p32, r32, b32 = f32(sp), f32(sr), f32(belly)
            if abs(p32) > ch.max_pitch:
                st = PITCH
            elif abs(r32) > ch.max_roll:
                st = ROLL
            elif b32 < ch.min_clearance:
                st = BELLY
            else:
                st = OK
            arow.append((p32, r32, b32))
            srow.append(st)
        att.append(arow)
        status.append(srow)
    att, status = np.array(att, np.float32), np.array(status, np.uint8)
    summary = []
    for k in range(K):
        first = next((t for t in range(T) if status[k][t] != OK), T)
        row = [int(status[k][first]) if first < T else OK, first]
        for j, sign in ((0, 1), (1, 1), (2, -1)):
            best, arg = None, -1
            for t in range(first):
                v = float(att[k][t][j])
                key = -v if sign < 0 else (-1.0 if v != v else abs(v))
                if best is None or key > best:
                    best, arg = key, t
            row.append(arg)
        summary.append(row)
    return np.array(summary, np.int32), att, status


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def ground_map(xy, pattern, res, origin_cells, seed=0):
    """float64 [x, y] heights in metres, a few cells' worth of relief"""
    rng = np.random.default_rng(2000 + 11 * xy + seed)
    i, j = np.meshgrid(np.arange(xy, dtype=np.float64), np.arange(xy, dtype=np.float64), indexing="ij")
    if pattern == "flat":
        return np.full((xy, xy), 0.75)
    if pattern == "plane":                                               # z = p*xw + q*yw + r at the cell centres
        return plane_ground(xy, res, origin_cells, 0.21, -0.13, 1.5)
    if pattern == "steps":                                               # terraces: runs of equal heights, ties of every extreme
        return np.floor(i / 5.0) * (0.8 * res) - np.floor(j / 7.0) * (0.5 * res)
    if pattern == "unknown":
        return np.full((xy, xy), -1000.0)
    g = rng.uniform(0.0, 1.2 * res, (xy, xy)) + 0.1 * res * (i - j)
    if pattern == "random":                                              # 10 % unknown, in every way a cell can be
        hole = rng.random((xy, xy)) < 0.1
        kinds = rng.integers(0, 6, (xy, xy))
        for n, v in enumerate((np.nan, np.inf, -np.inf, -1000.0, -2000.5, np.nextafter(-1000.0, -np.inf))):
            g[hole & (kinds == n)] = v
    return g


def plane_ground(xy, res, origin_cells, p, q, r):
    i, j = np.meshgrid(np.arange(xy, dtype=np.float64), np.arange(xy, dtype=np.float64), indexing="ij")
    return p * ((origin_cells[0] + i + 0.5) * res) + q * ((origin_cells[1] + j + 0.5) * res) + r


def case_chassis(res, limits):
    """a vehicle a few cells long; limits: None (none), or tangents and a clearance the random ground reaches on both sides"""
    geo = (2.3 * res, -1.7 * res, 2.6 * res, 1.0 * res)
    if limits is None:
        return make_chassis(*geo)
    return make_chassis(*geo, max_pitch=np.float32(0.3), max_roll=np.float32(0.35), min_clearance=np.float32(0.1 * res))


def _case(name, xy, pattern, table, K, T, seed, device, limits, poses=None, ch=None, ground=None):
    res, oc = rr.RES[xy], rr.ORIGIN_CELLS[xy]
    H = len(table[0]) - 1
    return dict(name=name, xy=xy, res=res, origin_cells=oc, origin=(oc[0] * res, oc[1] * res),
                g=ground_map(xy, pattern, res, oc, seed) if ground is None else ground, table=table,
                poses=rr.make_poses(K, T, xy, res, oc, H, seed) if poses is None else poses, device=device,
                chassis=case_chassis(res, limits) if ch is None else ch, cos_sin=cos_sin(H), pattern=pattern)


@functools.lru_cache(maxsize=None)
def cases(shape):
    """the synthetic inputs of one (K, T): a tuple of dicts {name, xy, res, origin_cells, origin, g, table, poses, device, chassis, cos_sin}"""
    K, T = shape
    i = SHAPES.index(shape)
    out = []
    for j, M in enumerate(CELLS):
        xy = SIZES[(i + j) % 4] if M < 1000 else (64, 100)[i % 2]
        pattern = GROUNDS[(i + 3 * j) % 5] if M < 1000 else "random"
        H = HEADINGS[(i + j) % 3]
        limits = None if (i + j) % 3 == 1 else True
        out.append(_case("%dx%d M%d H%d xy%d %s%s" % (K, T, M, H, xy, pattern, "" if limits else " no limits"), xy, pattern,
                         rr.patch_table(H, M, seed=i), K, T, seed=100 * i + j, device=(i + j) % 3 == 0, limits=limits))
    for j, xy in enumerate(SIZES):
        if (i + j) % 2 == 0:
            pattern = ("plane", "steps", "random")[(i + j) % 3]
            out.append(_case("%dx%d asymmetric xy%d %s" % (K, T, xy, pattern), xy, pattern, rr.asymmetric_table(7), K, T,
                             seed=900 + 10 * i + j, device=j % 2 == 1, limits=True if j % 2 else None))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def limit_cases():
    """a stored value one float32 ulp above, on and one ulp below each limit: the base case scored without limits, then each limit
    put next to a value the base case stores.  Rollouts hover about the window's centre: most poses are OK."""
    xy, H, M, K, T = 33, 7, 65, 6, 12
    res, oc = rr.RES[xy], rr.ORIGIN_CELLS[xy]
    table = rr.patch_table(H, M, seed=3)
    rng = np.random.default_rng(77)
    i, j = np.meshgrid(np.arange(xy, dtype=np.float64), np.arange(xy, dtype=np.float64), indexing="ij")
    ground = rng.uniform(0.0, 1.2 * res, (xy, xy)) + 0.1 * res * (i - j)
    poses = rr.arc_poses(K, T, xy, res, oc, 78, spread=3.0, centre=(xy // 2, xy // 2))
    base = _case("limits base", xy, "random", table, K, T, 0, False, None, poses=poses, ground=ground)
    _, att, status = score(base["g"], poses, table, base["chassis"], base["cos_sin"], res, oc)
    assert (status == OK).sum() > K * T // 3
    k, t = np.argwhere(status == OK)[len(np.argwhere(status == OK)) // 2]
    geo = base["chassis"][:4]
    out = []
    for n, field in enumerate(("max_pitch", "max_roll", "min_clearance")):
        v = att[k, t, n] if n == 2 else np.abs(att[k, t, n])
        for side, lim in (("above", np.nextafter(v, -INF32)), ("on", v), ("below", np.nextafter(v, INF32))):
            ch = make_chassis(*geo, **{field: lim})
            out.append(dict(_case("limit %s, value %s" % (field, side), xy, "random", table, K, T, 0, n % 2 == 0, None, poses=poses,
                                  ground=ground, ch=ch), probe=(int(k), int(t), n)))
    return tuple(out)


def all_cases():
    return [case for shape in SHAPES for case in cases(shape)] + list(limit_cases())


def _score_case(q):
    return score(q["g"], q["poses"], q["table"], q["chassis"], q["cos_sin"], q["res"], q["origin_cells"])


@functools.lru_cache(maxsize=None)
def expected(shape):
    """score() of every case of cases(shape), computed once"""
    return tuple(_score_case(q) for q in cases(shape))


@functools.lru_cache(maxsize=None)
def expected_limits():
    return tuple(_score_case(q) for q in limit_cases())


CAR_CHASSIS = dict(front_axle=2.7, rear_axle=0.0, track=1.7, belly_height=0.25)     # metres: the car of rollouts_ref.CAR


@functools.lru_cache(maxsize=None)
def large_case(footprint):
    """xy 1024 at a negative origin: K = 1024 rollouts of T = 64 poses spread over the map with the car footprint (`footprint` =
    (start bytes, offsets bytes, H), the caller's rectangle_footprint table) on rolling ground with one unknown cell in a thousand"""
    xy = 1024
    start = np.frombuffer(footprint[0], np.int32)
    table = (start, np.frombuffer(footprint[1], np.int16).reshape(-1, 2))
    res, oc = rr.RES[xy], rr.ORIGIN_CELLS[xy]
    rng = np.random.default_rng(99)
    i, j = np.meshgrid(np.arange(xy, dtype=np.float64), np.arange(xy, dtype=np.float64), indexing="ij")
    g = 1.5 * np.sin(i * 0.021) * np.cos(j * 0.017) + rng.uniform(0.0, 0.08, (xy, xy))
    g[rng.random((xy, xy)) < 0.001] = -1000.0
    ch = make_chassis(max_pitch=np.float32(np.tan(0.12)), max_roll=np.float32(np.tan(0.11)), min_clearance=np.float32(0.14), **CAR_CHASSIS)
    q = _case("large xy1024", xy, "random", table, 1024, 64, 5, True, None, poses=rr.arc_poses(1024, 64, xy, res, oc, 4242), ch=ch, ground=g)
    return q, _score_case(q)


def census(inputs):
    """what a list of (case, (summary, attitude, status)) reaches, as counters"""
    n = dict(status=[0] * 7, summary_status=[0] * 7, first_0=0, first_T=0, wheel_unknown_only=0, belly_unknown_only=0, belly_inf=0,
             tie_pitch=0, tie_roll=0, tie_belly=0, on_border=0, heading_ties=set(), map_nan=0, map_inf=0, map_m1000=0,
             west=0, east=0, south=0, north=0, wheel_outside_only=0, ulp=set())
    for q, (summary, att, status) in inputs:
        K, T = status.shape
        xy, res, oc = q["xy"], q["res"], q["origin_cells"]
        g = q["g"]
        for s in range(7):
            n["status"][s] += int((status == s).sum())
            n["summary_status"][s] += int((summary[:, 0] == s).sum())
        first = summary[:, 1]
        n["first_0"] += int((first == 0).sum())
        n["first_T"] += int((first == T).sum())
        keys = _keys(att)
        for k in range(K):
            for j, name in enumerate(("tie_pitch", "tie_roll", "tie_belly")):
                if first[k] > 1:
                    row = keys[j][k, :first[k]]
                    n[name] += int((row == row.max()).sum() > 1)
        start, offsets = q["table"]
        H = len(start) - 1
        cx, cy, h, valid = rr.pose_frame(q["poses"], res, oc, H)
        W = wheel_table(q["chassis"], q["cos_sin"])
        with np.errstate(all="ignore"):
            p = q["poses"]
            qx, qy = p[..., 0].astype(np.float64) / res, p[..., 1].astype(np.float64) / res
            n["on_border"] += int((valid & ((qx == np.floor(qx)) | (qy == np.floor(qy)))).sum())
            a = p[..., 2] * rr.heading_scale(H)
            for target in (0.5, 1.5, 2.5, -0.5):
                if (valid & (a == np.float32(target))).any():
                    n["heading_ties"].add(target)
        n["map_nan"] += int(np.isnan(g).sum())
        n["map_inf"] += int(np.isinf(g).sum())
        n["map_m1000"] += int((g == -1000.0).sum())
        lo = np.array([offsets[start[k]:start[k + 1]].min(axis=0) for k in range(H)], np.int64)
        hi = np.array([offsets[start[k]:start[k + 1]].max(axis=0) for k in range(H)], np.int64)
        inside = valid & (cx >= 0) & (cx < xy) & (cy >= 0) & (cy < xy)
        n["west"] += int((inside & (cx + lo[h, 0] < 0)).sum())
        n["east"] += int((inside & (cx + hi[h, 0] >= xy)).sum())
        n["south"] += int((inside & (cy + lo[h, 1] < 0)).sum())
        n["north"] += int((inside & (cy + hi[h, 1] >= xy)).sum())
        # per pose, over Python loops only where it matters: the unknown cells under wheels and belly
        kn = known(g)
        for k, t in np.argwhere(valid & (status != LEFT_WINDOW))[:4000]:
            offs = offsets[start[h[k, t]]:start[h[k, t] + 1]]
            fk = kn[cx[k, t] + offs[:, 0], cy[k, t] + offs[:, 1]]
            if status[k, t] == UNKNOWN_GROUND:
                n["wheel_unknown_only"] += int(fk.all())
            else:
                n["belly_unknown_only"] += int(not fk.all())
                n["belly_inf"] += int(att[k, t, 2] == np.inf and not fk.any())
        fp_in = valid & (cx + lo[h, 0] >= 0) & (cx + hi[h, 0] < xy) & (cy + lo[h, 1] >= 0) & (cy + hi[h, 1] < xy)
        n["wheel_outside_only"] += int((fp_in & (status == LEFT_WINDOW)).sum())
        ch = q["chassis"]
        with np.errstate(all="ignore"):
            live = status < UNKNOWN_GROUND
            for j, (lim, v) in enumerate(((ch.max_pitch, np.abs(att[..., 0])), (ch.max_roll, np.abs(att[..., 1])), (ch.min_clearance, att[..., 2]))):
                if np.isfinite(lim):
                    for side, w in (("above", np.nextafter(lim, INF32)), ("on", lim), ("below", np.nextafter(lim, -INF32))):
                        if (live & (v == w)).any():
                            n["ulp"].add((j, side))
    return n
