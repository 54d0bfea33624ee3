"""The numpy referee of body clearance scoring (include/gvom_hip.h "body clearance scoring"; gvom_score_body, k_body) and the inputs of
tests/test_body.py and tests/test_body_cpu.py.

score() is the definition, vectorised, every float64 operation one numpy operation in the header's order: the pose frame is rollout
scoring's (tests/rollouts_ref.py pose_frame); the four wheels stand where terrain attitude scoring puts them (tests/attitude_ref.py
wheel_table, known) and give sp, sr and z0; the frame e1, e2, n and q0; per sphere the centre, its voxel, the margin d - r in float32;
the status the first of INVALID, LEFT_WINDOW, UNKNOWN_GROUND, LEFT_BOX, COLLISION, OK; per rollout the first bad pose and the least
clearance in front of it.  score_loops() says the same a second time as plain Python loops over Python numbers.  Tolerance 0.

cases() are the GPU test's synthetic inputs (every one also scored here, once, by expected()); census() counts what they reach."""
import functools
import math

import numpy as np

import attitude_ref as ar
import rollouts_ref as rr

OK, COLLISION, LEFT_BOX, UNKNOWN_GROUND, LEFT_WINDOW, INVALID = range(6)
N_STATUS = 6
NO_SPHERE = 255

# the grids of the synthetic cases: xy_size -> (xy_resolution, z_resolution, z_size, origin_cells, field origin in world voxels); at 0.3 / 0.2
# the divisions round; the field's box is the window's shifted a voxel or two, its floor below zero
GRIDS = {16: (0.4, 0.4, 8, (-5, 3), (-4, 2, -1)), 33: (0.25, 0.25, 8, (7, -40), (6, -40, -2)), 40: (0.3, 0.2, 6, (-13, 21), (-14, 22, 0))}
SHAPES = ((1, 1), (3, 63), (2, 64), (2, 65), (1, 256), (2, 257), (2, 4096))
SPHERES = (1, 2, 63, 64, 65, 256)
HEADINGS = (1, 7, 64)
GROUNDS = ar.GROUNDS


# ---- the definition, vectorised -------------------------------------------------------------------------------------------------------
def stance(g, poses, ch, cs, res, origin_cells):
    """what terrain attitude scoring makes of the four wheels: dict(x, y, h, valid, wheel_in, wheels_known, sp, sr, z0), arrays [K, T]"""
    g = np.asarray(g, np.float64)
    xy = g.shape[0]
    cs = np.asarray(cs, np.float64)
    H = len(cs)
    poses = np.asarray(poses, np.float32)
    _, _, h, valid = rr.pose_frame(poses, res, origin_cells, H)
    W = ar.wheel_table(ch, cs)
    wb = ch.front_axle - ch.rear_axle
    with np.errstate(all="ignore"):
        x, y = poses[..., 0].astype(np.float64), poses[..., 1].astype(np.float64)
        x, y = np.where(valid, x, 0.0), np.where(valid, y, 0.0)
        wheel_in = valid.copy()
        wc = []
        for i in range(4):
            cells = []
            for v, j in ((x, 0), (y, 1)):
                q = (v + W[h, i, j]) / res
                near = np.abs(q) < 2.0 ** 30
                c = np.where(near, np.floor(np.where(near, q, 0.0)).astype(np.int64) - int(origin_cells[j]), -(1 << 40))
                wheel_in &= (c >= 0) & (c < xy)
                cells.append(c)
            wc.append(cells)
        z = [np.where(wheel_in, g[np.clip(c[0], 0, xy - 1), np.clip(c[1], 0, xy - 1)], np.nan) for c in wc]
        wheels_known = wheel_in & ar.known(z[0]) & ar.known(z[1]) & ar.known(z[2]) & ar.known(z[3])
        z = [np.where(wheels_known, v, 0.0) for v in z]
        zF, zR, zL, zT = 0.5 * (z[0] + z[1]), 0.5 * (z[2] + z[3]), 0.5 * (z[0] + z[2]), 0.5 * (z[1] + z[3])
        sp = (zF - zR) / wb
        sr = (zL - zT) / ch.track
        z0 = 0.25 * ((z[0] + z[1]) + (z[2] + z[3]))
    return dict(x=x, y=y, h=h, valid=valid, wheel_in=wheel_in, wheels_known=wheels_known, sp=sp, sr=sr, z0=z0)


def frame(sp, sr, z0, am):
    """FRAME: (e1u, e1w, nu, nv, nw, e2u, e2v, e2w, q0)"""
    with np.errstate(all="ignore"):
        one = 1.0 + sp * sp
        lu, ln = np.sqrt(one), np.sqrt(one + sr * sr)
        e1u, e1w = 1.0 / lu, sp / lu
        nu, nv, nw = -sp / ln, -sr / ln, 1.0 / ln
        e2u, e2v, e2w = nv * e1w, nw * e1u - nu * e1w, -(nv * e1u)
        q0 = z0 - sp * am
    return e1u, e1w, nu, nv, nw, e2u, e2v, e2w, q0


def centres(x, y, c, s, fr, body):
    """SPHERE CENTRE: X, Y, Z float64 [..., S] of body float32 [S, 4] at poses whose arrays have the shape of x"""
    e1u, e1w, nu, nv, nw, e2u, e2v, e2w, q0 = (np.asarray(v, np.float64)[..., None] for v in fr)
    b = np.asarray(body, np.float32).astype(np.float64)
    bx, by, bz = b[:, 0], b[:, 1], b[:, 2]
    c, s = np.asarray(c, np.float64)[..., None], np.asarray(s, np.float64)[..., None]
    with np.errstate(all="ignore"):
        Cu = (bx * e1u + by * e2u) + bz * nu
        Cv = by * e2v + bz * nv
        Cw = ((bx * e1w + by * e2w) + bz * nw) + q0
        X = np.asarray(x, np.float64)[..., None] + (Cu * c - Cv * s)
        Y = np.asarray(y, np.float64)[..., None] + (Cu * s + Cv * c)
    return X, Y, Cw


def voxels(X, Y, Z, res, zres, B, n, zs):
    """(vx, vy, vz, inside): the voxel of every centre in the box at B, int64, 0 where outside"""
    out, inside = [], np.ones(X.shape, bool)
    with np.errstate(all="ignore"):
        for v, r, o, size in ((X, res, B[0], n), (Y, res, B[1], n), (Z, zres, B[2], zs)):
            q = v / float(r)
            near = np.abs(q) < 2.0 ** 30
            c = np.floor(np.where(near, q, 0.0)).astype(np.int64) - int(o)
            ok = near & (c >= 0) & (c < size)
            inside &= ok
            out.append(np.where(ok, c, 0))
    return out[0], out[1], out[2], inside


def summarise(clearance, pairs):
    K, T = clearance.shape
    status = pairs[..., 0]
    summary = np.zeros((K, 4), np.int32)
    bad = status != OK
    first = np.where(bad.any(axis=1), bad.argmax(axis=1), T)
    for k in range(K):
        f = int(first[k])
        tp = -1 if f == 0 else int(np.argmin(clearance[k, :f]))             # (the first of equal minima; a clearance is never NaN)
        summary[k] = (int(status[k, f]) if f < T else OK, f, tp, -1 if f == 0 else int(pairs[k, tp, 1]))
    return summary


def score(field, B, g, poses, body, ch, cs, res, zres, origin_cells, min_margin, tilt=True, parts=False):
    """field float32 [n, n, zs] with its corner at world voxel B; g float64 [x, y]; poses float32 [K, T, 3]; body float32 [S, 4]; ch a
    Chassis (attitude_ref); cs float64 [H, 2] -> (summary int32 [K, 4], clearance float32 [K, T], pairs uint8 [K, T, 2]).  tilt=False: the
    untilted frame (sp = sr = 0, the same z0), for the census.  parts=True: also the voxels' (vx, vy, vz, inside)."""
    field = np.asarray(field, np.float32)
    n, zs = field.shape[0], field.shape[2]
    body = np.asarray(body, np.float32)
    st = stance(g, poses, ch, cs, res, origin_cells)
    cs = np.asarray(cs, np.float64)
    am = 0.5 * (ch.front_axle + ch.rear_axle)
    sp, sr = (st["sp"], st["sr"]) if tilt else (np.zeros_like(st["sp"]), np.zeros_like(st["sr"]))
    fr = frame(sp, sr, st["z0"], am)
    X, Y, Z = centres(st["x"], st["y"], cs[st["h"], 0], cs[st["h"], 1], fr, body)
    vx, vy, vz, inside = voxels(X, Y, Z, res, zres, B, n, zs)
    with np.errstate(all="ignore"):
        d = field[vx, vy, vz]
        m = (d - body[:, 3]).astype(np.float32)                              # one float32 subtraction
        live = inside & ~np.isnan(m)
        mm = np.where(live, m, np.float32(np.inf))
        clr = mm.min(axis=2)
        attains = live & (mm == clr[..., None])
        tight = np.where(attains.any(axis=2), attains.argmax(axis=2), NO_SPHERE)
        status = np.where(clr < np.float32(min_margin), COLLISION, OK)
    status[~inside.all(axis=2)] = LEFT_BOX
    status[~st["wheels_known"]] = UNKNOWN_GROUND
    status[~st["wheel_in"]] = LEFT_WINDOW
    status[~st["valid"]] = INVALID
    clr = np.where(status >= LEFT_BOX, np.float32(0), clr).astype(np.float32)
    tight = np.where(status >= LEFT_BOX, 0, tight)
    pairs = np.stack([status, tight], axis=2).astype(np.uint8)
    out = (summarise(clr, pairs), clr, pairs)
    return out + ((vx, vy, vz, inside),) if parts else out


def score_loops(field, B, g, poses, body, ch, cs, res, zres, origin_cells, min_margin):
    """the same, pose by pose and sphere by sphere over Python numbers; field [x][y][z] and g [x][y] anything indexable"""
    n, zs, xy = len(field), len(field[0][0]), len(g)
    H = len(cs)
    s32 = np.float32(H / (2.0 * math.pi))
    res, zres = float(res), float(zres)
    K, T = len(poses), len(poses[0])
    half = ch.track / 2
    ab = ((ch.front_axle, half), (ch.front_axle, -half), (ch.rear_axle, half), (ch.rear_axle, -half))
    am = 0.5 * (ch.front_axle + ch.rear_axle)
    is_known = lambda v: v > -1000.0 and v < math.inf
    mm32 = np.float32(min_margin)

    def cell(v, r, o, size):
        q = v / r
        if not abs(q) < 2.0 ** 30:
            return None
        c = math.floor(q) - int(o)
        return c if 0 <= c < size else None
    clearance, pairs = [], []
    for k in range(K):
        crow, prow = [], []
        for t in range(T):
            x, y, yaw = (np.float32(v) for v in poses[k][t])
            with np.errstate(all="ignore"):
                a = np.float32(yaw * s32)
            if not (math.isfinite(float(x)) and math.isfinite(float(y)) and math.isfinite(float(yaw)) and abs(float(a)) < 2.0 ** 24):
                crow.append(np.float32(0)); prow.append((INVALID, 0))
                continue
            r = float(a)
            i = math.floor(r)
            if r - i > 0.5 or (r - i == 0.5 and i % 2 == 1):               # round half to even
                i += 1
            h = i % H
            x, y = float(x), float(y)
            c, s = float(cs[h][0]), float(cs[h][1])
            zw, left = [], False
            for a_, b_ in ab:
                wx, wy = a_ * c - b_ * s, a_ * s + b_ * c
                wcx, wcy = cell(x + wx, res, origin_cells[0], xy), cell(y + wy, res, origin_cells[1], xy)
                if wcx is None or wcy is None:
                    left = True
                else:
                    zw.append(float(g[wcx][wcy]))
            if left:
                crow.append(np.float32(0)); prow.append((LEFT_WINDOW, 0))
                continue
            if not all(is_known(v) for v in zw):
                crow.append(np.float32(0)); prow.append((UNKNOWN_GROUND, 0))
                continue
            zFL, zFR, zRL, zRR = (np.float64(v) for v in zw)                 # (numpy scalars: an overflow is an infinity, not an exception)
            with np.errstate(all="ignore"):
                zF, zR, zL, zT = 0.5 * (zFL + zFR), 0.5 * (zRL + zRR), 0.5 * (zFL + zRL), 0.5 * (zFR + zRR)
                sp = (zF - zR) / np.float64(ch.front_axle - ch.rear_axle)
                sr = (zL - zT) / np.float64(ch.track)
                z0 = 0.25 * ((zFL + zFR) + (zRL + zRR))
                lu = np.sqrt(1.0 + sp * sp)
                ln = np.sqrt((1.0 + sp * sp) + sr * sr)
                e1u, e1w = 1.0 / lu, sp / lu
                nu, nv, nw = -sp / ln, -sr / ln, 1.0 / ln
                e2u, e2v, e2w = nv * e1w, nw * e1u - nu * e1w, -(nv * e1u)
                q0 = z0 - sp * am
                clr, tight, out = np.float32(np.inf), None, False
                for j, sph in enumerate(body):
                    bx, by, bz = (np.float64(np.float32(v)) for v in sph[:3])
                    Cu = (bx * e1u + by * e2u) + bz * nu
                    Cv = by * e2v + bz * nv
                    Cw = ((bx * e1w + by * e2w) + bz * nw) + q0
                    X = x + (Cu * c - Cv * s)
                    Y = y + (Cu * s + Cv * c)
                    v = (cell(float(X), res, B[0], n), cell(float(Y), res, B[1], n), cell(float(Cw), zres, B[2], zs))
                    if None in v:
                        out = True
                        continue
                    m = np.float32(np.float32(field[v[0]][v[1]][v[2]]) - np.float32(sph[3]))
                    if m != m:
                        continue
                    if tight is None or m < clr:
                        clr, tight = m, j
            if out:
                crow.append(np.float32(0)); prow.append((LEFT_BOX, 0))
            else:
                crow.append(clr); prow.append((COLLISION if clr < mm32 else OK, NO_SPHERE if tight is None else tight))
        clearance.append(crow)
        pairs.append(prow)
    clearance, pairs = np.array(clearance, np.float32), np.array(pairs, np.uint8)
    summary = []
    for k in range(K):
        first = next((t for t in range(T) if pairs[k][t][0] != OK), T)
        best, arg = None, -1
        for t in range(first):
            if best is None or clearance[k][t] < best:
                best, arg = clearance[k][t], t
        summary.append([int(pairs[k][first][0]) if first < T else OK, first, arg, -1 if first == 0 else int(pairs[k][arg][1])])
    return np.array(summary, np.int32), clearance, pairs


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def random_field(xy, zs, res, zres, seed, nan=False):
    """float32 [xy, xy, zs]: values the distance field can hold -- 0, float32 roots of a*n + b*m, +inf -- at random; nan: a tenth NaN"""
    rng = np.random.default_rng(3000 + seed)
    a, b = res * res, zres * zres
    nn, mm = rng.integers(0, 40, (xy, xy, zs)).astype(np.float64), rng.integers(0, 12, (xy, xy, zs)).astype(np.float64)
    f = np.sqrt(a * nn + b * mm).astype(np.float32)
    u = rng.random((xy, xy, zs))
    f[u < 0.01] = 0.0
    f[u > 0.85] = np.inf
    if nan:
        f[rng.random((xy, xy, zs)) < 0.1] = np.nan
    return f


def random_body(S, res, zres, seed, small=False):
    """float32 [S, 4]: centres a few cells about the pose and up to a few levels above the contact plane; radii up to half a cell (a
    tenth of one where `small`: a body of many spheres that still passes somewhere)"""
    rng = np.random.default_rng(4000 + 17 * S + seed)
    b = np.stack([rng.uniform(-2.0 * res, 3.0 * res, S), rng.uniform(-1.5 * res, 1.5 * res, S), rng.uniform(0.2 * zres, 2.6 * zres, S),
                  rng.uniform(0.0, (0.1 if small else 0.5) * res, S)], axis=1).astype(np.float32)
    b[0, 3] = 0.0
    return b


def make_poses(K, T, xy, res, origin_cells, H, seed):
    """arcs about the window's middle, a cell per pose, with rollouts_ref's special poses -- cell borders, the four sides, heading
    ties, the invalid ones -- written over poses of the second half of the rollouts; one pose: a special one or the middle"""
    p = rr.arc_poses(K, T, xy, res, origin_cells, seed, spread=xy / 5.0, centre=(xy // 2, xy // 2))
    sp = rr.special_poses(xy, res, origin_cells, H)
    rng = np.random.default_rng(seed + 1)
    if T == 1:
        p[:, 0] = sp[(seed * 3) % len(sp)]
        return p
    slots = rng.permutation(K * (T - T // 2))[:min(len(sp), max(1, K * T // 6))]
    for i, slot in enumerate(slots):
        p[slot // (T - T // 2), T // 2 + slot % (T - T // 2)] = sp[len(sp) - 1 - i]   # (the invalid ones first)
    return p


def _case(name, xy, pattern, H, S, K, T, seed, device, min_margin, nan=False, poses=None, body=None, field=None, ground=None, B=None):
    res, zres, zs, oc, fo = GRIDS[xy]
    g = ar.ground_map(xy, pattern, res, oc, seed) if ground is None else ground
    if B is None:                                                          # the box's floor a level or two under the middle of the known ground
        kn = g[ar.known(g)]
        B = (fo[0], fo[1], fo[2] + (int(math.floor(float(np.median(kn)) / zres)) if len(kn) else 0))
    return dict(name=name, xy=xy, zs=zs, res=res, zres=zres, origin_cells=oc, origin=(oc[0] * res, oc[1] * res), g=g,
                field=random_field(xy, zs, res, zres, seed, nan) if field is None else field, field_origin=B,
                body=random_body(S, res, zres, seed, small=S > 8) if body is None else body, table=rr.patch_table(H, 1, seed=seed),
                poses=make_poses(K, T, xy, res, oc, H, seed) if poses is None else poses, device=device,
                chassis=ar.case_chassis(res, None), cos_sin=ar.cos_sin(H), pattern=pattern, min_margin=np.float32(min_margin))


@functools.lru_cache(maxsize=None)
def cases(shape):
    """the synthetic inputs of one (K, T): three cases that turn through the grids, the grounds, S, H, the route and min_margin"""
    K, T = shape
    i = SHAPES.index(shape)
    out = []
    for j in range(3):
        xy = (16, 33, 40)[(i + j) % 3]
        pattern = GROUNDS[(2 * i + j) % 5]
        S, H = SPHERES[(i + 2 * j) % 6], HEADINGS[(i + j + 1) % 3]
        mm = (0.0, -0.05, 0.12)[(i + 2 * j) % 3] if S <= 8 else (-0.3, -0.08, 0.0)[(i + j) % 3]
        out.append(_case("%dx%d S%d H%d xy%d %s" % (K, T, S, H, xy, pattern), xy, pattern, H, S, K, T, seed=10 * i + j, device=(i + j) % 2 == 0,
                         min_margin=mm))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def nan_case():
    """a field with NaN entries, and a body whose first sphere often reads one: margins that are skipped, poses whose every margin is"""
    q = _case("NaN field", 33, "plane", 7, 2, 3, 63, seed=71, device=True, min_margin=0.0, nan=True)
    return q


def _hover_poses(xy, K, T, seed):
    res, _, _, oc, _ = GRIDS[xy]
    return rr.arc_poses(K, T, xy, res, oc, seed, spread=2.0, centre=(xy // 2, xy // 2))


@functools.lru_cache(maxsize=None)
def limit_cases():
    """a stored clearance one float32 ulp above, on and one ulp below min_margin: the base case scored once, then the limit put next to
    a clearance it stores"""
    xy, K, T = 33, 4, 12
    poses = _hover_poses(xy, K, T, 5)
    base = _case("limit base", xy, "plane", 7, 2, K, T, seed=33, device=False, min_margin=-100.0, poses=poses)
    _, clr, pairs = score_case(base)
    idx = np.argwhere((pairs[..., 0] == OK) & np.isfinite(clr))
    assert len(idx) > 4
    k, t = idx[len(idx) // 2]
    v = clr[k, t]
    out = []
    for n, (side, lim) in enumerate((("above", np.nextafter(v, np.float32(-np.inf))), ("on", v), ("below", np.nextafter(v, np.float32(np.inf))))):
        out.append(dict(_case("limit, value %s" % side, xy, "plane", 7, 2, K, T, seed=33, device=n % 2 == 0, min_margin=lim, poses=poses),
                        probe=(int(k), int(t)), expect=COLLISION if side == "below" else OK))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def edge_cases():
    """box and window edges on flat ground at heading 0, where X = x + bx, Y = y + by and Z = z0 + bz exactly: a sphere exactly on a box
    face (inside on the low face, outside on the high one), at a negative coordinate, at |quotient| >= 2^30; a wheel outside the window
    while every sphere is inside the box, and the reverse"""
    xy = 16
    res, zres, zs, oc, _ = GRIDS[xy]
    ground = np.full((xy, xy), 0.0)
    field = random_field(xy, zs, res, zres, 91)
    field[field == 0] = np.float32(res)
    out = []
    mid = (np.float32((oc[0] + 8) * res), np.float32((oc[1] + 8) * res), np.float32(0))
    B = (oc[0], oc[1], 0)
    one = lambda name, body, poses, BB=B, expect=None: out.append(dict(_case(name, xy, "flat", 1, len(body), 1, len(poses), seed=0, device=len(out) % 2 == 0,
        min_margin=-100.0, poses=np.array([poses], np.float32), body=np.array(body, np.float32), field=field, ground=ground, B=BB), expect=expect))
    lo_face = float(np.float32(B[0] * res)) - float(mid[0])                   # body x that puts X on the box's low face (a float32 or not: the referee decides)
    one("sphere on the low box face", [(np.float32(lo_face), 0, 0.2, 0)], [mid], expect=None)
    one("sphere on the high box face", [(np.float32((B[0] + xy) * res - float(mid[0])), 0, 0.2, 0)], [mid])
    one("sphere on the floor and on the ceiling", [(0, 0, 0.0, 0), (0, 0, np.float32(zs * zres), 0)], [mid])
    neg = (np.float32(-1.2), mid[1], np.float32(0))                          # world x < 0 under the pose and every wheel; the ground below zero
    out.append(dict(_case("spheres at negative coordinates", xy, "flat", 1, 2, 1, 2, seed=0, device=True, min_margin=-100.0,
                          poses=np.array([[neg, neg]], np.float32), body=np.array([(-0.3, 0.1, 0.3, 0.05), (0.2, -0.2, 0.5, 0.1)], np.float32),
                          field=field, ground=np.full((xy, xy), -0.9), B=(oc[0], oc[1], -3)), expect=OK))
    one("sphere beyond 2^30 voxels", [(np.float32(2.0 ** 30 * res), 0, 0.2, 0), (0, 0, 0.2, 0)], [mid], expect=LEFT_BOX)
    one("sphere beyond 2^30 levels", [(0, 0, np.float32(2.0 ** 30 * zres), 0)], [mid], expect=LEFT_BOX)
    edge = (np.float32((oc[0] + 0.5) * res), mid[1], np.float32(0))          # rear axle outside the window's west side
    one("wheel outside the window, spheres inside the box", [(0.5, 0, 0.3, 0)], [edge], BB=(oc[0] - 4, oc[1], 0), expect=LEFT_WINDOW)
    one("spheres outside the box, wheels inside the window", [(0.5, 0, 0.3, 0)], [mid], BB=(oc[0] + 12, oc[1], 0), expect=LEFT_BOX)
    return tuple(out)


def all_cases():
    return [q for shape in SHAPES for q in cases(shape)] + [nan_case()] + list(limit_cases()) + list(edge_cases())


def score_case(q, **kw):
    return score(q["field"], q["field_origin"], q["g"], q["poses"], q["body"], q["chassis"], q["cos_sin"], q["res"], q["zres"], q["origin_cells"],
                 q["min_margin"], **kw)


@functools.lru_cache(maxsize=None)
def expected(shape):
    """score() of every case of cases(shape), computed once"""
    return tuple(score_case(q) for q in cases(shape))


@functools.lru_cache(maxsize=None)
def expected_other():
    """score() of the NaN case, the limit cases and the edge cases, in that order, computed once"""
    return tuple(score_case(q) for q in [nan_case()] + list(limit_cases()) + list(edge_cases()))


def census(inputs):
    """what a list of (case, (summary, clearance, pairs)) reaches, as counters"""
    n = dict(status=[0] * N_STATUS, ok_finite=0, ok_inf=0, tightest=set(), all_skipped=0, tilt_voxel=0, tilt_clearance=0, tilt_status=0,
             free_prefix=0, tightest_pose_not_0=0, first_0=0, first_T=0, nan_read=0)
    for q, (summary, clr, pairs) in inputs:
        status = pairs[..., 0]
        for s in range(N_STATUS):
            n["status"][s] += int((status == s).sum())
        ok = status == OK
        n["ok_finite"] += int((ok & np.isfinite(clr)).sum())
        n["ok_inf"] += int((ok & (clr == np.inf)).sum())
        n["all_skipped"] += int((ok & (pairs[..., 1] == NO_SPHERE)).sum()) if len(q["body"]) < 256 else 0
        if len(q["body"]) >= 8:
            n["tightest"] |= set(int(v) for v in np.unique(pairs[..., 1][status <= COLLISION]))
        T = status.shape[1]
        n["first_0"] += int((summary[:, 1] == 0).sum())
        n["first_T"] += int((summary[:, 1] == T).sum())
        free = summary[:, 1] >= 2
        n["free_prefix"] += int(free.sum())
        n["tightest_pose_not_0"] += int((free & (summary[:, 2] != 0)).sum())
        _, clr0, pairs0, v0 = score_case(q, tilt=False, parts=True)
        _, _, _, v1 = score_case(q, parts=True)
        live = (status <= LEFT_BOX) & (pairs0[..., 0] <= LEFT_BOX)             # (the stance is the same in both frames)
        moved = live & ((v0[0] != v1[0]) | (v0[1] != v1[1]) | (v0[2] != v1[2]) | (v0[3] != v1[3])).any(axis=2)
        n["tilt_voxel"] += int(moved.sum())
        n["tilt_clearance"] += int((moved & (clr.view(np.uint32) != clr0.view(np.uint32))).sum())
        n["tilt_status"] += int((moved & (status != pairs0[..., 0])).sum())
        n["nan_read"] += int(np.isnan(q["field"]).any())
    return n
