"""The numpy referee of attitude volumes (include/gvom_hip.h "attitude volumes"; gvom_attitude_volume, k_volume_attitude,
gvom_pose_field_attitude, k_cspace_attitude) and the inputs of tests/test_attitude_volume.py and tests/test_attitude_volume_cpu.py.

volume() is the definition, vectorised over the cells of one heading, every float64 operation one numpy operation in the header's
order: wheel i of heading h stands in cell (cx + floor(0.5 + wx / res), cy + floor(0.5 + wy / res)); pitch and roll tangents from the
four heights; the belly the least of ((z0 + sp*U) + sr*V + belly_height) - g over the footprint's known cells, with U = u - am and V =
v of terrain attitude scoring at fx = fy = 0.5; the status the first of LEFT_WINDOW, UNKNOWN_GROUND, PITCH, ROLL, BELLY, OK, decided
on the float32 values; the tilt the percentage of the nearer limit.  volume_loops() says the same a second time as plain Python loops
over Python numbers; the CPU test holds the two together, and both against attitude_ref.score() at the cell-centre poses.
masked_cost() is the pose cost volume with an attitude volume taken in; field() is the pose-field referee of tests/posefield_ref.py
applied to it.  Everything is compared with tolerance 0.

cases() are the GPU test's synthetic inputs (each also scored here, once, by expected())."""
import functools
import math

import numpy as np

import attitude_ref as ar
import posefield_ref as pf
import rollouts_ref as rr

OK, PITCH, ROLL, BELLY, UNKNOWN_GROUND, LEFT_WINDOW, INVALID = range(7)

SIZES = (16, 31, 33, 64, 65, 100)
HEADINGS = (1, 4, 16)
CELLS = tuple(m for m in ar.CELLS if m in (1, 63, 64, 65, 257))
GROUNDS = ar.GROUNDS
RES = dict(rr.RES)
RES.update({31: 0.4, 65: 0.25})
assert CELLS == (1, 63, 64, 65, 257) and GROUNDS == ("flat", "plane", "steps", "random", "unknown")


def wheel_offsets(ch, cs, res):
    """int64 [H, 4, 2]: floor(0.5 + w / res) of the wheel table"""
    W = ar.wheel_table(ch, cs)
    return np.floor(0.5 + W / float(res)).astype(np.int64)


def _share(a32, limit):
    """(double)fabsf(a) / (double)limit * 100.0, 0 for a limit that is not finite"""
    if not np.isfinite(limit):
        return np.zeros(a32.shape, np.float64)
    with np.errstate(all="ignore"):
        return np.abs(a32).astype(np.float64) / np.float64(limit) * 100.0


def tilt_of(p32, r32, ch, status):
    """uint8 tilt of float32 tangents (arrays) under the chassis' limits; 0 where the status is UNKNOWN_GROUND or LEFT_WINDOW"""
    tp, tr = _share(p32, ch.max_pitch), _share(r32, ch.max_roll)
    with np.errstate(all="ignore"):
        t = np.where(tp > tr, tp, tr)
        tl = np.where(~(t > 0), 0.0, np.where(t >= 100, 100.0, np.floor(np.where(t >= 100, 0.0, t))))
    tl = np.where(np.isnan(tl), 0.0, tl).astype(np.uint8)
    return np.where(status >= UNKNOWN_GROUND, np.uint8(0), tl).astype(np.uint8)


def volume(g, table, ch, cs, res):
    """g float64 [x, y]; table = (start, offsets); ch an attitude_ref.Chassis; cs float64 [H, 2] -> (status uint8 [H, x, y], tilt
    uint8 [H, x, y], counts int32 [8])"""
    g = np.asarray(g, np.float64)
    xy = g.shape[0]
    start, offsets = np.asarray(table[0], np.int64), np.asarray(table[1], np.int64)
    H = len(start) - 1
    cs = np.asarray(cs, np.float64)
    assert cs.shape == (H, 2)
    res = float(res)
    WO = wheel_offsets(ch, cs, res)
    wb, am = ch.front_axle - ch.rear_axle, 0.5 * (ch.front_axle + ch.rear_axle)
    X, Y = np.meshgrid(np.arange(xy), np.arange(xy), indexing="ij")
    status = np.zeros((H, xy, xy), np.uint8)
    tilt = np.zeros((H, xy, xy), np.uint8)
    with np.errstate(all="ignore"):
        for h in range(H):
            wheel_in = np.ones((xy, xy), bool)
            z = []
            for i in range(4):
                wx, wy = X + WO[h, i, 0], Y + WO[h, i, 1]
                inside = (wx >= 0) & (wx < xy) & (wy >= 0) & (wy < xy)
                wheel_in &= inside
                z.append(g[np.clip(wx, 0, xy - 1), np.clip(wy, 0, xy - 1)])
            z = [np.where(wheel_in, v, np.nan) for v in z]
            wheels_known = wheel_in & ar.known(z[0]) & ar.known(z[1]) & ar.known(z[2]) & ar.known(z[3])
            z = [np.where(wheels_known, v, 0.0) for v in z]
            zF, zR, zL, zT = 0.5 * (z[0] + z[1]), 0.5 * (z[2] + z[3]), 0.5 * (z[0] + z[2]), 0.5 * (z[1] + z[3])
            sp = (zF - zR) / wb
            sr = (zL - zT) / ch.track
            z0 = 0.25 * ((z[0] + z[1]) + (z[2] + z[3]))
            belly = np.full((xy, xy), np.inf)
            out = np.zeros((xy, xy), bool)
            c, s = cs[h]
            for dx, dy in offsets[start[h]:start[h + 1]].tolist():
                fx, fy = X + dx, Y + dy
                inside = (fx >= 0) & (fx < xy) & (fy >= 0) & (fy < xy)
                out |= ~inside
                gg = g[np.clip(fx, 0, xy - 1), np.clip(fy, 0, xy - 1)]
                use = inside & ar.known(gg) & wheels_known
                gg = np.where(use, gg, 0.0)
                du = ((float(dx) + 0.5) - 0.5) * res
                dv = ((float(dy) + 0.5) - 0.5) * res
                u = du * c + dv * s
                v = dv * c - du * s
                plane = (z0 + sp * (u - am)) + sr * v
                clr = (plane + ch.belly_height) - gg
                belly = np.where(use & (clr < belly), clr, belly)            # (a NaN clearance is skipped)
            p32, r32, b32 = sp.astype(np.float32), sr.astype(np.float32), belly.astype(np.float32)
            st = np.full((xy, xy), OK, np.uint8)
            st[b32 < ch.min_clearance] = BELLY
            st[np.abs(r32) > ch.max_roll] = ROLL
            st[np.abs(p32) > ch.max_pitch] = PITCH
            st[~wheels_known] = UNKNOWN_GROUND
            st[~wheel_in | out] = LEFT_WINDOW
            status[h] = st
            tilt[h] = tilt_of(p32, r32, ch, st)
    return status, tilt, counts_of(status)


def counts_of(status):
    """int32 [8]: the states per status code 0 .. 6, then H"""
    return np.concatenate([np.bincount(status.ravel(), minlength=7)[:7], [status.shape[0]]]).astype(np.int32)


def volume_loops(g, table, ch, cs, res):
    """the same, state by state and cell by cell over Python numbers (tiny inputs only); g a list of lists [x][y]"""
    xy = len(g)
    start, offsets = [int(v) for v in table[0]], [(int(a), int(b)) for a, b in table[1]]
    H = len(start) - 1
    res = float(res)
    half = ch.track / 2
    ab = ((ch.front_axle, half), (ch.front_axle, -half), (ch.rear_axle, half), (ch.rear_axle, -half))
    is_known = lambda v: v > -1000.0 and v < math.inf
    inside = lambda a: 0 <= a < xy
    am = 0.5 * (ch.front_axle + ch.rear_axle)

    def share(a32, limit):
        if not math.isfinite(float(limit)):
            return 0.0
        with np.errstate(all="ignore"):
            return float(np.float64(abs(float(a32))) / np.float64(float(limit)) * np.float64(100.0))
    status = np.zeros((H, xy, xy), np.uint8)
    tilt = np.zeros((H, xy, xy), np.uint8)
    for h in range(H):
        c, s = float(cs[h][0]), float(cs[h][1])
        wo = []
        for a_, b_ in ab:
            wx, wy = a_ * c - b_ * s, a_ * s + b_ * c
            wo.append((math.floor(0.5 + wx / res), math.floor(0.5 + wy / res)))
        for cx in range(xy):
            for cy in range(xy):
                left = False
                zs = []
                for ox, oy in wo:
                    if inside(cx + ox) and inside(cy + oy):
                        zs.append(float(g[cx + ox][cy + oy]))
                    else:
                        left = True
                cells = []
                for dx, dy in offsets[start[h]:start[h + 1]]:
                    if inside(cx + dx) and inside(cy + dy):
                        cells.append((dx, dy, float(g[cx + dx][cy + dy])))
                    else:
                        left = True
                if left:
                    status[h, cx, cy] = LEFT_WINDOW
                    continue
                if not all(is_known(v) for v in zs):
                    status[h, cx, cy] = UNKNOWN_GROUND
                    continue
                zFL, zFR, zRL, zRR = zs
                with np.errstate(all="ignore"):
                    zF, zR, zL, zT = 0.5 * (zFL + zFR), 0.5 * (zRL + zRR), 0.5 * (zFL + zRL), 0.5 * (zFR + zRR)
                    sp = float(np.float64(zF - zR) / np.float64(ch.front_axle - ch.rear_axle))
                    sr = float(np.float64(zL - zT) / np.float64(ch.track))
                    z0 = 0.25 * ((zFL + zFR) + (zRL + zRR))
                    belly = math.inf
                    for dx, dy, gg in cells:
                        if not is_known(gg):
                            continue
                        du = ((dx + 0.5) - 0.5) * res
                        dv = ((dy + 0.5) - 0.5) * res
                        u = du * c + dv * s
                        v = dv * c - du * s
                        plane = (z0 + sp * (u - am)) + sr * v
                        clr = (plane + ch.belly_height) - gg
                        if clr < belly:
                            belly = clr
                    p32, r32, b32 = np.float32(sp), np.float32(sr), np.float32(belly)
                if abs(p32) > ch.max_pitch:
                    st = PITCH
                elif abs(r32) > ch.max_roll:
                    st = ROLL
                elif b32 < ch.min_clearance:
                    st = BELLY
                else:
                    st = OK
                status[h, cx, cy] = st
                tp, tr = share(p32, ch.max_pitch), share(r32, ch.max_roll)
                t = tp if tp > tr else tr
                tilt[h, cx, cy] = 0 if not t > 0 else (100 if t >= 100 else int(math.floor(t)))
    return status, tilt, counts_of(status)


def centre_poses(xy, H, res, origin_cells):
    """float32 [H * xy, xy, 3]: the pose at the centre (o + c + 0.5) * res of every window cell with yaw h * 2 pi / H; rollout h * xy + x,
    pose y.  AssertionError where a centre is no float32 number"""
    x, y = np.meshgrid(np.arange(xy, dtype=np.float64), np.arange(xy, dtype=np.float64), indexing="ij")
    wx, wy = (origin_cells[0] + x + 0.5) * res, (origin_cells[1] + y + 0.5) * res
    p = np.zeros((H, xy, xy, 3), np.float32)
    p[..., 0], p[..., 1] = wx[None], wy[None]
    assert np.array_equal(p[0, ..., 0].astype(np.float64), wx) and np.array_equal(p[0, ..., 1].astype(np.float64), wy), "a cell centre is no float32 number"
    p[..., 2] = (np.arange(H, dtype=np.float64) * (2.0 * np.pi) / H).astype(np.float32)[:, None, None]
    return p.reshape(H * xy, xy, 3)


def wheel_rules_agree(ch, cs, res, xy, origin_cells):
    """the number of (heading, wheel, axis, cell) at which the window-relative wheel-cell rule and the pose rule of terrain attitude
    scoring at the cell centres differ"""
    W = ar.wheel_table(ch, cs)
    WO = wheel_offsets(ch, cs, res)
    bad = 0
    for j in range(2):
        c = np.arange(xy, dtype=np.float64)
        centre = ((origin_cells[j] + c + 0.5) * res).astype(np.float32).astype(np.float64)
        for h in range(len(cs)):
            for i in range(4):
                pose_rule = np.floor((centre + W[h, i, j]) / res).astype(np.int64) - int(origin_cells[j])
                bad += int((pose_rule != np.arange(xy) + WO[h, i, j]).sum())
    return bad


def masked_cost(C, status, tilt, block_mask, tilt_weight):
    """C' uint16 [H, x, y]: 0 where C == 0 or bit `status` of block_mask is set, min(65535, C + tilt_weight * tilt) elsewhere"""
    C = np.asarray(C).astype(np.int64)
    blocked = (C == 0) | (((int(block_mask) >> status.astype(np.int64)) & 1) != 0)
    return np.where(blocked, 0, np.minimum(65535, C + int(tilt_weight) * tilt.astype(np.int64))).astype(np.uint16)


def mask_of(blocks):
    m = 0
    for b in blocks:
        m |= 1 << int(b)
    return m


def field(c, footprint, table, goals, status, tilt, block_mask, tilt_weight, max_cost=None):
    """posefield_ref.field() with the attitude volume taken into the pose cost: (C', D, action, seeds, (reached, seeded))"""
    C = masked_cost(pf.volume(c, footprint), status, tilt, block_mask, tilt_weight)
    seeds = pf.seed_mask(C, goals)
    D = pf.relax(C, table, seeds, max_cost)
    return C, D, pf.actions(C, table, D, seeds), seeds, (int((D < pf.UNREACHED).sum()), int(seeds.sum()))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _case(xy, M, H, pattern, seed, device):
    res = RES[xy]
    oc = (0, 0)
    table = rr.patch_table(H, M, seed=seed) if M > 1 else pf.point_footprint(H)
    return dict(name="xy%d M%d H%d %s" % (xy, M, H, pattern), xy=xy, res=res, H=H, M=M, pattern=pattern, table=table,
                g=ar.ground_map(xy, pattern, res, oc, seed), chassis=ar.case_chassis(res, True), cos_sin=ar.cos_sin(H), device=device)


@functools.lru_cache(maxsize=None)
def cases(xy):
    """the synthetic inputs of one window side: every footprint size, the grounds and the headings in rotation (over the six sides every
    footprint meets every ground, and every heading count every ground)"""
    i = SIZES.index(xy)
    return tuple(_case(xy, M, HEADINGS[(i + 2 * j) % 3], GROUNDS[(i + j) % 5], 10 * i + j, (i + j) % 2 == 1) for j, M in enumerate(CELLS))


def score_case(q):
    return volume(q["g"], q["table"], q["chassis"], q["cos_sin"], q["res"])


@functools.lru_cache(maxsize=None)
def expected(xy):
    """volume() of every case of cases(xy), computed once"""
    return tuple(score_case(q) for q in cases(xy))


def side_slope(xy, res, slope, base=0.5):
    """float64 [x, y]: a plane tilted across y, z = base + slope * (y + 0.5) * res"""
    j = np.arange(xy, dtype=np.float64)
    return np.tile(base + slope * ((j + 0.5) * res), (xy, 1))
