"""The numpy referee of body volumes (include/gvom_hip.h "body volumes"; gvom_body_volume, k_volume_body, gvom_pose_field_volumes) and
the inputs of tests/test_body_volume.py and tests/test_body_volume_cpu.py.

volume() is the definition, vectorised over the cells of one heading, every float64 operation one numpy operation in the header's
order.  It is put together from the pieces of the two referees the definition refers to word for word: the wheels stand where attitude
volumes put them (attitude_volume_ref.wheel_offsets), the frame, the sphere centres and their voxels are body clearance scoring's
(body_ref.frame / centres / voxels); the pose is the cell's centre ((o + c) + 0.5) * res.  squeeze_of() is the SQUEEZE rule.
volume_loops() says the same a second time as plain Python loops over Python numbers; the CPU test holds the two together, and both
against body_ref.score() at the cell-centre poses.  masked_cost2() takes a body volume into a pose cost volume; field() is the
pose-field referee of tests/posefield_ref.py behind attitude_volume_ref.masked_cost and masked_cost2.  Tolerance 0; floats by bit pattern.

cases() are the GPU test's synthetic inputs (each also scored here, once, by expected())."""
import functools
import math

import numpy as np

import attitude_ref as ar
import attitude_volume_ref as avr
import body_ref as br
import posefield_ref as pf

OK, COLLISION, LEFT_BOX, UNKNOWN_GROUND, LEFT_WINDOW, INVALID = range(6)
GRIDS = br.GRIDS
HEADINGS = (1, 7, 16)
SPHERES = (1, 64, 65, 256)
GROUNDS = ar.GROUNDS


# ---- the definition, vectorised -------------------------------------------------------------------------------------------------------
def squeeze_of(clr, status, min_margin, soft_margin):
    """uint8 squeeze of float32 clearances (an array) and their statuses under the float32 margins m <= f"""
    k = np.asarray(clr, np.float32)
    m, f = np.float32(min_margin), np.float32(soft_margin)
    with np.errstate(all="ignore"):
        t = (np.float64(f) - k.astype(np.float64)) / (np.float64(f) - np.float64(m)) * 100.0
        band = np.where(~(t > 0), 0.0, np.where(t >= 100, 100.0, np.floor(np.where(t >= 100, 0.0, t))))
    band = np.where(np.isnan(band), 0.0, band)
    sq = np.where(k >= f, 0.0, np.where((k <= m) | (f == m), 100.0, band))
    return np.where(np.asarray(status) >= LEFT_BOX, 0, sq).astype(np.uint8)


def counts_of(status, S):
    """int32 [8]: the states per status code 0 .. 5, then H and S"""
    return np.concatenate([np.bincount(status.ravel(), minlength=6)[:6], [status.shape[0], S]]).astype(np.int32)


def volume(field, B, g, body, ch, cs, res, zres, origin_cells, min_margin, soft_margin, tilt=True):
    """field float32 [n, n, zs] with its corner at world voxel B; g float64 [x, y]; body float32 [S, 4]; ch a Chassis (attitude_ref);
    cs float64 [H, 2] -> (status uint8 [H, x, y], squeeze uint8 [H, x, y], clearance float32 [H, x, y], counts int32 [8]).
    tilt=False: the untilted frame (sp = sr = 0, the same z0), for the census."""
    field = np.asarray(field, np.float32)
    n, zs = field.shape[0], field.shape[2]
    body = np.asarray(body, np.float32)
    g = np.asarray(g, np.float64)
    xy = g.shape[0]
    cs = np.asarray(cs, np.float64)
    H = len(cs)
    res = float(res)
    WO = avr.wheel_offsets(ch, cs, res)
    wb, am = ch.front_axle - ch.rear_axle, 0.5 * (ch.front_axle + ch.rear_axle)
    CX, CY = np.meshgrid(np.arange(xy), np.arange(xy), indexing="ij")
    X0 = ((int(origin_cells[0]) + CX).astype(np.float64) + 0.5) * res
    Y0 = ((int(origin_cells[1]) + CY).astype(np.float64) + 0.5) * res
    status = np.zeros((H, xy, xy), np.uint8)
    clearance = np.zeros((H, xy, xy), np.float32)
    with np.errstate(all="ignore"):
        for h in range(H):
            wheel_in = np.ones((xy, xy), bool)
            z = []
            for i in range(4):
                wx, wy = CX + WO[h, i, 0], CY + WO[h, i, 1]
                wheel_in &= (wx >= 0) & (wx < xy) & (wy >= 0) & (wy < xy)
                z.append(g[np.clip(wx, 0, xy - 1), np.clip(wy, 0, xy - 1)])
            z = [np.where(wheel_in, v, np.nan) for v in z]
            wheels_known = wheel_in & ar.known(z[0]) & ar.known(z[1]) & ar.known(z[2]) & ar.known(z[3])
            z = [np.where(wheels_known, v, 0.0) for v in z]
            zF, zR, zL, zT = 0.5 * (z[0] + z[1]), 0.5 * (z[2] + z[3]), 0.5 * (z[0] + z[2]), 0.5 * (z[1] + z[3])
            sp = (zF - zR) / wb
            sr = (zL - zT) / ch.track
            z0 = 0.25 * ((z[0] + z[1]) + (z[2] + z[3]))
            if not tilt:
                sp, sr = np.zeros_like(sp), np.zeros_like(sr)
            fr = br.frame(sp, sr, z0, am)
            X, Y, Z = br.centres(X0, Y0, np.full((xy, xy), cs[h, 0]), np.full((xy, xy), cs[h, 1]), fr, body)
            vx, vy, vz, inside = br.voxels(X, Y, Z, res, zres, B, n, zs)
            d = field[vx, vy, vz]
            m = (d - body[:, 3]).astype(np.float32)                          # one float32 subtraction
            live = inside & ~np.isnan(m)
            clr = np.where(live, m, np.float32(np.inf)).min(axis=2)
            st = np.where(clr < np.float32(min_margin), COLLISION, OK)
            st[~inside.all(axis=2)] = LEFT_BOX
            st[~wheels_known] = UNKNOWN_GROUND
            st[~wheel_in] = LEFT_WINDOW
            status[h] = st
            clearance[h] = np.where(st >= LEFT_BOX, np.float32(0), clr)
    return status, squeeze_of(clearance, status, min_margin, soft_margin), clearance, counts_of(status, len(body))


def volume_loops(field, B, g, body, ch, cs, res, zres, origin_cells, min_margin, soft_margin):
    """the same, state by state and sphere by sphere over Python numbers; field [x][y][z] and g [x][y] nested lists"""
    n, zs, xy = len(field), len(field[0][0]), len(g)
    H = len(cs)
    res, zres = float(res), float(zres)
    half = ch.track / 2
    ab = ((ch.front_axle, half), (ch.front_axle, -half), (ch.rear_axle, half), (ch.rear_axle, -half))
    am = 0.5 * (ch.front_axle + ch.rear_axle)
    wb, track = float(ch.front_axle - ch.rear_axle), float(ch.track)
    is_known = lambda v: v > -1000.0 and v < math.inf
    m32, f32 = np.float32(min_margin), np.float32(soft_margin)
    spheres = [(float(np.float32(b[0])), float(np.float32(b[1])), float(np.float32(b[2])), np.float32(b[3])) for b in body]
    f32s = [[[np.float32(v) for v in col] for col in plane] for plane in field]
    inf32 = np.float32(np.inf)

    def cell(v, r, o, size):
        q = v / r
        if not abs(q) < 2.0 ** 30:
            return None
        c = math.floor(q) - int(o)
        return c if 0 <= c < size else None

    def squeeze(k):
        if k >= f32:
            return 0
        if k <= m32 or f32 == m32:
            return 100
        t = (float(f32) - float(k)) / (float(f32) - float(m32)) * 100.0
        return 0 if not t > 0 else (100 if t >= 100 else int(math.floor(t)))
    status = np.zeros((H, xy, xy), np.uint8)
    sq = np.zeros((H, xy, xy), np.uint8)
    clearance = np.zeros((H, xy, xy), np.float32)
    with np.errstate(all="ignore"):
        for h in range(H):
            c, s = float(cs[h][0]), float(cs[h][1])
            wo = [(math.floor(0.5 + (a_ * c - b_ * s) / res), math.floor(0.5 + (a_ * s + b_ * c) / res)) for a_, b_ in ab]
            for cx in range(xy):
                for cy in range(xy):
                    if not all(0 <= cx + ox < xy and 0 <= cy + oy < xy for ox, oy in wo):
                        status[h, cx, cy] = LEFT_WINDOW
                        continue
                    zFL, zFR, zRL, zRR = (float(g[cx + ox][cy + oy]) for ox, oy in wo)
                    if not (is_known(zFL) and is_known(zFR) and is_known(zRL) and is_known(zRR)):
                        status[h, cx, cy] = UNKNOWN_GROUND
                        continue
                    zF, zR, zL, zT = 0.5 * (zFL + zFR), 0.5 * (zRL + zRR), 0.5 * (zFL + zRL), 0.5 * (zFR + zRR)
                    sp = (zF - zR) / wb
                    sr = (zL - zT) / track
                    z0 = 0.25 * ((zFL + zFR) + (zRL + zRR))
                    lu = math.sqrt(1.0 + sp * sp)
                    ln = math.sqrt((1.0 + sp * sp) + sr * sr)
                    e1u, e1w = 1.0 / lu, sp / lu
                    nu, nv, nw = -sp / ln, -sr / ln, 1.0 / ln
                    e2u, e2v, e2w = nv * e1w, nw * e1u - nu * e1w, -(nv * e1u)
                    q0 = z0 - sp * am
                    x0 = (float(int(origin_cells[0]) + cx) + 0.5) * res
                    y0 = (float(int(origin_cells[1]) + cy) + 0.5) * res
                    clr, seen, out = inf32, False, False
                    for bx, by, bz, r in spheres:
                        Cu = (bx * e1u + by * e2u) + bz * nu
                        Cv = by * e2v + bz * nv
                        Cw = ((bx * e1w + by * e2w) + bz * nw) + q0
                        X = x0 + (Cu * c - Cv * s)
                        Y = y0 + (Cu * s + Cv * c)
                        vx, vy, vz = cell(X, res, B[0], n), cell(Y, res, B[1], n), cell(Cw, zres, B[2], zs)
                        if vx is None or vy is None or vz is None:
                            out = True
                            break                                            # (LEFT_BOX whatever the other spheres read)
                        m = f32s[vx][vy][vz] - r
                        if m != m:
                            continue
                        if not seen or m < clr:
                            clr, seen = m, True
                    if out:
                        status[h, cx, cy] = LEFT_BOX
                        continue
                    status[h, cx, cy] = COLLISION if clr < m32 else OK
                    clearance[h, cx, cy] = clr
                    sq[h, cx, cy] = squeeze(clr)
    return status, sq, clearance, counts_of(status, len(body))


def masked_cost2(C, status, squeeze, block_mask, squeeze_weight):
    """C'' uint16 [H, x, y]: 0 where C' == 0 or bit `status` of block_mask is set, min(65535, C' + squeeze_weight * squeeze) elsewhere
    -- attitude volumes' elementwise rule on a body volume's two uint8 parts"""
    return avr.masked_cost(C, status, squeeze, block_mask, squeeze_weight)


def field(c, footprint, table, goals, attitude=None, body=None, max_cost=None):
    """posefield_ref.field() with the volumes taken into the pose cost, the attitude volume first: attitude = (status, tilt, block_mask,
    tilt_weight) or None, body = (status, squeeze, block_mask, squeeze_weight) or None -> (C'', D, action, seeds, (reached, seeded))"""
    C = pf.volume(c, footprint)
    if attitude is not None:
        C = avr.masked_cost(C, *attitude)
    if body is not None:
        C = masked_cost2(C, *body)
    seeds = pf.seed_mask(C, goals)
    D = pf.relax(C, table, seeds, max_cost)
    return C, D, pf.actions(C, table, D, seeds), seeds, (int((D < pf.UNREACHED).sum()), int(seeds.sum()))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _case(xy, H, S, pattern, seed, device, min_margin, band, nan=False):
    q = br._case("xy%d H%d S%d %s" % (xy, H, S, pattern), xy, pattern, H, S, 1, 1, seed, device, min_margin, nan=nan)
    q["soft_margin"] = np.float32(np.float32(min_margin) + np.float32(band))
    return q


@functools.lru_cache(maxsize=None)
def cases():
    """the synthetic inputs: the three grids (33 and 40 leave partial tiles and partial waves on both axes), H of 1, 7 and 16, S of 1,
    64, 65 and 256, the five grounds, both routes, soft_margin == min_margin and above it; the last: a field with NaN entries"""
    return (_case(16, 16, 65, "flat", 1, False, 0.0, 0.4),
            _case(33, 7, 64, "plane", 2, True, -0.02, 0.3),
            _case(40, 1, 256, "steps", 3, False, -0.03, 0.25),
            _case(16, 7, 256, "random", 4, True, -0.02, 0.0),
            _case(40, 16, 1, "random", 5, False, 0.3, 0.6),
            _case(33, 1, 65, "unknown", 6, True, -0.1, 0.5),
            _case(40, 7, 2, "plane", 8, True, 0.2, 0.7),
            _case(33, 7, 2, "plane", 71, True, 0.0, 0.35, nan=True))


def score_case(q, **kw):
    return volume(q["field"], q["field_origin"], q["g"], q["body"], q["chassis"], q["cos_sin"], q["res"], q["zres"], q["origin_cells"],
                  q["min_margin"], q["soft_margin"], **kw)


@functools.lru_cache(maxsize=None)
def expected():
    """volume() of every case of cases(), computed once"""
    return tuple(score_case(q) for q in cases())


def census(inputs):
    """what a list of (case, (status, squeeze, clearance, counts)) reaches, as counters"""
    n = dict(status=[0] * 6, finite=0, inf=0, tilt_status=0, squeeze_between=0, squeeze_0=0, squeeze_100=0, nan_read=0)
    for q, (status, sq, clr, counts) in inputs:
        for s in range(6):
            n["status"][s] += int((status == s).sum())
        live = status <= COLLISION
        n["finite"] += int((live & np.isfinite(clr)).sum())
        n["inf"] += int((live & (clr == np.inf)).sum())
        n["squeeze_between"] += int((live & (sq > 0) & (sq < 100)).sum())
        n["squeeze_0"] += int((live & (sq == 0)).sum())
        n["squeeze_100"] += int((live & (sq == 100)).sum())
        flat = score_case(q, tilt=False)[0]
        n["tilt_status"] += int(((status <= LEFT_BOX) & (flat <= LEFT_BOX) & (status != flat)).sum())
        n["nan_read"] += int(np.isnan(q["field"]).any())
    return n
