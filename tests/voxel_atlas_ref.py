"""Referee of the voxel atlas (include/gvom_hip.h "voxel atlas"): pure numpy, NOT toroidal -- the extent is a plain uint8 array of class
codes indexed [z - Ez, y - Ey, x - Ex]; a move allocates a NEVER extent and copies the overlap.  It applies the definition literally: the
class of a fused state, the move, the merge, the eleven counts, the box, and -- on dense_state() -- the ray walk and the viewpoint
product.  It is fed with dense fused states in the reference's voxel order (x + y * xy + z * xy * xy: Gvom.read_dense(GVOM_WHICH_FUSED),
or the CPU referee's combined_index_map) and their window origins: it referees the atlas, not the mapper.

walk() is tests/raycast_ref.py's walk restated with explicit sizes (A, A, Z) -- that one indexes its sizes by grid name --;
tests/test_voxel_atlas_cpu.py holds the two equal on window-sized extents, so this one cannot drift from the one that is pinned to the
CPU referee of the whole pipeline.  Also here: the climbing drive and the ray and pose sets that the CPU census and the GPU tests share."""
import functools
import math

import numpy as np

import atlas_ref
import raycast_ref as rr
import viewpoint_ref as vr

F32 = np.float32
NEVER, FREE, OCCUPIED = 0, 1, 2
CLEAR, HIT, UNKNOWN, LEFT, INVALID = rr.CLEAR, rr.OCCUPIED, rr.UNKNOWN, rr.LEFT_WINDOW, rr.INVALID
COUNT_NAMES = ("first_seen", "free_to_occupied", "occupied_to_free", "confirmed", "uninformative", "outside", "cleared", "cleared_observed",
               "observed", "occupied", "seq")


def classes(state):
    """CLASS of a fused state: s >= 0 OCCUPIED, s == -1 NEVER, otherwise FREE"""
    s = np.asarray(state)
    return np.where(s >= 0, OCCUPIED, np.where(s == -1, NEVER, FREE)).astype(np.uint8)


class VoxelAtlasRef(object):
    def __init__(self, cells, levels, xy, zs, follow=True, origin=(0, 0, 0)):
        A, Z = int(cells), int(levels)
        assert 64 <= A <= 4096 and A & (A - 1) == 0 and A >= xy and Z & (Z - 1) == 0 and zs <= Z <= A and A * A * Z <= 1 << 32
        self.A, self.Z, self.xy, self.zs, self.follow = A, Z, int(xy), int(zs), bool(follow)
        self.E = tuple(int(v) for v in origin)
        self.cls = np.zeros((Z, A, A), np.uint8)
        self.seq = 0
        self.last = dict.fromkeys(COUNT_NAMES[:8], 0)
        self.last_origin = None
        self.total = dict.fromkeys(COUNT_NAMES[:8], 0)         # the counts summed over every integrate: the census

    def sizes(self):
        return (self.A, self.A, self.Z)

    def _overlap(self, origin, shape):
        """the part of a box of `shape` (x, y, z) at `origin` that lies in the extent: (box slices, extent slices), both [z, y, x], or None"""
        b, e = [], []
        for k in (2, 1, 0):
            r = int(origin[k]) - self.E[k]
            lo, hi = max(r, 0), min(r + shape[k], self.sizes()[k])
            if lo >= hi:
                return None
            b.append(slice(lo - r, hi - r)); e.append(slice(lo, hi))
        return tuple(b), tuple(e)

    def move(self, to):
        """the extent goes to `to`; every voxel of the new extent that was not in the old one becomes NEVER.  Returns (voxels made
        NEVER, of those how many were observed): as many voxels entered as left, and what left is what its storage knew."""
        old, size = self.cls, self.sizes()
        d = [int(to[k]) - self.E[k] for k in range(3)]
        self.cls = np.zeros_like(old)
        stayed = np.zeros(old.shape, bool)
        if all(abs(d[k]) < size[k] for k in range(3)):
            src = tuple(slice(max(d[k], 0), size[k] + min(d[k], 0)) for k in (2, 1, 0))
            dst = tuple(slice(max(-d[k], 0), size[k] + min(-d[k], 0)) for k in (2, 1, 0))
            self.cls[dst] = old[src]
            stayed[src] = True
        self.E = tuple(int(v) for v in to)
        return int(old.size - stayed.sum()), int((old[~stayed] != NEVER).sum())

    def integrate(self, state, W):
        """state: the dense fused state of the window whose origin is W (three integers).  Returns the counts of this integrate."""
        xy, zs = self.xy, self.zs
        c = classes(state).reshape(zs, xy, xy)
        W = tuple(int(v) for v in W)
        assert all(abs(v) < 1 << 30 for v in W)
        cleared = cleared_observed = 0
        if self.follow:
            to = (W[0] + xy // 2 - self.A // 2, W[1] + xy // 2 - self.A // 2, W[2] + zs // 2 - self.Z // 2)
            cleared, cleared_observed = self.move(to)
        self.seq += 1
        n = dict.fromkeys(COUNT_NAMES[:8], 0)
        ov = self._overlap(W, (xy, xy, zs))
        inside = 0
        if ov is not None:
            b, e = ov
            new, old = c[b], self.cls[e]
            inside = new.size
            n["first_seen"] = int(((new != NEVER) & (old == NEVER)).sum())
            n["free_to_occupied"] = int(((new == OCCUPIED) & (old == FREE)).sum())
            n["occupied_to_free"] = int(((new == FREE) & (old == OCCUPIED)).sum())
            n["confirmed"] = int(((new != NEVER) & (new == old)).sum())
            n["uninformative"] = int((new == NEVER).sum())
            self.cls[e] = np.where(new == NEVER, old, new)
        n["outside"] = xy * xy * zs - inside
        n["cleared"], n["cleared_observed"] = cleared, cleared_observed
        assert sum(n[k] for k in COUNT_NAMES[:6]) == xy * xy * zs
        for k in n:
            self.total[k] += n[k]
        self.last, self.last_origin = n, W
        return dict(n)

    def counts(self):
        out = dict(self.last)
        out["observed"], out["occupied"], out["seq"] = int((self.cls != NEVER).sum()), int((self.cls == OCCUPIED).sum()), self.seq
        return out

    def box(self, origin=None):
        """(classes uint8 [xy, xy, z] indexed [x, y, z], counts int32 [4] {occupied, free, outside the extent, seq})"""
        origin = self.last_origin if origin is None else tuple(int(v) for v in origin)
        out = np.zeros((self.zs, self.xy, self.xy), np.uint8)
        ov = self._overlap(origin, (self.xy, self.xy, self.zs))
        inside = 0
        if ov is not None:
            b, e = ov
            out[b] = self.cls[e]
            inside = out[b].size
        counts = np.array([(out == OCCUPIED).sum(), (out == FREE).sum(), out.size - inside, self.seq], np.int32)
        return np.ascontiguousarray(out.transpose(2, 1, 0)), counts

    def dense_state(self):
        """the extent as a state array in the reference's voxel order over (A, A, Z): 0 occupied, -2 free, -1 never observed"""
        return np.where(self.cls == OCCUPIED, 0, np.where(self.cls == FREE, -2, -1)).astype(np.int32).reshape(-1)

    def world_class(self, voxels):
        """the class of world voxels int [n, 3]; NEVER outside the extent"""
        v = np.asarray(voxels, np.int64) - np.array(self.E, np.int64)
        ok = ((v >= 0) & (v < np.array(self.sizes()))).all(axis=1)
        out = np.zeros(len(v), np.uint8)
        out[ok] = self.cls[v[ok, 2], v[ok, 1], v[ok, 0]]
        return out

    def clear(self):
        self.cls[:] = NEVER
        self.last = dict.fromkeys(self.last, 0)


# ---- the walk with explicit sizes ----------------------------------------------------------------------------------------------------------
def setup(res, cap, a, b, f32_sqrt=False):
    """(p, inc, S) of the rays a -> b (float32 [n, 3], metres): tests/raycast_ref.py setup with the resolutions res (x, y, z) and the
    step cap given (sizes A + Z + 1)"""
    res = np.asarray(res, np.float64)
    with np.errstate(all="ignore"):
        p = (a.astype(np.float64) / res).astype(F32)                       # gvom.py:1097-1099
        e = (b.astype(np.float64) / res).astype(F32)                       # :1101-1103
        s = e - p                                                          # :1105-1107 (float32)
        ss = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]   # :1110, float32, left to right
        assert ss.dtype == F32
        ray_length = np.sqrt(ss).astype(np.float64) if f32_sqrt else np.sqrt(ss.astype(np.float64))
        s = (s.astype(np.float64) / ray_length[:, None]).astype(F32)       # :1112-1114
        ab = np.abs(s)
        inner = np.where(ab[:, 2] > ab[:, 1], ab[:, 2], ab[:, 1])          # Python's max(a, b): b if b > a else a
        smax = np.where(inner > ab[:, 0], inner, ab[:, 0])                 # :1116
        si = np.zeros(len(a), np.int64)
        si[smax == ab[:, 1]] = 1
        si[smax == ab[:, 2]] = 2                                           # ties: z over y over x
        sd = s[np.arange(len(a)), si]
        inc = s / np.abs(sd)[:, None]                                      # :1126, 1129-1132: float32 / float32
        assert inc.dtype == F32
        step_len = np.abs(1.0 / sd.astype(np.float64))                     # :1150
        lim = ray_length - 1.0
        S = np.zeros(len(a), np.int64)
        length = np.zeros(len(a), np.float64)
        for _ in range(cap):
            go = length < lim                                              # :1127
            if not go.any():
                break
            S[go] += 1
            length = np.where(go, length + step_len, length)
    return p, inc, S


def walk(state, E, sizes, res, a, b, unknown_blocks=False, check_target=False, f32_sqrt=False, record=False):
    """result int32 [n, 3] {status, steps, unknown}, position float32 [n, 3], voxel int32 [n, 3] (the WORLD voxel of the stop, (0, 0, 0)
    where there is none) -- and, with record, the list of (ray, extent voxel index x + y * A + z * A * A) pairs examined, in step order --
    of the rays a[i] -> b[i] through the dense `state` of an extent of `sizes` (A, A, Z) voxels whose corner is world voxel E."""
    A, A2, Z = (int(v) for v in sizes)
    assert A == A2
    res = np.asarray(res, np.float64)
    a = np.ascontiguousarray(a, F32).reshape(-1, 3)
    b = np.ascontiguousarray(b, F32).reshape(-1, 3)
    n = len(b)
    if len(a) == 1 and n > 1:
        a = np.repeat(a, n, axis=0)
    E = np.asarray(E, np.float64)
    size = np.array([A, A, Z], np.float64)
    result = np.zeros((n, 3), np.int32)
    voxel = np.zeros((n, 3), np.int32)
    position = np.full((n, 3), np.nan, F32)
    finite = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1)
    result[~finite, 0] = INVALID
    p, inc, S = setup(res, A + Z + 1, a, b, f32_sqrt)
    run = finite.copy()
    unknown = np.zeros(n, np.int64)
    visits = []

    def examine(who, v, steps, pos):
        vi = v.astype(np.int64)
        vox = vi[:, 0] + vi[:, 1] * A + vi[:, 2] * A * A
        if record:
            visits.extend(zip(who.tolist(), vox.tolist()))
        s = state[vox]
        unk = s == -1
        unknown[who[unk]] += 1
        stop = (s >= 0) | (unk & bool(unknown_blocks))
        w = who[stop]
        result[w, 0] = np.where(s[stop] >= 0, HIT, UNKNOWN)
        result[w, 1] = steps[stop]
        voxel[w] = (vi[stop] + E.astype(np.int64)).astype(np.int32)
        position[w] = pos[stop]
        run[w] = False

    with np.errstate(all="ignore"):
        j = 0
        while (run & (S > j)).any():
            j += 1
            p = p + inc                                                    # every ray: three float32 additions
            assert p.dtype == F32
            who = np.flatnonzero(run & (S >= j))
            v = np.floor(p[who].astype(np.float64) - E)
            inside = ((v >= 0) & (v < size)).all(axis=1)                   # NaN compares false: outside
            out = who[~inside]
            result[out, 0] = LEFT
            result[out, 1] = j - 1
            run[out] = False
            who, v = who[inside], v[inside]
            examine(who, v, np.full(len(who), j), (p[who].astype(np.float64) * res).astype(F32))
        who = np.flatnonzero(run)
        result[who, 0] = CLEAR
        result[who, 1] = S[who]
        if check_target and len(who):
            v = np.floor(b[who].astype(np.float64) / res - E)              # gvom.py:1072-1080
            inside = ((v >= 0) & (v < size)).all(axis=1)
            result[who[~inside], 0] = LEFT
            run[who[~inside]] = False
            who, v = who[inside], v[inside]
            examine(who, v, S[who] + 1, b[who])
    result[:, 2] = np.where(finite, unknown, 0)
    return (result, position, voxel, visits) if record else (result, position, voxel)


def atlas_walk(ref, res, a, b, **kw):
    """walk() on a VoxelAtlasRef"""
    return walk(ref.dense_state(), ref.E, ref.sizes(), res, a, b, **kw)


# ---- the viewpoint product, from viewpoint_ref's pieces on that walk ---------------------------------------------------------------------------
def _origin_status(state, E, sizes, res, a):
    A, _, Z = sizes
    with np.errstate(all="ignore"):
        v = np.floor(a.astype(np.float64) / np.asarray(res, np.float64) - np.asarray(E, np.float64))
    if not ((v >= 0) & (v < np.array([A, A, Z]))).all():
        return LEFT
    s = state[int(v[0]) + int(v[1]) * A + int(v[2]) * A * A]
    return HIT if s >= 0 else (UNKNOWN if s == -1 else CLEAR)


def viewpoints(state, E, sizes, res, directions, offsets, poses, max_range, strides=(1, 1), unknown_blocks=False, f32_sqrt=False):
    """(rows int32 [K, 8], best int32 [4]): parts 0 and 1 of the product, as tests/viewpoint_ref.py product on an extent"""
    H, Wm = np.asarray(directions).shape[:2]
    nb = len(vr.selected(H, Wm, strides)[0])
    rows = []
    for pose in vr.rows34(poses):
        row = np.zeros(8, np.int64)
        if not np.isfinite(pose).all():
            row[0], row[7] = INVALID, nb
            rows.append(row)
            continue
        a, b = vr.targets(directions, offsets, pose, max_range, strides)
        result, _, _, visits = walk(state, E, sizes, res, a[None], b, unknown_blocks=unknown_blocks, f32_sqrt=f32_sqrt, record=True)
        row[0] = _origin_status(state, E, sizes, res, a)
        v = np.asarray(visits, np.int64).reshape(-1, 2)
        unknown = v[state[v[:, 1]] == -1, 1]
        row[1] = len(np.unique(unknown))
        row[2] = result[:, 2].sum()
        for col, code in ((3, HIT), (4, CLEAR), (5, LEFT), (6, UNKNOWN), (7, INVALID)):
            row[col] = (result[:, 0] == code).sum()
        assert row[3:].sum() == nb and row[2] == len(unknown)
        rows.append(row)
    rows = np.stack(rows).astype(np.int32)
    return rows, vr.best_of(rows, nb)


# ---- the climbing drive ----------------------------------------------------------------------------------------------------------------------
DRIVE_XY, DRIVE_ZS, DRIVE_A, DRIVE_Z = atlas_ref.DRIVE_XY, 8, atlas_ref.DRIVE_A, 16
DRIVE_RES = (atlas_ref.DRIVE_RES, atlas_ref.DRIVE_RES, atlas_ref.DRIVE_ZRES)
DRIVE_PARAMS = (atlas_ref.DRIVE_RES, atlas_ref.DRIVE_ZRES, DRIVE_XY, DRIVE_ZS)      # + (ring slots,) + the tail below
DRIVE_TAIL = (1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)


@functools.lru_cache(maxsize=None)
def drive_scans():
    """((cloud, ego), ...): tests/atlas_ref.py's drive (17 scans out and back) with the ego additionally climbing one z level per leg on
    the way out and descending on the way back, so that the extent's Ez moves"""
    scans = atlas_ref.drive_scans()
    legs = atlas_ref.DRIVE_LEGS
    out = []
    for k, (pc, ego) in enumerate(scans):
        leg = k if k <= legs else 2 * legs - k
        out.append((pc, (ego[0], ego[1], float(F32(ego[2] + atlas_ref.DRIVE_ZRES * leg)))))
    return tuple(out)


def window_origin(ego):
    return tuple(int(math.floor(ego[k] / DRIVE_RES[k] - (DRIVE_XY, DRIVE_XY, DRIVE_ZS)[k] / 2)) for k in range(3))


def fixed_origin():
    """the extent of the fixed-mode run of the drive: around its start, so that windows lie inside it, across its edge and outside it"""
    W = window_origin(drive_scans()[0][1])
    return (W[0] - 20, W[1] - 70, W[2] - 3)


def box_origins(ref, first):
    """where the tests take boxes after an integrate: the current window, the first window, half outside the extent, wholly outside it"""
    E = ref.E
    return [ref.last_origin, first, (E[0] + ref.A - ref.xy // 2, E[1] - ref.xy // 2, E[2] + ref.Z - ref.zs // 2), (E[0] + ref.A + 7, E[1] - 2 * ref.xy, E[2])]


def centres(voxels):
    """the centres of world voxels int [n, 3], metres float64"""
    return (np.asarray(voxels, np.float64) + 0.5) * np.array(DRIVE_RES)


def remembered_outside(ref, W, cls):
    """world voxels int64 [n, 3] of class `cls` that the atlas holds OUTSIDE the window at W, in index order"""
    z, y, x = np.nonzero(ref.cls == cls)
    v = np.stack([x, y, z], axis=1).astype(np.int64) + np.array(ref.E, np.int64)
    w = v - np.array(W, np.int64)
    inside = ((w >= 0) & (w < np.array([ref.xy, ref.xy, ref.zs]))).all(axis=1)
    return v[~inside]


def in_window(ref, W, cls):
    """world voxels int64 [n, 3] of class `cls` that the atlas holds INSIDE the window at W, in index order"""
    z, y, x = np.nonzero(ref.cls == cls)
    v = np.stack([x, y, z], axis=1).astype(np.int64) + np.array(ref.E, np.int64)
    w = v - np.array(W, np.int64)
    return v[((w >= 0) & (w < np.array([ref.xy, ref.xy, ref.zs]))).all(axis=1)]


def drive_rays(ref, W, ego):
    """(origins, targets) float32 [n, 3] of the remembered-space test, 3,072 rays: from the final ego to the centres of 1,536 remembered
    occupied and 512 remembered free voxels outside the final window; 256 from remembered free voxels outside the window to observed free
    voxels in its far half in x, 256 between remembered free voxels far apart and 256 between the two halves in x of the window's
    observed free voxels (the drive's start, where the final window stands, lies on the storage seams of x and y); 64 from outside the extent, 64 with a non-finite component, 64 origin == target, 64 short ones"""
    ego = np.asarray(ego, np.float64)
    occ, free = remembered_outside(ref, W, OCCUPIED), remembered_outside(ref, W, FREE)
    near = in_window(ref, W, FREE)
    east = near[near[:, 0] >= W[0] + ref.xy // 2 + 4]
    near = near[near[:, 0] < W[0] + ref.xy // 2 - 4]
    rng = np.random.default_rng(5)
    A, B = [], []

    def add(a, b):
        a = np.broadcast_to(np.asarray(a, np.float64), np.shape(b))
        A.append(np.array(a)); B.append(np.asarray(b, np.float64))
    add(ego, centres(rr._spread(occ, 1536)))
    add(ego, centres(rr._spread(free, 512)))
    add(centres(rr._spread(free, 256)), centres(rr._spread(near, 256)))
    add(centres(rr._spread(free, 256)), centres(rr._spread(free[::-1], 256)))
    add(centres(rr._spread(near, 256)), centres(rr._spread(east[::-1], 256)))
    lo = np.array(ref.E, np.float64) * np.array(DRIVE_RES)
    size = np.array(ref.sizes(), np.float64) * np.array(DRIVE_RES)
    add(lo + rng.uniform(-0.3, -0.05, (64, 3)) * size, lo + rng.uniform(0.2, 0.8, (64, 3)) * size)
    bad = np.repeat(ego[None], 64, axis=0)
    bad[np.arange(64), np.arange(64) % 3] = np.array([np.nan, np.inf, -np.inf])[(np.arange(64) // 3) % 3]
    add(ego, bad)
    same = ego + rng.uniform(-3.0, 3.0, (64, 3))
    add(same, same.copy())
    add(ego, ego + rng.uniform(-0.3, 0.3, (64, 3)))
    A32, B32 = np.ascontiguousarray(np.concatenate(A).astype(F32)), np.ascontiguousarray(np.concatenate(B).astype(F32))
    return A32, B32


def seam_crossers(ref, visits, n):
    """rays (of n) whose examined voxels lie on both sides of the storage seam, per axis (x, y, z): storage coordinate = world coordinate
    & (size - 1)"""
    v = np.asarray(visits, np.int64).reshape(-1, 2)
    A, Z = ref.A, ref.Z
    e = np.stack([v[:, 1] % A, v[:, 1] // A % A, v[:, 1] // (A * A)], axis=1)
    out = []
    for k, size in enumerate((A, A, Z)):
        wrap = (-ref.E[k]) & (size - 1)                        # the extent coordinate whose storage coordinate is 0: the seam lies below it
        elo, ehi = np.full(n, size, np.int64), np.full(n, -1, np.int64)
        np.minimum.at(elo, v[:, 0], e[:, k]); np.maximum.at(ehi, v[:, 0], e[:, k])
        out.append(int(((wrap > 0) & (elo < wrap) & (ehi >= wrap)).sum()))
    return out


def drive_poses(ref, W, ego):
    """float64 [32, 4, 4]: 16 sensor poses at remembered free places outside the final window (next to never-observed space where there
    is some), 16 inside it"""
    free = remembered_outside(ref, W, FREE)
    out = [vr.pose_of(c, 0.37 * k, 0.11 * (k % 5 - 2)) for k, c in enumerate(centres(rr._spread(free, 16)))]
    Wv = np.array(W, np.int64)
    z, y, x = np.nonzero(ref.cls == FREE)
    v = np.stack([x, y, z], axis=1).astype(np.int64) + np.array(ref.E, np.int64)
    w = v - Wv
    inside = v[((w >= 0) & (w < np.array([ref.xy, ref.xy, ref.zs]))).all(axis=1)]
    out += [vr.pose_of(c, 0.37 * k, 0.11 * (k % 5 - 2)) for k, c in enumerate(centres(rr._spread(inside, 15)))]
    out.append(vr.pose_of(np.asarray(ego, np.float64)))
    return np.stack(out)
