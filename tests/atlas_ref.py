"""Referee of the map atlas (include/gvom_hip.h "map atlas"): pure numpy, NOT toroidal -- the extent is held as plain arrays indexed by
(Y - Ey, X - Ex), a move allocates an UNKNOWN extent and copies the overlap.  It applies the definition literally: the move, the merge,
the counters, the recall and the extent export, and it keeps a census of what every integrate and recall met.  Also here: the
generator of synthetic nine-map sets, the walks of the synthetic scenarios and the drive of the end-to-end scenario, which
tests/test_atlas_cpu.py (the census) and tests/test_atlas.py (the GPU) share.

Maps are [y][x] arrays here (cell (x, y) at [y, x]); the binding's are [x, y]: the tests pass `.T`.  The f64 maps are carried as int64
bit patterns, so that NaN payloads count."""
import functools

import numpy as np

N_MAPS = 9
# set order: 0 positive, 1 negative, 2 visibility (int32); 3 roughness, 4 height, 5 inferred height, 6 x slope, 7 y slope, 8 guessed delta (f64)
UNKNOWN_I = (0, 0, 0)
UNKNOWN_F = (-1.0, -1000.0, -1000.0, 0.0, 0.0, 0.0)
CENSUS_KEYS = ("written_over_0", "written_over_equal", "written_2_over_1", "kept_2_over_1", "uninformative", "outside", "cleared",
               "cleared_known", "recalled_outside", "seam_x", "seam_y")


def bits(a):
    """an f64 array as its int64 bit patterns (a view)"""
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def rank(vis, neg, inferred_bits):
    """2 observed iff visibility > 0; 1 inferred iff visibility <= 0 and (negative > 0 or inferred height > -1000.0); 0 otherwise"""
    with np.errstate(invalid="ignore"):
        inferred = np.asarray(inferred_bits, np.int64).view(np.float64) > -1000.0
    return np.where(np.asarray(vis) > 0, 2, np.where((np.asarray(neg) > 0) | inferred, 1, 0)).astype(np.int32)


def unknown(shape):
    """(three int32 maps, six int64 bit-pattern maps, stamps) of UNKNOWN cells"""
    i = [np.full(shape, v, np.int32) for v in UNKNOWN_I]
    f = [np.full(shape, np.float64(v).view(np.int64), np.int64) for v in UNKNOWN_F]
    return i, f, np.zeros(shape, np.int32)


def split(maps):
    """nine [y][x] maps in set order -> (three int32, six int64 bit patterns); dtypes are checked, nothing is cast"""
    assert len(maps) == N_MAPS
    for k, m in enumerate(maps):
        assert m.dtype == (np.int32 if k < 3 else np.float64), (k, m.dtype)
    return [np.ascontiguousarray(m) for m in maps[:3]], [bits(m) for m in maps[3:]]


class AtlasRef(object):
    def __init__(self, cells, xy, follow=True, origin=(0, 0)):
        A = int(cells)
        assert 64 <= A <= 4096 and A & (A - 1) == 0 and A >= xy
        self.A, self.xy, self.follow = A, int(xy), bool(follow)
        self.E = (int(origin[0]), int(origin[1]))
        self.i, self.f, self.stamp = unknown((A, A))
        self.seq = 0
        self.last = dict.fromkeys(("written", "kept", "uninformative", "outside", "cleared", "cleared_known"), 0)
        self.last_origin = None
        self.census = dict.fromkeys(CENSUS_KEYS, 0)

    # ---- helpers ----
    def known(self):
        return int((rank(self.i[2], self.i[1], self.f[2]) >= 1).sum())

    def _overlap(self, origin, n):
        """the part of the n x n window at `origin` that lies in the extent: (window slices, extent slices) or None"""
        A = self.A
        x0, y0 = origin[0] - self.E[0], origin[1] - self.E[1]
        lx, hx, ly, hy = max(x0, 0), min(x0 + n, A), max(y0, 0), min(y0 + n, A)
        if lx >= hx or ly >= hy:
            return None
        return (slice(ly - y0, hy - y0), slice(lx - x0, hx - x0)), (slice(ly, hy), slice(lx, hx))

    def _seams(self, origin, n):
        m = self.A - 1
        self.census["seam_x"] += int((origin[0] & m) + n > self.A)
        self.census["seam_y"] += int((origin[1] & m) + n > self.A)

    # ---- the definition ----
    def move(self, to):
        """the extent goes to `to`; every cell of the new extent that was not in the old one becomes UNKNOWN"""
        A = self.A
        old = (self.i, self.f, self.stamp)
        old_rank = rank(self.i[2], self.i[1], self.f[2])
        dx, dy = to[0] - self.E[0], to[1] - self.E[1]
        self.i, self.f, self.stamp = unknown((A, A))
        stayed = np.zeros((A, A), bool)                        # cells of the OLD extent that are still in the new one
        if abs(dx) < A and abs(dy) < A:
            src = (slice(max(dy, 0), A + min(dy, 0)), slice(max(dx, 0), A + min(dx, 0)))
            dst = (slice(max(-dy, 0), A + min(-dy, 0)), slice(max(-dx, 0), A + min(-dx, 0)))
            for new, was in zip(self.i + self.f + [self.stamp], old[0] + old[1] + [old[2]]):
                new[dst] = was[src]
            stayed[src] = True
        self.E = (int(to[0]), int(to[1]))
        cleared = int(A * A - stayed.sum())                   # as many cells entered as left
        cleared_known = int((old_rank[~stayed] >= 1).sum())   # what the cells that left knew: their storage is what is cleared
        return cleared, cleared_known

    def integrate(self, maps, origin):
        """maps: nine [y][x] arrays in set order; origin: (Ox, Oy) integers.  Returns the counters of this integrate."""
        n, A = self.xy, self.A
        mi, mf = split(maps)
        assert all(m.shape == (n, n) for m in mi + mf)
        origin = (int(origin[0]), int(origin[1]))
        cleared = cleared_known = 0
        if self.follow:
            cleared, cleared_known = self.move((origin[0] + n // 2 - A // 2, origin[1] + n // 2 - A // 2))
        self.seq += 1
        c = dict.fromkeys(("written", "kept", "uninformative"), 0)
        ov = self._overlap(origin, n)
        inside = 0
        if ov is not None:
            w, e = ov
            r_new = rank(mi[2][w], mi[1][w], mf[2][w])
            r_old = rank(self.i[2][e], self.i[1][e], self.f[2][e])
            write = (r_new >= 1) & (r_new >= r_old)
            for dst, src in zip(self.i + self.f, mi + mf):
                dst[e][write] = src[w][write]                  # (dst[e] is a view: the assignment lands in the extent)
            self.stamp[e][write] = self.seq
            inside = r_new.size
            c["written"], c["kept"] = int(write.sum()), int(((r_new >= 1) & ~write).sum())
            c["uninformative"] = int((r_new == 0).sum())
            self.census["written_over_0"] += int((write & (r_old == 0)).sum())
            self.census["written_over_equal"] += int((write & (r_old == r_new)).sum())
            self.census["written_2_over_1"] += int((write & (r_old == 1) & (r_new == 2)).sum())
            self.census["kept_2_over_1"] += c["kept"]
            self.census["uninformative"] += c["uninformative"]
        c["outside"] = n * n - inside
        c["cleared"], c["cleared_known"] = cleared, cleared_known
        self.census["outside"] += c["outside"]
        self.census["cleared"] += cleared
        self.census["cleared_known"] += cleared_known
        self._seams(origin, n)
        self.last, self.last_origin = c, origin
        return dict(c)

    def counts(self):
        out = dict(self.last)
        out["known"], out["seq"] = self.known(), self.seq
        return out

    def _window(self, origin, n):
        i, f, stamp = unknown((n, n))
        ov = self._overlap(origin, n)
        inside = 0
        if ov is not None:
            w, e = ov
            for dst, src in zip(i + f + [stamp], self.i + self.f + [self.stamp]):
                dst[w] = src[e]
            inside = dst[w].size
        return i, f, stamp, n * n - inside

    def recall(self, origin=None):
        """-> (nine [y][x] maps: int32 and int64 BIT PATTERNS, stamps, int32 [4] {rank 2, rank 1, outside, seq})"""
        origin = self.last_origin if origin is None else (int(origin[0]), int(origin[1]))
        i, f, stamp, outside = self._window(origin, self.xy)
        r = rank(i[2], i[1], f[2])
        self.census["recalled_outside"] += outside
        self._seams(origin, self.xy)
        return i + f, stamp, np.array([(r == 2).sum(), (r == 1).sum(), outside, self.seq], np.int32)

    def extent(self):
        """-> ((positive, negative, visibility, roughness bits, height bits, stamp), each [A][A] as [y][x], extent origin)"""
        return (self.i[0].copy(), self.i[1].copy(), self.i[2].copy(), self.f[0].copy(), self.f[1].copy(), self.stamp.copy()), self.E

    def clear(self):
        self.i, self.f, self.stamp = unknown((self.A, self.A))
        self.last = dict.fromkeys(self.last, 0)


# ---- synthetic nine-map sets ---------------------------------------------------------------------------------------------------------
def synthetic_set(rng, xy, p=(0.3, 0.3, 0.2, 0.2)):
    """nine [y][x] maps with cells of rank 0, rank 2, rank 1 through negative > 0 and rank 1 through the inferred height alone, mixed
    at random with probabilities p; arbitrary f64 bit patterns (NaNs of every payload, infinities, denormals) in every plane that
    does not decide the rank, and in the inferred height wherever something else decides it."""
    n = (xy, xy)
    cls = rng.choice(4, n, p=p)                                  # 0 nothing, 1 observed, 2 negative, 3 inferred height only
    any_i = lambda: rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
    any_f = lambda: rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64, endpoint=True)
    not_above = np.array([-1000.0, -1000.5, -1e300, -np.inf, np.nan], np.float64).view(np.int64)
    not_above = np.concatenate([not_above, [np.int64(0x7ff8dead0000beef), np.int64(-0x000fffff00000001)]])     # NaNs with payloads, either sign
    above = np.array([-999.9999999, -1.0, -0.0, 0.0, 5e-324, 1.5, 1e300, np.inf], np.float64).view(np.int64)
    vis = np.where(cls == 1, rng.integers(1, 2 ** 31, n), -rng.integers(0, 3, n) * rng.integers(0, 2 ** 30, n)).astype(np.int32)
    neg = np.where(cls == 2, rng.integers(1, 2 ** 31, n), np.where(cls == 1, any_i(), -rng.integers(0, 2 ** 31, n))).astype(np.int32)
    inferred = np.where(cls == 3, rng.choice(above, n), np.where(cls == 0, rng.choice(not_above, n), any_f()))
    maps = [any_i(), neg, vis, any_f(), any_f(), inferred, any_f(), any_f(), any_f()]
    out = [m if k < 3 else m.astype(np.int64).view(np.float64) for k, m in enumerate(maps)]
    want = np.where(cls == 1, 2, np.where(cls == 0, 0, 1))
    assert np.array_equal(rank(out[2], out[1], bits(out[5])), want)
    return out


# ---- the synthetic scenarios: (xy_size, A) and their walks ---------------------------------------------------------------------------------
SCENARIOS = tuple((xy, A) for xy in (16, 33, 64) for A in (64, 128))
N_INTEGRATES = 12


def walk(xy, A):
    """the 12 origins of a scenario: they start below zero next to the storage seam, cross it, and move by 0 cells, 1 cell, xy cells,
    more than (A - xy) / 2 (the entered strips overlap the new window), and once by A or more"""
    big = (A - xy) // 2 + 3
    steps = [(0, 0), (1, 0), (0, 1), (xy, 0), (-1, -1), (0, xy), (big, 2), (-2, big), (-big, -big), (A + 5, 0), (-3, -2)]
    assert len(steps) == N_INTEGRATES - 1
    o = [(-xy // 2 - 3, -5)]
    for dx, dy in steps:
        o.append((o[-1][0] + dx, o[-1][1] + dy))
    return o


def fixed_origin(xy, A):
    """the extent of the fixed-mode run of a scenario: around the walk's start, so that sets lie inside, across its edge and outside"""
    return (-A // 2 + 4, -A // 2 + 9)


def recall_origins(xy, A, ref, origins, k):
    """where the tests recall after integrate k: the current origin, the first origin, half outside the extent, wholly outside it"""
    E = ref.E
    return [origins[k], origins[0], (E[0] + A - xy // 2, E[1] - xy // 2), (E[0] + A + 7, E[1] - 2 * xy)]


@functools.lru_cache(maxsize=None)
def scenario_sets(xy, A):
    """the 12 sets of a scenario, built once, shared, read-only; the mix changes along the walk so that observed ground meets
    inferences, and inferences meet observed ground"""
    rng = np.random.default_rng(1000 * xy + A)
    mixes = [(0.3, 0.3, 0.2, 0.2), (0.5, 0.1, 0.2, 0.2), (0.2, 0.6, 0.1, 0.1), (0.4, 0.0, 0.3, 0.3)]
    sets = []
    for k in range(N_INTEGRATES):
        s = synthetic_set(rng, xy, mixes[k % 4])
        for m in s:
            m.setflags(write=False)
        sets.append(tuple(s))
    return tuple(sets)


def census_ok(c):
    """what every scenario must have met (the issue's list)"""
    need = ("written_over_0", "written_over_equal", "kept_2_over_1", "uninformative", "cleared_known", "recalled_outside", "seam_x", "seam_y")
    return all(c[k] >= 1 for k in need)


# ---- the end-to-end drive ---------------------------------------------------------------------------------------------------------------------
DRIVE_XY, DRIVE_A, DRIVE_RES, DRIVE_ZRES = 64, 128, 0.4, 0.2
DRIVE_STEP_CELLS, DRIVE_LEGS = 9, 8                              # 8 steps of 9 cells out (72 cells > xy_size), then the same way back
DRIVE_Z = -0.6                                                   # the 8 levels of 0.2 m around this hold the scene's ground at -1 m


def drive_egos():
    out = [(DRIVE_STEP_CELLS * DRIVE_RES * k + 0.13, -0.5 * DRIVE_STEP_CELLS * DRIVE_RES * k + 0.07, DRIVE_Z) for k in range(DRIVE_LEGS + 1)]
    return out + out[-2::-1]


@functools.lru_cache(maxsize=None)
def drive_scans():
    """((cloud, ego), ...): tests/obstacle_scenes.py's post scene around every ego of the drive; on the way back the sensor sees half
    as far (cells re-enter the window unseen)"""
    import obstacle_scenes as ob
    out = []
    for k, ego in enumerate(drive_egos()):
        pc = ob.post_scene(300 + k, DRIVE_XY, DRIVE_RES, DRIVE_ZRES, ego, n_posts=25, ground_pts=2500)
        if k > DRIVE_LEGS:
            near = np.abs(pc[:, :2] - np.asarray(ego[:2], np.float32)).max(axis=1) < 0.25 * DRIVE_XY * DRIVE_RES
            pc = np.ascontiguousarray(pc[near])
        pc.setflags(write=False)
        out.append((pc, ego))
    return tuple(out)


def mapper_set(g, combined):
    """the nine [x, y] maps of the last combine_maps() of a mapper with the reference's attributes (the CPU referee of the whole
    pipeline has them), in set order, and the integer origin of their window"""
    _, positive, negative, roughness, visibility = combined[:5]
    maps = [positive, negative, visibility, roughness, g.height_map, g.inferred_height_map, g.x_slope_map, g.y_slope_map, g.guessed_height_delta]
    maps = [np.asarray(m).astype(np.int32 if k < 3 else np.float64) for k, m in enumerate(maps)]
    return maps, tuple(int(v) for v in np.asarray(g.combined_origin)[:2])
