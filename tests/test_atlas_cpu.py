"""The map atlas without a GPU: the referee of tests/atlas_ref.py against hand-written cases and against a tiny toroidal twin, the
census of every input tests/test_atlas.py gives the GPU (the synthetic scenarios in both modes, and the end-to-end drive with the maps
of the CPU oracle), the constants of header and binding, and what the binding refuses and hands over (a Gvom made with __new__ whose
`_lib` notes the calls)."""
import ctypes
import os
import re

import numpy as np
import pytest

import atlas_ref as ar
import gvom

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_UNKNOWN = [np.float64(v).view(np.int64) for v in ar.UNKNOWN_F]


def _set(xy, vis=0, neg=0, inferred=-1000.0, positive=0, height=0.0):
    """nine [y][x] maps of one value each (arrays are accepted: they broadcast)"""
    n = (xy, xy)
    full = lambda v, t: np.ascontiguousarray(np.broadcast_to(np.asarray(v, t), n))
    return [full(positive, np.int32), full(neg, np.int32), full(vis, np.int32), full(-0.5, np.float64), full(height, np.float64),
            full(inferred, np.float64), full(0.25, np.float64), full(-0.25, np.float64), full(0.125, np.float64)]


def _ranked(xy, ranks, tag):
    """a set whose cell ranks are `ranks` [y][x] (rank 1 through negative where x is even, through the inferred height where odd),
    positive = tag + the cell's index"""
    x = np.arange(xy)[None, :]
    vis = np.where(ranks == 2, 7, 0)
    neg = np.where((ranks == 1) & (x % 2 == 0), 3, 0)
    inferred = np.where((ranks == 1) & (x % 2 == 1), -2.5, -1000.0)
    return _set(xy, vis, neg, inferred, positive=tag + np.arange(xy * xy).reshape(xy, xy), height=float(tag))


def test_the_header_and_the_binding_agree():
    header = open(os.path.join(ROOT, "include", "gvom_hip.h")).read()
    for name, value in (("GVOM_PRODUCT_ATLAS_RECALL", gvom.PRODUCT_ATLAS_RECALL), ("GVOM_PRODUCT_ATLAS_EXTENT", gvom.PRODUCT_ATLAS_EXTENT),
                        ("GVOM_ATLAS_FOLLOW", gvom.ATLAS_FOLLOW), ("GVOM_ATLAS_FIXED", gvom.ATLAS_FIXED)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1)) == value, name
    assert (gvom.PRODUCT_ATLAS_RECALL, gvom.PRODUCT_ATLAS_EXTENT) == (22, 24)
    assert int(re.search(r"#define\s+GVOM_ABI_VERSION\s+(\d+)", header).group(1)) == 10 == gvom.ABI_VERSION      # an addition: the version stays
    for word in ("DEFINITION", "INPUT", "GVOM_ERR_INVALID", "NOT PROVIDED", "pyramid", "latest wins", "Time decay".lower(), "saving to disk"):
        assert word in header[header.index("--- map atlas"):header.index("--- one map sharded")], word
    bound = {n for n, _, _ in gvom.ABI}
    assert {"gvom_atlas_configure", "gvom_atlas_integrate", "gvom_atlas_recall", "gvom_atlas_extent", "gvom_atlas_clear", "gvom_atlas_counts",
            "gvom_device_map_origin"} <= bound
    layout = open(os.path.join(ROOT, "g-vom_amd", "csrc", "gvom_setlayout.h")).read()
    assert "GVOM_PRODUCT_ATLAS_RECALL" in layout and "GVOM_PRODUCT_ATLAS_EXTENT" in layout
    assert gvom._PRODUCT_DTYPES[22] == (np.int32, np.int32) and len(gvom._PRODUCT_DTYPES[24]) == 6


# ---- the referee against hand-written cases -------------------------------------------------------------------------------------------
def test_nine_rank_combinations_exactly_those_the_rule_names_are_written():
    """one cell of each new rank over each old rank.  Written iff r_new >= 1 and r_new >= r_old: (0,1) (0,2) (1,1) (1,2) (2,2) -- five of
    the nine (r_new = 1 over two old ranks, r_new = 2 over three); (2,1) is kept, the three with r_new = 0 are uninformative"""
    xy = 4
    old = np.zeros((xy, xy), np.int32)
    new = np.zeros((xy, xy), np.int32)
    cells = []
    for r_old in range(3):
        for r_new in range(3):
            k = 3 * r_old + r_new + 2                            # (cells 2 .. 10: both sorts of rank 1 occur, x even and odd)
            old[k // xy, k % xy], new[k // xy, k % xy] = r_old, r_new
            cells.append((k // xy, k % xy, r_old, r_new))
    ref = ar.AtlasRef(64, xy, follow=False, origin=(-2, -2))
    c1 = ref.integrate(_ranked(xy, old, 100), (-1, -1))
    assert c1["written"] == 6 and c1["uninformative"] == 10 and c1["kept"] == 0 and c1["outside"] == 0
    c2 = ref.integrate(_ranked(xy, new, 200), (-1, -1))
    maps, stamp, counts = ref.recall((-1, -1))
    written = 0
    for y, x, r_old, r_new in cells:
        should = r_new >= 1 and r_new >= r_old
        written += should
        if should:
            assert stamp[y, x] == 2 and maps[0][y, x] == 200 + y * xy + x and maps[4][y, x] == np.float64(200.0).view(np.int64), (r_old, r_new)
        elif r_old >= 1:
            assert stamp[y, x] == 1 and maps[0][y, x] == 100 + y * xy + x and maps[4][y, x] == np.float64(100.0).view(np.int64), (r_old, r_new)
        else:
            assert stamp[y, x] == 0 and maps[0][y, x] == 0 and [int(m[y, x]) for m in maps[3:]] == F_UNKNOWN, (r_old, r_new)
    assert written == 5 and c2["written"] == 5 and c2["kept"] == 1 and c2["uninformative"] == 3 + 7 and c2["outside"] == 0
    assert ref.counts()["known"] == 8 and ref.counts()["seq"] == 2 and counts.tolist() == [int((ar.rank(maps[2], maps[1], maps[5]) == 2).sum()),
                                                                                            int((ar.rank(maps[2], maps[1], maps[5]) == 1).sum()), 0, 2]


def _ids(origin, n):
    """positive = a number that names the world cell"""
    x = origin[0] + np.arange(n)[None, :]
    y = origin[1] + np.arange(n)[:, None]
    return (x * 10007 + y * 13 + 5).astype(np.int32)


@pytest.mark.parametrize("start", [(0, 0), (-40, -70), (-64, 31), (1000003, -999983)])
@pytest.mark.parametrize("d", [0, 1, 63, 64])
@pytest.mark.parametrize("axes", [(1, 0), (0, 1), (1, 1), (-1, 1), (-1, -1)])
def test_moves(start, d, axes):
    """an extent full of observed cells moves by (d, d) * axes: what stays keeps its values, what enters is UNKNOWN, a move of A
    clears everything; extents on both sides of zero"""
    A = xy = 64
    ref = ar.AtlasRef(A, xy)
    ref.integrate(_set(xy, vis=1, positive=_ids(start, xy)), start)
    assert ref.E == start and ref.known() == A * A
    to = (start[0] + d * axes[0], start[1] + d * axes[1])
    c = ref.integrate(_set(xy), to)                                # knows nothing: only the move acts
    ox, oy = (A - abs(to[0] - start[0])), (A - abs(to[1] - start[1]))
    stay = max(ox, 0) * max(oy, 0)
    assert c["cleared"] == c["cleared_known"] == A * A - stay and c["written"] == 0 and c["uninformative"] == A * A
    assert ref.E == to and ref.known() == stay and ref.counts()["known"] == stay
    (pos, neg, vis, rough, height, stamp), E = ref.extent()
    X, Y = np.meshgrid(to[0] + np.arange(A), to[1] + np.arange(A))
    was = (X >= start[0]) & (X < start[0] + A) & (Y >= start[1]) & (Y < start[1] + A)
    assert int(was.sum()) == stay and E == to
    assert np.array_equal(pos, np.where(was, _ids(to, A), 0)) and np.array_equal(vis, was.astype(np.int32)) and np.array_equal(stamp, was.astype(np.int32))
    assert np.array_equal(rough, np.where(was, np.float64(-0.5).view(np.int64), F_UNKNOWN[0]))
    assert np.array_equal(height, np.where(was, np.float64(0.0).view(np.int64), F_UNKNOWN[1]))


def test_the_counters_identity_and_the_sums():
    """known cells after = known before - cleared known + written over rank 0; the four merge counters sum to the window"""
    for xy, A in ((16, 64), (33, 128)):
        for follow in (True, False):
            ref = ar.AtlasRef(A, xy, follow, (0, 0) if follow else ar.fixed_origin(xy, A))
            w0 = 0
            for k, o in enumerate(ar.walk(xy, A)):
                before = ref.known()
                c = ref.integrate(ar.scenario_sets(xy, A)[k], o)
                over0, w0 = ref.census["written_over_0"] - w0, ref.census["written_over_0"]
                assert ref.known() == before - c["cleared_known"] + over0 == ref.counts()["known"]
                assert c["written"] + c["kept"] + c["uninformative"] + c["outside"] == xy * xy
                assert c["cleared_known"] <= c["cleared"] and (follow or c["cleared"] == 0)


# ---- the toroidal twin ------------------------------------------------------------------------------------------------------------------
class _Torus(object):
    """the same definition over storage addressed with & (A-1), cell by cell"""

    def __init__(self, A, xy, follow, origin):
        self.A, self.xy, self.follow, self.E, self.seq = A, xy, follow, tuple(origin), 0
        self.cell = [[self._unknown() for _ in range(A)] for _ in range(A)]

    @staticmethod
    def _unknown():
        return list(ar.UNKNOWN_I) + F_UNKNOWN + [0]

    @staticmethod
    def _rank(v):
        return int(ar.rank(np.int32(v[2]), np.int32(v[1]), np.int64(v[5])))

    def _inside(self, X, Y):
        return self.E[0] <= X < self.E[0] + self.A and self.E[1] <= Y < self.E[1] + self.A

    def integrate(self, maps, origin):
        A, n, m = self.A, self.xy, self.A - 1
        mi, mf = ar.split(maps)
        if self.follow:
            to = (origin[0] + n // 2 - A // 2, origin[1] + n // 2 - A // 2)
            old, self.E = self.E, to
            for Y in range(to[1], to[1] + A):
                for X in range(to[0], to[0] + A):
                    if not (old[0] <= X < old[0] + A and old[1] <= Y < old[1] + A):
                        self.cell[Y & m][X & m] = self._unknown()
        self.seq += 1
        for y in range(n):
            for x in range(n):
                X, Y = origin[0] + x, origin[1] + y
                if not self._inside(X, Y):
                    continue
                v = [int(a[y, x]) for a in mi + mf]
                r_new, r_old = self._rank(v), self._rank(self.cell[Y & m][X & m])
                if r_new >= 1 and r_new >= r_old:
                    self.cell[Y & m][X & m] = v + [self.seq]

    def recall(self, origin):
        n, m = self.xy, self.A - 1
        out = np.empty((10, n, n), np.int64)
        for y in range(n):
            for x in range(n):
                X, Y = origin[0] + x, origin[1] + y
                out[:, y, x] = self.cell[Y & m][X & m] if self._inside(X, Y) else self._unknown()
        return out


def test_the_toroidal_twin_equals_the_referee_on_200_random_sequences():
    rng = np.random.default_rng(77)
    A = 64
    for s in range(200):
        xy = int(rng.integers(3, 13))
        follow = bool(s % 3)
        start = tuple(int(v) for v in rng.integers(-200, 200, 2))
        e0 = (0, 0) if follow else (start[0] - 20, start[1] - 30)
        ref, twin = ar.AtlasRef(A, xy, follow, e0), _Torus(A, xy, follow, e0)
        o = start
        for _ in range(int(rng.integers(2, 5))):
            reach = int(rng.choice([1, 3, xy, 40, 70]))
            o = (o[0] + int(rng.integers(-reach, reach + 1)), o[1] + int(rng.integers(-reach, reach + 1)))
            maps = ar.synthetic_set(rng, xy)
            ref.integrate(maps, o)
            twin.integrate(maps, o)
            assert ref.E == twin.E
            for r in (o, start, (ref.E[0] + A - xy // 2, ref.E[1] - 1), (o[0] + int(rng.integers(-70, 70)), o[1] + int(rng.integers(-70, 70)))):
                got, stamp, _ = ref.recall(r)
                want = twin.recall(r)
                assert np.array_equal(np.stack([g.astype(np.int64) for g in got] + [stamp.astype(np.int64)]), want), (s, o, r)


# ---- the census of every input the GPU tests use ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("follow", [True, False])
@pytest.mark.parametrize("xy,A", ar.SCENARIOS)
def test_census_of_the_synthetic_scenarios(xy, A, follow):
    """every scenario meets: a cell written over rank 0, over an equal rank, kept (old 2, new 1), uninformative, recalled outside the
    extent, a window row across the storage seam in x, a window across it in y -- and a known cell cleared by a move where the extent
    follows; a fixed extent never moves, so there the sets must lie inside it, across its edge (cells outside) and wholly outside"""
    ref = ar.AtlasRef(A, xy, follow, (0, 0) if follow else ar.fixed_origin(xy, A))
    origins, sets = ar.walk(xy, A), ar.scenario_sets(xy, A)
    steps = [(origins[k][0] - origins[k - 1][0], origins[k][1] - origins[k - 1][1]) for k in range(1, ar.N_INTEGRATES)]
    assert (0, 0) in steps and (1, 0) in steps and (xy, 0) in steps and any(abs(dx) >= A for dx, _ in steps)
    assert any((A - xy) // 2 < abs(dx) < A for dx, _ in steps) and any((A - xy) // 2 < abs(dy) < A for _, dy in steps)
    assert min(o[0] for o in origins) < 0 < max(o[0] + xy for o in origins)
    whole = partly = 0
    for k in range(ar.N_INTEGRATES):
        c = ref.integrate(sets[k], origins[k])
        whole += c["outside"] == xy * xy
        partly += 0 < c["outside"] < xy * xy
        for r in ar.recall_origins(xy, A, ref, origins, k):
            _, _, counts = ref.recall(r)
        assert counts[2] == xy * xy                               # the last of them lies wholly outside
    c = dict(ref.census)
    print(xy, A, follow, c)
    if follow:
        assert ar.census_ok(c), c
    else:
        c["cleared_known"] = 1                                    # (no move: nothing to clear)
        assert ar.census_ok(c) and whole >= 1 and partly >= 1, (c, whole, partly)


@pytest.mark.parametrize("ring", [1, 2])
def test_census_of_the_drive_with_the_cpu_oracle(ring):
    """the end-to-end drive, its maps from the CPU oracle: the same census, and after the return leg the recall at the first origin
    knows ground the last combine does not"""
    from oracle import oracle
    o = oracle.OracleGvom(ar.DRIVE_RES, ar.DRIVE_ZRES, ar.DRIVE_XY, 8, ring, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
    ref = ar.AtlasRef(ar.DRIVE_A, ar.DRIVE_XY)
    origins = []
    for pc, ego in ar.drive_scans():
        o.process_pointcloud(pc, ego)
        maps, org = ar.mapper_set(o, o.combine_maps())
        origins.append(org)
        ref.integrate([m.T for m in maps], org)
        ref.recall()
        ref.recall(origins[0])
    assert origins[-1] == origins[0] and max(abs(p[0] - origins[0][0]) for p in origins) > ar.DRIVE_XY
    ref.recall((origins[0][0] + ar.DRIVE_A, origins[0][1]))
    print(ring, ref.census)
    assert ar.census_ok(ref.census), ref.census
    got, _, counts = ref.recall(origins[0])
    seen_live, seen_atlas = int((maps[2] > 0).sum()), int(counts[0])
    assert seen_atlas > seen_live + 100, (seen_atlas, seen_live)
    assert ((got[2] > 0) & (maps[2].T <= 0)).sum() > 100


# ---- the binding without a GPU -------------------------------------------------------------------------------------------------------------
XY = 6


class _Lib(object):
    """stands in for the loaded library: notes every call (pointed-to maps and origins read at call time) and returns 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            got = list(args)
            if name == "gvom_atlas_integrate" and got[2] is not None and got[3] == 0:
                got[2] = [np.array(((ctypes.c_int32 if k < 3 else ctypes.c_int64) * (XY * XY)).from_address(int(p))) for k, p in enumerate(got[2])]
            elif name == "gvom_atlas_integrate" and got[2] is not None:
                got[2] = [int(p) for p in got[2]]
            for k, a in enumerate(got):
                if isinstance(a, ctypes.Array):
                    got[k] = tuple(a)
            self.calls.append((name, got))
            if name == "gvom_atlas_recall":
                args[2]._obj.value, args[3]._obj.value = 11, 12
            if name == "gvom_device_map_origin":
                args[2][0], args[2][1], args[2][2] = 5, -6, 7
            if name == "gvom_device_product_export":
                args[4]._obj.value = 4096
            return 0
        return entry

    def named(self, name):
        return [a for n, a in self.calls if n == name]


def _mapper():
    g = gvom.Gvom.__new__(gvom.Gvom)
    g._lib, g._h, g._device = _Lib(), ctypes.c_void_p(1), 0
    g.xy_size, g.xy_resolution = XY, 0.5
    return g


def test_create_atlas_refuses_bad_sizes_and_origins_in_python():
    g = _mapper()
    g.xy_size = 100
    for cells in (0, 63, 96, 100, 8192, 64.5, -128):
        with pytest.raises(ValueError):
            g.create_atlas(cells)
    with pytest.raises(ValueError, match="xy_size"):
        g.create_atlas(64)                                         # a power of two in range, below the window
    with pytest.raises(ValueError):
        g.create_atlas(128, follow=False)                          # a fixed extent needs its corner
    for bad in ((1.5, 2.0), (1, 2, 3), 7, (1 << 41, 0)):
        with pytest.raises(ValueError):
            g.create_atlas(128, follow=False, origin_cells=bad)
    assert g._lib.calls == []
    a = g.create_atlas(128, follow=False, origin_cells=(-5, 9))
    assert g._lib.named("gvom_atlas_configure") == [[g._h, 128, gvom.ATLAS_FIXED, (-5, 9)]] and a.extent_origin == (-5, 9) and a.cells == 128
    b = g.create_atlas(256)
    assert g._lib.named("gvom_atlas_configure")[1] == [g._h, 256, gvom.ATLAS_FOLLOW, None] and b.follow and b.seq == 0


def test_integrate_of_checks_the_nine_maps_and_hands_them_over_bit_for_bit():
    g = _mapper()
    a = g.create_atlas(64)
    maps = [m.T for m in ar.synthetic_set(np.random.default_rng(5), XY)]          # [x, y], as DeviceMap.copy_to_host() gives them
    for bad in (maps[:8], maps + maps[:1]):
        with pytest.raises(ValueError):
            a.integrate_of(bad, (0, 0))
    with pytest.raises(ValueError):
        a.integrate_of(maps[:4] + [maps[4][:5]] + maps[5:], (0, 0))            # a wrong shape
    with pytest.raises(TypeError):
        a.integrate_of([maps[0].astype(np.int64)] + maps[1:], (0, 0))           # a wrong dtype is not cast
    with pytest.raises(TypeError):
        a.integrate_of(maps[:3] + [np.zeros((XY, XY), np.float32)] + maps[4:], (0, 0))
    with pytest.raises(ValueError):
        a.integrate_of(maps, (0.5, 1))
    assert g._lib.named("gvom_atlas_integrate") == []
    a.integrate_of(maps, (-7, 1 << 33))
    (h, sid, got, on_device, org), = g._lib.named("gvom_atlas_integrate")
    assert sid == -1 and on_device == 0 and org == (-7, 1 << 33)
    for k in range(9):                                             # cell (x, y) at [y * xy + x], every bit as given
        want = maps[k].T.reshape(-1)
        assert np.array_equal(got[k], want if k < 3 else want.view(np.int64)), k
    assert a.seq == 1 and a.extent_origin == (-7 + XY // 2 - 32, (1 << 33) + XY // 2 - 32)
    with pytest.raises(ValueError):
        a.integrate_of_device([4096] * 8, (0, 0))
    with pytest.raises(ValueError):
        a.integrate_of_device([4096] * 8 + [0], (0, 0))
    a.integrate_of_device([4096 + 256 * k for k in range(9)], (3, 4))
    assert g._lib.named("gvom_atlas_integrate")[1][1:] == [-1, [4096 + 256 * k for k in range(9)], 1, (3, 4)] and a.seq == 2


def test_recall_takes_cells_or_a_centre_with_the_scans_arithmetic():
    g = _mapper()
    a = g.create_atlas(64)
    with pytest.raises(ValueError, match="not both"):
        a.recall(origin_cells=(0, 0), center=(0.0, 0.0))
    for bad in ((1.0,), (np.nan, 0.0), (0.0, np.inf)):
        with pytest.raises(ValueError):
            a.recall(center=bad)
    with pytest.raises(ValueError):
        a.recall(origin_cells=(0.0, 1.0))
    assert g._lib.named("gvom_atlas_recall") == []
    m = a.recall()
    assert g._lib.named("gvom_atlas_recall")[0][1] is None                     # the library's default: the last integrated set's origin
    assert m.set_id == 11 and m.origin_cells == (5, -6, 7) and m.stamps.product_id == 12 and m.recall_counts.product_id == 12
    a.recall(origin_cells=(-3, 8))
    a.recall(center=(-1.3, 7.49))                                  # floor(c / 0.5 - 6 / 2)
    assert [c[1] for c in g._lib.named("gvom_atlas_recall")[1:]] == [(-3, 8), (-6, 11)]
    assert np.array_equal(gvom.cells_of([[0.0, -0.01], [1.49, 1.5]], 0.5), [[0, -1], [2, 3]]) and gvom.cells_of([0.2], 0.5).dtype == np.int64
