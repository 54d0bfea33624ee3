"""Atlas frontiers without a GPU: the constants of header and binding, the referee of tests/atlas_frontier_ref.py in its two forms, the
census of every input tests/test_atlas_frontiers.py gives the GPU -- with two deliberately wrong twins as the witnesses that a kernel
which wrapped its neighbours around the extent, or forgot the storage phase, would be caught --, the moved extent, negative visibility,
the drive's outward leg with the maps of the CPU oracle, and what the binding refuses and computes without a library call."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import atlas_field_ref as afr
import atlas_frontier_ref as af
import atlas_ref as ar
import costfield_ref as cf
import frontier_ref as fr
import gvom

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = cf.UNREACHED
CASES = [(xy, A, follow) for xy, A in afr.SCENARIOS for follow in (True, False)]


def _same(a, b, what):
    for k, name in enumerate(("clusters", "sums", "cluster map", "counts")):
        assert np.array_equal(a[k], b[k]), (what, name)
    assert list(a[4]) == list(b[4]), what


def test_the_header_and_the_binding_agree():
    header = open(os.path.join(ROOT, "include", "gvom_hip.h")).read()
    assert int(re.search(r"#define\s+GVOM_PRODUCT_ATLAS_FRONTIERS\s+(\d+)", header).group(1)) == gvom.PRODUCT_ATLAS_FRONTIERS == 28
    assert int(re.search(r"#define\s+GVOM_ABI_VERSION\s+(\d+)", header).group(1)) == 10 == gvom.ABI_VERSION      # an addition: the version stays
    section = header[header.index("--- atlas frontiers"):header.index("--- one map sharded")]
    for word in ("DEFINITION", "MAPS", "VISIBILITY", "FRONTIER CELL", "visibility <= 0", "NEITHER", "FLAT", "SNAPSHOT", "WAITS", "GVOM_ERR_INVALID",
                 "GVOM_ERR_CAPACITY", "NOT PROVIDED", "atlas_frontiers", "atlas_frontier_rounds", "atlas_frontier_tiles", "atlas_frontier_allocations",
                 "frontier_batch", "frontier_inner", "stopped early", "Kind 27 is not assigned"):
        assert word in section, word
    assert ("int gvom_atlas_frontiers(gvom_t *h, int64_t field_id, int32_t min_cells, int32_t max_clusters,\n"
            "                         int64_t *product_id, int64_t info[4], int64_t extent_origin[2] /* may be NULL */);") in section
    bound = {n: a for n, _, a in gvom.ABI}
    assert len(bound["gvom_atlas_frontiers"]) == 7
    layout = open(os.path.join(ROOT, "g-vom_amd", "csrc", "gvom_setlayout.h")).read()
    assert layout.count("GVOM_PRODUCT_ATLAS_FRONTIERS") >= 2
    assert gvom._PRODUCT_DTYPES[28] == (np.int32, np.int64, np.int32, np.int32) == gvom._PRODUCT_DTYPES[gvom.PRODUCT_FRONTIERS]
    assert issubclass(gvom.DeviceAtlasFrontiers, gvom.DeviceFrontiers)


def test_the_layout_under_sanitizers(tmp_path):
    """kind 28 at small and the largest shapes, part for part kind 16 of a window of that side, and the marking kernel's visibility
    address in its own int arithmetic, in a program of its own"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "atlas_frontier_layout_host_test")
    src = os.path.join(ROOT, "tests", "atlas_frontier_layout_host_test.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src, "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "atlas frontier layout host test ok" in run.stdout


# ---- the referee and the census of what the GPU is given -----------------------------------------------------------------------------------
@pytest.mark.parametrize("xy,A,follow", CASES)
def test_the_referees_two_forms_agree_and_the_census_holds(xy, A, follow):
    ref, _ = afr.scenario(xy, A, follow)
    assert ref.E[0] & (A - 1) and ref.E[1] & (A - 1)                    # a storage phase on both axes
    for k in af.VARIANTS:
        f = afr.expected(xy, A, follow, k)
        for min_cells, cap in af.LIMITS:
            _same(af.of_field(f, ref, min_cells, cap), af.of_field(f, ref, min_cells, cap, loops=True), (xy, A, follow, k, min_cells, cap))
        c = af.census(xy, A, follow, k)
        print(xy, A, follow, k, c)
        if k == 5:                                                      # the nearly empty case
            assert c["kept"] <= 2, c
            continue
        assert c["kept"] >= 4 and c["dropped"] >= 4 and c["largest"] >= 114 and c["spanning"] >= 2, c
        assert c["wrap_differs"] >= 8 and c["unphased_differs"] >= 1, c
        if k == 1:
            assert c["unreachable"] >= 59, c                             # frontier cells the field cannot reach, and only those, are gone


def test_the_exact_zero_and_the_case_beyond_the_cap():
    assert af.census(16, 64, False, 5)["cells"] == 0
    rows, _, cmap, counts, _ = af.expected(64, 128, True, 0, 1, 8)
    assert counts[0] == 58 + af.census(64, 128, True, 0)["dropped"] > 8   # (min_cells 1 keeps the small ones too)
    rows4, _, cmap4, counts4, _ = af.expected(64, 128, True, 0, 4, 1024)
    assert counts4[0] == 58 > 8
    rows8 = af.of_field(afr.expected(64, 128, True, 0), afr.scenario(64, 128, True)[0], 4, 8)
    assert np.array_equal(rows8[0], rows4[:8]) and np.array_equal(rows8[2], cmap4) and rows8[2].max() == 57


def test_the_moved_extent():
    """(33, 128, follow): after the field is made one more set is integrated 20 columns and -5 rows on.  The frontier cells the unmoved
    referee has in the 20 columns and 5 rows that left the atlas's extent are gone -- they are neither known nor unknown now --, and
    the new set changes cells elsewhere"""
    xy, A = 33, 128
    ref, _ = afr.scenario(xy, A, True)
    f = afr.expected(xy, A, True, 0)
    now, (s, o) = af.moved(xy, A, True)
    assert (now.E[0] - ref.E[0], now.E[1] - ref.E[1]) == (20, -5) and f["E"] == ref.E
    before = af.mask(f["c"], af.visibility(ref, f["E"], A), f["D"])
    vis3 = af.visibility(now, f["E"], A)
    after = af.mask(f["c"], vis3, f["D"])
    left = np.zeros((A, A), bool)
    left[:20, :] = True
    left[:, A - 5:] = True
    assert np.array_equal(vis3 == -1, left)
    assert before[left].sum() >= 1 and not after[left].any()
    assert (before[~left] != after[~left]).sum() >= 1
    _same(af.of_field(f, now, 4, 1024), af.of_field(f, now, 4, 1024, loops=True), "moved")
    # and an atlas of another side: the frame stays the field's
    small = ar.AtlasRef(64, xy, False, (ref.E[0] + 40, ref.E[1] + 50))
    small.integrate(s, (ref.E[0] + 50, ref.E[1] + 60))
    v = af.visibility(small, f["E"], A)
    assert (v[40:104, 50:114] >= 0).all() and (v == -1).sum() == A * A - 64 * 64 and (v == 1).sum() >= 1


def test_negative_visibility_counts_as_unknown():
    xy, A = 16, 64
    E = ar.fixed_origin(xy, A)
    ref = ar.AtlasRef(A, xy, False, E)
    s = af.negative_set(xy)
    ref.integrate(s, (E[0] + 8, E[1] + 8))
    assert (ref.i[2] == -3).sum() == xy * (xy - xy // 2)                 # rank 1: the cells went in with their visibility as it is
    seed = (E[0] + 9, E[1] + 9)
    f = afr.field(ref, [seed], afr.params())
    got = af.of_field(f, ref, 1, 64)
    m = af.mask(f["c"], af.visibility(ref, E, A), f["D"])
    only_zero = fr.frontier_mask(f["c"].T, np.where(ref.i[2] == 0, 0, 1), f["D"].T).T       # a rule that read `== 0` as unknown
    assert (m & ~only_zero).sum() >= 1 and got[3][1] == m.sum()
    assert m[8 + xy // 2 - 1, 9] and not only_zero[8 + xy // 2 - 1, 9]    # beside the inferred cells, inside the observed patch


# ---- the drive, with the maps of the CPU oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring", [1, 2])
def test_census_of_the_drive_with_the_cpu_oracle(ring):
    """256 cells, the outward leg, no inflation, the field seeded at the free cell nearest the vehicle: clusters whose best cell lies
    outside the live window exist, and the way from each best cell leads to the seed at the row's best D"""
    from oracle import oracle
    o = oracle.OracleGvom(ar.DRIVE_RES, ar.DRIVE_ZRES, ar.DRIVE_XY, 8, ring, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
    ref = ar.AtlasRef(afr.DRIVE_A, ar.DRIVE_XY)
    scans = afr.drive_out()
    for pc, ego in scans:
        o.process_pointcloud(pc, ego)
        maps, org = ar.mapper_set(o, o.combine_maps())
        ref.integrate([m.T for m in maps], org)
    xy, A, E = ar.DRIVE_XY, afr.DRIVE_A, ref.E
    vehicle = tuple(int(v) for v in gvom.cells_of(scans[-1][1][:2], ar.DRIVE_RES))
    c = afr.cell_costs(*afr.extent_maps(ref)[0], afr.params())
    seed = afr.nearest_free(c, (vehicle[0] - E[0], vehicle[1] - E[1]))
    f = afr.field(ref, [(seed[0] + E[0], seed[1] + E[1])], afr.params())
    rows, sums, cmap, counts, info = af.of_field(f, ref, 4, 1024)
    _same((rows, sums, cmap, counts, info), af.of_field(f, ref, 4, 1024, loops=True), "the drive")
    n = int(counts[0])
    bx, by = rows[:n, 6] % A + E[0], rows[:n, 6] // A + E[1]
    outside = ~((bx >= org[0]) & (bx < org[0] + xy) & (by >= org[1]) & (by < org[1] + xy))
    print("ring", ring, "kept", n, "frontier cells", int(counts[1]), "largest", int(rows[:n, 1].max()), "best cells outside the window", int(outside.sum()))
    assert (n, int(counts[1]), int(rows[:n, 1].max())) == (38, 2535, 1363)
    assert outside.sum() >= 1
    for r in range(n):
        x, y = int(rows[r, 6] % A), int(rows[r, 6] // A)
        path = [(x, y)]
        while f["dir"][x, y] != cf.GOAL:
            k = int(f["dir"][x, y])
            x, y = x + cf.STEPS[k][0], y + cf.STEPS[k][1]
            path.append((x, y))
        assert path[-1] == tuple(seed) and cf.path_cost(path, f["c"]) == rows[r, 7] == f["D"][path[0]]


# ---- the binding without a library call ---------------------------------------------------------------------------------------------------
class _Lib(object):
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            if name == "gvom_atlas_frontiers":
                args[4]._obj.value = 31
                for k, v in enumerate((5, 3, 40, 2)):
                    args[5][k] = v
                args[6][0], args[6][1] = -40, 3
            if name == "gvom_device_product_export":
                args[4]._obj.value, args[5]._obj.value = 4096, 2
                for k in range(2):
                    args[6][k], args[7][k] = 64, (1, 64)[k]
            return 0
        return entry

    def named(self, name):
        return [a for n, a in self.calls if n == name]


class _Arr(object):
    def __init__(self, a):
        self.a, self.shape = a, a.shape

    def copy_to_host(self):
        return self.a.copy()


def test_frontiers_refuses_what_the_library_would_and_hands_the_rest_over():
    g = gvom.Gvom.__new__(gvom.Gvom)
    g._lib, g._h, g._device = _Lib(), ctypes.c_void_p(1), 0
    g.xy_size, g.xy_resolution = 6, 0.5
    hold = gvom._ProductHold(g, gvom.PRODUCT_ATLAS_FIELD, 21)
    f = gvom.DeviceAtlasField(hold, [1, 9, 100, 1], (-40, 3), 0.5)
    for kw in (dict(min_cells=0), dict(min_cells=1.5), dict(min_cells="a"), dict(min_cells=2 ** 31), dict(max_clusters=0), dict(max_clusters=2 ** 20 + 1),
               dict(max_clusters=None)):
        with pytest.raises(ValueError):
            f.frontiers(**kw)
    assert g._lib.named("gvom_atlas_frontiers") == []
    fr_ = f.frontiers(min_cells=2, max_clusters=2 ** 20)
    (_, field_id, min_cells, cap, _, _, _), = g._lib.named("gvom_atlas_frontiers")
    assert (field_id, min_cells, cap) == (21, 2, 2 ** 20)
    assert isinstance(fr_, gvom.DeviceAtlasFrontiers) and fr_.product_id == 31 and fr_.origin_cells == (-40, 3) and np.array_equal(fr_.origin, (-20.0, 1.5))
    assert (fr_.rounds, fr_.n_clusters, fr_.frontier_cells, fr_.dropped) == (5, 3, 40, 2)
    assert (fr_.clusters.dtype, fr_.sums.dtype, fr_.cluster_map.dtype, fr_.counts.dtype) == (np.int32, np.int64, np.int32, np.int32)
    f.frontiers()
    assert g._lib.named("gvom_atlas_frontiers")[1][2:4] == (4, 1024)


@pytest.mark.parametrize("origin", [(-40, 3), (7, -1000001), (0, 0)])
def test_goals_and_goal_cells_on_a_hand_made_product(origin):
    """three kept clusters of a cap of four in a field of side 64; 0.3 m cells, whose float origin would not round-trip"""
    A, res = 64, 0.3
    rows = np.zeros((4, 8), np.int32)
    #          label cells  box              best cell        best D
    rows[0] = (70, 10, 6, 1, 9, 3, 2 * A + 8, 500)
    rows[1] = (200, 30, 0, 3, 20, 9, 5 * A + 0, 120)
    rows[2] = (900, 10, 4, 14, 6, 20, 20 * A + 63, 120)
    sums = np.array([[75, 20], [300, 180], [50, 170], [0, 0]], np.int64)
    p = gvom.DeviceAtlasFrontiers.__new__(gvom.DeviceAtlasFrontiers)
    p.clusters, p.sums, p.cluster_map = _Arr(rows), _Arr(sums), _Arr(np.zeros((A, A), np.int32))
    p.n_clusters, p._res, p.origin_cells = 3, res, origin
    p.origin = np.array(origin, np.float64) * res
    cells, pick = p.goal_cells()
    assert pick.tolist() == [1, 2, 0] and cells.dtype == np.int64                       # best D ascending, then label
    assert cells.tolist() == [[origin[0] + 0, origin[1] + 5], [origin[0] + 63, origin[1] + 20], [origin[0] + 8, origin[1] + 2]]
    cells_s, pick_s = p.goal_cells(order="size")
    assert pick_s.tolist() == [1, 0, 2] and cells_s.tolist() == [cells.tolist()[0], cells.tolist()[2], cells.tolist()[1]]
    best, centroid, pick_g = p.goals()
    assert pick_g.tolist() == pick.tolist()
    assert np.array_equal(best, (cells + 0.5) * res)                                    # exactly the centres of goal_cells()
    assert np.array_equal(gvom.cells_of(best, res), cells)                              # and they fall back into their cells
    want_c = (np.array([[10.0, 6.0], [5.0, 17.0], [7.5, 2.0]]) + np.array(origin, np.float64) + 0.5) * res
    assert np.array_equal(centroid, want_c)
    with pytest.raises(ValueError):
        p.goals(order="label")
    with pytest.raises(ValueError):
        p.goal_cells(order=None)
    p.n_clusters = 9                                                                    # more kept than rows: the cap bounds n
    assert len(p.goal_cells()[0]) == 4
