"""Cost-to-go fields (gvom_cost_to_go), the part that needs no GPU: the referee's two forms agree, the direction rule on hand-made
cases, header / library / binding agree, the binding's argument checks, the kernels' registers, the metres-to-cells conversion,
and the census of every input tests/test_costfield.py runs."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import costfield_ref as cf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = cf.UNREACHED


@pytest.mark.parametrize("xy", cf.SIZES)
def test_the_two_referee_forms_agree(xy):
    for name, (c, goals, cap) in cf.patterns(xy).items():
        D = cf.dijkstra(c, goals, cap)
        assert np.array_equal(D, cf.relax(c, goals, cap)), (xy, name)
        assert D.dtype == np.int32 and np.array_equal(D, cf.expected(xy, name)[0])
        assert ((D == 0).sum() <= len(goals)) and (D[c == 0] == U).all(), (xy, name)
        if cap:
            full = cf.dijkstra(c, goals)
            assert np.array_equal(D, np.where(full <= cap, full, U)), (xy, name)      # a cut field is the full one, cut
            cut, reach = int(((full != U) & (D == U)).sum()), int((full != U).sum())
            assert reach / 4 <= cut <= 3 * reach / 4, (xy, name, cut, reach)


@pytest.mark.parametrize("xy", cf.SIZES)
def test_the_bellman_check_accepts_dijkstra_and_nothing_else(xy):
    """cf.bellman -- what tests/test_costfield.py holds the 4096-cell random map to -- on every small pattern: no violation on
    Dijkstra's field and the same directions; a single cell raised by 1, lowered by 1, or marked unreached although reachable is
    rejected, each under the condition it breaks"""
    rng = np.random.default_rng(xy)
    for name, (c, goals, cap) in cf.patterns(xy).items():
        D, d, _ = cf.expected(xy, name)
        bad, dirs = cf.bellman(D, c, goals, cap)
        assert bad == {} and np.array_equal(dirs, d), (xy, name, bad)
        inner = np.argwhere((D != U) & (D != 0))
        if len(inner) == 0:
            continue
        for x, y in inner[rng.choice(len(inner), min(6, len(inner)), replace=False)]:
            for delta, word in ((1, "no_match"), (-1, "offers_less")):
                M = D.copy()
                M[x, y] += delta
                bad, _ = cf.bellman(M, c, goals, cap)
                # raised: a neighbour now offers less than the cell holds; lowered: none of its offers equals it any more
                assert word in bad or "no_match" in bad or "offers_less" in bad, (xy, name, x, y, delta, bad)
            M = D.copy()
            M[x, y] = U
            bad, _ = cf.bellman(M, c, goals, cap)
            assert "left_out" in bad, (xy, name, x, y, bad)         # (its best offer is the value it had: at or below the cap)
    c, goals, cap = cf.patterns(xy)["random"]
    D = cf.expected(xy, "random")[0]
    gx, gy = np.argwhere(D == 0)[0]
    for M, word in ((np.where(D == 0, 5, D), "goal"), (np.where(c == 0, 7, D), "blocked")):
        assert word in cf.bellman(M, c, goals, cap)[0], (xy, word)
    twice = D.copy()
    twice[D != U] *= 2                                            # every value doubled: consistent with nothing
    assert cf.bellman(twice, c, goals, cap)[0]
    c, goals, cap = cf.patterns(xy)["random_cut"]
    over = cf.dijkstra(c, goals)                                   # the uncut field under the cut's cap
    assert "above_cap" in cf.bellman(over, c, goals, cap)[0]


def test_the_closed_form_of_the_open_map_and_the_large_patterns():
    for xy, goal in ((100, (0, 0)), (129, (0, 0)), (65, (64, 0)), (50, (17, 30))):
        assert np.array_equal(cf.open_field(xy, goal), cf.dijkstra(np.ones((xy, xy), np.int32), [goal])), (xy, goal)
    for xy in (65, 129):                                           # large_patterns builds what patterns builds, without the other ten
        small, large = cf.patterns(xy), cf.large_patterns(xy)
        for name in ("open", "random", "seventeen_goals"):
            assert np.array_equal(small[name][0], large[name][0]) and np.array_equal(small[name][1], large[name][1]), (xy, name)
        c, goals, cap, D, d, info = cf.large_expected(xy, "random_cut")
        assert cap == small["random_cut"][2] and np.array_equal(D, cf.expected(xy, "random_cut")[0]) and info == cf.expected(xy, "random_cut")[2]
    assert cf.LARGE == (1024, 4096) and [(xy + cf.TILE - 1) // cf.TILE for xy in cf.SIZES[-1:] + cf.LARGE] == [5, 32, 128]
    assert 129 % cf.TILE == 1                                      # the last tile of 129 cells is one cell wide


def test_weights_and_the_early_stop_of_the_sweeps():
    c = np.array([[1, 1], [65535, 65535]], np.int32)
    D = cf.dijkstra(c, [(0, 0)])
    assert D.tolist() == [[0, 10], [5 * 65536, 10 + 5 * 65536]]                          # straight 5 (cu + cv); the diagonal, 7 * 65536, is dearer
    assert cf.dijkstra(np.array([[1, 9], [9, 1]], np.int32), [(0, 0)])[1, 1] == 14            # diagonal 7 (cu + cv)
    assert 7 * (65535 + 65535) < 2 ** 20
    assert cf.dijkstra(c, [(0, 0)], max_cost=5 * 65536).tolist() == [[0, 10], [5 * 65536, U]]
    serp, goals, _ = cf.patterns(33)["serpentine"]
    full, part = cf.dijkstra(serp, goals), cf.relax(serp, goals, sweeps=40)
    assert ((part == U) | (part >= full)).all() and (part != full).any() and (part[full == U] == U).all()


@pytest.mark.parametrize("xy,inner", [(33, 256), (33, 3), (65, 256), (100, 256), (100, 5)])
def test_the_tile_schedule_reaches_the_same_fixed_point(xy, inner):
    """the solver's schedule simulated on the CPU (cf.tiled): active tiles, halos as the round found them, rim wake-ups, a tile
    that runs out of sweeps marking itself; measured rounds at 100 cells, inner 256: open 5, random 11, walls 14, serpentine 155"""
    rounds = {}
    for name, (c, goals, cap) in cf.patterns(xy).items():
        D, n, relaxations, converged = cf.tiled(c, goals, cap, inner)
        assert converged and np.array_equal(D, cf.expected(xy, name)[0]), (xy, name, inner)
        assert relaxations <= n * ((xy + 31) // 32) ** 2
        rounds[name] = n
    assert rounds["all_blocked"] == rounds["single_free_goal"] == 1 and rounds["serpentine"] > rounds["open"]
    c, goals, _ = cf.patterns(xy)["serpentine"]
    full = cf.expected(xy, "serpentine")[0]
    part, n, _, converged = cf.tiled(c, goals, 0, inner, max_rounds=2)
    assert n == 2 and not converged and ((part == U) | (part >= full)).all() and (part != full).any() and (part[full == U] == U).all()


def test_the_direction_rule_on_hand_made_cases():
    # a tie: from (1, 1) of an open 3 x 3 map towards the goals (2, 1) [k = 0] and (1, 2) [k = 2] both cost 10: the smallest k wins
    one = np.ones((3, 3), np.int32)
    D = cf.dijkstra(one, [(2, 1), (1, 2)])
    d = cf.directions(D, one)
    assert D[1, 1] == 10 and sum(int(m[1, 1]) for m in cf.matches(D, one)) == 2 and d[1, 1] == 0
    assert d[2, 1] == d[1, 2] == cf.GOAL and d[2, 2] == 4 and d[0, 0] == 0 and D[0, 0] == 24      # (2, 2): k = 4 and 6; (0, 0): k = 0, 1, 2
    # a diagonal forbidden by ONE blocked corner cell: (0, 0) -> (1, 1) with (1, 0) blocked goes round through (0, 1)
    c = np.ones((3, 3), np.int32)
    c[1, 0] = 0
    D = cf.dijkstra(c, [(1, 1)])
    d = cf.directions(D, c)
    assert D[0, 0] == 20 and d[0, 0] == 2 and D[1, 0] == U and d[1, 0] == cf.NONE
    assert cf.dijkstra(c, [(1, 1)], corner_rule=False)[0, 0] == 14
    assert D[2, 0] == 20 and d[2, 0] == 2                                               # the other side of the blocked cell, likewise
    # 4 x 4: a wall with its gap at the top; unreached pocket; an unsettled cell in a field that is not final
    c = np.ones((4, 4), np.int32)
    c[2, 0:3] = 0
    D = cf.dijkstra(c, [(3, 0)])
    d = cf.directions(D, c)
    assert D[3, 3] == 30 and D[2, 3] == 40 and D[1, 3] == 50 and D[1, 2] == 60 and D[0, 1] == 74 and D[0, 0] == 84
    assert d[3, 1] == 6 and d[2, 3] == 0 and d[1, 3] == 0 and d[1, 2] == 2 and d[0, 0] == 1      # (0, 0): k = 1 and 2 tie
    assert cf.path_cost([(0, 0), (0, 1), (0, 2), (1, 3), (2, 3), (3, 3), (3, 2), (3, 1), (3, 0)], c) >= D[0, 0]
    stale = D.copy()
    stale[0, 0] += 1
    assert cf.directions(stale, c)[0, 0] == cf.UNSETTLED
    sealed = np.ones((4, 4), np.int32)
    sealed[1, :] = 0
    assert (cf.directions(cf.dijkstra(sealed, [(3, 3)]), sealed)[0, :] == cf.NONE).all()


def test_travcost_from_the_definition():
    pos = np.array([[0, 50, 51, 10]], np.int32)
    neg = np.array([[0, 0, 0, 3]], np.int32)
    vis = np.array([[0, 1, 1, 1]], np.int32)
    rough = np.array([[-1.0, -7.0, float("nan"), -20.0]])
    d2 = np.array([[9, 4, 0, 0]], np.int32)
    P = dict(density_threshold=50, base=2, soft_weight=10, unknown_cost=100, rough_weight=3, min_roughness=-10.0, max_roughness=-4.0)
    assert cf.travcost(pos, neg, vis, rough, d2, P).tolist() == [[2 + 100 + 300, 2 + 500 + 3 * 50, 0, 0]]
    assert cf.travcost(pos, neg, vis, rough, d2, dict(P, include_negative=False)).tolist() == [[402, 652, 0, 2 + 100]]
    assert cf.travcost(pos, neg, vis, rough, d2, dict(P, inflation_cells2=4)).tolist() == [[402, 0, 0, 0]]
    assert cf.travcost(pos, neg, vis, rough, d2, dict(P, unknown_blocks=True)).tolist() == [[0, 652, 0, 0]]
    assert cf.travcost(pos, neg, vis, rough, d2, dict(P, soft_weight=65535, density_threshold=50.5)).tolist()[0][1:3] == [65535, 0]
    assert cf.roughness_q(np.array([-10.0, -9.99, -4.0, 0.0, -4.06]), 1, -10.0, -4.0).tolist() == [0, 0, 100, 100, 99]


def test_abi_10_the_symbol_the_defines_and_the_binding():
    import gvom
    header = open(os.path.join(ROOT, "include", "gvom_hip.h")).read()
    assert int(re.search(r"#define\s+GVOM_ABI_VERSION\s+(\d+)", header).group(1)) == 10
    assert gvom.ABI_VERSION == 10 and gvom.load_library().gvom_abi_version() == 10
    assert re.search(r"\bint\s+gvom_cost_to_go\s*\(", header) and "typedef struct gvom_ctg_params" in header
    for word, value in (("GVOM_PRODUCT_COSTFIELD", gvom.PRODUCT_COSTFIELD), ("GVOM_CTG_UNREACHED", gvom.CTG_UNREACHED),
                        ("GVOM_CTG_GOAL", gvom.CTG_GOAL), ("GVOM_CTG_NONE", gvom.CTG_NONE), ("GVOM_CTG_UNSETTLED", gvom.CTG_UNSETTLED),
                        ("GVOM_CTG_MAX_COST", gvom.CTG_MAX_COST), ("GVOM_CTG_NO_NEGATIVE", 1), ("GVOM_CTG_UNKNOWN_BLOCKS", 2)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % word, header).group(1)) == value, word
    assert (gvom.PRODUCT_COSTFIELD, gvom.CTG_UNREACHED, gvom.CTG_GOAL, gvom.CTG_UNSETTLED, gvom.CTG_NONE) == (7, 2 ** 31 - 1, 8, 254, 255)
    assert (cf.UNREACHED, cf.GOAL, cf.UNSETTLED, cf.NONE, cf.MAX_COST) == (gvom.CTG_UNREACHED, 8, 254, 255, gvom.CTG_MAX_COST)
    assert gvom.CTG_STEPS == cf.STEPS
    L = ctypes.CDLL(gvom.library_path())
    assert hasattr(L, "gvom_cost_to_go")
    row = [r for r in gvom.ABI if r[0] == "gvom_cost_to_go"]
    assert len(row) == 1 and len(row[0][2]) == 12
    nm = subprocess.run(["nm", "-D", "--defined-only", gvom.library_path()], capture_output=True, text=True, check=True)
    assert re.search(r" T gvom_cost_to_go$", nm.stdout, re.M)
    # the struct as the header declares it: three doubles, five int32
    body = re.search(r"typedef struct gvom_ctg_params \{(.*?)\} gvom_ctg_params;", header, re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", body)
    assert names == [n for n, _ in gvom.GvomCtgParams._fields_] and ctypes.sizeof(gvom.GvomCtgParams) == 48
    for m in ("cost_to_go_of", "cost_to_go_of_device"):
        assert callable(getattr(gvom.Gvom, m))
    assert callable(gvom.DeviceMaps.cost_to_go)
    for attr in ("copy_to_host", "release", "path_from", "__enter__", "__exit__"):
        assert callable(getattr(gvom.DeviceCostField, attr))
    for root, _, files in os.walk(os.path.join(ROOT, "g-vom_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h")) or f == "Makefile":
                assert "oracle" not in open(os.path.join(root, f), errors="replace").read().lower(), f
    assert "gvom_costfield" in open(os.path.join(ROOT, "g-vom_amd", "Makefile")).read()


def test_the_four_kernels_use_no_scratch_and_the_solver_fits_four_waves_per_simd():
    import gvom
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    if not os.path.exists(os.path.join(kernel_regs.LLVM, "clang-offload-bundler")):
        pytest.skip("no ROCm LLVM tools")
    kernels = {k: v for k, v in kernel_regs.kernels(gvom.library_path()).items() if "k_ctg_" in k or "k_travcost" in k}
    assert len(kernels) == 4, sorted(kernels)
    for k, v in kernels.items():
        assert v["scratch"] == 0, (k, v)
        assert v["lds"] <= 8192, (k, v)                       # (34 x 34 x 6 bytes and a word: well under 64 KB)
        if "k_ctg_relax" in k:
            assert v["vgpr"] <= 128 and v["lds"] >= 34 * 34 * 6, (k, v)


def _bare(xy=16, res=0.4):
    import gvom
    g = gvom.Gvom.__new__(gvom.Gvom)              # no handle, no library: a call that got as far as the library would not raise ValueError
    g.xy_size, g.xy_resolution, g._lib, g._h = xy, res, None, None
    return gvom, g


def test_python_arguments_are_checked_before_any_library_call():
    gvom, g = _bare()
    cost = np.ones((16, 16), np.int32)
    ok = [(1, 2)]
    for bad, word in ((np.ones((16, 15)), "shape"), (np.full((16, 16), -1), "0 .. 65535"), (np.full((16, 16), 65536), "0 .. 65535"),
                      (np.full((16, 16), float("nan")), "finite"), (np.full((16, 16), 1.5), "whole")):
        with pytest.raises(ValueError, match=word):
            g.cost_to_go_of(bad, ok)
    for bad, word in (([], "shape"), ([(1, 2, 3)], "shape"), (np.zeros((65537, 2), np.int32), "shape"), ([(0, 16)], "outside the window"),
                      ([(-1, 0)], "outside the window"), ([(0.5, 1)], "whole"), ([(float("nan"), 1)], "finite")):
        with pytest.raises(ValueError, match=word):
            g.cost_to_go_of(cost, bad)
        with pytest.raises(ValueError, match=word):
            g.cost_to_go_of_device(1 << 20, bad)
    for bad in (0, -5, 2 ** 30 + 1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="max_cost"):
            g.cost_to_go_of(cost, ok, max_cost=bad)
    for bad in (-1, 0.5, 2 ** 31):
        with pytest.raises(ValueError, match="max_rounds"):
            g.cost_to_go_of(cost, ok, max_rounds=bad)
    with pytest.raises(ValueError, match="cost_ptr"):
        g.cost_to_go_of_device(0, ok)
    assert gvom._ctg_max_cost(None) == 0 and gvom._ctg_max_cost(2 ** 30) == 2 ** 30 and gvom._ctg_max_cost(1) == 1
    # the map-set route: DeviceMaps.cost_to_go checks before it touches its owner's library
    m = gvom.DeviceMaps.__new__(gvom.DeviceMaps)
    m._owner, m.set_id, m.origin = g, 1, np.zeros(3)
    for kw, word in ((dict(inflation_radius=-1.0), "inflation_radius"), (dict(inflation_radius=0.1), "inflation_radius"),
                     (dict(inflation_radius=float("nan")), "inflation_radius"), (dict(density_threshold=float("nan")), "density_threshold"),
                     (dict(unknown="maybe"), "unknown"), (dict(unknown=-1), "unknown"), (dict(unknown=65536), "unknown"),
                     (dict(base=0), "base"), (dict(soft_weight=-1), "soft_weight"), (dict(soft_weight=70000), "soft_weight"),
                     (dict(rough_weight=1.5), "rough_weight"), (dict(rough_weight=1), "roughness_range"),
                     (dict(rough_weight=1, roughness_range=(0.0, 0.0)), "roughness_range"),
                     (dict(rough_weight=1, roughness_range=(0.0, float("inf"))), "roughness_range"), (dict(max_cost=0), "max_cost"),
                     (dict(max_rounds=-1), "max_rounds")):
        with pytest.raises(ValueError, match=word):
            m.cost_to_go([(1.0, 1.0)], **kw)
    with pytest.raises(ValueError, match="outside the window"):
        m.cost_to_go([(6.4, 0.0)])                                # 16 cells of 0.4 m: x = 6.4 is cell 16
    with pytest.raises(ValueError, match="outside the window"):
        m.cost_to_go([(16, 0)], goals_in_cells=True)
    P, flags = gvom._ctg_params(0.4, 2.0, 50, False, "blocked", 1, 2, 3, (-10, 0))
    assert (P.inflation_cells2, P.base, P.soft_weight, P.rough_weight, P.unknown_cost, flags) == (25, 1, 2, 3, 0, 3)
    P, flags = gvom._ctg_params(0.4, None, 12.5, True, 77, 9, 0, 0, None)
    assert (P.inflation_cells2, P.density_threshold, P.unknown_cost, P.base, flags) == (0, 12.5, 77, 9, 0)
    for obj in (g, m):
        for a in ("_h", "_held"):
            obj.__dict__.pop(a, None)                             # (nothing for __del__ to destroy)


def test_world_metres_to_cells_at_cell_edges_and_negative_origins():
    import gvom
    w2c = gvom.world_to_cells
    res = 0.4
    for origin in ((0.0, 0.0, 0.0), (-12.8, -6.4, 0.0), (-13.2, 2.4, 0.0), (4.0, -0.4, 1.0)):
        o = np.round(np.array(origin[:2]) / res)
        pts, want = [], []
        for cx, cy in ((0, 0), (5, 9), (31, 63)):
            lo = (o + (cx, cy)) * res
            for fx, fy in ((0.0, 0.0), (0.5, 0.5), (0.999, 0.001)):
                pts.append((lo[0] + fx * res, lo[1] + fy * res))
                want.append((cx, cy))
        got = w2c(np.array(pts), res, origin)
        exact = np.floor(np.array(pts) / res) - o                  # (a point ON an edge belongs to the cell float64 division says)
        assert np.array_equal(got, exact.astype(np.int64)) and np.array_equal(got, cf.world_to_cells(pts, res, origin))
        inside = [k for k in range(len(pts)) if k % 3]              # off the lower edge: the cell is beyond doubt
        assert np.array_equal(got[inside], np.array(want)[inside]), origin
    assert w2c([(-0.01, -0.4)], 0.4, (0, 0, 0)).tolist() == [[-1, -1]] and w2c([(-0.4, 0.39)], 0.4, (-0.4, 0, 0)).tolist() == [[0, 0]]
    assert w2c([(-12.9, 0.0)], 0.4, (-12.8, -12.8, 0)).tolist() == [[-1, 32]]


# floors: about four fifths of what the referee measures (sum over the patterns of a size)
CENSUS_FLOOR = {
    16: dict(blocked=900, reached=1300, pocket=200, cut=240, corner_rule=900, ties=600, crossings3=0),
    31: dict(blocked=3000, reached=5900, pocket=55, cut=950, corner_rule=3600, ties=2800, crossings3=0),
    32: dict(blocked=3200, reached=6300, pocket=55, cut=1000, corner_rule=3800, ties=3000, crossings3=0),
    33: dict(blocked=3300, reached=6700, pocket=90, cut=1100, corner_rule=4300, ties=3200, crossings3=400),
    50: dict(blocked=7900, reached=15000, pocket=140, cut=2500, corner_rule=9700, ties=7800, crossings3=1800),
    64: dict(blocked=12900, reached=25000, pocket=290, cut=4100, corner_rule=15900, ties=13000, crossings3=3400),
    65: dict(blocked=13200, reached=26000, pocket=270, cut=4300, corner_rule=16500, ties=13500, crossings3=9000),
    100: dict(blocked=31000, reached=61000, pocket=700, cut=10000, corner_rule=39000, ties=32000, crossings3=33000),
    129: dict(blocked=51000, reached=103000, pocket=1000, cut=16900, corner_rule=66000, ties=55000, crossings3=66000),
}


@pytest.mark.parametrize("xy", cf.SIZES)
def test_census_of_the_synthetic_patterns(xy):
    """Measured on the referee, summed over the patterns of a size (blocked / reached / unreachable pocket / cut off by max_cost /
    D differs with the corner rule off / direction ties / shortest path crosses >= 3 tile boundaries):
       16:  1110 /  1657 / 256 /   305 /  1155 /   793 /     0        31:  3793 /  7406 /  72 /  1222 /  4578 /  3530 /     0
       32:  3998 /  7925 /  74 /  1315 /  4802 /  3782 /     0        33:  4201 /  8452 / 114 /  1390 /  5429 /  4071 /   551
       50:  9916 / 19239 / 181 /  3164 / 12231 /  9779 /  2278        64: 16186 / 31511 / 366 /  5185 / 19943 / 16394 /  4258
       65: 16507 / 32694 / 342 /  5382 / 20712 / 16904 / 11379       100: 39096 / 77302 / 897 / 12705 / 48941 / 41150 / 42208
      129: 64563 / 129251 / 1302 / 21217 / 82551 / 69358 / 83125
    (a map of one tile has no tile boundary: the crossings are held from 33 cells on)"""
    total, per = {}, {}
    for name, (c, goals, cap) in cf.patterns(xy).items():
        per[name] = cf.census(c, goals, cap)
        for k, v in per[name].items():
            total[k] = total.get(k, 0) + v
    for k, floor in CENSUS_FLOOR[xy].items():
        assert total[k] >= floor, (xy, k, total[k], floor)
    assert per["diagonal_wall"]["corner_rule"] > 0 and per["pocket"]["pocket"] > 0 and per["open"]["ties"] > 0
    assert per["all_blocked"]["reached"] == 0 and per["single_free_goal"]["reached"] == 1
    assert per["seventeen_goals"]["blocked"] > 0 and cf.expected(xy, "seventeen_goals")[2][1] == 13     # 12 free + one twice
    assert cf.expected(xy, "two_goals")[2][1] == 1 and cf.expected(xy, "all_blocked")[2] == (0, 0)


@pytest.mark.parametrize("name", cf.SCENES)
def test_census_of_the_map_set_scenes(name):
    """measured at the last combine (one_round / two_rounds): 166 / 348 cells with 0 < positive <= 50, 387 / 587 with positive > 50,
    5 / 1 with negative > 0, 378 / 368 never observed, 2311 / 2618 with 0 < q < 100 in ROUGHNESS_RANGE (455 / 535 at 100, 1330 / 943
    at 0).  Floors: 100, 250, 1, 250, 1500."""
    import clearance_ref as cr
    import obstacle_scenes as ob
    from oracle import oracle
    o = oracle.OracleGvom(*ob.params(name))
    for pc, ego in ob.scans(name):
        o.process_pointcloud(pc, ego)
        maps = o.combine_maps()
    pos, neg, rough, vis = maps[1], maps[2], maps[3], maps[4]
    q = cf.roughness_q(rough, 1, *cf.ROUGHNESS_RANGE)
    counts = (int(((pos > 0) & (pos <= 50)).sum()), int((pos > 50).sum()), int((neg > 0).sum()), int((vis == 0).sum()),
              int(((q > 0) & (q < 100)).sum()))
    assert all(c >= f for c, f in zip(counts, (100, 250, 1, 250, 1500))), (name, counts)
    assert (q == 0).any() and (q == 100).any()
    # every variant blocks a different set of cells, and inflation blocks more
    blocked = []
    for v in cf.VARIANTS:
        P = cf.variant_params(v, ob.XY_RES, cr.max_cells2_of)
        d2 = cr.separable(cr.obstacle_mask(pos, neg if v["include_negative"] else None, 50), P["inflation_cells2"])
        c = cf.travcost(pos, neg, vis, rough, d2, P)
        blocked.append(int((c == 0).sum()))
        assert c.min() == 0 and (c.max() > 1) == (v != cf.VARIANTS[0] and v != cf.VARIANTS[1])
    assert blocked[0] < blocked[1] and blocked[0] < blocked[3] < blocked[6] and blocked[3] < blocked[4], blocked
