"""Frontier extraction (gvom_frontiers), the part that needs no GPU: header, library and binding agree; the referee's two forms agree
on every pattern; the simulated round schedule converges to the same labels; the census of every input tests/test_frontier.py runs;
what the three binding entry points hand to the library; the product's layout under sanitizers; the kernels' resources."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import costfield_ref as cf
import frontier_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbol_the_defines_and_the_binding():
    import gvom
    header = open(os.path.join(ROOT, "include", "gvom_hip.h")).read()
    assert int(re.search(r"#define\s+GVOM_ABI_VERSION\s+(\d+)", header).group(1)) == 10 == gvom.ABI_VERSION
    assert int(re.search(r"#define\s+GVOM_PRODUCT_FRONTIERS\s+(\d+)", header).group(1)) == gvom.PRODUCT_FRONTIERS == 16
    assert int(re.search(r"#define\s+GVOM_CTG_UNREACHED\s+(\d+)", header).group(1)) == fr.UNREACHED == gvom.CTG_UNREACHED
    assert not re.search(r"#define\s+GVOM_PRODUCT_\w+\s+(8|9|11|13|15)\b", header)        # kinds 8, 9, 11, 13 and 15 stay unassigned
    assert re.search(r"\bint\s+gvom_frontiers\s*\(", header)
    for word in ("4-connected", "window edge", "3-D", "splitting", "distance-to-robot", "sharded handles", "early stop"):
        assert word in header[header.index("frontier extraction"):], word                # NOT PROVIDED, said in the header
    nm = subprocess.run(["nm", "-D", "--defined-only", gvom.library_path()], capture_output=True, text=True, check=True)
    assert re.search(r" T gvom_frontiers$", nm.stdout, re.M) and hasattr(ctypes.CDLL(gvom.library_path()), "gvom_frontiers")
    row = [r for r in gvom.ABI if r[0] == "gvom_frontiers"]
    assert len(row) == 1 and len(row[0][2]) == 11
    assert (gvom.FRONTIER_NONE, gvom.FRONTIER_SMALL, gvom.FRONTIER_MAX_CLUSTERS) == (fr.NONE, fr.SMALL, 1 << 20) == (-1, -2, 1 << 20)
    assert gvom._PRODUCT_DTYPES[gvom.PRODUCT_FRONTIERS] == (np.int32, np.int64, np.int32, np.int32)
    for m in ("frontiers_of", "frontiers_of_device"):
        assert callable(getattr(gvom.Gvom, m))
    assert callable(gvom.DeviceCostField.frontiers)
    for attr in ("copy_to_host", "goals", "release", "__enter__", "__exit__"):
        assert callable(getattr(gvom.DeviceFrontiers, attr))
    assert "gvom_frontier" in open(os.path.join(ROOT, "g-vom_amd", "Makefile")).read()


def test_the_two_referee_forms_agree_on_every_pattern():
    for xy in fr.SIZES:
        for name, (c, vis, D, mc, cap) in fr.patterns(xy).items():
            if xy > 65 and name.startswith("random") and name != "random_m2_c7":         # (the same maps under other limits)
                continue
            a, b = fr.expected(xy, name), fr.product_loops(c, vis, D, mc, cap)
            for u, v, what in zip(a, b, ("clusters", "sums", "cluster map", "counts", "info")):
                assert np.array_equal(np.asarray(u), np.asarray(v)), (xy, name, what)
            assert a[0].dtype == np.int32 and a[1].dtype == np.int64 and a[2].dtype == np.int32 and a[3].dtype == np.int32
            n = min(int(a[3][0]), cap)
            assert not a[0][n:].any() and not a[1][n:].any()                              # rows past the kept clusters are zero
            assert (np.diff(a[0][:n, 0]) > 0).all()                                       # ascending label order
    # by hand: 5 x 5, the middle row unknown: the rows above and below it are frontiers, apart from one another
    vis = np.ones((5, 5), np.int32)
    vis[2, :] = 0
    c = np.ones((5, 5), np.uint16)
    c[1, 2] = 0                                                                           # a blocked cell cuts the upper row
    D = np.arange(25, dtype=np.int32).reshape(5, 5)[:, ::-1].copy()                      # D[y, x] = 5 y + 4 - x
    D[3, 4] = fr.UNREACHED
    rows, sums, cmap, counts, info = fr.product(c, vis, D, 2, 4)
    assert cmap.tolist() == [[-1] * 5, [0, 0, -1, 1, 1], [-1] * 5, [2, 2, 2, 2, -1], [-1] * 5]
    assert rows[:3].tolist() == [[5, 2, 0, 1, 1, 1, 6, 8], [8, 2, 3, 1, 4, 1, 9, 5], [15, 4, 0, 3, 3, 3, 18, 16]]
    assert sums[:3].tolist() == [[1, 2], [7, 2], [6, 12]] and counts.tolist() == [3, 8, 8, 4] and info == [3, 8, 0]
    assert fr.product(c, vis, D, 3, 4)[4] == [1, 8, 2] and fr.product(c, vis, None, 3, 4)[0][0].tolist() == [15, 5, 0, 3, 4, 3, 15, fr.UNREACHED]


def test_the_simulated_round_schedule_converges_to_the_same_labels():
    rounds = {}
    for xy, names in ((33, ("disc", "serpentine", "spiral", "u_shape", "diagonal_pairs", "cut_ring", "random_m1_c7")),
                      (65, ("disc", "serpentine", "u_shape", "diagonal_pairs", "random_m1_c7")), (100, ("disc", "u_shape", "diagonal_pairs"))):
        for name in names:
            c, vis, D, _, _ = fr.patterns(xy)[name]
            mask = fr.frontier_mask(c, vis, D)
            L, rounds[xy, name], relaxed = fr.tiled(mask)
            assert np.array_equal(L, fr.labels_scipy(mask)), (xy, name)
            assert relaxed >= rounds[xy, name] - 1
    assert rounds[65, "serpentine"] > 4 * rounds[65, "disc"] and rounds[33, "serpentine"] > rounds[33, "disc"], rounds
    assert rounds[65, "diagonal_pairs"] >= 2                                              # a label crosses the corner of four tiles


def test_census_of_every_gpu_input():
    """floors: what the inputs held when they were written; the referee alone meets them"""
    for xy in fr.SIZES:
        n = {name: fr.census(xy, name) for name in fr.patterns(xy)}
        assert n["nothing_known"]["frontier"] == 0 and n["all_known"]["frontier"] == 0
        assert n["corners"]["frontier"] == n["corners"]["kept"] == 4 and n["corners"]["largest"] == 1
        for name in ("disc", "serpentine", "spiral", "u_shape", "tie", "no_D_disc"):
            assert n[name]["kept"] == 1 and n[name]["dropped"] == 0, (xy, name, n[name])
        assert n["serpentine"]["frontier"] >= xy * xy // 2 and n["spiral"]["frontier"] >= xy * xy // 2 - 2 * xy
        c, vis, D, _, _ = fr.patterns(xy)["spiral"]
        label = int(fr.expected(xy, "spiral")[0][0, 0])
        # the least index has the path on both sides (the corner cell itself has no unknown neighbour: it is no frontier cell)
        assert label == 1 and vis[0, 2] > 0 and vis[2, 0] > 0 and not fr.frontier_mask(c, vis, D)[0, 0]
        # the U's arms join only at the bottom row
        c, vis, D, _, _ = fr.patterns(xy)["u_shape"]
        upper = vis.copy()
        upper[xy - 2:, :] = 0
        assert len(np.unique(fr.labels_scipy(fr.frontier_mask(c, upper, D)))) == 3       # (-1 and two arms)
        # the diagonal pairs exist: cells of one cluster that touch only by a corner, and under 4-connectivity they come apart
        c, vis, D, _, _ = fr.patterns(xy)["diagonal_pairs"]
        mask = fr.frontier_mask(c, vis, D)
        four = fr.ndimage.label(mask)[1]
        eight = n["diagonal_pairs"]["kept"]
        assert four - eight == (1 if xy < 48 else 2 if xy < 80 else 3), (xy, four, eight)
        if xy >= 48:
            assert mask[31, 31] and mask[32, 32] and not mask[31, 32] and not mask[32, 31]
        if xy >= 80:
            assert mask[63, 64] and mask[64, 63] and not mask[63, 63] and not mask[64, 64]
        assert n["cut_ring"]["kept"] >= 4 and n["cut_ring"]["blocked_beside_unknown"] > 0 and n["cut_ring"]["unreached"] >= 2 * xy
        assert n["cut_ring"]["frontier"] < n["disc"]["frontier"]
        assert n["tie"]["best_ties"] == 1 and fr.expected(xy, "tie")[0][0, 6] == fr.expected(xy, "tie")[0][0, 0]
        assert n["disc"]["best_is_not_label"] == 1
        assert fr.expected(xy, "no_D_disc")[0][0, 7] == fr.UNREACHED
        r = {k: v for k, v in n.items() if k.startswith("random")}
        assert r["random_m1_c7"]["beyond_cap"] >= 1 and r["random_m1_c1"]["beyond_cap"] >= 7 and r["random_m1_cbig"]["beyond_cap"] == 0
        assert r["random_m2_c7"]["dropped"] >= 4 and r["random_m5_c1"]["dropped"] > r["random_m2_c7"]["dropped"], (xy, r)
        assert r["random_m1_c7"]["frontier"] >= 100
        assert n["no_D_random"]["dropped"] >= 5 and n["no_D_random"]["kept"] >= 3
        if xy >= 64:
            assert r["random_m1_cbig"]["kept"] >= 75 and r["random_m1_cbig"]["frontier"] >= 1500 and r["random_m1_cbig"]["best_ties"] >= 1
    case, want = fr.large_case(1024)
    assert want[3][0] > case[4] and want[3][1] > 400000 and want[0][0, 1] > 60000 and want[4][2] > 100, (want[3], want[4])


@pytest.mark.parametrize("name", cf.SCENES)
def test_census_of_the_scenes(name):
    """the maps of the last combine from the CPU oracle, a plain cost map, the field from the ego's cell: with min_cells 3 both scenes
    keep at least one cluster (measured: one_round 38 kept clusters and 9 dropped of 294 frontier cells, two_rounds 29 and 10 of 253)"""
    import obstacle_scenes as ob
    from oracle import oracle
    o = oracle.OracleGvom(*ob.params(name))
    for pc, ego in ob.scans(name):
        o.process_pointcloud(pc, ego)
        maps = o.combine_maps()
    origin, pos, neg, rough, vis = maps[0], maps[1], maps[2], maps[3], maps[4]
    c = cf.travcost(pos, neg, vis, rough, None, dict(density_threshold=cf.SCENE_THRESHOLD))
    cell = cf.world_to_cells([ego[:2]], ob.XY_RES, origin)
    D = cf.dijkstra(c, cell)
    rows, sums, cmap, counts, info = fr.product(np.asarray(c).T, np.asarray(vis).T, np.asarray(D).T, 3, 64)
    print(name, counts, info)
    assert counts[0] >= 1 and counts[1] > 20 and info[2] >= 1, (name, counts, info)


class _Recorder(object):
    """stands in for the loaded library: notes gvom_frontiers' arguments, the maps read through their pointers at call time"""

    def __init__(self, n2):
        self.calls, self.n2 = [], n2

    def __getattr__(self, name):
        def entry(*args):
            if name == "gvom_frontiers":
                got = list(args)
                for k, t in ((3, ctypes.c_uint16), (4, ctypes.c_int32), (5, ctypes.c_int32)):
                    p = got[k].value if isinstance(got[k], ctypes.c_void_p) else got[k]
                    got[k] = None if not p else (tuple((t * self.n2).from_address(p)) if got[6] == 0 else p)
                self.calls.append(got)
                args[9]._obj.value = 5
                for k, v in enumerate((3, 2, 40, 1)):
                    args[10][k] = v
            elif name == "gvom_device_product_export":
                args[4]._obj.value = 4096
            return 0
        return entry


def _bare(xy=6, res=0.5):
    import gvom
    g = gvom.Gvom.__new__(gvom.Gvom)
    g.xy_size, g.xy_resolution, g._lib, g._h = xy, res, _Recorder(xy * xy), None
    return gvom, g


def test_what_the_three_entry_points_hand_to_the_library():
    gvom, g = _bare()
    xy = 6
    c = (np.arange(36).reshape(6, 6) * 1000 % 65536)                                       # [x, y], not symmetric
    vis = np.arange(36).reshape(6, 6) % 3
    D = np.arange(36).reshape(6, 6) - 7
    f = g.frontiers_of(c.astype(np.float64), np.ascontiguousarray(vis), np.asfortranarray(D), min_cells=2, max_clusters=9, origin=(1.0, -2.0))
    a = g._lib.calls[0]
    assert a[1:3] == [-1, -1] and a[6:9] == [0, 2, 9]
    assert a[3] == tuple(c.ravel(order="F")) and a[5] == tuple(vis.ravel(order="F")) and a[4] == tuple(D.ravel(order="F"))   # x fastest
    assert (f.rounds, f.n_clusters, f.frontier_cells, f.dropped, f.product_id) == (3, 2, 40, 1, 5) and f.origin.tolist() == [1.0, -2.0]
    g.frontiers_of(c, vis)
    a = g._lib.calls[1]
    assert a[4] is None and a[7:9] == [4, 1024]
    g.frontiers_of_device(1 << 20, 1 << 21, min_cells=1, max_clusters=1)
    g.frontiers_of_device(1 << 20, 1 << 21, 1 << 22)
    a, b = g._lib.calls[2:4]
    assert a[1:9] == [-1, -1, 1 << 20, None, 1 << 21, 1, 1, 1] and b[3:6] == [1 << 20, 1 << 22, 1 << 21]
    # the ids route: a field's own method hands over both ids and no pointer
    m = gvom.DeviceMaps.__new__(gvom.DeviceMaps)
    m._owner, m.set_id, m.origin = g, 17, np.zeros(3)
    field = gvom.DeviceCostField(gvom._ProductHold(g, gvom.PRODUCT_COSTFIELD, 23), [1, 1, 1, 1], origin=(0.5, 1.5))
    fx = field.frontiers(m, min_cells=6, max_clusters=11)
    a = g._lib.calls[4]
    assert a[1:9] == [23, 17, None, None, None, 0, 6, 11] and fx.origin.tolist() == [0.5, 1.5]
    n = len(g._lib.calls)
    for bad, word in ((dict(min_cells=0), "min_cells"), (dict(min_cells=2.5), "min_cells"), (dict(min_cells=None), "min_cells"),
                      (dict(max_clusters=0), "max_clusters"), (dict(max_clusters=(1 << 20) + 1), "max_clusters"), (dict(max_clusters="x"), "min_cells|max_clusters")):
        with pytest.raises(ValueError, match=word):
            g.frontiers_of(c, vis, **bad)
        with pytest.raises(ValueError, match=word):
            field.frontiers(m, **bad)
    for args, word in (((c[:, :5], vis), "cell_cost must have shape"), ((c, None), "visibility must be an array"), ((c - 1, vis), "cell_cost must lie in"),
                       ((c + 0.5, vis), "whole numbers"), ((None, vis), "cell_cost must be an array"), ((c, vis, D[:5]), "cost_to_go must have shape")):
        with pytest.raises(ValueError, match=word):
            g.frontiers_of(*args)
    for cp, vp in ((0, 1 << 20), (1 << 20, None)):
        with pytest.raises(ValueError, match="device addresses"):
            g.frontiers_of_device(cp, vp)
    with pytest.raises(ValueError, match="DeviceMaps"):
        field.frontiers(field)
    assert len(g._lib.calls) == n                                                          # nothing of that reached the library
    # goals(): rows in the order asked for, cell centres in world metres
    fx.n_clusters = 3
    table = np.array([[4, 5, 0, 0, 0, 0, 10, 90], [9, 7, 0, 0, 0, 0, 9, 20], [20, 7, 0, 0, 0, 0, 33, 20], [0] * 8], np.int32)
    sums = np.array([[5, 10], [7, 14], [21, 28], [0, 0]], np.int64)

    class _Part(object):
        def __init__(self, a):
            self.a, self.shape = a, a.shape

        def copy_to_host(self):
            return self.a
    fx.clusters, fx.sums, fx.cluster_map = _Part(table), _Part(sums), _Part(np.zeros((6, 6), np.int32))
    best, centroid, rows = fx.goals("cost")
    assert rows.tolist() == [1, 2, 0] and fx.goals("size")[2].tolist() == [1, 2, 0]
    oc = np.round(np.array([0.5, 1.5]) / 0.5)
    assert np.array_equal(best, (np.array([[3, 1], [3, 5], [4, 1]]) + oc + 0.5) * 0.5)
    assert np.array_equal(centroid, (np.array([[1.0, 2.0], [3.0, 4.0], [1.0, 2.0]]) + oc + 0.5) * 0.5)
    with pytest.raises(ValueError, match="order"):
        fx.goals("nearest")
    for obj in (g, m, field._hold, fx._hold):
        for a in ("_h", "_held"):
            obj.__dict__.pop(a, None)                                                      # (nothing for __del__ to release)


def test_the_frontier_layout_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "frontier_layout_host_test")
    src = os.path.join(ROOT, "tests", "frontier_layout_host_test.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src, "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "frontier layout host test ok" in run.stdout


def test_the_solve_arithmetic_and_work_layouts_under_sanitizers(tmp_path):
    """g-vom_amd/csrc/gvom_solvework.h: the look at a batch's counters, the batch lengths and the work buffers' layouts of every call
    that waits (tests/solvework_host_test.cpp)"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "solvework_host_test")
    src = os.path.join(ROOT, "tests", "solvework_host_test.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src, "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "solvework host test ok" in run.stdout


def test_the_kernels_use_no_scratch_and_the_relaxation_fits_8_kb_of_lds():
    import gvom
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    if not os.path.exists(os.path.join(kernel_regs.LLVM, "clang-offload-bundler")):
        pytest.skip("no ROCm LLVM tools")
    every = kernel_regs.kernels(gvom.library_path())
    kernels = {k: v for k, v in every.items() if "k_frontier_" in k}
    assert sorted(re.search(r"\d+(k_frontier_[a-z]+?)i", k).group(1) for k in kernels) == [
        "k_frontier_count", "k_frontier_mark", "k_frontier_rank", "k_frontier_relax", "k_frontier_rows", "k_frontier_stats"]
    for k, v in kernels.items():
        assert v["scratch"] == 0 and v["vgpr"] <= 64 and v["code"] > 0, (k, v)
        assert v["lds"] <= (8192 if "relax" in k else 1024), (k, v)
    # the solver next door, whose structure the relaxation has, is what it was (every other kernel parent against new, register for
    # register and byte for byte: profiles/frontier_resources.json)
    ctg = [v for k, v in every.items() if "k_ctg_relax" in k]
    assert len(ctg) == 1 and ctg[0]["scratch"] == 0 and ctg[0]["lds"] <= 8192
