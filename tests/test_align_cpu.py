"""Scan alignment scoring (gvom_score_alignments), the part that needs no GPU: header, library and binding agree; the referee of
tests/align_ref.py pinned to the CPU referee's transform and scan kernels; the census of the GPU test's inputs on maps the CPU referee
built; the unperturbed candidate as the unique best; what those inputs leave open, and numpy models of eleven defects of the class grid
that the planted maps and line probes of tests/test_align.py tell from the referee; the census of its edge inputs; pose_candidates;
the binding's argument checks; the product's layout under sanitizers; the kernels' registers.

Census on the CPU referee's maps (cloud of the last scan, 245 candidates: 7 x 7 offsets of one cell, 5 yaws of 0.02 rad about the ego),
class counts {occupied, near, free, unknown, outside} summed over the candidates, buffer_size 1 / 2, dilate 0 and dilate 1:
    p2     195259 / 0 / 866807 / 271849 / 673125    195320 / ...     dilate 1: near 1051503 / free 46731 / unknown 40422
    np2    427035 / 0 / 796741 / 137596 / 645668    420317 / ...     dilate 1: near  925208 / free  5236 / unknown  3893
    tall     9827 / 0 /  29939 /  20659 /  33655      9816 / ...     dilate 1: near   47943 / free   771 (722) / unknown 1884
    w128    82346 / 0 / 785271 / 467516 / 671907     82196 / ...     dilate 1: near  743596 / free 280668 / unknown 228523
    w192    60861 / 0 / 791137 / 497540 / 657502     60999 / ...     dilate 1: near  582867 / free 398011 / unknown 307799
Best against second-best score under the default weights (2, 1, -1, 0, 0): p2 10846 / 3899, np2 11045 / 6555, tall 513 / 450, w128
10862 / -474, w192 10976 / -1867; distinct count rows 242 to 245 of 245.  The far grid (window origin beyond 2^24 voxels) is in the
referee match of tests/test_align.py but not in the census: see tests/align_ref.py CENSUS_GRIDS.

What those inputs leave open (test_the_gap_the_planted_maps_close): a dilation that wraps around the bottom and top face of the window
changes the class of 2,508 (p2), 2,107 (np2), 160 (tall), 3,523 (w128) and 4,953 (w192) voxels, either ring length, and the counts of
0 of the 249 candidates -- the clouds stop 0.15 window heights above the ego and no candidate moves them in z.

The planted maps (tests/align_ref.py planted_map) under the line probes close it.  Census on the CPU referee's planted maps, the same
for ring lengths 1 and 2 -- planted voxels (all occupied) / occupied voxels in all / the fewest voxels on one side of a multiple of
16 in x that are NEAR only by an occupied voxel on the other side (floor 21): np2 44 / 178 / 59, tall 20 / 155 / -, w128 76 / 215 /
24, w192 134 / 273 / 39, r72 64 / 203 / 37, r37 27 / 156 / 39.  Voxels whose class each modelled defect (classes_with_defect) changes
there; wherever that is not 0, candidates of ALL three probes differ from the referee's counts (the test asks for one):
             xwrap ywrap zwrap top lastrow carry_left carry_right zhalo_lo zhalo_hi sub16 lastword
    np2        115   115   143  61      49          0           0      118       85   778        0
    tall       118   132    63  26      79          0           0       14       59     0        0
    w128        66    79   373  36      19         36          30      177      213  2512        0
    w192        97   103   140  63      21         78          94      249      330  4504        0
    r72        119   106   314  69      29         54          48      153      131  1490    11498
    r37         91    69   222  89      56          0           0        0        0   483     2201

The edge inputs of the score kernel (test_the_edge_census; 2,048 returns, 498 on tall, under 49 candidates), class counts summed over
the candidates, dilate 0 then {near, free, unknown} of dilate 1, ring length 1 (2 is within 5 %), pairs in the upper 30 % of
the window, boundary points inside / outside the window under the identity:
    p2      6106 / 0 / 18941 /  9436 / 65869    23642 /  684 / 4051    2998    87 / 27
    np2    10755 / 0 / 16410 /  5908 / 67279    19534 /   72 / 2712    3110    88 / 26
    tall    2167 / 0 /  4073 /  2823 / 15339     6083 /  100 /  713     526    86 / 28     (ring 2: occupied 2262, free 3978, near 5994)
    w192    2455 / 0 / 16399 / 12637 / 68861    15340 / 6086 / 7610    2914    87 / 27
    far    19318 / 0 /     5 / 10851 / 70178     8014 /    0 / 2842    2799    46 / 71
    third   8229 / 0 / 16695 /  4527 / 70901    18708 /  342 / 2172    2716    91 / 26
    odd    10503 / 0 / 19372 /  5761 / 64716    22951 /   73 / 2109    2268    90 / 24
The floors (tests/align_ref.py EDGE_FLOORS, EDGE_FLOORS_FAR, UPPER_FLOOR) lie a little under the smallest of these."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import align_ref as ar
import raycast_ref as rr
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_binding_and_library_agree():
    import gvom
    header = open(os.path.join(ROOT, "include", "gvom_hip.h")).read()
    assert int(re.search(r"#define\s+GVOM_ABI_VERSION\s+(\d+)", header).group(1)) == 10 == gvom.ABI_VERSION      # an addition: the version stays
    m = re.search(r"\bint\s+gvom_score_alignments\s*\(([^;]*)\)\s*;", header)
    assert m, "gvom_score_alignments is not declared in include/gvom_hip.h"
    assert len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == 9
    bound = {name: (res, args) for name, res, args in gvom.ABI}
    assert bound["gvom_score_alignments"][0] is ctypes.c_int and len(bound["gvom_score_alignments"][1]) == 9
    assert hasattr(gvom.load_library(), "gvom_score_alignments")
    nm = subprocess.run(["nm", "-D", "--defined-only", gvom.library_path()], capture_output=True, text=True, check=True)
    assert re.search(r" T gvom_score_alignments$", nm.stdout, re.M)
    assert re.search(r"#define\s+GVOM_PRODUCT_ALIGNMENT\s+12\b", header) and gvom.PRODUCT_ALIGNMENT == 12
    assert not re.search(r"#define\s+GVOM_PRODUCT_\w+\s+(8|9|11)\b", header)            # kinds 8, 9 and 11 stay unassigned
    assert gvom._PRODUCT_DTYPES[gvom.PRODUCT_ALIGNMENT] == (np.int32, np.int32)
    for word in ('"alignments"', '"alignment_allocations"', '"alignment_grid_bytes"', "min_distance rejection is NOT applied",
                 "NOT PROVIDED: float64 clouds"):
        assert word in header, word
    for name in ("score_alignments", "score_alignments_device"):
        assert callable(getattr(gvom.Gvom, name))
    for name in ("counts", "best", "origin", "copy_to_host", "release", "__enter__", "__exit__"):
        assert name in gvom.DeviceAlignments.__init__.__code__.co_names or hasattr(gvom.DeviceAlignments, name), name
    assert gvom.ALIGN_DEFAULT_WEIGHTS == ar.DEFAULT_WEIGHTS
    assert (gvom.ALIGN_MAX_POINTS, gvom.ALIGN_MAX_CANDIDATES, gvom.ALIGN_MAX_PAIRS, gvom.ALIGN_MAX_WEIGHT) == (1 << 20, 65536, 1 << 32, 1024)
    assert "gvom_align" in open(os.path.join(ROOT, "g-vom_amd", "Makefile")).read()


@pytest.mark.parametrize("grid", ar.CENSUS_GRIDS)
def test_the_referee_transforms_as_the_scan_does(grid):
    """world() against the CPU referee's transform_pointcloud, bit for bit: rotations about each axis and about all three, with
    translations of metres and of 7e6 m, and the yaw + translation candidates of the grid"""
    cloud = ar.cloud_of(grid)[::7]
    M = np.concatenate([ar.rotations(), ar.grid_candidates(grid)[::9]])
    got = ar.world(cloud, M)
    assert got.dtype == np.float32 and got.shape == (len(M), len(cloud), 3)
    moved = 0
    for k in range(len(M)):
        want = oracle.transform_pointcloud(cloud, M[k])
        assert want.dtype == np.float32
        assert np.array_equal(got[k].view(np.uint32), want.view(np.uint32)), (grid, k)
        moved += int(not np.array_equal(want, cloud))
    assert moved >= len(M) - 1
    assert np.array_equal(ar.world(cloud, M[:, :3, :]), got)                          # rows 0..2 are all that is read


@pytest.mark.parametrize("grid", ["p2", "np2", "tall"])
def test_the_referee_places_returns_where_the_scan_does(grid):
    """the histogram of voxels() over its inside points against `hit` of the CPU referee's scan kernel with min_distance 0: points on
    exact voxel boundaries and their float32 neighbours on both sides, on both signs, and the cloud under three candidates"""
    xr, zr, xy, zs = ar.GRIDS[grid]
    ego = rr.ego_of(grid, ar.SCAN)
    for W in (rr.window_origin(grid, ego), np.array([-3.0, -xy + 5.0, -zs / 2.0]), np.array([2.0, 1.0, 0.0])):
        edge = ar.boundary_points(grid, W)
        M = ar.grid_candidates(grid)
        pts = np.concatenate([edge, ar.world(ar.cloud_of(grid)[::5], M[[0, ar.CENTRE, ar.N_GRID - 1]]).reshape(-1, 3)])
        v, inside = ar.voxels(pts, grid, W)
        assert inside[:len(edge)].sum() >= 20 and (~inside[:len(edge)]).sum() >= 20
        assert (pts[:len(edge)] < 0).any() and (pts[:len(edge)] > 0).any()
        vi = v[inside].astype(np.int64)
        want = np.bincount(vi[:, 0] + vi[:, 1] * xy + vi[:, 2] * xy * xy, minlength=xy * xy * zs)
        hit, _, _ = oracle.point_2_map(xr, zr, xy, zs, 0.0, pts, np.asarray(ego, np.float64), W)
        assert np.array_equal(hit, want), (grid, W, np.flatnonzero(hit != want)[:8])
    # the neighbours of a boundary fall on both sides of it
    b = ar.boundary_points(grid, np.zeros(3))
    vx, _ = ar.voxels(b, grid, np.zeros(3))
    assert len(np.unique(vx[:, 0])) >= 6


def test_classes_known_answers():
    grid = "tall"
    _, _, xy, zs = ar.GRIDS[grid]
    state = np.full(xy * xy * zs, -1, np.int32)
    vox = lambda x, y, z: x + y * xy + z * xy * xy
    state[vox(0, 0, 0)] = 7                                                           # a corner: its neighbours inside the window only
    state[vox(8, 8, 16)] = 0
    state[vox(9, 9, 17)] = -2
    state[vox(12, 3, 5)] = -5
    c0, c1 = ar.classes(state, grid, 0), ar.classes(state, grid, 1)
    assert c0[0, 0, 0] == c1[0, 0, 0] == ar.OCCUPIED and c0[16, 8, 8] == ar.OCCUPIED
    assert c0[17, 9, 9] == ar.FREE and c1[17, 9, 9] == ar.NEAR and c0[5, 3, 12] == c1[5, 3, 12] == ar.FREE
    assert (c0 == ar.NEAR).sum() == 0 and (c1 == ar.NEAR).sum() == 7 + 26 and (c1 == ar.OCCUPIED).sum() == 2
    assert c1[15, 7, 7] == ar.NEAR and c1[14, 8, 8] == ar.UNKNOWN and c1[1, 1, 1] == ar.NEAR and c1[0, 2, 0] == ar.UNKNOWN
    # by hand: three returns, two candidates
    W = np.array([-8.0, -8.0, -16.0])
    cloud = np.array([[0.2, 0.2, 0.1], [0.6, 0.6, 0.3], [100.0, 0.0, 0.0]], np.float32)           # voxels (8, 8, 16), (9, 9, 17), outside
    M = np.array([np.identity(4), ar.yaw_about((0, 0, 0), 0.0, (0.4, 0.4, 0.2))])                 # the second moves all one voxel up
    counts, best = ar.score(state, W, grid, cloud, M, 0)
    assert counts.tolist() == [[1, 1, 0, 1, 0, 1], [-1, 0, 0, 1, 1, 1]] and best.tolist() == [0, 1, 3, 2]
    counts, best = ar.score(state, W, grid, cloud, M, 1, weights=(-3, 5, 0, 0, 1))
    assert counts.tolist() == [[3, 1, 1, 0, 0, 1], [6, 0, 1, 0, 1, 1]] and best.tolist() == [1, 6, 3, 2]


@pytest.fixture(scope="module")
def maps():
    """per (grid, buffer_size): (dense fused state, window origin) of the CPU referee after the shared scans"""
    out = {}
    for grid in ar.CENSUS_GRIDS:
        for bs in (1, 2):
            g = rr.build_map(oracle.OracleGvom, grid, bs)
            out[grid, bs] = (np.asarray(g.combined_index_map).copy(), np.asarray(g.combined_origin, np.float64))
    return out


@pytest.mark.parametrize("bs", [1, 2])
@pytest.mark.parametrize("grid", ar.CENSUS_GRIDS)
def test_census_and_the_unique_best(maps, grid, bs):
    state, W = maps[grid, bs]
    cloud, M = ar.cloud_of(grid), ar.candidates(grid)
    assert cloud.dtype == np.float32 and len(cloud) == (384 if grid == "tall" else 8192) and len(M) == ar.N_GRID + 4 == 249
    for dilate in (0, 1):
        counts, best = ar.score(state, W, grid, cloud, M, dilate)
        t = ar.census_holds(grid, dilate, counts)
        srt = np.sort(counts[:ar.N_GRID, 0])
        print(grid, bs, "dilate", dilate, "totals", t, "best", best.tolist(), "second", int(srt[-2]))
        assert best.tolist() == [ar.CENTRE, int(srt[-1]), len(cloud), len(M)]
        assert srt[-1] > srt[-2]                                                      # the unperturbed candidate is the UNIQUE best of the grid
        assert len(np.unique(counts[:ar.N_GRID], axis=0)) >= ar.DISTINCT_ROWS
        # the specials: the centre again ties and loses to the lower index; every return outside; a NaN entry puts the returns it
        # touches outside; a translation beyond float32 all of them
        assert np.array_equal(counts[ar.N_GRID], counts[ar.CENTRE])
        assert counts[ar.N_GRID + 1].tolist() == [0, 0, 0, 0, 0, len(cloud)] == counts[ar.N_GRID + 3].tolist()
        assert counts[ar.N_GRID + 2, 5] == len(cloud)
    if dilate:
        assert (counts[:, 2] > 0).any()
    d0, _ = ar.score(state, W, grid, cloud, M[:ar.N_GRID], 0)
    assert (d0[:, 2] == 0).all() and np.array_equal(d0[:, 1], counts[:ar.N_GRID, 1]) and np.array_equal(d0[:, 5], counts[:ar.N_GRID, 5])


DEFECTS = ("xwrap", "ywrap", "zwrap", "top", "lastrow", "carry_left", "carry_right", "zhalo_lo", "zhalo_hi", "sub16", "lastword")


def classes_with_defect(state, grid, kind, dilate=1):
    """ar.classes() with one of the defects the structure of k_align_field makes plausible (any other `kind`: none) --
    xwrap, ywrap, zwrap: a neighbour beyond a face of the window is taken from the opposite face; top: the top level takes no z
    neighbours; lastrow: row xy - 1 takes no y neighbours; carry_left, carry_right: no neighbour across a multiple of 64 in x (the
    64-bit mask words); zhalo_lo, zhalo_hi: no neighbour across a multiple of 16 in z (the chunks of levels); sub16: the first code of
    each 16-voxel word is the first of the word before; lastword: a partial last word of a row is left unwritten (reads OCCUPIED)"""
    _, _, xy, zs = ar.GRIDS[grid]
    s = np.asarray(state).reshape(zs, xy, xy)
    occ = s >= 0
    coord, size = np.ogrid[:zs, :xy, :xy], (zs, xy, xy)
    z, y, x = coord
    wraps = (kind == "zwrap", kind == "ywrap", kind == "xwrap")
    near = np.zeros_like(occ)
    for d in itertools.product((-1, 0, 1), repeat=3) if dilate else ():
        dz, dy, dx = d
        take = np.ones_like(occ)
        for axis in range(3):
            if d[axis] and not wraps[axis]:
                take = take & (coord[axis] + d[axis] >= 0) & (coord[axis] + d[axis] < size[axis])
        if kind == "top" and dz:
            take = take & (z != zs - 1)
        if kind == "lastrow" and dy:
            take = take & (y != xy - 1)
        if (kind == "carry_left" and dx == -1) or (kind == "carry_right" and dx == 1):
            take = take & (x % 64 != (0 if dx == -1 else 63))
        if (kind == "zhalo_lo" and dz == -1) or (kind == "zhalo_hi" and dz == 1):
            take = take & (z % 16 != (0 if dz == -1 else 15))
        near |= np.roll(occ, (-dz, -dy, -dx), axis=(0, 1, 2)) & take            # (rolled: the voxel at + d, wrapped)
    cls = np.where(occ, ar.OCCUPIED, np.where(near, ar.NEAR, np.where(s <= -2, ar.FREE, ar.UNKNOWN))).astype(np.uint8)
    if kind == "sub16":
        first = np.arange(16, xy, 16)
        cls[:, :, first] = cls[:, :, first - 16]
    if kind == "lastword" and xy % 16:
        cls[:, :, xy - xy % 16:] = ar.OCCUPIED
    return cls


def _oracle_map(build, grid, bs):
    g = build(oracle.OracleGvom, grid, bs)
    return np.asarray(g.combined_index_map).copy(), np.asarray(g.combined_origin, np.float64)


def test_the_line_probes_on_planted_maps_catch_every_defect_of_the_class_grid():
    """on the CPU referee's planted maps: the census of tests/align_ref.py holds; wherever a defect changes a voxel's class, the
    counts of at least one candidate of at least one probe differ from the referee's; every defect changes a voxel somewhere"""
    changed_somewhere = dict.fromkeys(DEFECTS, 0)
    print("\ngrid  ring  planted / occupied / least carry | per defect: voxels changed, candidates that differ per probe axis (x y z)")
    for grid in ar.PROBE_GRIDS:
        first = None
        for bs in (1, 2):
            state, W = _oracle_map(ar.planted_map, grid, bs)
            assert np.array_equal(W, rr.window_origin(grid, rr.ego_of(grid, ar.SCAN)))
            census = ar.planted_census_holds(state, grid)
            good = ar.classes(state, grid, 1)
            assert np.array_equal(classes_with_defect(state, grid, "none"), good)
            assert np.array_equal(classes_with_defect(state, grid, "none", 0), ar.classes(state, grid, 0))
            if bs == 2 and np.array_equal(good, first):                    # (the same map as with ring length 1: the same table)
                print("%-5s %d     %r | as ring length 1" % (grid, bs, census))
                continue
            first = good
            at = [ar.voxels(ar.world(cloud, M), grid, W) for cloud, M in ar.line_probes(grid, W)]
            want = [ar.class_counts(good, v, inside) for v, inside in at]
            row = []
            for kind in DEFECTS:
                bad = classes_with_defect(state, grid, kind)
                changed = int((bad != good).sum())
                differ = [int((ar.class_counts(bad, v, inside) != w).any(axis=1).sum()) for (v, inside), w in zip(at, want)]
                row.append("%s %d: %d %d %d" % ((kind, changed) + tuple(differ)))
                changed_somewhere[kind] += changed
                assert (changed > 0) == (max(differ) > 0), (grid, bs, kind, changed, differ)
            print("%-5s %d     %r | %s" % (grid, bs, census, "; ".join(row)))
    assert min(changed_somewhere.values()) > 0, changed_somewhere


def test_the_gap_the_planted_maps_close(maps):
    """the record of what the shared maps and their last scan's cloud leave open: a dilation that wraps around the bottom and the top
    face of the window changes thousands of voxels' class on every one of them and not one count of the 249 candidates"""
    print()
    for grid in ar.CENSUS_GRIDS:
        for bs in (1, 2):
            state, W = maps[grid, bs]
            cloud, M = ar.cloud_of(grid), ar.candidates(grid)
            bad =classes_with_defect(state, grid, "zwrap")
            changed = int((bad != ar.classes(state, grid, 1)).sum())
            v, inside = ar.voxels(ar.world(cloud, M), grid, W)
            differ = int((ar.class_counts(ar.classes(state, grid, 1), v, inside) != ar.class_counts(bad, v, inside)).any(axis=1).sum())
            print("%-5s ring %d: zwrap changes %d voxels, %d of %d candidates" % (grid, bs, changed, differ, len(M)))
            assert changed >= 100 and differ == 0


def test_the_edge_census():
    """the inputs of the score kernel's edge test (tests/test_align.py) on the CPU referee's maps: the floors of tests/align_ref.py"""
    print()
    for grid in ar.EDGE_GRIDS:
        for bs in (1, 2):
            state, W = _oracle_map(rr.build_map, grid, bs)
            (cloud, m), M = ar.edge_cloud(grid, W), ar.edge_candidates(grid, W)
            assert len(M) == 49 and len(cloud) == min(ar.EDGE_RETURNS, m + (384 if grid == "tall" else 8192)) and m >= 100
            seen = np.zeros(5, np.int64)
            for dilate in (0, 1):
                counts, best = ar.score(state, W, grid, cloud, M, dilate)
                t, up, inside, outside = ar.edge_census_holds(grid, W, dilate, cloud, m, M, counts)
                print("%-5s ring %d dilate %d: totals %r, upper 30 %% %d, boundary points inside %d outside %d" % (grid, bs, dilate, t, up, inside, outside))
                seen += t
            assert (seen > 0).all(), (grid, bs, seen)                      # every class, OUTSIDE included, occurs


def test_pose_candidates():
    import gvom
    rng = np.random.default_rng(5)
    T = ar.rotations()[13]
    T[:3, 3] = (12.5, -3.25, 0.75)
    P = gvom.pose_candidates(T, 0.4, 3, 0.02, 2)
    assert P.dtype == np.float64 and P.shape == (245, 4, 4) and P.flags.c_contiguous
    assert np.array_equal(P[122].view(np.uint64), T.view(np.uint64))                 # the all-zero offset: the input, bit for bit
    assert np.array_equal(P[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (245, 1)))
    # index order: x offset fastest, then y, then yaw, then z; the pivot defaults to the transform's translation and stays in place
    for k in rng.choice(245, 40, replace=False):
        i, j, a = k % 7 - 3, k // 7 % 7 - 3, k // 49 - 2
        want = ar.yaw_about(T[:3, 3], a * 0.02, (i * 0.4, j * 0.4, 0.0)).dot(T)
        assert np.allclose(P[k], want, rtol=0, atol=1e-12), k
        assert np.allclose(P[k][:3, 3], T[:3, 3] + (i * 0.4, j * 0.4, 0.0), atol=1e-12)
    Z = gvom.pose_candidates(T, 0.4, 1, 0.1, 0, z_step=0.2, z_steps=1, pivot=(1.0, 2.0, 3.0))
    assert Z.shape == (27, 4, 4) and np.array_equal(Z[13], T)
    assert np.allclose(Z[0][:3, 3], T[:3, 3] + (-0.4, -0.4, -0.2), atol=1e-12) and np.allclose(Z[26][:3, 3], T[:3, 3] + (0.4, 0.4, 0.2), atol=1e-12)
    Y = gvom.pose_candidates(np.identity(4), 0.0, 0, 0.5, 1, pivot=(1.0, 2.0, 3.0))
    assert Y.shape == (3, 4, 4) and np.allclose(Y[2].dot([1.0, 2.0, 3.0, 1.0]), [1.0, 2.0, 3.0, 1.0]) and np.allclose(Y[2][:2, :2], [[np.cos(0.5), -np.sin(0.5)], [np.sin(0.5), np.cos(0.5)]])
    # the inputs of the tests are such a grid about the ego
    for grid in ("p2", "far"):
        ego = rr.ego_of(grid, ar.SCAN)
        assert np.array_equal(gvom.pose_candidates(np.identity(4), ar.GRIDS[grid][0], 3, 0.02, 2, pivot=ego), ar.grid_candidates(grid))
    for kw, word in ((dict(xy_steps=-1), "xy_steps"), (dict(yaw_steps=1.5), "yaw_steps"), (dict(xy_step=float("nan")), "xy_step"),
                     (dict(xy_steps=200), "65536"), (dict(pivot=(0.0, float("inf"), 0.0)), "pivot"), (dict(transform=np.identity(3)), "4x4")):
        args = dict(transform=np.identity(4), xy_step=0.4, xy_steps=1, yaw_step=0.1, yaw_steps=1)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            gvom.pose_candidates(**args)


def test_python_arguments_are_checked_before_any_library_call():
    import gvom
    g = gvom.Gvom.__new__(gvom.Gvom)              # no handle, no library: a call that got as far as the library would not raise these
    g._lib, g._h = None, None
    cloud, M = np.zeros((5, 3), np.float32), np.tile(np.identity(4), (2, 1, 1))
    for bad in (cloud.astype(np.float64), cloud.astype(np.float16), cloud.astype(np.int32)):
        with pytest.raises(TypeError, match="float32"):
            g.score_alignments(bad, M)                                 # no silent cast
    for bad in (np.zeros((5, 2), np.float32), np.zeros(3, np.float32), np.zeros((0, 3), np.float32)):
        with pytest.raises(ValueError):
            g.score_alignments(bad, M)
    with pytest.raises(TypeError, match="float64"):
        g.score_alignments(cloud, M.astype(np.float32))
    for bad in (np.zeros((2, 4, 3)), np.zeros((4, 4)), np.zeros((0, 4, 4)), np.zeros((65537, 3, 4))):
        with pytest.raises(ValueError):
            g.score_alignments(cloud, bad)
    for dilate in (2, -1, 0.5, None):
        with pytest.raises(ValueError, match="dilate"):
            g.score_alignments(cloud, M, dilate=dilate)
    for w in ((1, 2, 3, 4), (1025, 0, 0, 0, 0), (0, 0, -1025, 0, 0), (1.0, 0.0, 0.0, 0.0, 0.0)):
        with pytest.raises(ValueError, match="weights"):
            g.score_alignments(cloud, M, weights=w)
    for cp, tp in ((0, 1 << 20), (1 << 20, 0), (None, 1 << 20)):
        with pytest.raises(ValueError, match="device addresses"):
            g.score_alignments_device(cp, 5, tp, 2)
    for n, K in ((0, 1), (1, 0), ((1 << 20) + 1, 1), (1, 65537), (1 << 20, 4097), (1.5, 1)):
        with pytest.raises(ValueError):
            g.score_alignments_device(1 << 20, n, 1 << 21, K)
    g.__dict__.pop("_h", None)


def test_the_alignment_layout_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "align_layout_host_test")
    src = os.path.join(ROOT, "tests", "align_layout_host_test.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src, "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "align layout host test ok" in run.stdout


def test_the_kernels_use_no_scratch():
    import gvom
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    if not os.path.exists(os.path.join(kernel_regs.LLVM, "clang-offload-bundler")):
        pytest.skip("no ROCm LLVM tools")
    kernels = {k: v for k, v in kernel_regs.kernels(gvom.library_path()).items() if "k_align" in k}
    assert len(kernels) == 4, sorted(kernels)                         # k_align_field, k_align_score<true / false>, k_align_best
    for k, v in kernels.items():
        assert v["scratch"] == 0, (k, v)
        assert v["vgpr"] <= 128, (k, v)                                # four waves per SIMD at the least
