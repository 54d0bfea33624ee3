"""Obstacle clearance (gvom_clearance), the part that needs no GPU: the referee's two forms agree, header / library / binding
agree, the kernels' registers, the binding's argument checks, and the census of the scenes tests/test_clearance.py runs."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import clearance_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPS, SCENES, SCENE_THRESHOLD, CENSUS_FLOOR, census = cr.CAPS, cr.SCENES, cr.SCENE_THRESHOLD, cr.CENSUS_FLOOR, cr.census


@pytest.mark.parametrize("xy", [16, 50, 64, 256])
def test_the_two_referee_forms_agree(xy):
    """every pattern and cap; at 256 the brute force takes a sample of 1500 cells where obstacles x cells exceeds 2e8"""
    sample = np.random.default_rng(xy).integers(0, xy, (1500, 2))
    for name, (pos, neg) in cr.patterns(xy).items():
        for thr in ((49.5, 50) if name == "threshold_edge" else (50,)):
            mask = cr.obstacle_mask(pos, neg, thr)
            sep = cr.separable(mask)
            cells = None if int(mask.sum()) * xy * xy <= 2e8 else sample
            brute = cr.brute_force(mask, 0, cells)
            assert np.array_equal(sep if cells is None else sep[cells[:, 0], cells[:, 1]], brute), (xy, name, thr)
            assert (sep == cr.FAR).all() == (not mask.any()) and ((sep == 0) == mask).all(), (xy, name)
            for c in CAPS[1:]:
                capped = cr.separable(mask, c)
                assert np.array_equal(capped, cr.cap(sep, c)), (xy, name, c)
                assert np.array_equal(capped == cr.FAR, sep > c) and np.array_equal(capped[sep <= c], sep[sep <= c])


@pytest.mark.parametrize("xy", cr.LARGE)
def test_the_large_map_referees_agree(xy):
    """by_rows and feature_transform (what tests/test_clearance.py compares the kernels with from 300 cells on) against the two
    older forms: separable on the full map up to 520 cells, brute_force on cr.boundary_sample beyond (both sides of every chunk,
    strip and row-tile boundary and 2,048 random cells).  At 4096 the feature transform takes 2 to 3 s a mask: there it is held on
    the map it is the referee of (random_0.1) and on corner_far."""
    sample = cr.boundary_sample(xy)
    nx = 2 * len(range(8, xy, 8))                              # the sample's first part: both sides of every x boundary
    assert len(sample) >= 2048 + nx and sample.min() >= 0 and sample.max() < xy
    for b in range(64, xy, 64):                                # both sides of every chunk boundary, next to a row-tile boundary
        for x in (b - 1, b):
            ys = sample[:nx][sample[:nx, 0] == x, 1]
            assert len(ys) and ((ys % 16 == 0) | (ys % 16 == 15)).all(), (xy, x)
    T = cr.row_tile(xy)
    for t in range(T, xy, T):
        assert (sample[:, 1] == t - 1).any() and (sample[:, 1] == t).any(), (xy, t)
    for name, pos in cr.large_patterns(xy, short=xy == 4096).items():
        mask = cr.obstacle_mask(pos, None, 50)
        ref = cr.large_referee(mask)
        if ref is None:                                        # (no scipy: the GPU test holds this map on the sample instead)
            assert name.startswith("random") and not cr.have_scipy()
            continue
        assert ref.dtype == np.int32 and (ref == cr.FAR).all() == (not mask.any()) and ((ref == 0) == mask).all(), (xy, name)
        if cr.have_scipy() and (xy < 4096 or name in ("random_0.1", "corner_far")):
            assert np.array_equal(ref, cr.feature_transform(mask)), (xy, name)
        if xy <= 520:
            assert np.array_equal(ref, cr.separable(mask)), (xy, name)
            if name in ("random_0.1", "full_column", "all", "lonely"):
                assert np.array_equal(ref, cr.by_rows(mask)), (xy, name)      # (by_rows on many rows too, where that is cheap)
        else:
            assert np.array_equal(ref[sample[:, 0], sample[:, 1]], cr.brute_force_near(mask, sample)), (xy, name)


def test_brute_force_near_is_brute_force():
    xy = 200
    cells = cr.boundary_sample(xy)
    for name, (pos, neg) in cr.patterns(xy).items():
        mask = cr.obstacle_mask(pos, neg, 50)
        assert np.array_equal(cr.brute_force_near(mask, cells, r=5 if name == "random_1" else 48), cr.brute_force(mask, 0, cells)), name
    far = cr.brute_force_near(cr.obstacle_mask(cr.patterns(xy)["random_0.1"][0]), cells, r=5)
    assert (far > 25).sum() > 100                              # cells the window did not settle: they went to the full list


@pytest.mark.parametrize("xy", cr.LARGE)
def test_large_patterns_reach_the_code_they_are_meant_for(xy):
    """on the referee alone: what of k_clearance_rows / k_clearance_cols the large maps run that the four small sizes cannot"""
    pats = cr.large_patterns(xy, short=xy == 4096)
    chunks = (xy + 63) // 64
    assert chunks > 4                                          # a wave's chunk loop makes a second trip
    far = cr.large_referee(pats["corner_far"] > 50)
    assert far[0, xy - 1] == far.max() == 2 * (xy - 1) ** 2 < cr.FAR
    caps = cr.large_caps(xy)
    assert caps[:4] == (0, 1, 25, 2500) and int(np.sqrt(caps[4])) >= xy and ((far > caps[4]) & (far < cr.FAR)).sum() > 0 and (far <= caps[4]).sum() > 0
    for c in caps[1:4]:                                        # each cap has cells on both sides
        assert (far <= c).any() and (far == c).any() and (far > c).any()
    same, adj = pats["boundary_same_row"] > 50, pats["boundary_adjacent_rows"] > 50
    bounds = list(range(64, xy, 64))
    assert len(bounds) == (xy - 1) // 64 and same.sum() == adj.sum() == 2 * len(bounds)
    for b in bounds:
        assert same[b - 1, 5] and same[b, 5] and adj[b - 1, xy // 2] and adj[b, xy // 2 + 1]
    if xy == 4096:
        assert bounds[-1] == 4032 and same[4031, 5] and same[4032, 5] and chunks == 64      # chunk 62 | 63
    assert same[:, 5].reshape(-1)[:64 * (xy // 64)].reshape(-1, 64).any(axis=1).all()   # every whole chunk of that row holds an obstacle
    lonely = pats["lonely"] > 50
    d = cr.large_referee(lonely)
    assert lonely[:, 16].sum() == 2 and lonely[0, 16] and lonely[xy - 1, 16]                # chunks 1 .. chunks - 2 of row 16 are empty
    xs = np.arange(xy)
    assert lonely.sum() == 2 and np.array_equal(d[:, 16], np.minimum(xs, xy - 1 - xs) ** 2)
    # one obstacle in the map, at the end of its row: the row's first cell finds it across every mask, xy - 1 cells away
    assert far[0, 0] == (xy - 1) ** 2 and (pats["corner_far"] > 50).sum() == 1 and pats["corner_far"][xy - 1, 0] > 50
    left = cr.large_referee(pats["corner_0n"] > 50)
    assert left[xy - 1, xy - 1] == (xy - 1) ** 2 and left[xy - 1, 0] == 2 * (xy - 1) ** 2 and (pats["corner_0n"] > 50).sum() == 1
    rnd = pats["random_0.1"] > 50
    assert 0.0005 * xy * xy <= rnd.sum() <= 0.002 * xy * xy
    if xy < 4096:
        dense = pats["random_30"] > 50
        assert 0.25 * xy * xy <= dense.sum() <= 0.35 * xy * xy and not pats["none"].any() and (pats["all"] > 50).all()
        assert (pats["full_row"] > 50)[:, xy // 3].all() and (pats["full_column"] > 50)[xy // 3, :].all()
        assert (pats["corners"] > 50).sum() == 4


def test_the_launch_shape_names_are_documented():
    header = open(os.path.join(ROOT, "include", "gvom_hip.h")).read()
    source = open(os.path.join(ROOT, "g-vom_amd", "csrc", "gvom_handle.hip")).read()
    for name in ("clearance_lgw", "clearance_rows_per_tile", "clearance_lds_bytes", "clearance_chunks"):
        assert '"%s"' % name in header and '"%s"' % name in source, name


def test_referee_mask_threshold_negative_and_distance():
    pos = np.array([[49, 50], [51, 0]], np.int32)
    neg = np.array([[0, 0], [0, 100]], np.int32)
    assert cr.obstacle_mask(pos, neg, 49.5).tolist() == [[False, True], [True, True]]
    assert cr.obstacle_mask(pos, neg, 50).tolist() == [[False, False], [True, True]]
    assert cr.obstacle_mask(pos, neg, 50, include_negative=False).tolist() == [[False, False], [True, False]]
    assert cr.obstacle_mask(pos, None, 50).tolist() == [[False, False], [True, False]]
    d = cr.distance(np.array([0, 1, 2, 25, cr.FAR], np.int32), 0.4)
    assert d.dtype == np.float32 and d[0] == 0 and d[1] == np.float32(0.4) and d[3] == np.float32(5 * 0.4) and np.isinf(d[4])
    assert d[2] == np.float32(np.sqrt(2.0) * 0.4)
    assert cr.separable(np.eye(3, dtype=bool) & (np.arange(3) == 0)[:, None]).tolist() == [[0, 1, 4], [1, 2, 5], [4, 5, 8]]
    assert cr.max_cells2_of(2.0, 0.4) == 25 and cr.max_cells2_of(1.99, 0.4) == 24 and cr.max_cells2_of(None, 0.4) == 0


def test_abi_10_the_symbol_and_the_three_defines():
    import gvom
    header = open(os.path.join(ROOT, "include", "gvom_hip.h")).read()
    assert int(re.search(r"#define\s+GVOM_ABI_VERSION\s+(\d+)", header).group(1)) == 10
    assert gvom.ABI_VERSION == 10 and gvom.load_library().gvom_abi_version() == 10
    assert re.search(r"\bint\s+gvom_clearance\s*\(", header)
    for word, value in (("GVOM_PRODUCT_CLEARANCE", gvom.PRODUCT_CLEARANCE), ("GVOM_CLEARANCE_FAR", gvom.CLEARANCE_FAR),
                        ("GVOM_CLEARANCE_NO_NEGATIVE", 1)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % word, header).group(1)) == value, word
    assert gvom.PRODUCT_CLEARANCE == 5 and gvom.CLEARANCE_FAR == 2 ** 31 - 1 == cr.FAR
    L = ctypes.CDLL(gvom.library_path())
    assert hasattr(L, "gvom_clearance") and "gvom_clearance" in {n for n, _, _ in gvom.ABI}
    nm = subprocess.run(["nm", "-D", "--defined-only", gvom.library_path()], capture_output=True, text=True, check=True)
    assert re.search(r" T gvom_clearance$", nm.stdout, re.M)
    for m in ("clearance_of", "clearance_of_device"):
        assert callable(getattr(gvom.Gvom, m))
    assert callable(gvom.DeviceMaps.clearance)
    for attr in ("copy_to_host", "release", "__enter__", "__exit__"):
        assert callable(getattr(gvom.DeviceClearance, attr))


def test_library_still_imports_nothing_from_the_checker():
    import gvom
    r = subprocess.run(["readelf", "-d", gvom.library_path()], capture_output=True, text=True, check=True)
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[(.*?)\]", r.stdout)
    assert needed and not any("oracle" in n for n in needed), needed
    nm = subprocess.run(["nm", "-D", "--undefined-only", gvom.library_path()], capture_output=True, text=True, check=True)
    assert "orc_" not in nm.stdout


def test_clearance_kernels_use_no_scratch_and_fit_four_waves_per_simd():
    import gvom
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    if not os.path.exists(os.path.join(kernel_regs.LLVM, "clang-offload-bundler")):
        pytest.skip("no ROCm LLVM tools")
    kernels = {k: v for k, v in kernel_regs.kernels(gvom.library_path()).items() if "k_clearance" in k}
    assert len(kernels) == 2, sorted(kernels)
    for k, v in kernels.items():
        assert v["scratch"] == 0, (k, v)
        assert v["vgpr"] <= 128, (k, v)


def test_python_arguments_are_checked_before_any_library_call():
    import gvom
    g = gvom.Gvom.__new__(gvom.Gvom)              # no handle, no library: a call that got as far as the library would not raise ValueError
    g.xy_size, g.xy_resolution, g._lib, g._h = 16, 0.4, None, None
    pos = np.zeros((16, 16), np.int32)
    for bad in (-1.0, float("nan"), 0.39, 0.0):
        with pytest.raises(ValueError, match="max_distance"):
            g.clearance_of(pos, max_distance=bad)
        with pytest.raises(ValueError, match="max_distance"):
            g.clearance_of_device(1 << 20, max_distance=bad)
    with pytest.raises(ValueError, match="density_threshold"):
        g.clearance_of(pos, density_threshold=float("nan"))
    with pytest.raises(ValueError, match="shape"):
        g.clearance_of(np.zeros((16, 15), np.int32))
    with pytest.raises(ValueError, match="shape"):
        g.clearance_of(pos, np.zeros((4, 4), np.int32))
    with pytest.raises(ValueError, match="positive"):
        g.clearance_of(None)
    with pytest.raises(ValueError, match="positive_ptr"):
        g.clearance_of_device(0)
    cap = gvom._clearance_cap
    assert cap(None, 0.4) == 0 and cap(float("inf"), 0.4) == 0 and cap(1e9, 0.4) == 0
    assert cap(2.0, 0.4) == cr.max_cells2_of(2.0, 0.4) == 25 and cap(1.99, 0.4) == 24 and cap(0.4, 0.4) == 1 and cap(4.0, 0.4) == 100
    try:
        del g._h                                      # (nothing for __del__ to destroy)
    except AttributeError:
        pass


@pytest.mark.parametrize("name", SCENES)
def test_scenes_hold_cells_on_both_sides_of_the_threshold(name):
    """measured at the last combine, threshold 50 (one_round / ragged): 166 / 368 cells with 0 < positive <= 50, 387 / 493 with
    positive > 50, 5 / 1 with negative > 0"""
    import obstacle_scenes as ob
    from oracle import oracle
    o = oracle.OracleGvom(*ob.params(name))
    for pc, ego in ob.scans(name):
        o.process_pointcloud(pc, ego)
        maps = o.combine_maps()
    soft, hard, negative = census(maps[1], maps[2], SCENE_THRESHOLD)
    assert soft >= CENSUS_FLOOR and hard >= CENSUS_FLOOR and negative >= 1, (name, soft, hard, negative)
