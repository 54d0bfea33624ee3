"""Terrain attitude scoring (gvom_chassis_set / gvom_score_attitude), the part that needs no GPU: header, library and binding agree;
the referee's two forms agree; what the stored numbers mean on a plane; the census of every input tests/test_attitude.py runs; the
binding's argument checks; the product's layout under sanitizers; the kernels' registers."""
import ctypes
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import attitude_ref as ar
import rollouts_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_10_the_symbols_the_defines_and_the_binding():
    import gvom
    header = open(os.path.join(ROOT, "include", "gvom_hip.h")).read()
    assert int(re.search(r"#define\s+GVOM_ABI_VERSION\s+(\d+)", header).group(1)) == 10
    assert gvom.ABI_VERSION == 10 and gvom.load_library().gvom_abi_version() == 10
    assert re.search(r"\bint\s+gvom_chassis_set\s*\(", header) and re.search(r"\bint\s+gvom_score_attitude\s*\(", header)
    assert re.search(r"\}\s*gvom_chassis_t\s*;", header)
    for word, value in (("GVOM_PRODUCT_ATTITUDE", gvom.PRODUCT_ATTITUDE), ("GVOM_ATTITUDE_OK", gvom.ATTITUDE_OK), ("GVOM_ATTITUDE_PITCH", gvom.ATTITUDE_PITCH),
                        ("GVOM_ATTITUDE_ROLL", gvom.ATTITUDE_ROLL), ("GVOM_ATTITUDE_BELLY", gvom.ATTITUDE_BELLY),
                        ("GVOM_ATTITUDE_UNKNOWN_GROUND", gvom.ATTITUDE_UNKNOWN_GROUND), ("GVOM_ATTITUDE_LEFT_WINDOW", gvom.ATTITUDE_LEFT_WINDOW),
                        ("GVOM_ATTITUDE_INVALID", gvom.ATTITUDE_INVALID), ("GVOM_ATTITUDE_INFERRED_GROUND", gvom._ATTITUDE_INFERRED_GROUND)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % word, header).group(1)) == value, word
    assert gvom.PRODUCT_ATTITUDE == 14
    assert (gvom.ATTITUDE_OK, gvom.ATTITUDE_PITCH, gvom.ATTITUDE_ROLL, gvom.ATTITUDE_BELLY, gvom.ATTITUDE_UNKNOWN_GROUND, gvom.ATTITUDE_LEFT_WINDOW,
            gvom.ATTITUDE_INVALID) == (ar.OK, ar.PITCH, ar.ROLL, ar.BELLY, ar.UNKNOWN_GROUND, ar.LEFT_WINDOW, ar.INVALID) == tuple(range(7))
    assert not re.search(r"#define\s+GVOM_PRODUCT_\w+\s+(8|9|11|13)\b", header)           # kinds 8, 9, 11 and 13 stay unassigned
    L = ctypes.CDLL(gvom.library_path())
    nm = subprocess.run(["nm", "-D", "--defined-only", gvom.library_path()], capture_output=True, text=True, check=True)
    for name, nargs in (("gvom_chassis_set", 4), ("gvom_score_attitude", 10)):
        assert hasattr(L, name)
        row = [r for r in gvom.ABI if r[0] == name]
        assert len(row) == 1 and len(row[0][2]) == nargs
        assert re.search(r" T %s$" % name, nm.stdout, re.M)
    for m in ("set_chassis", "score_attitude_of", "score_attitude_of_device"):
        assert callable(getattr(gvom.Gvom, m))
    assert callable(gvom.DeviceMaps.score_attitude) and callable(gvom.chassis)
    for attr in ("copy_to_host", "release", "__enter__", "__exit__"):
        assert callable(getattr(gvom.DeviceAttitude, attr))
    assert gvom._PRODUCT_DTYPES[gvom.PRODUCT_ATTITUDE] == (np.int32, np.float32, np.uint8)
    assert ctypes.sizeof(gvom.GvomChassis) == 48                                          # four doubles, three floats, padded to 8
    make = open(os.path.join(ROOT, "g-vom_amd", "Makefile")).read()
    assert "gvom_attitude" in make and "csrc/gvom_rollouts.h" in make
    # the binding's chassis: angles in radians, stored as float32 tangents; None is no limit
    c = gvom.chassis(2.7, 0.0, 1.7, 0.25, max_pitch=0.3, max_roll=0.2, min_clearance=0.1)
    assert (c.front_axle, c.rear_axle, c.track, c.belly_height) == (2.7, 0.0, 1.7, 0.25)
    assert c.max_pitch == np.float32(np.tan(0.3)) and c.max_roll == np.float32(np.tan(0.2)) and c.min_clearance == np.float32(0.1)
    c = gvom.chassis(2.7, 0.0, 1.7, 0.25)
    assert c.max_pitch == np.inf and c.max_roll == np.inf and c.min_clearance == -np.inf
    for H in (1, 4, 7, 64):
        assert np.array_equal(gvom.heading_cos_sin(H), ar.cos_sin(H))


def test_the_two_referee_forms_agree_on_tiny_inputs():
    rng = np.random.default_rng(5)
    n = 0
    for xy, H, M in ((5, 1, 1), (6, 3, 4), (7, 7, 9), (9, 4, 12)):
        res, oc = (0.4, 0.25, 0.1, 0.5)[n % 4], ((-2, 1), (3, -4), (0, 0), (-7, -7))[n % 4]
        for pattern in ar.GROUNDS + ("huge",):
            g = ar.ground_map(xy, "random" if pattern == "huge" else pattern, res, oc, seed=n)
            if pattern == "huge":                                                        # sums that overflow: infinite and NaN tangents
                g[rng.random((xy, xy)) < 0.3] = 1.5e308
                g[rng.random((xy, xy)) < 0.2] = -999.0
            table = rr.patch_table(H, M, seed=n) if n % 2 == 0 else rr.asymmetric_table(H)
            poses = rr.make_poses(6, 9, xy, res, oc, H, seed=n)
            poses[5, 2:7] = rr.special_poses(xy, res, oc, H)[rng.choice(20, 5)]
            ch = ar.make_chassis(1.3 * res, -0.8 * res, 1.7 * res, 0.9 * res, *((0.3, 0.35, 0.1 * res) if n % 3 else ()))
            cs = ar.cos_sin(H)
            got = ar.score(g, poses, table, ch, cs, res, oc)
            want = ar.score_loops(g.tolist(), poses.tolist(), table, ch, cs, res, oc)
            for a, b, what in zip(got, want, ("summary", "attitude", "status")):
                assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (xy, H, M, pattern, what, a, b)
            assert got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[2].dtype == np.uint8
            n += 1
    # by hand: a 4 x 4 map that rises 1 m per cell in x, 1 m cells, one heading, wheels at (+-1, +-1) about the pose
    g = np.repeat(np.arange(4.0)[:, None], 4, axis=1)
    g[2, 3] = np.nan
    table = (np.array([0, 2], np.int32), np.array([[0, 0], [1, 0]], np.int16))
    ch = ar.make_chassis(1.0, -1.0, 2.0, 0.5, max_pitch=2.0)
    poses = np.array([[(1.5, 1.5, 0.0), (1.5, 1.5, np.nan), (3.5, 1.5, 0.0), (1.5, 2.5, 0.0), (1.5, 1.5, 0.0)]], np.float32)
    summary, att, status = ar.score(g, poses, table, ch, np.array([[1.0, 0.0]]), 1.0, (0, 0))
    # pose 0: wheels on cells x = 2 and x = 0: pitch (2 - 0) / 2 = 1, roll 0; the plane is 1 at the pose and has the ground's slope, the
    # pose sits at its cell's centre: the clearance is the belly's height over both cells
    assert att[0, 0].tolist() == [1.0, 0.0, 0.5] and status[0].tolist() == [ar.OK, ar.INVALID, ar.LEFT_WINDOW, ar.UNKNOWN_GROUND, ar.OK]
    assert summary.tolist() == [[ar.INVALID, 1, 0, 0, 0]]


@pytest.mark.parametrize("grad", [(0.0, 0.0), (0.21, -0.13), (-0.4, 0.05), (0.0, 0.3)])
def test_on_a_plane_the_numbers_are_the_gradient_in_the_body_frame(grad):
    """ground z = p*xw + q*yw + r sampled at cell centres: a wheel's height is read at most res*sqrt(2)/2 from where the wheel stands,
    so it is off by at most E = |grad|*res*sqrt(2)/2; a difference of two axle means by 2 E, the tangent by 2 E / lever =
    |grad|*res*sqrt(2)/lever.  The estimated plane at a belly cell is off by the error of z0 (<= E) plus the tangents' errors times
    their arms: |clr - belly_height| <= |grad|*res*sqrt(2) * (0.5 + |u - am| / wheelbase + |v| / track), the factor taken at the worst
    cell of the pose.  float32 storage adds half an ulp.  A sign error in pitch, roll, u or v breaks the bound at once."""
    import gvom
    xy, res, oc, H = 64, 0.4, (-100, -31), 16
    p, q = grad
    g = ar.plane_ground(xy, res, oc, p, q, 1.5)
    table = gvom.rectangle_footprint(1.4, 0.6, 0.5, res, headings=H)
    ch = ar.make_chassis(1.2, -0.4, 0.9, 0.375)
    cs = ar.cos_sin(H)
    poses = rr.arc_poses(40, 30, xy, res, oc, 3, spread=12.0, centre=(xy // 2, xy // 2))
    _, att, status = ar.score(g, poses, table, ch, cs, res, oc)
    ok = status == ar.OK
    assert ok.sum() > 600 and set(np.unique(status)) <= {ar.OK, ar.LEFT_WINDOW}
    _, _, h, _ = rr.pose_frame(poses, res, oc, H)
    c, s = cs[h, 0], cs[h, 1]
    pitch, roll = p * c + q * s, q * c - p * s                      # the gradient along body x (forward) and body y (left)
    norm = math.hypot(p, q)
    wb, am = ch.front_axle - ch.rear_axle, 0.5 * (ch.front_axle + ch.rear_axle)
    half_ulp = lambda v: 2.0 ** -24 * np.abs(v) + 1e-12
    assert (np.abs(att[..., 0] - pitch)[ok] <= (norm * res * math.sqrt(2.0) / wb + half_ulp(pitch))[ok]).all()
    assert (np.abs(att[..., 1] - roll)[ok] <= (norm * res * math.sqrt(2.0) / ch.track + half_ulp(roll))[ok]).all()
    if norm > 0:                                                    # ... and the bound is not vacuous: the signs are seen
        assert (np.sign(att[..., 0]) == np.sign(pitch))[ok & (np.abs(pitch) > 0.2)].all() and (ok & (np.abs(pitch) > 0.2)).sum() > 50
        assert (np.sign(att[..., 1]) == np.sign(roll))[ok & (np.abs(roll) > 0.2)].all() and (ok & (np.abs(roll) > 0.2)).sum() > 50
    start, offsets = table
    x, y = poses[..., 0].astype(np.float64) / res, poses[..., 1].astype(np.float64) / res
    fx, fy = x - np.floor(x), y - np.floor(y)
    for k, t in np.argwhere(ok):
        o = offsets[start[h[k, t]]:start[h[k, t] + 1]].astype(np.float64)
        du, dv = (o[:, 0] + 0.5 - fx[k, t]) * res, (o[:, 1] + 0.5 - fy[k, t]) * res
        u, v = du * c[k, t] + dv * s[k, t], dv * c[k, t] - du * s[k, t]
        factor = 0.5 + (np.abs(u - am) / wb + np.abs(v) / ch.track).max()
        assert abs(att[k, t, 2] - ch.belly_height) <= norm * res * math.sqrt(2.0) * factor + 2.0 ** -24 * 0.375 + 1e-12, (k, t, factor)
    if norm == 0:                                                   # flat ground: exact
        assert (att[ok] == np.array([0.0, 0.0, 0.375], np.float32)).all()
    else:
        assert np.abs(att[..., 2][ok] - ch.belly_height).max() > 1e-3


def test_census_of_every_gpu_input():
    import gvom
    inputs = []
    for shape in ar.SHAPES:
        qs, ex = ar.cases(shape), ar.expected(shape)
        assert len(qs) == len(ex) >= 7
        inputs += list(zip(qs, ex))
        assert all(q["poses"].shape == shape + (3,) and q["poses"].dtype == np.float32 for q in qs)
    inputs += list(zip(ar.limit_cases(), ar.expected_limits()))
    assert set(ar.CELLS) <= {int(np.diff(q["table"][0])[0]) for q, _ in inputs}
    assert {q["xy"] for q, _ in inputs} == set(ar.SIZES)
    assert {len(q["table"][0]) - 1 for q, _ in inputs} == set(ar.HEADINGS)
    assert {q["device"] for q, _ in inputs} == {True, False}
    assert {q["pattern"] for q, _ in inputs} == set(ar.GROUNDS)
    n = ar.census(inputs)
    print(n)
    # floors: what the inputs reached when they were written (the counts may only grow)
    for s, floor, rollouts in zip(range(7), (40000, 250, 350, 13000, 20000, 65000, 80), (250, 15, 15, 150, 400, 1800, 30)):
        assert n["status"][s] >= floor, (s, n)                   # poses
        assert n["summary_status"][s] >= rollouts, (s, n)        # rollouts that end so
    for what, floor in (("first_0", 2000), ("first_T", 250), ("wheel_unknown_only", 2000), ("belly_unknown_only", 7000), ("belly_inf", 10),
                        ("tie_pitch", 400), ("tie_roll", 400), ("tie_belly", 200), ("on_border", 70), ("map_nan", 1200), ("map_inf", 2500),
                        ("map_m1000", 20000), ("west", 6000), ("east", 5000), ("south", 6000), ("north", 4000), ("wheel_outside_only", 3000)):
        assert n[what] >= floor, (what, n)
    assert n["heading_ties"] == {0.5, 1.5, 2.5, -0.5}
    assert n["ulp"] == {(j, side) for j in range(3) for side in ("above", "on", "below")}
    # the limit cases decide as the definition says: one ulp above a tangent limit is bad, on it and below it is not; for the belly
    # one ulp below the least clearance is bad
    for q, (summary, att, status) in zip(ar.limit_cases(), ar.expected_limits()):
        k, t, j = q["probe"]
        bad = status[k, t] == (ar.PITCH, ar.ROLL, ar.BELLY)[j]
        side = q["name"].rsplit(" ", 1)[1]
        assert bad == (side == ("above" if j < 2 else "below")), (q["name"], status[k, t])
    car = gvom.rectangle_footprint(rr.CAR["front"], rr.CAR["rear"], rr.CAR["half_width"], rr.RES[1024], headings=64)
    q, (summary, att, status) = ar.large_case((car[0].tobytes(), car[1].tobytes(), 64))
    assert q["poses"].shape == (1024, 64, 3) and min(q["origin_cells"]) < 0
    assert all((status == s).sum() >= 100 for s in (ar.OK, ar.PITCH, ar.ROLL, ar.BELLY, ar.UNKNOWN_GROUND, ar.LEFT_WINDOW)), np.bincount(status.ravel())
    assert (summary[:, 1] > 5).sum() > 50


def _bare(xy=16, res=0.4):
    import gvom
    g = gvom.Gvom.__new__(gvom.Gvom)              # no handle, no library: a call that got as far as the library would not raise ValueError
    g.xy_size, g.xy_resolution, g._lib, g._h = xy, res, None, None
    return gvom, g


def test_python_arguments_are_checked_before_any_library_call():
    gvom, g = _bare()
    ground = np.zeros((16, 16))
    poses = np.zeros((2, 3, 3), np.float32)
    for bad, word in ((np.ones((16, 15)), "shape"), (None, "ground"), (np.zeros((4, 4, 4)), "shape")):
        with pytest.raises(ValueError, match=word):
            g.score_attitude_of(bad, poses)
    for bad, word in ((np.zeros((2, 3)), "shape"), (np.zeros((2, 3, 2)), "shape"), (np.zeros((2, 4097, 3)), "4096"), (np.zeros((0, 3, 3)), "K >= 1"),
                      (np.zeros((2, 0, 3)), "4096"), (np.zeros((2, 3, 3), dtype=object), "numbers")):
        with pytest.raises(ValueError, match=word):
            g.score_attitude_of(ground, bad)
    for K, T, word in ((0, 5, "K >= 1"), (5, 0, "4096"), (5, 4097, "4096"), ((1 << 26) // 4096 + 1, 4096, "2\\*\\*26"), (1.5, 3, "K >= 1"),
                       (float("nan"), 3, "K >= 1")):
        with pytest.raises(ValueError, match=word):
            g.score_attitude_of_device(1 << 20, 1 << 21, K, T)
    for g_ptr, p_ptr in ((0, 1 << 20), (1 << 20, 0), (None, 1 << 20)):
        with pytest.raises(ValueError, match="device addresses"):
            g.score_attitude_of_device(g_ptr, p_ptr, 1, 1)
    for bad in ((float("nan"), 0.0), (0.0, float("inf")), (1e30, 0.0), (1.0,)):
        with pytest.raises(ValueError, match="origin"):
            g.score_attitude_of(ground, poses, origin=bad)
    for kw, word in ((dict(front_axle=float("nan")), "finite"), (dict(track=float("inf")), "finite"), (dict(belly_height=float("-inf")), "finite"),
                     (dict(front_axle=0.0, rear_axle=0.0), "in front of"), (dict(front_axle=-1.0, rear_axle=0.5), "in front of"), (dict(track=0.0), "track"),
                     (dict(track=-1.0), "track"), (dict(max_pitch=float("nan")), "max_pitch"), (dict(max_pitch=-0.1), "max_pitch"),
                     (dict(max_roll=math.pi / 2), "max_roll"), (dict(max_roll=float("inf")), "max_roll"), (dict(min_clearance=float("nan")), "min_clearance")):
        args = dict(front_axle=2.0, rear_axle=0.0, track=1.5, belly_height=0.3)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            gvom.chassis(**args)
    c = gvom.chassis(2.0, 0.0, 1.5, 0.3)
    with pytest.raises(ValueError, match="set_footprint comes first"):
        g.set_chassis(c)
    for bad in (None, (2.0, 0.0, 1.5, 0.3), dict(front_axle=2.0)):
        with pytest.raises(ValueError, match="chassis\\(\\) returns"):
            g.set_chassis(bad)
    # a map set's own route checks its poses before it touches its owner's library
    m = gvom.DeviceMaps.__new__(gvom.DeviceMaps)
    m._owner, m.set_id, m.origin = g, 1, np.zeros(3)
    with pytest.raises(ValueError, match="shape"):
        m.score_attitude(np.zeros((3, 3)))
    for obj in (g, m):
        for a in ("_h", "_held"):
            obj.__dict__.pop(a, None)                             # (nothing for __del__ to destroy)


def test_the_attitude_layout_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "attitude_layout_host_test")
    src = os.path.join(ROOT, "tests", "attitude_layout_host_test.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src, "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "attitude layout host test ok" in run.stdout


def test_the_kernels_use_no_scratch_and_stay_inside_their_budget():
    import gvom
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    if not os.path.exists(os.path.join(kernel_regs.LLVM, "clang-offload-bundler")):
        pytest.skip("no ROCm LLVM tools")
    every = kernel_regs.kernels(gvom.library_path())
    kernels = {k: v for k, v in every.items() if "k_attitude" in k}
    assert len(kernels) == 2 and sum("k_attitude_ground" in k for k in kernels) == 1, sorted(kernels)
    for k, v in kernels.items():
        assert v["scratch"] == 0, (k, v)
        assert v["vgpr"] <= 128, (k, v)
        assert v["lds"] <= 65536, (k, v)                           # static; k_attitude's 13 bytes per pose are dynamic: <= 53,248
    assert 4096 * 13 <= 65536
    # k_rollouts next door keeps its budget with the pose frame in the shared header (parent against new, register for register
    # and byte for byte: profiles/attitude_<lib sha8>.json "resources")
    ro = [v for k, v in every.items() if "k_rollouts" in k]
    assert len(ro) == 1 and ro[0]["lds"] == 12288 and ro[0]["scratch"] == 0 and ro[0]["vgpr"] <= 64
    assert all("code" in v and v["code"] > 0 for v in kernels.values())
