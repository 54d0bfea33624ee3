"""Rollout scoring (gvom_footprint_set / gvom_score_rollouts), the part that needs no GPU: header, library and binding agree; the
footprint builders are conservative and tight; the referee's two forms agree; the census of every input tests/test_rollouts.py
runs; the binding's argument checks; the product's layout under sanitizers; the kernel's registers."""
import ctypes
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import rollouts_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_10_the_symbols_the_defines_and_the_binding():
    import gvom
    header = open(os.path.join(ROOT, "include", "gvom_hip.h")).read()
    assert int(re.search(r"#define\s+GVOM_ABI_VERSION\s+(\d+)", header).group(1)) == 10
    assert gvom.ABI_VERSION == 10 and gvom.load_library().gvom_abi_version() == 10
    assert re.search(r"\bint\s+gvom_footprint_set\s*\(", header) and re.search(r"\bint\s+gvom_score_rollouts\s*\(", header)
    for word, value in (("GVOM_PRODUCT_ROLLOUTS", gvom.PRODUCT_ROLLOUTS), ("GVOM_ROLLOUT_CLEAR", gvom.ROLLOUT_CLEAR),
                        ("GVOM_ROLLOUT_COLLISION", gvom.ROLLOUT_COLLISION), ("GVOM_ROLLOUT_LEFT_WINDOW", gvom.ROLLOUT_LEFT_WINDOW),
                        ("GVOM_ROLLOUT_INVALID", gvom.ROLLOUT_INVALID)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % word, header).group(1)) == value, word
    assert gvom.PRODUCT_ROLLOUTS == 10
    assert (gvom.ROLLOUT_CLEAR, gvom.ROLLOUT_COLLISION, gvom.ROLLOUT_LEFT_WINDOW, gvom.ROLLOUT_INVALID) == (0, 1, 2, 3)
    assert (rr.CLEAR, rr.COLLISION, rr.LEFT_WINDOW, rr.INVALID, rr.UNREACHED) == (0, 1, 2, 3, gvom.CTG_UNREACHED)
    assert not re.search(r"#define\s+GVOM_PRODUCT_\w+\s+[89]\b", header)              # kinds 8 and 9 stay unassigned
    L = ctypes.CDLL(gvom.library_path())
    nm = subprocess.run(["nm", "-D", "--defined-only", gvom.library_path()], capture_output=True, text=True, check=True)
    for name, nargs in (("gvom_footprint_set", 4), ("gvom_score_rollouts", 10)):
        assert hasattr(L, name)
        row = [r for r in gvom.ABI if r[0] == name]
        assert len(row) == 1 and len(row[0][2]) == nargs
        assert re.search(r" T %s$" % name, nm.stdout, re.M)
    for m in ("set_footprint", "score_rollouts_of", "score_rollouts_of_device"):
        assert callable(getattr(gvom.Gvom, m))
    assert callable(gvom.DeviceCostField.score_rollouts) and callable(gvom.rectangle_footprint) and callable(gvom.disc_footprint)
    for attr in ("copy_to_host", "release", "__enter__", "__exit__"):
        assert callable(getattr(gvom.DeviceRollouts, attr))
    assert gvom._PRODUCT_DTYPES[gvom.PRODUCT_ROLLOUTS] == (np.int32, np.uint16)
    assert "gvom_rollouts" in open(os.path.join(ROOT, "g-vom_amd", "Makefile")).read()
    assert (gvom.ROLLOUT_MAX_T, gvom.ROLLOUT_MAX_POSES) == (rr.MAX_T, 1 << 26)


def _body_samples(front, rear, hw, n=41):
    bx, by = np.meshgrid(np.linspace(-rear, front, n), np.linspace(-hw, hw, n))
    return bx.ravel(), by.ravel()


def _distance_to_rectangle(px, py, c, s, front, rear, hw):
    """distance of world points from the rectangle turned by (c, s)"""
    u, v = c * px + s * py, -s * px + c * py
    return np.hypot(np.maximum(np.maximum(u - front, -rear - u), 0.0), np.maximum(np.abs(v) - hw, 0.0))


@pytest.mark.parametrize("H", [1, 7, 64])
@pytest.mark.parametrize("margin", [0.0, 0.3])
def test_rectangle_footprint_is_conservative_and_tight(H, margin):
    import gvom
    front, rear, hw, res = 1.9, 0.7, 0.55, 0.25
    start, offsets = gvom.rectangle_footprint(front, rear, hw, res, headings=H, margin=margin)
    assert start.dtype == np.int32 and offsets.dtype == np.int16 and start.shape == (H + 1,) and offsets.shape == (start[-1], 2)
    assert start[0] == 0 and (np.diff(start) >= 1).all()                              # every heading has a cell
    rng = np.random.default_rng(H)
    bx, by = _body_samples(front, rear, hw)
    for h in range(H):
        a = 2.0 * math.pi * h / H
        c, s = math.cos(a), math.sin(a)
        if (4 * h) % H == 0:
            c, s = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[(4 * h) // H]
        cells = {(int(dx), int(dy)) for dx, dy in offsets[start[h]:start[h + 1]]}
        assert len(cells) == start[h + 1] - start[h]                                  # no cell twice
        # conservative: wherever inside its cell the pose lies, every cell a point of the rectangle falls into is in the mask
        for px, py in np.concatenate([rng.uniform(0.0, res, (12, 2)), [[0.0, 0.0], [np.nextafter(res, 0), np.nextafter(res, 0)]]]):
            wx, wy = px + c * bx - s * by, py + s * bx + c * by
            touched = set(zip(np.floor(wx / res).astype(int).tolist(), np.floor(wy / res).astype(int).tolist()))
            assert touched <= cells, (h, sorted(touched - cells)[:4])
        # tight: no cell further from the rectangle than a square's half diagonal and the margin
        o = offsets[start[h]:start[h + 1]].astype(np.float64) * res
        d = _distance_to_rectangle(o[:, 0], o[:, 1], c, s, front, rear, hw)
        assert d.max() <= res * math.sqrt(2.0) + margin + 1e-9, (h, d.max())
    if H == 1 and margin == 0.0:                                                       # heading 0 is the axis-aligned rectangle itself
        want = {(dx, dy) for dx in range(-30, 31) for dy in range(-30, 31)
                if dx * res + res > -rear and dx * res - res < front and dy * res + res > -hw and dy * res - res < hw}
        assert {(int(a), int(b)) for a, b in offsets} == want


def test_quarter_turns_are_exact_and_margins_only_add():
    import gvom
    start, offsets = gvom.rectangle_footprint(2.0, 1.0, 0.5, 0.5, headings=4)
    sets = [{(int(a), int(b)) for a, b in offsets[start[h]:start[h + 1]]} for h in range(4)]
    assert sets[1] == {(-dy, dx) for dx, dy in sets[0]} and sets[2] == {(-dx, -dy) for dx, dy in sets[0]}
    assert sets[3] == {(dy, -dx) for dx, dy in sets[0]} and sets[0] != sets[2]          # (front != rear: not symmetric)
    for H in (7, 16):
        small, large = (gvom.rectangle_footprint(2.0, 1.0, 0.5, 0.5, headings=H, margin=m) for m in (0.0, 0.4))
        for h in range(H):
            a = {tuple(v) for v in small[1][small[0][h]:small[0][h + 1]].tolist()}
            b = {tuple(v) for v in large[1][large[0][h]:large[0][h + 1]].tolist()}
            assert a < b
    s1, o1 = gvom.disc_footprint(1.0, 0.4)
    assert s1.tolist() == [0, len(o1)] and {(0, 0), (3, 0), (-3, 0), (0, 3), (2, 2)} <= {tuple(v) for v in o1.tolist()}
    assert (4, 0) not in {tuple(v) for v in o1.tolist()}                               # its square starts at 1.2 m
    assert gvom.disc_footprint(0.0, 0.4)[1].tolist() == [[0, 0]]
    car = gvom.rectangle_footprint(rr.CAR["front"], rr.CAR["rear"], rr.CAR["half_width"], 0.2, headings=64)
    assert 250 <= np.diff(car[0]).min() and np.diff(car[0]).max() <= 400 and abs(np.diff(car[0]).mean() - 325) < 30


def test_the_two_referee_forms_agree_on_tiny_inputs():
    rng = np.random.default_rng(3)
    n = 0
    for xy, H, M, with_field in ((5, 1, 1, True), (6, 3, 4, False), (7, 7, 9, True), (9, 4, 12, True)):
        res, oc = (0.4, 0.25, 0.1, 0.5)[n % 4], ((-2, 1), (3, -4), (0, 0), (-7, -7))[n % 4]
        for pattern in rr.PATTERNS:
            c = rr.cost_map(xy, pattern, seed=n)
            D = rr.field_of(c) if with_field else None
            table = rr.patch_table(H, M, seed=n) if n % 2 == 0 else rr.asymmetric_table(H)
            poses = rr.make_poses(6, 9, xy, res, oc, H, seed=n)
            poses[5, 2:7] = rr.special_poses(xy, res, oc, H)[rng.choice(20, 5)]
            got = rr.score(c, poses, table, res, oc, D)
            want = rr.score_loops(c.tolist(), poses.tolist(), table, res, oc, None if D is None else D.tolist())
            assert np.array_equal(got[0], want[0]), (xy, H, M, pattern, got[0], want[0])
            assert np.array_equal(got[1], want[1]), (xy, H, M, pattern)
            assert got[0].dtype == np.int32 and got[1].dtype == np.uint16
            n += 1
    # by hand: a 4 x 4 map, the footprint {(0, 0), (1, 0)}, one heading
    c = np.array([[5, 5, 5, 5], [5, 40000, 5, 5], [5, 5, 0, 5], [5, 5, 5, 5]], np.uint16)
    D = np.arange(16, dtype=np.int32).reshape(4, 4)
    table = (np.array([0, 2], np.int32), np.array([[0, 0], [1, 0]], np.int16))
    poses = np.array([[(0.5, 1.5, 0.0), (1.5, 1.5, 0.0), (1.5, 2.5, 0.0), (0.5, 0.5, 0.0)],        # 40000, 40000, hits (2, 2), clear again
                      [(3.5, 0.5, 0.0), (0.5, 0.5, 0.0), (0.5, 0.5, 0.0), (0.5, 0.5, 0.0)],        # (4, 0) is outside at once
                      [(0.5, 0.5, 0.0), (0.5, 0.5, 0.0), (0.5, 0.5, 0.0), (0.5, 0.5, np.nan)]], np.float32)
    summary, cost, _ = rr.score(c, poses, table, 1.0, (0, 0), D)
    assert cost.tolist() == [[40000, 40000, 0, 5], [0, 5, 5, 5], [5, 5, 5, 0]]
    assert summary.tolist() == [[rr.COLLISION, 2, 80000, 5], [rr.LEFT_WINDOW, 0, 0, rr.UNREACHED], [rr.INVALID, 3, 15, 0]]


def test_census_of_every_gpu_input():
    import gvom
    inputs = []
    for shape in rr.SHAPES:
        qs, ex = rr.cases(shape), rr.expected(shape)
        assert len(qs) == len(ex) >= 7
        inputs += list(zip(qs, ex))
        assert {len(q["table"][0]) - 1 for q in qs} >= {1, 7, 64} or shape == (1, 1) or len({len(q["table"][0]) - 1 for q in qs}) >= 2
        assert all(q["poses"].shape == shape + (3,) and q["poses"].dtype == np.float32 for q in qs)
    cells = {int(np.diff(q["table"][0])[0]) for q, _ in inputs}
    assert set(rr.CELLS) <= cells
    assert {q["xy"] for q, _ in inputs} == set(rr.SIZES)
    assert {len(q["table"][0]) - 1 for q, _ in inputs} == set(rr.HEADINGS)
    assert {q["D"] is None for q, _ in inputs} == {True, False} and {q["device"] for q, _ in inputs} == {True, False}
    assert all(any(pattern in q["name"] for q, _ in inputs) for pattern in rr.PATTERNS)
    n = rr.census(inputs)
    print(n)
    for status in ("clear", "collision", "left_window", "invalid"):
        assert n[status] >= 10, (status, n)
    for what in ("first_0", "first_last", "first_T", "clear_after_blocked", "high_cost", "cost_65535", "terminal_finite",
                 "terminal_unreached_with_field", "on_border", "negative", "west", "east", "south", "north", "wrap_to_0", "pi", "nan", "inf",
                 "yaw_bound", "far"):
        assert n[what] >= 1, (what, n)
    assert n["ties"] == {0.5, 1.5, 2.5, -0.5}
    # the rounding ties land where round-half-even puts them: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> 0
    for H in (7, 64):
        yaws = [rr._tie_yaw(H, t) for t in (0.5, 1.5, 2.5, -0.5)]
        p = np.array([[(0.0, 0.0, y) for y in yaws]], np.float32)
        assert rr.pose_frame(p, 0.4, (0, 0), H)[2].tolist() == [[0, 2, 2, 0]]
    two_pi = np.float32(2.0 * np.pi)
    p = np.array([[(0.0, 0.0, np.float32(np.pi)), (0.0, 0.0, np.float32(-np.pi)), (0.0, 0.0, np.nextafter(two_pi, np.float32(0)))]], np.float32)
    assert rr.pose_frame(p, 0.4, (0, 0), 64)[2].tolist() == [[32, 32, 0]]
    # the large inputs: the car at a negative, non-zero origin; the largest map with poses at its far corner
    car = gvom.rectangle_footprint(rr.CAR["front"], rr.CAR["rear"], rr.CAR["half_width"], rr.RES[1024], headings=64)
    q, (summary, cost, status) = rr.large_case(1024, (car[0].tobytes(), car[1].tobytes(), 64))
    assert q["poses"].shape == (1024, 64, 3) and min(q["origin_cells"]) < 0 and 0 not in q["origin_cells"]
    assert all((summary[:, 0] == s).sum() >= 10 for s in (rr.CLEAR, rr.COLLISION, rr.LEFT_WINDOW)) and (cost > 0).mean() > 0.3
    assert (summary[:, 3] != rr.UNREACHED).sum() > 100


def test_the_centre_cell_is_world_to_cells():
    import gvom
    rng = np.random.default_rng(11)
    for res, origin in ((0.4, (-2.0, 1.2)), (0.25, (1.75, -10.0)), (0.1, (1.2, 0.9))):
        pts = rng.uniform(-30, 30, (500, 2)).astype(np.float32)
        pts[:50] = np.float32(np.round(pts[:50] / res) * res)                       # on cell borders, as float32 sees them
        oc = tuple(int(v) for v in np.round(np.array(origin) / res))
        poses = np.concatenate([pts, np.zeros((500, 1), np.float32)], axis=1)[None]
        cx, cy, _, valid = rr.pose_frame(poses, res, oc, 1)
        want = gvom.world_to_cells(pts.astype(np.float64), res, origin)
        assert valid.all() and np.array_equal(np.stack([cx[0], cy[0]], axis=1), want)
        assert tuple(gvom._rollout_origin(origin, res)) == oc


def _bare(xy=16, res=0.4):
    import gvom
    g = gvom.Gvom.__new__(gvom.Gvom)              # no handle, no library: a call that got as far as the library would not raise ValueError
    g.xy_size, g.xy_resolution, g._lib, g._h = xy, res, None, None
    return gvom, g


def test_python_arguments_are_checked_before_any_library_call():
    gvom, g = _bare()
    cost = np.ones((16, 16), np.uint16)
    poses = np.zeros((2, 3, 3), np.float32)
    for bad, word in ((np.ones((16, 15)), "shape"), (np.full((16, 16), -1), "0 .. 65535"), (np.full((16, 16), 65536), "0 .. 65535"),
                      (np.full((16, 16), float("nan")), "finite"), (np.full((16, 16), 1.5), "whole"), (None, "cell_cost")):
        with pytest.raises(ValueError, match=word):
            g.score_rollouts_of(bad, poses)
    with pytest.raises(ValueError, match="cost_to_go must have shape"):
        g.score_rollouts_of(cost, poses, cost_to_go=np.zeros((4, 4), np.int32))
    with pytest.raises(ValueError, match="cost_to_go must lie"):
        g.score_rollouts_of(cost, poses, cost_to_go=np.full((16, 16), 2 ** 31))
    for bad, word in ((np.zeros((2, 3)), "shape"), (np.zeros((2, 3, 2)), "shape"), (np.zeros((2, 4097, 3)), "4096"), (np.zeros((0, 3, 3)), "K >= 1"),
                      (np.zeros((2, 0, 3)), "4096"), (np.zeros((2, 3, 3), dtype=object), "numbers")):
        with pytest.raises(ValueError, match=word):
            g.score_rollouts_of(cost, bad)
    for K, T, word in ((0, 5, "K >= 1"), (5, 0, "4096"), (5, 4097, "4096"), ((1 << 26) // 4096 + 1, 4096, "2\\*\\*26"), (1.5, 3, "K >= 1"),
                       (float("nan"), 3, "K >= 1")):
        with pytest.raises(ValueError, match=word):
            g.score_rollouts_of_device(1 << 20, 1 << 21, K, T)
    for c_ptr, p_ptr in ((0, 1 << 20), (1 << 20, 0), (None, 1 << 20)):
        with pytest.raises(ValueError, match="device addresses"):
            g.score_rollouts_of_device(c_ptr, p_ptr, 1, 1)
    for bad in ((float("nan"), 0.0), (0.0, float("inf")), (1e30, 0.0), (1.0,)):
        with pytest.raises(ValueError, match="origin"):
            g.score_rollouts_of(cost, poses, origin=bad)
    st, of = np.array([0, 2], np.int32), np.array([[0, 0], [1, 0]], np.int16)
    for bad, word in (((st, of, of), "pair"), (7, "pair"), ((st, of[:1]), "offsets"), ((np.array([1, 2]), of), "begin at 0"), ((np.array([0, 0, 2]), of), "between 1 and"),
                      ((np.array([0]), of[:0]), "start must be"), ((st, of.astype(np.float64)), "offsets must be integers"),
                      ((st, np.array([[0, 0], [40000, 0]])), "int16"), ((st, of.ravel()), "offsets must be integers"),
                      ((np.arange(1026), np.zeros((1025, 2), np.int16)), "start must be"),
                      ((np.array([0, 16385]), np.zeros((16385, 2), np.int16)), "between 1 and")):
        with pytest.raises(ValueError, match=word):
            g.set_footprint(bad)
    for kw, word in ((dict(headings=0), "headings"), (dict(headings=1025), "headings"), (dict(headings=2.5), "headings"), (dict(margin=-0.1), "margin"),
                     (dict(margin=float("nan")), "margin"), (dict(xy_resolution=0.0), "xy_resolution"), (dict(half_width=-1.0), "half_width"),
                     (dict(front=float("inf")), "front"), (dict(front=100.0, xy_resolution=0.01), "cells")):
        args = dict(front=2.0, rear=1.0, half_width=0.5, xy_resolution=0.4)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            gvom.rectangle_footprint(**args)
    for r, res, word in ((-1.0, 0.4, "radius"), (float("nan"), 0.4, "radius"), (1.0, 0.0, "xy_resolution"), (100.0, 0.01, "cells")):
        with pytest.raises(ValueError, match=word):
            gvom.disc_footprint(r, res)
    # a cost field's own route checks its poses before it touches its owner's library
    f = gvom.DeviceCostField.__new__(gvom.DeviceCostField)
    hold = gvom._ProductHold.__new__(gvom._ProductHold)
    hold._owner, hold.product_id = g, 1
    f._hold, f.product_id, f.origin = hold, 1, np.zeros(2)
    with pytest.raises(ValueError, match="shape"):
        f.score_rollouts(np.zeros((3, 3)))
    for obj in (g, hold):
        for a in ("_h", "_held"):
            obj.__dict__.pop(a, None)                             # (nothing for __del__ to destroy)


def test_the_rollout_layout_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "rollouts_layout_host_test")
    src = os.path.join(ROOT, "tests", "rollouts_layout_host_test.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src, "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "rollouts layout host test ok" in run.stdout


def test_the_kernel_uses_no_scratch_and_leaves_room_for_eight_waves():
    import gvom
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    if not os.path.exists(os.path.join(kernel_regs.LLVM, "clang-offload-bundler")):
        pytest.skip("no ROCm LLVM tools")
    kernels = {k: v for k, v in kernel_regs.kernels(gvom.library_path()).items() if "k_rollouts" in k}
    assert len(kernels) == 1, sorted(kernels)
    for k, v in kernels.items():
        assert v["scratch"] == 0, (k, v)
        assert v["vgpr"] <= 64, (k, v)                             # 8 waves per SIMD: the gathers' latency is hidden by other poses
        assert v["lds"] == rr.MAX_T * 3, (k, v)                    # a uint16 cost and a uint8 status per pose
