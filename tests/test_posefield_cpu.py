"""Pose fields without a GPU: the referee of tests/posefield_ref.py held together (volume, Dijkstra, whole-volume relaxation, the
Bellman check and its single-state mutations), the helpers gvom.arc_primitives and gvom.pose_states against their definitions, the
binding's argument checks, and the census of what the GPU test's inputs reach."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gvom
import posefield_ref as ref
import rollouts_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_library_and_binding_agree():
    header = open(os.path.join(ROOT, "include", "gvom_hip.h")).read()
    assert int(re.search(r"#define\s+GVOM_PRODUCT_POSEFIELD\s+(\d+)", header).group(1)) == 20 == gvom.PRODUCT_POSEFIELD
    assert int(re.search(r"#define\s+GVOM_POSE_GOAL\s+(\d+)", header).group(1)) == 253 == gvom.POSE_GOAL == ref.GOAL
    assert "pose fields" in header
    L = gvom.load_library()
    assert hasattr(L, "gvom_pose_field") and hasattr(L, "gvom_primitives_set")
    assert (ref.UNSETTLED, ref.NONE, ref.UNREACHED, ref.MAX_COST) == (gvom.CTG_UNSETTLED, gvom.CTG_NONE, gvom.CTG_UNREACHED, gvom.CTG_MAX_COST)
    assert ref.CTG_STEPS == gvom.CTG_STEPS


def test_the_products_layout_under_sanitizers(tmp_path):
    """tests/posefield_layout_host_test.cpp, a program with its own main, built with AddressSanitizer and UndefinedBehaviorSanitizer"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "posefield_layout_host_test")
    src = os.path.join(ROOT, "tests", "posefield_layout_host_test.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src, "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "posefield layout host test ok" in run.stdout


# ---- the referee ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xy,H,M", [(9, 1, 1), (12, 7, 5), (16, 4, 65)])
def test_volume_is_the_rollout_pose_cost_at_the_cell_centres(xy, H, M):
    c = rollouts_ref.cost_map(xy, "random", seed=H, zeros=0.03)
    table = rollouts_ref.patch_table(H, M) if M > 1 else ref.point_footprint(H)
    C = ref.volume(c, table)
    assert np.array_equal(C, ref.volume_by_rollouts(c, table))
    if M == 1:
        assert np.array_equal(C[0], c)
    else:
        assert (C == 0).sum() > H * (c == 0).sum() and (C >= 32768).any()


SMALL = [(6, 1, 1, 0), (7, 3, 2, 1), (9, 4, 4, 2), (10, 8, 3, 3)]


@pytest.mark.parametrize("xy,H,reach,seed", SMALL)
def test_dijkstra_relaxation_and_bellman_check_agree(xy, H, reach, seed):
    c = ref.cost_map(xy, 40 + seed)
    table = ref.random_table(H, reach, seed, most=9)
    C = ref.volume(c, ref.point_footprint(H))
    goals = ref.random_goals(xy, H, seed, with_heading=seed % 2 == 1)
    seeds = ref.seed_mask(C, goals)
    for cap in (None, 1500):
        D = ref.dijkstra(C, table, seeds, cap)
        assert np.array_equal(D, ref.relax(C, table, seeds, cap))
        assert ref.bellman_violations(C, table, D, seeds, cap) == 0
        assert (D[seeds] == 0).all() and (D[C == 0] == ref.UNREACHED).all()
        if cap:
            assert D[D < ref.UNREACHED].max() <= cap and (ref.dijkstra(C, table, seeds) != D).any()
    assert 0 < (D < ref.UNREACHED).sum() < D.size


def test_bellman_check_sees_every_single_state_mutation():
    xy, H = 7, 3
    c = ref.cost_map(xy, 77)
    table = ref.random_table(H, 2, 5, most=6)
    C = ref.volume(c, ref.point_footprint(H))
    seeds = ref.seed_mask(C, [(3, 3, -1)])
    assert seeds.any()
    D = ref.dijkstra(C, table, seeds)
    n = 0
    for idx in np.ndindex(D.shape):
        for value in (int(D[idx]) - 1, int(D[idx]) + 1, ref.UNREACHED, 0, 12345):
            if value == D[idx] or value < 0 or value > ref.UNREACHED:
                continue
            E = D.copy()
            E[idx] = value
            assert ref.bellman_violations(C, table, E, seeds) > 0, (idx, int(D[idx]), int(value))
            n += 1
    assert n > 3 * D.size


def test_actions_name_the_first_primitive_that_attains_the_minimum():
    xy, H = 8, 2
    c = np.full((xy, xy), 2, np.uint16)
    table = (np.array([0, 3, 4], np.int32), np.array([(1, 0, 0, 5), (1, 0, 0, 5), (0, 1, 1, 3), (0, 1, 0, 3)], np.int16))   # a duplicate: a tie
    C = ref.volume(c, ref.point_footprint(H))
    seeds = ref.seed_mask(C, [(6, 6, 0)])
    D = ref.dijkstra(C, table, seeds)
    A = ref.actions(C, table, D, seeds)
    assert A[0, 6, 6] == ref.GOAL and A[0, 5, 6] == 0 and D[0, 5, 6] == 20           # the first of the two equal primitives
    assert A[0, 7, 6] == ref.NONE and D[0, 7, 6] == ref.UNREACHED                     # nothing drives in -x
    assert A[1, 6, 5] == 0 and D[1, 6, 5] == 12 and A[0, 6, 4] == 2 and D[0, 6, 4] == 24 and A[0, 6, 5] == ref.NONE
    path = [(3, 4, 0)]
    while A[path[-1][2], path[-1][0], path[-1][1]] != ref.GOAL:
        x, y, h = path[-1]
        dx, dy, ht, _ = table[1][table[0][h] + A[h, x, y]]
        path.append((x + int(dx), y + int(dy), int(ht)))
    assert ref.path_price(path, C, table) == D[0, 3, 4]


class _Held(object):
    """what a DevicePoseField asks of its hold, without a library"""
    product_id, kind = 1, gvom.PRODUCT_POSEFIELD

    def describe(self, part, hold=False):
        return 0, (2, 8, 8), (64, 1, 8)

    def release(self):
        pass


def test_path_from_on_a_host_copy_follows_and_raises():
    """DevicePoseField.path_from on an action volume set by hand: a path to the goal, None where unreached, RuntimeError at CTG_UNSETTLED
    -- at the start and further along --, ValueError outside the field"""
    table = (np.array([0, 3, 4], np.int32), np.array([(1, 0, 0, 5), (1, 0, 0, 5), (0, 1, 1, 3), (0, 1, 0, 3)], np.int16))
    f = gvom.DevicePoseField(_Held(), [0, 2, 0, 1], (0.0, 0.0), table)
    assert not f.converged and f.rounds == 2 and f.goals_seeded == 1
    A = np.full((2, 8, 8), gvom.CTG_NONE, np.uint8)
    A[0, 6, 6] = gvom.POSE_GOAL
    A[0, 3:6, 6] = 0                                                 # +x, +x, +x to the goal
    A[1, 3, 5] = 0                                                   # heading 1: (0, 1) to heading 0
    A[0, 2, 6] = gvom.CTG_UNSETTLED
    A[0, 1, 6] = 1                                                   # leads into the unsettled state
    A[0, 3, 2], A[1, 3, 3], A[0, 3, 4] = 2, 0, gvom.CTG_UNSETTLED    # ... and so does this one, two steps on
    A[0, 0, 0] = 3                                                   # no such primitive in heading 0's list of three
    f._host = A
    assert f.path_from(3, 5, 1) == [(3, 5, 1), (3, 6, 0), (4, 6, 0), (5, 6, 0), (6, 6, 0)]
    assert f.path_from(6, 6, 0) == [(6, 6, 0)] and f.path_from(7, 7, 1) is None
    for state in ((2, 6, 0), (1, 6, 0), (3, 2, 0), (0, 0, 0)):
        with pytest.raises(RuntimeError, match="unsettled"):
            f.path_from(*state)
    for state in ((8, 0, 0), (0, -1, 0), (0, 0, 2)):
        with pytest.raises(ValueError):
            f.path_from(*state)
    A[0, 5, 6], A[0, 6, 6] = 0, 2                                    # a chain that runs into an unreached state: (5, 6, 0) -> (6, 6, 0) -> (6, 7, 1)
    A[1, 6, 7] = gvom.CTG_NONE
    assert f.path_from(5, 6, 0) is None


# ---- arc_primitives -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,radius,res,reach,rev", [(16, 3.0, 0.5, 3, None), (16, 4.0, 0.4, 4, 2.0), (64, 6.0, 0.4, 3, 1.5), (8, 1.0, 0.5, 3, None), (12, 2.0, 0.5, 4, 3.0), (6, 1.0, 0.5, 3, None)])
def test_arc_primitives_follow_their_definition(H, radius, res, reach, rev):
    start, prims = gvom.arc_primitives(H, radius, res, reach=reach, reverse_weight=rev)
    per = 3 if rev is None else 6
    assert start.dtype == np.int32 and prims.dtype == np.int16 and np.array_equal(start, per * np.arange(H + 1))
    length, step = reach * res, 2 * math.pi / H
    k = min(int(math.floor(length / radius / step)), H // 4)
    assert k >= 1 and length / (k * step) >= radius                                   # the implied radius
    P = prims.astype(np.int64).reshape(H, per, 4)
    assert (np.abs(P[..., :2]) <= 4).all() and (P[..., 3] >= 1).all() and (P[..., 3] <= 255).all() and (P[..., 2] >= 0).all() and (P[..., 2] < H).all()
    h = np.arange(H)
    assert np.array_equal(P[:, 0, 2], h) and np.array_equal(P[:, 1, 2], (h + k) % H) and np.array_equal(P[:, 2, 2], (h - k) % H)   # straight, left, right
    for hh in range(H):
        th = hh * step
        fwd = P[hh, 0, :2] @ np.array([math.cos(th), math.sin(th)])
        left = P[hh, 1, :2] @ np.array([-math.sin(th), math.cos(th)])
        right = P[hh, 2, :2] @ np.array([-math.sin(th), math.cos(th)])
        assert fwd > 0 and left > -0.75 and right < 0.75 and left >= right
        assert abs(np.hypot(*P[hh, 0, :2]) - reach) <= 0.75 and P[hh, 0, 3] == max(1, int(np.rint(10 * np.hypot(*P[hh, 0, :2]))))
        chord = np.hypot(*P[hh, 1, :2])
        assert P[hh, 1, 3] == min(255, max(1, int(np.rint(10 * chord * (k * step / 2) / math.sin(k * step / 2)))))
        if rev is not None:
            assert np.array_equal(P[hh, 3, :3], [-P[hh, 0, 0], -P[hh, 0, 1], hh])                                      # straight back
            assert P[hh, 4, 2] == (hh - k) % H and P[hh, 5, 2] == (hh + k) % H                                         # backing up turns the other way
            assert (P[hh, 3:, :2] @ np.array([math.cos(th), math.sin(th)]) < 0).all()                                  # all three lead backwards
            for j, turn in ((3, 0), (4, k), (5, k)):                                                                   # w from its own rounded chord, times r
                arc = np.hypot(*P[hh, j, :2]) * (1.0 if turn == 0 else (turn * step / 2) / math.sin(turn * step / 2))
                assert P[hh, j, 3] == min(255, max(1, int(np.rint(max(1, int(np.rint(10 * arc))) * rev))))
    if H % 4 == 0:                                                                    # exactly symmetric under quarter turns
        q = H // 4
        R = P.copy()
        R[..., 0], R[..., 1], R[..., 2] = -P[..., 1], P[..., 0], (P[..., 2] + q) % H
        assert np.array_equal(np.roll(R, q, axis=0), P)
    assert gvom._primitive_arrays((start, prims))[1].shape == prims.shape


def test_arc_primitives_refuse_what_they_cannot_build():
    with pytest.raises(ValueError, match="does not reach"):
        gvom.arc_primitives(16, 6.0, 0.4, reach=3)                                   # 1.2 m on 6 m: 0.2 rad < one bin of 0.39
    for bad in (dict(headings=3), dict(headings=65), dict(reach=5), dict(reach=0), dict(min_turn_radius=0.0), dict(xy_resolution=float("nan")), dict(reverse_weight=-1.0)):
        kw = dict(headings=16, min_turn_radius=3.0, xy_resolution=0.5)
        kw.update(bad)
        with pytest.raises(ValueError):
            gvom.arc_primitives(**kw)


def test_primitive_tables_outside_the_limits_are_refused():
    ok = (np.array([0, 2, 3], np.int32), np.array([(1, 0, 0, 5), (0, 0, 1, 9), (-4, 4, 0, 255)], np.int16))
    gvom._primitive_arrays(ok)
    for k, col, value in ((0, 0, 5), (0, 1, -5), (0, 2, 2), (0, 2, -1), (0, 3, 0), (0, 3, 256), (1, 2, 0), (2, 0, 0)):
        pr = ok[1].astype(np.int64).copy()
        pr[k, col] = value
        if (k, col, value) == (2, 0, 0):
            pr[2] = (0, 0, 1, 3)                                                      # (0, 0, its own heading)
        with pytest.raises(ValueError, match="outside the limits"):
            gvom._primitive_arrays((ok[0], pr))
    for bad in ((np.array([1, 2, 3]), ok[1]), (np.array([0, 2, 4]), ok[1]), (np.array([0, 3, 2]), ok[1]), (ok[0], ok[1][:, :3]), (ok[0].astype(np.float64), ok[1]),
                (np.arange(67), np.zeros((66, 4), np.int16)), (np.array([0, 65]), np.tile([(1, 0, 0, 1)], (65, 1))), None, (ok[0],)):
        with pytest.raises(ValueError):
            gvom._primitive_arrays(bad)


# ---- pose_states ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xy,H", [(16, 1), (33, 7), (64, 64), (100, 16)])
def test_pose_states_are_the_rollout_pose_frame(xy, H):
    res, oc = rollouts_ref.RES[xy], rollouts_ref.ORIGIN_CELLS[xy]
    poses = np.concatenate([rollouts_ref.special_poses(xy, res, oc, H), rollouts_ref.arc_poses(40, 9, xy, res, oc, seed=xy).reshape(-1, 3)])
    states, valid = gvom.pose_states(poses, (oc[0] * res, oc[1] * res), res, H)
    cx, cy, h, want_valid = rollouts_ref.pose_frame(poses, res, oc, H)
    assert states.dtype == np.int32 and states.shape == poses.shape and valid.dtype == bool
    assert np.array_equal(valid, want_valid) and np.array_equal(states[:, 2], h)
    for got, want in ((states[:, 0], cx), (states[:, 1], cy)):
        assert np.array_equal(got, np.clip(np.where(want == rollouts_ref._OUT, -100000, want), -100000, 100000))
    with np.errstate(all="ignore"):
        a = poses[:, 2] * rollouts_ref.heading_scale(H)
    assert (~valid).sum() >= 5 and np.isnan(poses).any() and np.isinf(poses).any()                      # NaN, inf, the yaw bound, far away
    assert (states[~valid, 2] == 0).all() and (states[:, :2] == -100000).any()
    if H > 1:
        assert (valid & (np.rint(a) == H) & (states[:, 2] == 0)).any()                                   # the wrap to heading 0
        assert any((valid & (a == np.float32(t))).any() for t in (0.5, 1.5, 2.5, -0.5))                 # rounding ties
    k = gvom.pose_states(poses.reshape(-1, 1, 3)[:5], (oc[0] * res, oc[1] * res), res, H)
    assert k[0].shape == (5, 1, 3) and k[1].shape == (5, 1)
    with pytest.raises(ValueError):
        gvom.pose_states(np.zeros((4, 2)), (0, 0), res, H)


def test_goals_with_a_yaw_follow_the_rollout_heading_rule():
    H = 16
    g = gvom._pose_goals([(3, 4, 0.0), (5, 6, math.pi), (7, 8, -0.1), (1, 1, 2 * math.pi - 0.01)], 20, H, None)
    assert g.dtype == np.int32 and g.tolist() == [[3, 4, 0], [5, 6, 8], [7, 8, 0], [1, 1, 0]]
    assert gvom._pose_goals([(3, 4)], 20, H, None).tolist() == [[3, 4, -1]]
    assert gvom._pose_goals(np.array([[1.0, 2.0, 0.4]]), 20, H, (0.5, (0.0, 0.0))).tolist() == [[2, 4, 1]]
    for bad in ([(20, 0)], [(0, -1, 0.0)], [(1, 1, float("nan"))], [(1, 1, 1e30)], np.zeros((0, 2)), np.zeros((2, 4)), [("a", "b")]):
        with pytest.raises(ValueError):
            gvom._pose_goals(bad, 20, H, None)


# ---- the census of the GPU test's inputs -------------------------------------------------------------------------------------------------
def test_census_of_the_gpu_inputs():
    cases = ref.cases()
    total = dict(footprint_blocked=0, some_headings=0, dead_goals=0, ties=0, reached=0, unreached_free=0)
    sizes, heads, halos = set(), set(), set()
    for i, q in enumerate(cases):
        C, D, A, seeds, info = ref.expected(i)
        n = ref.census(C, q["c"], D, q["table"], seeds, q["goals"])
        assert n["reached"] > 0 and n["dead_goals"] > 0, q["name"]
        assert ref.bellman_violations(C, q["table"], D, seeds, q["max_cost"]) == 0, q["name"]
        for key in total:
            total[key] += n[key]
        sizes.add(q["xy"]); heads.add(q["H"]); halos.add(int(np.abs(np.asarray(q["table"][1])[:, :2]).max()))
    T = ref.TILE
    assert {T - 1, T, T + 1, 2 * T + 1, 2 * T + 4} <= sizes and {1, 4, 8, 16, 64} <= heads and {1, 3, 4} <= halos
    assert total["footprint_blocked"] > 1000 and total["some_headings"] > 100 and total["ties"] > 10 and total["unreached_free"] > 100
    assert {q["inner"] for q in cases} >= {0, 1, 3} and {q["batch"] for q in cases} >= {0, 1, 5}
    # the cap cuts a field; high costs reach past 2^24
    capped = [i for i, q in enumerate(cases) if q["max_cost"]]
    for i in capped:
        q = cases[i]
        C, D, _, seeds, _ = ref.expected(i)
        assert (ref.relax(C, q["table"], seeds) != D).any()
    assert max(int(ref.expected(i)[1][ref.expected(i)[1] < ref.UNREACHED].max()) for i in range(len(cases))) > 1 << 24


def test_the_gap_is_passable_lengthways_only_and_reversing_reaches_more():
    cases = ref.cases()
    i_rev = [i for i, q in enumerate(cases) if q["name"].endswith("arcs+reverse gap")][0]
    i_fwd = [i for i, q in enumerate(cases) if q["name"].endswith("arcs gap")][0]
    q = cases[i_rev]
    C, D, A, seeds, _ = ref.expected(i_rev)
    _, rows = ref.gap_scene(q["footprint"])
    wall, mid, H = q["xy"] // 2, (rows[0] + rows[1]) // 2, q["H"]
    assert C[0, wall, mid] != 0 and C[H // 2, wall, mid] != 0                         # lengthways, either way round
    assert C[H // 4, wall, mid] == 0 and C[3 * H // 4, wall, mid] == 0                # broadside
    assert q["c"][wall, mid] != 0
    west = D[0, 4:wall - 8:3, mid]                                                     # 3 cells a step from the goal at x = 28
    assert (west < ref.UNREACHED).all() and (np.diff(west.astype(np.int64)) == -180).all()   # straight on: w = 30, C = 3 at both ends
    assert D[H // 2, 6, mid] > D[0, 6, mid]                                            # facing away costs more: it has to turn round
    D_fwd = ref.expected(i_fwd)[1]
    only_reverse = (D < ref.UNREACHED) & (D_fwd == ref.UNREACHED)
    assert only_reverse.sum() > 50                                                     # states that reach the goal only by backing up
    n_rev = len(q["table"][1]) // H
    backing = (A < ref.GOAL) & (A >= n_rev // 2)
    assert n_rev == 6 and backing.sum() > 50
