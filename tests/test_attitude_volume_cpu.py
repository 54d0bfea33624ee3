"""Attitude volumes without a GPU: the two forms of the referee of tests/attitude_volume_ref.py held together bit for bit, the referee
against attitude_ref.score() -- terrain attitude scoring itself -- on the float32 poses at the cell centres, the wheel-cell rule against
the pose rule at the inputs where the two must agree, the masked pose cost and its field, the product's layout as a stand-alone
program under sanitizers, the binding's argument checks, and the census of what the GPU test's inputs reach."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gvom
import attitude_ref as ar
import attitude_volume_ref as av
import posefield_ref as pf
import rollouts_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_library_and_binding_agree():
    header = open(os.path.join(ROOT, "include", "gvom_hip.h")).read()
    assert int(re.search(r"#define\s+GVOM_PRODUCT_ATTITUDE_VOLUME\s+(\d+)", header).group(1)) == 30 == gvom.PRODUCT_ATTITUDE_VOLUME
    assert "attitude volumes" in header
    L = gvom.load_library()
    assert hasattr(L, "gvom_attitude_volume") and hasattr(L, "gvom_pose_field_attitude")
    assert (av.OK, av.PITCH, av.ROLL, av.BELLY, av.UNKNOWN_GROUND, av.LEFT_WINDOW, av.INVALID) == (
        gvom.ATTITUDE_OK, gvom.ATTITUDE_PITCH, gvom.ATTITUDE_ROLL, gvom.ATTITUDE_BELLY, gvom.ATTITUDE_UNKNOWN_GROUND, gvom.ATTITUDE_LEFT_WINDOW,
        gvom.ATTITUDE_INVALID)
    assert gvom._ATTITUDE_BLOCKS == (gvom.ATTITUDE_PITCH, gvom.ATTITUDE_ROLL, gvom.ATTITUDE_BELLY)
    assert gvom._PRODUCT_DTYPES[30] == (np.uint8, np.uint8, np.int32)
    # one text of the definition: k_attitude and k_volume_attitude take the status words, the known-ground rule, the wheels and the
    # stance from gvom_rollouts.h; the volume kernel has no copy of its own
    csrc = os.path.join(ROOT, "g-vom_amd", "csrc")
    shared = open(os.path.join(csrc, "gvom_rollouts.h")).read()
    for word in ("#define AT_OK 0", "#define AT_LEFT_WINDOW 5", "#define AT_INVALID 6", "bool at_known(", "AtStance at_stance(", "AtWheels at_state_wheels(",
                 "bool at_pose_cells(", "bool at_pose_heights(", "void at_tally(", "int at_first_bad("):
        assert word in shared, word
    for unit, words in (("gvom_attitude.hip", ("at_pose_cells(", "at_pose_heights(", "at_stance(", "at_first_bad(", "AT_LEFT_WINDOW")),
                        ("gvom_attitude_volume.hip", ("at_state_wheels(", "at_stance(", "at_known(", "at_tally(", "AT_LEFT_WINDOW"))):
        text = open(os.path.join(csrc, unit)).read()
        assert '#include "gvom_rollouts.h"' in text
        for word in words:
            assert word in text, (unit, word)
        for own in ("av_known", "0.25 * (", "#define AT_OK", "#define AV_OK", "AV_LEFT_WINDOW", "wcell[h * 12 + 2", "wheels[(h * 4"):
            assert own not in text, (unit, own)


def test_the_products_layout_under_sanitizers(tmp_path):
    """tests/attitude_volume_layout_host_test.cpp, a program with its own main, built with AddressSanitizer and UndefinedBehaviorSanitizer"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "attitude_volume_layout_host_test")
    src = os.path.join(ROOT, "tests", "attitude_volume_layout_host_test.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src, "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "attitude volume layout host test ok" in run.stdout


def _rolling_ground(xy, seed, holes=0.02):
    rng = np.random.default_rng(400 + seed)
    i, j = np.meshgrid(np.arange(xy, dtype=np.float64), np.arange(xy, dtype=np.float64), indexing="ij")
    g = 0.4 * np.sin(i * 0.31 + seed) * np.cos(j * 0.27) + rng.uniform(0.0, 0.06, (xy, xy))
    hole = rng.random((xy, xy)) < holes
    kinds = rng.integers(0, 4, (xy, xy))
    for n, v in enumerate((np.nan, np.inf, -1000.0, -2000.5)):
        g[hole & (kinds == n)] = v
    return g


INF32 = ar.INF32
SMALL = [
    # xy, H, M, res, limits (max_pitch, max_roll, min_clearance)
    (9, 1, 1, 0.4, (np.float32(0.3), np.float32(0.35), np.float32(0.04))),
    (11, 3, 5, 0.25, (INF32, np.float32(0.2), -INF32)),
    (12, 4, 9, 0.5, (np.float32(0.0), INF32, np.float32(0.1))),
    (10, 7, 4, 0.4, (np.float32(0.15), np.float32(0.0), np.float32(0.3))),
    (13, 2, 17, 0.1, (np.float32(0.5), np.float32(0.5), np.float32(0.0))),
]


@pytest.mark.parametrize("xy,H,M,res,limits", SMALL)
def test_the_two_forms_of_the_referee_agree_bit_for_bit(xy, H, M, res, limits):
    table = rr.patch_table(H, M, seed=xy) if M > 1 else pf.point_footprint(H)
    ch = ar.make_chassis(2.3 * res, -1.7 * res, 2.6 * res, 1.0 * res, *limits)
    cs = ar.cos_sin(H)
    for seed, g in enumerate((_rolling_ground(xy, xy) * res, ar.ground_map(xy, "random", res, (0, 0), xy), ar.ground_map(xy, "steps", res, (0, 0)))):
        a = av.volume(g, table, ch, cs, res)
        b = av.volume_loops(g.tolist(), table, ch, cs, res)
        for name, x, y in zip(("status", "tilt", "counts"), a, b):
            assert x.dtype == y.dtype and np.array_equal(x, y), (name, seed, np.argwhere(x != y)[:3].tolist())
        assert a[2][7] == H and a[2][:7].sum() == H * xy * xy and a[2][av.INVALID] == 0
        assert a[1].max() <= 100 and (a[1][a[0] >= av.UNKNOWN_GROUND] == 0).all()


def test_the_tilt_is_the_share_of_the_nearer_limit():
    ch = ar.make_chassis(1.0, 0.0, 1.0, 0.2, max_pitch=np.float32(0.4), max_roll=np.float32(0.2))
    p = np.array([0.0, 0.1, -0.2, 0.39999, 0.4, 0.5, np.nan, np.inf, 0.0], np.float32)
    r = np.array([0.0, 0.0, 0.05, 0.0, 0.0, 0.0, 0.0, 0.0, -0.1999], np.float32)
    st = np.zeros(9, np.uint8)
    assert av.tilt_of(p, r, ch, st).tolist() == [0, 25, 50, 99, 100, 100, 0, 100, 99]
    assert av.tilt_of(p, r, ch, np.full(9, av.UNKNOWN_GROUND, np.uint8)).tolist() == [0] * 9
    free = ar.make_chassis(1.0, 0.0, 1.0, 0.2)                                            # no limits: no tilt
    assert av.tilt_of(p, r, free, st).tolist() == [0] * 9
    zero = ar.make_chassis(1.0, 0.0, 1.0, 0.2, max_pitch=np.float32(0.0), max_roll=np.float32(-1.0))
    assert av.tilt_of(p, r, zero, st).tolist() == [0, 100, 100, 100, 100, 100, 0, 100, 0]   # x / 0 = inf, 0 / 0 = NaN, a negative limit: below 0


AGREEING = [(res, o, H) for res in (0.5, 0.25) for o in (0, 37, -512) for H in (1, 4, 16, 64)]


def _car(res, H):
    table = gvom.rectangle_footprint(rr.CAR["front"], rr.CAR["rear"], rr.CAR["half_width"], res, headings=H)
    ch = ar.make_chassis(max_pitch=np.float32(np.tan(0.2)), max_roll=np.float32(np.tan(0.17)), min_clearance=np.float32(0.02), **ar.CAR_CHASSIS)
    return table, ch


@pytest.mark.parametrize("res,o,H", AGREEING)
def test_the_wheel_cell_rule_is_the_pose_rule_at_the_cell_centres(res, o, H):
    _, ch = _car(res, H)
    assert av.wheel_rules_agree(ch, ar.cos_sin(H), res, 64, (o, o)) == 0


def test_a_resolution_of_a_fifth_is_no_such_input():
    """res = 0.2: the rear axle falls on a cell boundary and the centres are no float32 numbers -- the volume is defined relative to
    the window and stays what it is, but it is not terrain attitude scoring at the rounded poses there"""
    _, ch = _car(0.2, 16)
    assert av.wheel_rules_agree(ch, ar.cos_sin(16), 0.2, 64, (37, 37)) > 0
    with pytest.raises(AssertionError, match="no float32 number"):
        av.centre_poses(16, 4, 0.2, (37, 37))


@pytest.mark.parametrize("res,o,H", AGREEING)
def test_the_volume_is_terrain_attitude_scoring_at_the_cell_centres(res, o, H):
    xy = 26 if res == 0.5 else 36
    oc = (o, -o + 3)
    table, ch = _car(res, H)
    cs = ar.cos_sin(H)
    assert av.wheel_rules_agree(ch, cs, res, xy, oc) == 0, "the wheel-cell rule and the pose rule differ at this input: the two referees cannot agree"
    g = _rolling_ground(xy, H + abs(o))
    status, tilt, counts = av.volume(g, table, ch, cs, res)
    poses = av.centre_poses(xy, H, res, oc)
    _, att, pose_status = ar.score(g, poses, table, ch, cs, res, oc)
    want = pose_status.reshape(H, xy, xy)
    assert np.array_equal(status, want), np.argwhere(status != want)[:3].tolist()
    att = att.reshape(H, xy, xy, 3)
    assert np.array_equal(tilt, av.tilt_of(att[..., 0], att[..., 1], ch, want))
    assert np.array_equal(counts[:7], np.bincount(want.ravel(), minlength=7)) and counts[7] == H


def test_those_inputs_reach_every_status():
    seen = np.zeros(7, np.int64)
    for res, o, H in AGREEING:
        if H <= 16:
            xy = 26 if res == 0.5 else 36
            table, ch = _car(res, H)
            seen += av.volume(_rolling_ground(xy, H + abs(o)), table, ch, ar.cos_sin(H), res)[2][:7]
    assert (seen[:6] > 0).all() and seen[6] == 0, seen.tolist()


def test_the_masked_pose_cost_and_its_field():
    xy, H = 12, 4
    q = dict(c=pf.cost_map(xy, 3, zeros=0.05), footprint=rr.patch_table(H, 3, seed=1), table=pf.random_table(H, 2, 4, most=6),
             goals=pf.random_goals(xy, H, 4, False))
    res = 0.4
    ch = ar.make_chassis(1.3 * res, -0.7 * res, 1.6 * res, 1.0 * res, max_pitch=np.float32(0.3), max_roll=np.float32(0.3), min_clearance=np.float32(0.05))
    status, tilt, _ = av.volume(ar.ground_map(xy, "random", res, (0, 0), 5), q["footprint"], ch, ar.cos_sin(H), res)
    C = pf.volume(q["c"], q["footprint"])
    assert np.array_equal(av.masked_cost(C, status, tilt, 0, 0), C)
    assert (av.masked_cost(C, status, tilt, 0x7f, 9) == 0).all()
    m = av.mask_of((av.PITCH, av.ROLL, av.BELLY))
    assert m == 0b1110 and av.mask_of(range(1, 6)) == 0b111110
    Cm = av.masked_cost(C, status, tilt, m, 7)
    blocked = (status >= av.PITCH) & (status <= av.BELLY)
    assert (Cm[blocked] == 0).all() and (Cm[C == 0] == 0).all()
    live = ~blocked & (C != 0)
    assert live.any() and np.array_equal(Cm[live], np.minimum(65535, C[live].astype(np.int64) + 7 * tilt[live].astype(np.int64)))
    big = np.full_like(C, 65000)
    assert av.masked_cost(big, status, np.full_like(tilt, 100), 0, 255).max() == 65535
    plain = pf.field(q["c"], q["footprint"], q["table"], q["goals"])
    same = av.field(q["c"], q["footprint"], q["table"], q["goals"], status, tilt, 0, 0)
    for a, b in zip(plain[:4], same[:4]):
        assert np.array_equal(a, b)
    masked = av.field(q["c"], q["footprint"], q["table"], q["goals"], status, tilt, m, 7)
    assert pf.bellman_violations(masked[0], q["table"], masked[1], masked[3]) == 0
    assert (masked[1][blocked] == pf.UNREACHED).all() and masked[4][0] <= plain[4][0]


class _Held(object):
    """what a DeviceAttitudeVolume asks of its hold, without a library"""
    product_id, kind = 5, gvom.PRODUCT_ATTITUDE_VOLUME

    def describe(self, part, hold=False):
        return (0, (8,), (1,)) if part == 2 else (0, (2, 8, 8), (64, 1, 8))

    def release(self):
        pass


def test_the_bindings_attitude_keywords():
    vol = gvom.DeviceAttitudeVolume(_Held())
    assert vol.status.shape == (2, 8, 8) and vol.tilt.strides == (64, 1, 8) and vol.counts.shape == (8,) and vol.counts.dtype == np.int32
    assert gvom._pose_attitude(None, gvom._ATTITUDE_BLOCKS, 0) is None
    assert gvom._pose_attitude(vol, gvom._ATTITUDE_BLOCKS, 0) == (5, 0b1110, 0)
    assert gvom._pose_attitude(vol, range(1, 6), 255) == (5, 0b111110, 255)
    assert gvom._pose_attitude(vol, (), np.int64(7)) == (5, 0, 7)
    with pytest.raises(TypeError, match="DeviceAttitudeVolume"):
        gvom._pose_attitude(np.zeros((2, 8, 8), np.uint8), gvom._ATTITUDE_BLOCKS, 0)
    with pytest.raises(ValueError, match="needs an attitude volume"):
        gvom._pose_attitude(None, gvom._ATTITUDE_BLOCKS, 3)
    for blocks in ((7,), (-1,), (1.5,), 3, ("roll",), (True,)):
        with pytest.raises(ValueError, match="attitude_blocks"):
            gvom._pose_attitude(vol, blocks, 0)
    for w in (-1, 256, 1.5, float("nan"), "7", True, None):
        with pytest.raises(ValueError, match="tilt_weight"):
            gvom._pose_attitude(vol, gvom._ATTITUDE_BLOCKS, w)


def test_census_of_the_gpu_inputs():
    total = np.zeros(7, np.int64)
    grounds, cells, heads = set(), set(), set()
    for xy in av.SIZES:
        for q, (status, tilt, counts) in zip(av.cases(xy), av.expected(xy)):
            assert status.shape == (q["H"], xy, xy) and np.array_equal(counts[:7], np.bincount(status.ravel(), minlength=7))
            total += counts[:7]
            grounds.add((q["M"], q["pattern"])); cells.add(q["M"]); heads.add((q["H"], q["pattern"]))
    assert (total[:6] > 100).all() and total[6] == 0, total.tolist()
    assert len(grounds) == 25 and cells == set(av.CELLS) and len(heads) == 15      # every footprint and every heading count on every ground
    big = [s for xy in (64, 65, 100) for s, _, _ in av.expected(xy)]
    assert sum(int(((s >= av.PITCH) & (s <= av.BELLY)).sum()) for s in big) > 1000
    tilts = np.concatenate([t.ravel() for xy in av.SIZES for _, t, _ in av.expected(xy)])
    assert tilts.max() == 100 and len(np.unique(tilts)) > 50
