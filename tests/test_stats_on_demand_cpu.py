"""CPU side of tests/test_stats_on_demand.py: every scene and script of that file run on the mirror of tests/stats_demand_ref.py alone
(g=None), with a plain oracle, an always-on oracle and the two wrong mirrors following.  No GPU.

MAPS.  The mirror's four maps, combined_hit_count, combined_total_count, combined_min_height and combined_index_map equal a plain
OracleGvom's after every combine, bit for bit, in every script: the statistics never reach them.  A mirror that is read after every
combine never pauses and equals an always-on oracle bit for bit in slot metrics, fused metrics, eigenvalues and debug cloud -- the
split of the previous map into rows with and without returns (stats_demand_ref's docstring) is inert there: no row has count 0.

DATA AND NO DATA.  Script A on rings of 1 to 4 slots: data after combines 0, 1 and 2; the fourth unread combine (number 6) merges none
and releases; the read after combine 9 gives none; the cloud returns after combine 9 + S.  A slot has metrics iff it was scanned after
the demand.  Reader periods: up to 3 the mirror never pauses; at 4 and 5 it NEVER returns data on any ring -- the fourth unread combine
has always just switched the statistics off when the reader comes (first finding; pinned as the present rule, not defended).

THAT THE GPU TESTS CAN FAIL.  At every restarted combine (one that merges statistics after a pause) the rows of combined_metrics in
which a wrong mirror differs from the right one by more than ten times parity.STATS_TOL["fused"] (stats_deviation's measure) or in its
count are counted.  "stale" differs at every one of them.  "no_prev" is EQUAL BY CONSTRUCTION at the first restarted combine behind
each pause -- the previous map has no statistics to merge in either -- and differs at every later one.  A library that answered with
either would therefore fail script A on every route: "stale" from the first restarted combine on, "no_prev" from the second (A has
five, one of them a first).  Measured, the least per case (rows of the fused map in brackets), and the floor asserted, half of it:

                       stale   no_prev   (rows)           floors
  encfuse_64x32         4558     2391    (5805-6132)      2279  1195
  encfuse_48x20         2619     1889    (3736-3822)      1309   944
  fuse1_36x32           1528     1378    (2323-2447)       764   689
  fuse4x2_64x32         4502     3621    (5887-6151)      2251  1810
  fuse4x4_64x32_b3      4507     4309    (5917-6073)      2253  2154
  fuse4x4_64x32_b4      4683     4838    (6066-6212)      2341  2419
  fuse_short_50x13      1503     1504    (2133-3076)       751   752
  fuse_tall_16x300       788     1230    (1887-2044)       394   615
  descs_mem_32x16       1664     1899    (2117-2378)       832   949
  B ring 1 / ring 2     1117 / 1116   1067 / 1345         558   533     (25 restarted combines each, 5 of them firsts)
  D ring 1 / ring 3     1198 / 1182   1077 / 1485         591   538     (5 each, 1 first)
  F ring 1 / ring 3     1201 / 1227   1075 / 1489         600   537     (8 each, 2 firsts)

THE NAN THIS FOUND.  With the reference's merge applied to a previous row of count 0 -- what k_fuse_stats did before this file -- the
same script leaves NaN rows from the second restarted combine on (32 x 16, ring of 1: 553 of 1893 rows at combine 11, and they spread
to voxels the ring holds: 499 NaN rows against 462 of count 0 at combine 12).  test_a_count_0_row_merged_as_the_reference_would_is_nan
keeps that arithmetic on record.

NO OVERLAP (case E).  Behind a jump of three window widths the restarted mirror and the always-on oracle are bitwise equal from the
first merged combine on, on rings of 1 and 3.

Wall time here: the file 6 s, no case above 0.8 s."""
import contextlib
import io

import numpy as np
import pytest

import stats_demand_ref as sd
from oracle import oracle

# name -> (floor for "stale", floor for "no_prev"): half of the least count measured (module docstring), rounded down
FLOORS = {
    "encfuse_64x32": (2279, 1195), "encfuse_48x20": (1309, 944), "fuse1_36x32": (764, 689), "fuse4x2_64x32": (2251, 1810),
    "fuse4x4_64x32_b3": (2253, 2154), "fuse4x4_64x32_b4": (2341, 2419), "fuse_short_50x13": (751, 752), "fuse_tall_16x300": (394, 615),
    "descs_mem_32x16": (832, 949), "B": (558, 533), "D": (591, 538), "F": (600, 537),
}
B_RINGS, CDEF_RINGS = (1, 2), (1, 3)                          # as tests/test_stats_on_demand.py
C_SCANS = 16


def _quiet(fn, *a):
    with contextlib.redirect_stdout(io.StringIO()):           # (the reference's warnings of rejected scans)
        return fn(*a)


def _census(params, scans, script, what, floors, *extra):
    """runs `script` on the mirror with a plain oracle and both wrong mirrors following; holds the maps after every combine and the
    floors at every restarted combine; returns (run, what the script returned, least counts)"""
    plain = oracle.OracleGvom(*params)
    fol = {"plain": plain, "stale": sd.DemandOracle(*params, wrong="stale"), "no_prev": sd.DemandOracle(*params, wrong="no_prev")}
    run = sd.Run(params, followers=fol, what=what)
    seen = {"stale": [], "no_prev": [], "firsts": 0}

    def hook(r):
        w = r.w
        for name in ("combined_hit_count", "combined_total_count", "combined_min_height", "combined_index_map", "combined_origin"):
            assert np.array_equal(getattr(w, name), getattr(plain, name)), (r.tag(), name)
        assert w.combined_cell_count_cpu == plain.combined_cell_count_cpu
        _, _, merged, restarted, prev_had = r.last
        assert (w.combined_metrics is not None) == merged == (w.voxels_eigenvalues is not None) and w.last_combined_metrics is w.combined_metrics
        if not restarted:
            return
        assert not np.isnan(w.combined_metrics).any() and not np.isnan(w.voxels_eigenvalues).any(), r.tag()
        stale = sd.rows_differing(fol["stale"].combined_metrics, w.combined_metrics)
        no_prev = sd.rows_differing(fol["no_prev"].combined_metrics, w.combined_metrics)
        assert stale >= floors[0], (r.tag(), stale)
        seen["stale"].append(stale)
        if prev_had:
            assert no_prev >= floors[1], (r.tag(), no_prev)
            seen["no_prev"].append(no_prev)
        else:                                                  # equal by construction: nothing to merge from the previous map
            assert np.array_equal(fol["no_prev"].combined_metrics, w.combined_metrics), r.tag()
            seen["firsts"] += 1
    run.on_combine = hook
    out = _quiet(script, run, scans, *extra)
    print(what, "restarted combines %d (%d firsts); least rows differing: stale %d, no_prev %d" % (
        len(seen["stale"]), seen["firsts"], min(seen["stale"]), min(seen["no_prev"])))
    return run, out, seen


@pytest.mark.parametrize("name", sd.ROUTE_SCENES)
def test_script_a_on_every_route_scene_can_tell_the_wrong_mirrors(name):
    params, scans, _ = sd.route_scene(name)
    bs = params[4]
    run, pattern, seen = _census(params, scans, sd.script_a, name, FLOORS[name])
    assert pattern == sd.a_pattern(bs)
    assert len(seen["stale"]) == 5 and seen["firsts"] == 1 and len(seen["no_prev"]) == 4
    # the fourth unread combine (number 6) is the first without statistics; number 9 + bs the first with them again
    merged = [t[2] for t in run.trail if t[0] == "combine"]
    assert merged == [True] * 6 + [False] * (3 + bs) + [True] * 5 and run.pauses == 1


@pytest.mark.parametrize("bs", [1, 2, 3, 4])
def test_the_pattern_of_data_and_no_data_per_ring_length(bs):
    params, scans = sd.small_scene(bs, sd.a_length(bs))
    run = sd.Run(params)
    assert _quiet(sd.script_a, run, scans) == sd.a_pattern(bs)
    reads = {t[1]: t for t in run.trail if t[0] == "read"}
    assert sorted(reads) == [0, 1, 2] + list(range(9, 9 + bs + 5))
    assert all(reads[k][2] for k in (0, 1, 2)) and not reads[9][2] and not any(reads[9][3])
    for k in range(10, 9 + bs + 5):
        # slot of scan j is j % bs; it has metrics iff scan j came after the demand (the read behind combine 9) and is still in the ring
        want = [False] * bs
        for j in range(max(0, k - bs + 1), k + 1):
            want[j % bs] = j >= 10
        assert list(reads[k][3]) == want, (k, reads[k])
        assert reads[k][2] == all(want) == (k >= 9 + bs)


@pytest.mark.parametrize("bs", CDEF_RINGS)
def test_a_mirror_that_never_pauses_is_the_always_on_oracle(bs):
    params, scans = sd.small_scene(bs, 8, 8)
    always = oracle.OracleGvom(*params, voxel_statistics=True)
    run = sd.Run(params, followers={"always": always})
    for s in scans:
        run.scan(*s)
        assert run.combine(read="full") is True
        w = run.w
        for i in range(bs):
            assert (w.metrics_buffer[i] is None) == (always.metrics_buffer[i] is None)
            if w.metrics_buffer[i] is not None:
                assert np.array_equal(w.metrics_buffer[i], always.metrics_buffer[i])
        assert np.array_equal(w.combined_metrics, always.combined_metrics) and np.array_equal(w.voxels_eigenvalues, always.voxels_eigenvalues)
        assert np.array_equal(w.make_debug_voxel_map(), always.make_debug_voxel_map())
    assert run.pauses == 0


@pytest.mark.parametrize("bs", CDEF_RINGS)
@pytest.mark.parametrize("period", [1, 2, 3, 4, 5])
def test_reader_periods(period, bs):
    """periods up to 3 never pause (the GPU file then holds every read to the always-on oracle: equal to the mirror, above); at 4 and 5
    no read ever returns data -- the present rule (`++stats_idle > 3`, no hysteresis: ADVICE.md's first finding)"""
    params, scans = sd.small_scene(bs, C_SCANS, 8)
    always = oracle.OracleGvom(*params, voxel_statistics=True)
    run = sd.Run(params, followers={"always": always})
    pattern = _quiet(sd.script_c, run, scans, period)
    assert len(pattern) == C_SCANS // period
    if period <= sd.IDLE_THRESHOLD:
        assert all(pattern) and run.pauses == 0
        assert np.array_equal(run.w.combined_metrics, always.combined_metrics)
    else:
        assert not any(pattern) and run.pauses == len(pattern)


@pytest.mark.parametrize("bs", B_RINGS)
def test_script_b_can_tell_the_wrong_mirrors(bs):
    params, scans = sd.small_scene(bs, sd.b_length(bs), 4)
    run, _, seen = _census(params, scans, sd.script_b, "B ring %d" % bs, FLOORS["B"])
    assert run.pauses == len(sd.READS) + 1 and seen["firsts"] == len(sd.READS) and len(seen["stale"]) == 5 * len(sd.READS)


@pytest.mark.parametrize("bs", CDEF_RINGS)
def test_script_d_can_tell_the_wrong_mirrors(bs):
    params, scans = sd.small_scene(bs, sd.d_length(bs), 5)
    run, pattern, seen = _census(params, scans, sd.script_d, "D ring %d" % bs, FLOORS["D"])
    assert pattern == sd.d_pattern(bs) and run.pauses == 1 and seen["firsts"] == 1 and len(seen["stale"]) == 5
    # the two combines without a scan count like any other: the one during the pause finds the statistics off, the one behind the
    # demand is the first unread ... read one
    assert [t[1] for t in run.trail if t[0] == "combine"] == list(range(d_combines(bs)))


def d_combines(bs):
    return sd.d_length(bs) + 2


@pytest.mark.parametrize("bs", CDEF_RINGS)
def test_script_f_can_tell_the_wrong_mirrors_behind_both_pauses(bs):
    params, scans = sd.small_scene(bs, sd.f_length(bs), 7)
    run, pattern, seen = _census(params, scans, sd.script_f, "F ring %d" % bs, FLOORS["F"])
    assert pattern == sd.f_pattern(bs) and run.pauses == 2 and seen["firsts"] == 2 and len(seen["stale"]) == 8


@pytest.mark.parametrize("bs", CDEF_RINGS)
def test_the_restart_behind_a_jump_equals_the_always_on_oracle(bs):
    params, scans = sd.small_scene(bs, sd.e_length(bs), 6)
    always = oracle.OracleGvom(*params, voxel_statistics=True)
    run = sd.Run(params, followers={"always": always, "plain": oracle.OracleGvom(*params)})
    checked = []

    def hook(r):
        if r.last[3]:
            w = r.w
            assert np.array_equal(w.combined_metrics, always.combined_metrics) and np.array_equal(w.voxels_eigenvalues, always.voxels_eigenvalues), r.tag()
            assert np.array_equal(w.make_debug_voxel_map(), always.make_debug_voxel_map())
            assert not (w.combined_metrics[:, 9] == 0).any()      # nothing of the map fused without statistics is left
            checked.append(r.k)
    run.on_combine = hook
    assert _quiet(sd.script_e, run, scans, always) == sd.e_pattern(bs)
    assert checked == list(range(9 + bs, sd.e_length(bs)))


def test_a_count_0_row_merged_as_the_reference_would_is_nan():
    """the arithmetic behind the rule "a previous row of count 0 contributes no statistics": gvom.py:858-909 on two rows of count 0
    divides 0 by 0, and a NaN mean then survives every later merge (NaN * 0 is NaN)"""
    L = oracle.lib()
    xy, zs = 2, 1
    index = np.array([0, -1, -1, -1], np.int32)
    origin = np.zeros(3)
    hit, total, minh = np.ones(1, np.int32), np.ones(1, np.int32), np.ones(1, np.float32)
    fused = np.zeros((1, 10), np.float32)
    prev = np.zeros((1, 10), np.float32)                       # a voxel known only from a map fused without statistics
    args = [sd._p(a) for a in (hit, total, minh, index, origin)]
    L.orc_combine_metrics_full_f32(sd._p(fused), *args, sd._p(prev), *args, xy, zs)
    assert np.isnan(fused[0, :9]).all() and fused[0, 9] == 0
    again = np.zeros((1, 10), np.float32)
    slot = np.array([[0.5, 0.5, 0.5, 0.01, 0, 0, 0.01, 0, 0.01, 3]], np.float64)
    L.orc_combine_metrics_full_f64(sd._p(again), *args, sd._p(slot), *args, xy, zs)
    assert not np.isnan(again).any() and again[0, 9] == 3
    L.orc_combine_metrics_full_f32(sd._p(again), *args, sd._p(fused), *args, xy, zs)
    assert np.isnan(again[0, :9]).all() and again[0, 9] == 3    # the voxel is hit later: still NaN


def test_the_threshold_is_one_named_constant():
    """the code's `++stats_idle > 3` in fuse_impl and the mirror's IDLE_THRESHOLD say the same"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "g-vom_amd", "csrc", "gvom_combine.hip")).read()
    m = re.findall(r"\+\+h->stats_idle > (\d+)", src)
    assert m == [str(sd.IDLE_THRESHOLD)], m
