"""CPU side of tests/test_voxel_changes_cycle.py: the scripts of tests/query_cycle.py run on tests/voxel_changes_cycle.py ChangesCycle with the
oracle mirror and the numpy referees of the voxel atlas and of its change query alone (g=None), and the conditions under which the GPU
tests can fail are asserted.  No GPU.

THE WRONG MAP.  At every point the referee also answers, against the same atlas, for each map a wrong answer could come from: the map of
the combine before (a stale buffer, a stale origin) and, behind a scan that has not been combined, the map a combine at that moment would
give (Cycle.speculated: the spare buffer of a one-slot ring).  That product must differ from the right one in origin_voxels and in words
4 .. 6 of part 3 {appeared, vanished, outside}.  E is the one exemption: a combine without a scan gives a map with the classes and the
origin of D's.

EVERY POINT (merged at all twelve points; the five cases of the GPU test).  At D, F, G and J the right answer has at least 100 coded
voxels and at least one kept cluster: the least is 158 at F on np2 ring 1 (157 appeared, 1 vanished), the most 4464 at G on np2 ring 2.  At B, C,
"H pending", H and I it is all zeros while the speculation has 205 (C, np2 ring 1) to 1355 coded voxels at B and C and 567 to 1282 at
the three points around H; there the map before (F's) has 1573 to 2729.  At K the window lies wholly outside the memory (46,080 /
131,072 outside) while J's map has 0 to 8064 outside.  The second call (min_cells 1, cap 3) keeps 7 to 101 clusters at D, F, G and J:
every one of them is cut off at 3.  The first call drops 1 to 46 clusters below min_cells 2 at each of them.
LAGGING (merged at A, D, F and K).  At G, "H pending", H and I the right answer is one product -- G's map against the memory of F -- with
1942 (p2 ring 1) to 4833 coded voxels; the speculation's totals differ (np2 ring 1: 2161 / 234 against 2431 / 451), F's map itself gives 0.
J answers against the memory of F too (seq 3) and differs from G's answer.
THE EPOCH SCRIPT.  "after combine 4", "after combine 5" and "the end" have 813 to 3157 coded voxels, "after scan 4" and "after scan 5"
none.  A read under the stale epoch takes every tile for unknown: a map without an observed voxel has no code.
THE THREAD (a following 128 x 128 x 64 atlas that holds the map of step 0 alone).  The ten products differ pairwise in words 4 .. 6, the
ten origins too; steps 1 .. 9 have 1179 to 2196 coded voxels.

The referees' share here: 0.4 to 1.0 s per case of run_script."""
import itertools

import numpy as np
import pytest

import query_cycle as qc
import voxel_atlas_cycle as vac
import voxel_changes_cycle as vcc
import voxel_changes_ref as vcr

EVERY_CASES = [("np2", 1, vac.FOLLOWING), ("np2", 2, vac.fixed((70, 20, 30))), ("np2", 4, vac.FOLLOWING), ("p2", 1, vac.fixed((50, 10, 20))),
               ("p2", 3, vac.FOLLOWING)]
EVERY_IDS = ["np2-1-following", "np2-2-fixed", "np2-4-following", "p2-1-fixed", "p2-3-following"]
LAGGING_CASES = [("np2", 1, vac.FOLLOWING), ("np2", 3, vac.fixed((70, 20, 30))), ("p2", 1, vac.fixed((50, 10, 20)))]
LAGGING_IDS = ["np2-1-following", "np2-3-fixed", "p2-1-fixed"]
UNCHANGED = ("B", "C", "H pending", "H", "I")
CODED_FLOOR = 100                                              # every point: D, F, G, J (and what the speculation would give at the unchanged points)
LAGGING_FLOOR = 1000                                           # lagging: G, "H pending", H, I; the thread's steps 1 .. 9
EPOCH_FLOOR = 500


def _wrong_maps(c, equal=("E",)):
    """every point's wrong maps give another origin and other totals than the right one; returns how many were compared"""
    n = 0
    for p in c.trail:
        who = (c.grid, c.bs, p["label"])
        for other, W, totals in p["others"]:
            if p["label"] in equal:
                assert W == p["W"] and totals == p["part3"][4:7], (who, other)
                continue
            assert W != p["W"], (who, other, W)
            assert totals != p["part3"][4:7], (who, other, totals)
            n += 1
    return n


def _truncated(c):
    """points whose second call keeps more clusters than its cap"""
    return [(p["label"], p["kept_second"]) for p in c.trail if p["kept_second"] > vcc.SECOND_CAP]


@pytest.mark.parametrize("grid,bs,kw", EVERY_CASES, ids=EVERY_IDS)
def test_the_every_point_schedule_can_tell_every_answer_from_a_wrong_one(grid, bs, kw):
    c = qc.run_script(vcc.ChangesCycle(grid, bs, **kw))
    assert tuple(p["label"] for p in c.trail) == qc.SCRIPT_POINTS and c.ref.seq == len(qc.SCRIPT_POINTS)
    assert all(p["merged"] and p["part3"][7] == k for k, p in enumerate(c.trail))
    by = {p["label"]: p for p in c.trail}
    for label in ("D", "F", "G", "J"):
        assert by[label]["coded"] >= CODED_FLOOR and by[label]["kept"] >= 1, (label, by[label])
    for label in UNCHANGED:                                    # the same map against a memory that holds it: nothing, and the speculation is not nothing
        p = by[label]
        assert p["part3"][:3] == [0, 0, 0] and p["part3"][4:7] == [0, 0, 0] and p["kept_second"] == 0, p
        spare = [t for name, _, t in p["others"] if name == "speculated"]
        assert len(spare) == 1 and spare[0][0] + spare[0][1] >= CODED_FLOOR, p
    volume = int(np.prod(c.window))
    assert by["K"]["part3"][4:7] == [0, 0, volume] and by["K"]["whole_side"] == kw["follow"], by["K"]
    assert _truncated(c) and any(p["dropped"] >= 1 for p in c.trail), c.trail
    compared = _wrong_maps(c)
    assert compared == 13, compared                            # B, C, D, F, G, J, K one each; "H pending", H and I two each (F's map and the speculation)
    print(grid, bs, "coded", [(p["label"], p["coded"]) for p in c.trail if p["coded"]], "kept by the second call", _truncated(c),
          "dropped", [(p["label"], p["dropped"]) for p in c.trail if p["dropped"]])


@pytest.mark.parametrize("grid,bs,kw", LAGGING_CASES, ids=LAGGING_IDS)
def test_the_lagging_schedule_asks_one_non_zero_answer_four_times(grid, bs, kw):
    c = qc.run_script(vcc.ChangesCycle(grid, bs, integrate_at=vcc.LAGGING, **kw))
    assert tuple(p["label"] for p in c.trail) == qc.SCRIPT_POINTS and c.ref.seq == len(vcc.LAGGING)
    assert tuple(p["label"] for p in c.trail if p["merged"]) == vcc.LAGGING
    by = {p["label"]: p for p in c.trail}
    g = by["G"]
    assert g["coded"] >= LAGGING_FLOOR and g["kept"] >= 1 and g["part3"][7] == 3, g
    for label in ("H pending", "H", "I"):
        p = by[label]
        assert p["part3"] == g["part3"] and p["W"] == g["W"] and (p["kept"], p["dropped"]) == (g["kept"], g["dropped"]), (label, p, g)
        assert [name for name, _, _ in p["others"]] == ["F", "speculated"], p
    assert by["J"]["part3"][7] == 3 and by["J"]["part3"][4:7] != g["part3"][4:7] and by["J"]["coded"] >= LAGGING_FLOOR, by["J"]
    for label in ("B", "C"):
        assert by[label]["coded"] == 0 and by[label]["part3"][7] == 1, by[label]
    assert _truncated(c) and any(p["dropped"] >= 1 for p in c.trail), c.trail
    assert _wrong_maps(c) == 13
    print(grid, bs, "G .. I", g["part3"], "the speculation", by["H"]["others"][1][2], "J", by["J"]["part3"], "kept by the second call", _truncated(c))


@pytest.mark.parametrize("bs", [1, 3])
def test_the_epoch_script_has_codes_behind_every_combine_and_none_behind_a_scan(bs):
    """(the renumbering itself needs the library: the mirror's maps do not depend on the site)"""
    c = vcc.ChangesCycle("np2", bs, **vac.FOLLOWING)
    c.P0("P0")
    qc.run_epoch_script(c, "combine")
    assert [p["label"] for p in c.trail] == ["after combine 3", "after scan 4", "after combine 4", "after scan 5", "after combine 5", "the end"]
    by = {p["label"]: p for p in c.trail}
    for label in ("after combine 4", "after combine 5", "the end"):
        assert by[label]["coded"] >= EPOCH_FLOOR and by[label]["kept"] >= 1, by[label]
    for label in ("after scan 4", "after scan 5"):
        assert by[label]["coded"] == 0 and by[label]["part3"][:3] == [0, 0, 0], by[label]
        assert [name for name, _, _ in by[label]["others"]] == ["combine %d" % (int(label[-1]) - 2), "speculated"], by[label]
    # a read under the epoch before finds no tile of the renumbered map current: every voxel unknown, none reported
    stale = np.full_like(c.cur.state, -1)
    parts, info = vcr.product(c.ref, stale, c.origin(), *vcc.FIRST)
    assert vcc.coded(parts) == 0 and info == [0, 0, 0] and not parts[5].any()
    assert _truncated(c) and _wrong_maps(c, equal=()) == 8
    print("np2", bs, "epoch script: coded", [(p["label"], p["coded"]) for p in c.trail], "kept by the second call", _truncated(c))


@pytest.mark.parametrize("bs", [3, 4])
def test_the_first_call_behind_an_asynchronous_combine_can_tell_its_map_from_the_one_before(bs):
    c = vac.run_async_first_script(vcc.ChangesCycle("np2", bs, **vac.FOLLOWING))
    assert [p["label"] for p in c.trail] == ["first", "second, pending", "second"] and c.ref.seq == 3
    pending = c.trail[1]
    assert pending["coded"] >= LAGGING_FLOOR and pending["kept"] >= 1 and pending["merged"], pending
    assert [o[0] for o in pending["others"]] == ["first"] and pending["others"][0][2] == [0, 0, 0] and not c.trail[0]["others"]
    assert c.trail[2]["coded"] == 0 and _wrong_maps(c, equal=()) == 2
    print("np2", bs, "asynchronous combine: the pending point", pending["part3"])


@pytest.mark.parametrize("bs", [1, 3])
def test_the_changes_thread_can_tell_the_ten_maps_apart(bs):
    maps, want = vcc.changes_thread_mirror("np2", bs)
    assert len(maps) == len(want) == qc.THREAD_STEPS
    assert len({tuple(int(v) for v in m.W) for m in maps}) == len(maps)
    totals = [tuple(int(v) for v in parts[3][4:7]) for parts, _ in want]
    for (i, a), (j, b) in itertools.combinations(enumerate(totals), 2):
        assert a != b, (i, j, a)
    assert totals[0] == (0, 0, 0) and want[0][1] == [0, 0, 0]
    for k in range(1, len(maps)):
        assert vcc.coded(want[k][0]) >= LAGGING_FLOOR and want[k][1][0] >= 1 and want[k][0][3][7] == 1, (k, list(want[k][0][3]))
        assert vcr.differing_parts(want[k][0], want[k - 1][0]), k
    print("np2", bs, "the thread's ten products {appeared, vanished, outside}:", totals)
