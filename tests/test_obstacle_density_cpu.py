"""The positive-obstacle density, the part that needs no GPU: the scenes of tests/obstacle_scenes.py REACH the branches that
tests/test_obstacle_density.py holds the kernels to.  Every count below is asserted on the unmodified oracle alone -- a
condition on the inputs, so that a green GPU run proves the branch was taken, not a measurement of the code under test -- and
the census that does the counting is itself pinned: to the reference's known answers and to the oracle's map.

Measured at the last combine (one_round / two_rounds / four_rounds / gate / ragged / tall):
  cells with a >10-hit voxel in the window, no slope override   204 / 427 / 339 / 297 / 446 / 274     floor 100 (tall: 50)
  of them, value strictly between 0 and 100                     201 / 399 / 329 / 285 / 426 / 262     floor 50  (25)
  of them, value 100                                              3 /  28 /  10 /  12 /  20 /  12     floor 3   (2)
  windows with a >10-hit and a 1..10-hit voxel                  164 / 378 / 335 / 281 / 403 / 267     floor 50  (25)
  windows with 1..10-hit voxels only                            463 / 407 / 556 / 538 / 234 /  73     floor 100 (50)"""
import os

import numpy as np
import pytest

import obstacle_scenes as ob
from oracle import oracle

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("name", sorted(ob.GRIDS))
def test_scenes_reach_the_density_branches(name):
    recs = ob.referee(name)
    last = recs[-1]["census"]
    for key, floor in ob.floors(name).items():
        assert last[key] >= floor, (name, key, last[key], floor)
    # the census's own arithmetic is the oracle's map, on every cell of every combine
    for k, rec in enumerate(recs):
        c = rec["census"]
        assert np.array_equal(c["positive"], rec["maps"][1]), "%s combine %d: %s" % (name, k, ob.explain_mismatch(c, c["positive"], rec["maps"][1]))
        assert c["gate_passed"] >= 900 and 0 < c["steep"].sum() < 0.5 * c["gate_passed"]


@pytest.mark.parametrize("name,longer_than", [("one_round", 6), ("two_rounds", 8), ("four_rounds", 24), ("ragged", 8), ("tall", 24),
                                              ("gate", 8)])
def test_window_lengths(name, longer_than):
    """two_rounds / ragged: every window needs a second round of the kernels' eight-level loop and ends inside it (padding
    lanes); four_rounds / tall: a fourth.  one_round: the reference's 7-8 levels, one round, one padding lane at most."""
    for rec in ob.referee(name):
        c = rec["census"]
        assert c["shortest_window"] > longer_than, (name, c["shortest_window"])
        assert c["longest_window"] % 8 != 0 or name == "one_round"       # the last round has padding lanes
    if name == "one_round":
        assert ob.referee(name)[-1]["census"]["longest_window"] <= 8


def test_the_gate_rejects_valid_cells():
    first = ob.referee("gate")[0]["census"]
    assert first["rejected_above"] >= 1000, first["rejected_above"]          # measured: 1,243
    assert first["gate_passed"] >= 1000                                      # ... and passes as many: both sides on one map
    for name in ("one_round", "two_rounds", "four_rounds", "ragged", "tall"):
        assert ob.referee(name)[0]["census"]["rejected_above"] == 0


def test_hit_counts_on_both_sides_of_the_threshold():
    first = ob.referee("one_round")[0]["census"]
    assert first["hits_10"] >= 5 and first["hits_11"] >= 5, (first["hits_10"], first["hits_11"])   # measured: 32 / 40
    for name in ob.GRIDS:
        c = ob.referee(name)[-1]["census"]
        assert c["hits_10"] >= 5 and c["hits_11"] >= 5, name


@pytest.mark.parametrize("name", sorted(ob.GRIDS))
def test_the_window_has_moved_on_every_storage_axis(name):
    recs = ob.referee(name)
    assert np.all(recs[-1]["combined_origin"] != recs[0]["combined_origin"]), (recs[0]["combined_origin"], recs[-1]["combined_origin"])


@pytest.mark.parametrize("name", ["two_rounds", "gate"])
def test_every_rank_of_a_sharded_map_owns_density_cells(name):
    for world in (2, 4):
        for k, rec in enumerate(ob.referee(name)):
            per_rank = ob.cells_per_slab(rec["census"], rec["combined_origin"][1], world)
            assert per_rank.min() >= (20 if k == ob.N_SCANS - 1 else 1), (name, world, k, per_rank)


@pytest.mark.parametrize("name", ["two_rounds", "ragged"])
def test_occupancy_planes_hold_densities_on_both_sides_of_the_threshold(name):
    rec = ob.referee(name)[-1]
    for setting in ob.OCCUPANCY_SETTINGS:
        thr = setting[0]
        assert ob.density_mask(rec["census"], 0, thr).sum() >= 20, (name, thr)        # soft plane, from a density
        assert ob.density_mask(rec["census"], thr, 100).sum() >= 20, (name, thr)      # hard plane, from a density


def test_census_reproduces_the_reference_known_answers():
    """tests/golden/kat_positive_fusion.npz P1-P4b (recorded from the reference) through the census's own arithmetic, no oracle
    call: 0 / 28 / 34 / 100 / 0 at cell (0, 0) and the whole recorded map"""
    rec = np.load(os.path.join(G, "kat_positive_fusion.npz"))
    for name, want in {"P1": 0, "P2": 28, "P3": 34, "P4a": 100, "P4b": 0}.items():
        xy, zs, z_res, pos_thr, robot_h, slope_thr = rec[name + "_scal"]
        c = ob.census_arrays(rec[name + "_index_map"], rec[name + "_height"], rec[name + "_hit"], rec[name + "_total"],
                             float(rec[name + "_origin"][2]), int(xy), int(zs), float(z_res), float(pos_thr), float(robot_h),
                             rec[name + "_sx"], rec[name + "_sy"], float(slope_thr))
        assert c["positive"][0, 0] == want, name
        assert np.array_equal(c["positive"], rec[name + "_out"]), name


def test_a_wrong_map_is_reported_with_its_cell_window_and_counts():
    """the report the GPU test prints: on a map with one density off by one it names the cell, the window and the sums"""
    rec = ob.referee("two_rounds")[-1]
    c, want = rec["census"], rec["maps"][1]
    x, y = np.argwhere(ob.density_mask(c, 0, 99))[0]
    got = want.copy()
    got[x, y] += 1
    text = ob.explain_mismatch(c, got, want)
    z0, z1 = int(c["zmin"][x, y]), int(c["zmax"][x, y])
    big = c["hit3"][z0:z1 + 1, y, x] > 10
    assert "differs from the referee in 1 cells" in text and "cell (%d, %d): window z %d..%d" % (x, y, z0, z1) in text
    assert "summed hit %d / total %d" % (c["hit3"][z0:z1 + 1, y, x][big].sum(), c["total3"][z0:z1 + 1, y, x][big].sum()) in text
    assert "no window" in ob.explain(c, *np.argwhere(~c["gate"])[0])


def test_referee_is_the_plain_oracle():
    """the shared records are an OracleGvom's results, and reading them changed nothing"""
    name = "one_round"
    o = oracle.OracleGvom(*ob.params(name))
    for (pc, ego), rec in zip(ob.scans(name), ob.referee(name)):
        assert pc.dtype == np.float32 and not pc.flags.writeable
        o.process_pointcloud(pc, ego)
        for a, b in zip(o.combine_maps(), rec["maps"]):
            assert np.array_equal(a, b)
