"""The scenes of tests/map2d_chain_scenes.py reach what tests/test_map2d_chain.py holds k_map2d to: shown on the CPU oracle's
maps alone, at every one of the six combines of both grids.  The counts are printed; each class must be non-empty."""
import numpy as np
import pytest

import map2d_chain_scenes as mc

CLASSES = ("ring_1", "ring_8_to_15", "ring_never",                    # the ring search ends at once, late, not within 15 rings
           "edge_x_lo", "edge_x_hi", "edge_y_lo", "edge_y_hi",        # searched cells within 15 cells of each window edge
           "two_rounds", "two_rounds_with_density", "slope_alone",    # the density chain twice over; positive by slope only
           "negative_cells")


@pytest.mark.parametrize("name", sorted(mc.GRIDS))
def test_every_class_at_every_combine(name):
    recs = mc.referee(name)
    assert len(recs) == len(mc.EGO_CELLS) >= 5
    for k, rec in enumerate(recs):
        c = rec["census"]
        print(name, "combine", k, c)
        for cls in CLASSES:
            assert c[cls] > 0, (name, k, cls, c)
        assert rec["density_census"]["longest_window"] > 8, (name, k)


@pytest.mark.parametrize("name", sorted(mc.GRIDS))
def test_runs_change_both_ways_while_the_window_moves(name):
    recs = mc.referee(name)
    # the window: one cell in +x per scan, once three cells back
    ox = [int(round(r["maps"][0][0] / mc.RES)) for r in recs]
    steps = list(np.diff(ox))
    print(name, "window steps in x, cells:", steps)
    assert steps.count(1) >= 4 and min(steps) < -1, steps
    gone, come = mc.run_changes(name)
    print(name, "runs gone back to default:", gone, "runs turned non-default:", come)
    assert len(gone) >= 4 and sum(1 for g in gone if g > 0) >= 4 and sum(1 for c in come if c > 0) >= 4, (gone, come)
    # what the delta form has to store is neither nothing nor everything
    for k in range(1, len(recs)):
        stored = mc.stored_runs(name, k)
        total = 4 * recs[k]["default_runs"][0].size
        print(name, "combine", k, "stored runs", stored, "of", total)
        assert 0 < sum(stored.values()) < total, (name, k, stored)


def test_ring_census_against_hand_made_maps():
    """which ring ends the search follows from the geometry"""
    inf = np.full((40, 40), 0.5)
    # one cell without height in a full map: every direction finds a cell in ring 1
    h = np.zeros((40, 40))
    h[20, 20] = -1000.0
    searched, end = mc.ring_census(h, inf)
    assert searched.sum() == 1 and end[20, 20] == 1
    # heights in the rows y >= 30 and the columns x <= 5 only.  From (20, 20): -x (column 20 - i, dy up to +i) and +y (row 20 + i)
    # reach row 30 at ring 10; -y (row 20 - i, dx from -i) reaches column 5 at ring 15
    h = np.full((40, 40), -1000.0)
    h[:, 30:] = 0.0
    h[:6, :] = 0.0
    searched, end = mc.ring_census(h, inf)
    assert searched[20, 20] and end[20, 20] == 15
    # from (10, 20): -x and -y (dx from -i) reach column 5 at ring 5, +y (dx from -i + 1) at ring 6
    assert end[10, 20] == 6
    # a single height far away: +y never finds it and never leaves the window
    h = np.full((40, 40), -1000.0)
    h[35, 2] = 0.0
    searched, end = mc.ring_census(h, inf)
    assert end[18, 18] == 16 and end[3, 20] == 16
    inf[5, 5] = -1000.0
    assert not mc.ring_census(h, inf)[0][5, 5]
