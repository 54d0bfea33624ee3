"""CPU side of tests/test_query_cycle.py: the scripts of tests/query_cycle.py run on the oracle alone, and the conditions under which
the GPU tests can fail are asserted.  No GPU.

At every point of a script the current map is compared with the maps a wrong answer would come from: the map of the combine before
(a stale buffer, a stale origin) and, where a scan has been accepted and not combined yet, the map a combine at that moment would
give (the spare buffer of a one-slot ring).  The bundle's own inputs for the current map are answered by the referees on the other
map, and must come out different:
  * at least 256 of the 512 rays change their answer, under unknown_blocks=True and under the default flags.  Measured: 345 to 463
    (np2 and p2, ring sizes 1 to 4; the least per case 347, 395, 425, 345, 364; the epoch script 397 and 432);
  * the viewpoint gains of at least 2 of the 3 finite poses and the alignment counts of at least 16 of the 20 candidates differ
    (measured: 3 of 3 but for one pair of the epoch script, where two gains happen to be 264; 17 of 20 -- the other three are the
    specials that put every return outside);
  * every ray status occurs in at least 12 of the 512 rays under unknown_blocks=True.  Measured minimum: 12, the invalid family
    (96 / 8); the next lowest is 15 (UNKNOWN at J, np2, ring of 4).
E is the exception, and is held for exactness only: a combine without a scan changes counts and no voxel's class, so 0 of 512 rays
change, the origin is the same, and no query of the bundle can tell E's map from D's.  test_a_combine_without_a_scan_changes_no_class
shows the same for a second and a third such combine: that is why F has a scan of its own in the script.
The referee of the 512 rays takes about 0.03 s per call here, the bundle's referees together 0.06 to 0.09 s per map."""
import numpy as np
import pytest

import costfield_ref as cf
import query_cycle as qc
import raycast_ref as rr

CASES = [("np2", 1), ("np2", 2), ("np2", 4), ("p2", 1), ("p2", 3)]          # (grid, ring slots) of the GPU test


def _census(points, what):
    """asserts the conditions of the module docstring at every point; returns the smallest ray change and status count seen"""
    least_change, least_status = 512, 512
    for label, cur, others in points:
        w = cur.want
        per_status = np.bincount(w["rays", True][0][:, 0], minlength=5)
        assert per_status.min() >= qc.STATUS_FLOOR, (what, label, per_status)
        least_status = min(least_status, int(per_status.min()))
        assert (w["viewpoints"][0][:, 0] == rr.INVALID).sum() == 1 and w["viewpoints"][0][2, 0] == rr.INVALID, (what, label)
        if label == "A":
            assert not others                                  # the first map: there is no other a query could answer for ...
            continue
        assert others, (what, label)
        if label == "E":                                       # held for exactness only: see the module docstring
            (d,) = others
            a = qc.answers(cur.inputs, d)
            assert np.array_equal(cur.W, d.W) and np.array_equal(rr.state_class(cur.state), rr.state_class(d.state)), what
            assert qc.rays_changed(w["rays", True], a["rays", True]) == 0 and qc.rays_changed(w["rays", False], a["rays", False]) == 0, what
            assert not np.array_equal(cur.dense[2], d.dense[2])            # ... while the counts moved on
            continue
        for other in others:
            a = qc.answers(cur.inputs, other)
            who = (what, label, other.label)
            assert not np.array_equal(cur.W, other.W), who
            for ub in (True, False):
                changed = qc.rays_changed(w["rays", ub], a["rays", ub])
                assert changed >= qc.CHANGED_FLOOR, (who, ub, changed)
                least_change = min(least_change, changed)
            finite = w["viewpoints"][0][:, 0] != rr.INVALID
            assert (w["viewpoints"][0][finite, 1] != a["viewpoints"][0][finite, 1]).sum() >= 2, (who, w["viewpoints"][0], a["viewpoints"][0])
            assert (w["alignments"][0] != a["alignments"][0]).any(axis=1).sum() >= 16, who
            assert (w["occupancy"] != a["occupancy"]).sum() >= 1024, who
    return least_change, least_status


@pytest.mark.parametrize("grid,bs", CASES)
def test_the_script_can_tell_every_point_from_its_neighbours(grid, bs):
    c = qc.run_script(qc.Cycle(grid, bs))
    assert tuple(label for label, _, _ in c.points) == qc.SCRIPT_POINTS
    # B, C, H and I come behind a scan that has not been combined: the speculated map is among the others
    for label, cur, others in c.points:
        assert ("speculated" in [m.label for m in others]) == (label in ("B", "C", "H pending", "H", "I")), label
    by_label = {label: cur for label, cur, _ in c.points}
    assert by_label["B"] is by_label["A"] and by_label["C"] is by_label["A"]
    assert by_label["H pending"] is by_label["G"] and by_label["H"] is by_label["G"] and by_label["I"] is by_label["G"]
    origins = [tuple(by_label[k].W.tolist()) for k in ("A", "D", "F", "G", "J", "K")]
    assert len(set(origins)) == 6, origins
    xr, zr, xy, zs = rr.GRIDS[grid]
    assert (np.abs(by_label["K"].W - by_label["J"].W)[:2] >= 9 * xy).all()        # K: nothing of the previous map is inside
    print(grid, bs, "least change, least status:", _census(c.points, "%s, ring of %d" % (grid, bs)))
    # L: the field on the cost map of F's own maps has a goal on a free cell near the ego (measured: at most 4 cells away), and
    # free and blocked cells to cross and to go round
    f = by_label["F"]
    cost = cf.travcost(f.maps2d[1], f.maps2d[2], f.maps2d[4], f.maps2d[3], None, {})
    cells = qc.goal_cells(cost, f.ego, xr, f.maps2d[0])
    assert cost[cells[1, 0], cells[1, 1]] > 0 and np.abs(cells[1] - cells[0]).max() <= 8, (grid, bs, cells)
    assert (cost > 0).sum() >= 256 and (cost == 0).sum() >= 16, (grid, bs)


@pytest.mark.parametrize("bs", [1, 3])
def test_the_epoch_script_can_tell_every_point_from_its_neighbours(bs):
    """(the renumbering itself needs the library: the mirror's maps do not depend on the site)"""
    c = qc.run_epoch_script(qc.Cycle("np2", bs), "combine")
    assert [label for label, _, _ in c.points] == ["after combine 3", "after scan 4", "after combine 4", "after scan 5", "after combine 5", "the end"]
    print("np2", bs, "least change, least status:", _census(c.points, "epoch script, ring of %d" % bs))
    assert sorted(qc.EPOCHS_LEFT) == [(1, "combine"), (1, "scan"), (3, "combine"), (3, "scan")]
    # the arithmetic of query_cycle.EPOCHS_LEFT: (epochs a scan takes, epochs a combine takes) per ring size; the call that finds the
    # counter at or beyond the limit renumbers
    for (ring, site), left in qc.EPOCHS_LEFT.items():
        scan_takes, combine_takes = (2, 0) if ring == 1 else (1, 1)
        counter, hit = -left, None
        for k in range(4, qc.EPOCH_STEPS):
            for call, takes in (("scan", scan_takes), ("combine", combine_takes)):
                if counter >= 0 and hit is None:
                    hit = (call, k)
                counter += takes
        assert hit is not None and hit[0] == site and hit[1] in (4, 5), (ring, site, hit)


@pytest.mark.parametrize("bs", [1, 3])
def test_the_query_thread_can_tell_the_ten_maps_apart(bs):
    maps, A, B = qc.thread_mirror("np2", bs)
    assert len(maps) == qc.THREAD_STEPS and len(B) == 512
    origins = [tuple(m.W.tolist()) for m in maps]
    assert len(set(origins)) == len(maps), origins             # pairwise distinct: an answer's origin names its map
    want = [rr.walk(m.state, m.W, "np2", A, B, unknown_blocks=True) for m in maps]
    changes = [qc.rays_changed(want[k], want[k + 1]) for k in range(len(maps) - 1)]
    print("np2", bs, "rays that change from step to step:", changes)
    assert min(changes) >= qc.CHANGED_FLOOR, changes           # (measured: 411 to 450) an answer for a neighbouring step under the right origin would show


def test_a_combine_without_a_scan_changes_no_class():
    """three combines in a row behind one scan: the window, and the class of every voxel, stay; hit and total counts grow.  No ray,
    viewpoint, alignment or occupancy query can tell these maps apart -- a point of the script that is to tell its map from the one
    before needs a scan of its own."""
    c = qc.Cycle("np2", 1)
    c.scan(0)
    c.scan(1)
    maps = []
    for k in range(3):
        c.combine("sync", "combine %d" % k)
        maps.append(c.cur)
    for a, b in zip(maps, maps[1:]):
        assert np.array_equal(a.W, b.W) and np.array_equal(rr.state_class(a.state), rr.state_class(b.state))
        assert not np.array_equal(a.dense[2], b.dense[2])
        w = qc.answers(a.inputs, b)
        assert qc.rays_changed(a.want["rays", True], w["rays", True]) == 0
        assert np.array_equal(a.want["viewpoints"][0], w["viewpoints"][0]) and np.array_equal(a.want["alignments"][0], w["alignments"][0])
