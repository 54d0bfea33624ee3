"""CPU side of tests/test_voxel_atlas_cycle.py: the scripts of tests/query_cycle.py run on tests/voxel_atlas_cycle.py AtlasCycle with the
oracle mirror and the numpy referee of the voxel atlas alone (g=None), and the conditions under which the GPU tests can fail are
asserted.  No GPU.

THE WRONG MAP.  At every point of a script the referee also merges, into a copy of the atlas as it stood, each map a wrong answer
would come from: the map of the combine before (a stale buffer, a stale origin) and, behind a scan that has not been combined, the map
a combine at that moment would give (Cycle.speculated: the spare buffer of a one-slot ring).  Merging it must report different counts
and leave at least CHANGED_VOXELS_FLOOR = 1000 world voxels in another class than merging the right one.  Measured on run_script, the
least per case: np2 ring 1 following 1549, p2 ring 3 following 8758, np2 ring 2 fixed 1257 ("H pending": the speculation), p2 ring 1
fixed 1573, np2 ring 4 following 1972.  Two exceptions by construction: at E (a combine without a scan) the map before has the same
classes and the same window, so both merges are equal in every count and voxel; at K on a fixed atlas the window lies wholly outside
the extent, the right merge changes nothing, and re-merging J's map changes nothing either -- only the counts differ.
The epoch script: 1262 to 11626, and 888 at "after scan 5" on the one-slot ring for the map of combine 3.  That one is below the floor
and no buffer holds it: of the two fused buffers one holds combine 4's map and the other, since scan 5, the speculation (8431 voxels).
There the counts must still differ; the floor is asserted for every map that some buffer holds.
The thread's ten maps (following, merged in step order): merging a neighbouring step's map instead leaves 2089 to 18408 voxels in
another class.

FOLLOWING 64 x 64 x 32.  cleared > 0 at D, F, G, J and K; cleared_observed > 0 at two or more points before K (np2: 582 at F on rings
of 1 slot, 1425 on a ring of 4; p2: 734 to 19,708); at K the whole extent is cleared (64 * 64 * 32) with cleared_observed of at
least 30,000 (36,344 np2 ring 1, 39,238 np2 ring 4, 71,939 p2).
FIXED 128 x 128 x 64.  0 < outside < the window's volume at F and J (3840 and 1920 on np2, 17,792 and 8064 on p2); at K outside is the
whole window, the other five merge counts are 0 and seq still advances; every window that meets the extent crosses the storage seams
at world 0 in x and y.

RAYS.  Of the 512 rays of a point, those the window answers LEFT_WINDOW and the atlas otherwise (unknown_blocks=True): they are what
tells an atlas walk from a window walk.  On following 128 x 128 x 64 atlases the mirror shows 29 to 62 before K.  The cases of the
GPU test show fewer: the fixed atlases 22 to 33 (np2, ring 2) and 16 to 43 (p2, ring 1) before K and 128 at K; following 64 x 64 x 32
on np2 22 to 50 and 99 at K (the extent is 8 voxels wider than the window on every side), the epoch script 22 to 24, the thread's maps
15 to 29.  The floor RESCUED_RAYS_FLOOR = 7 is no more than half of the least of these (15).  On p2 a 64 x 64 x 32 extent IS the
window: 0 rays, by construction -- that case is there for the merge with nothing to spare on any side.

The referee's share here: 0.5 to 0.75 s per case of run_script."""
import copy

import numpy as np
import pytest

import query_cycle as qc
import raycast_ref as rr
import voxel_atlas_cycle as vc
import voxel_atlas_ref as va

RESCUED_RAYS_FLOOR = 7                                         # half of the least the mirror shows (15, the thread's maps of steps 6 to 8), rounded down
CASES = [("np2", 1, vc.FOLLOWING), ("p2", 3, vc.FOLLOWING), ("np2", 2, vc.fixed((70, 20, 30))), ("p2", 1, vc.fixed((50, 10, 20))),
         ("np2", 4, vc.FOLLOWING)]
IDS = ["np2-1-following", "p2-3-following", "np2-2-fixed", "p2-1-fixed", "np2-4-following"]
UNCHANGED = ("B", "C", "H pending", "H", "I")


def _wrong_maps(c, equal=(), counts_only=(), unheld=()):
    """every point's wrong maps against the floors of the module docstring; returns the least number of voxels left in another class.
    `equal`: labels where the map before is equal by construction; `counts_only`: where only the counts differ; `unheld`: (label,
    other's label) pairs whose map no buffer holds any more"""
    least = None
    for p in c.trail:
        who = (c.grid, c.bs, p["label"])
        assert sum(p["n"][k] for k in va.COUNT_NAMES[:6]) == np.prod(c.window), who
        for other, counts, changed in p["others"]:
            if p["label"] in equal:
                assert counts == p["n"] and changed == 0, (who, other)
                continue
            assert counts != p["n"], (who, other, counts)
            if p["label"] in counts_only:
                assert changed == 0, (who, other, changed)
            elif (p["label"], other) in unheld:
                assert 0 < changed < vc.CHANGED_VOXELS_FLOOR, (who, other, changed)
            else:
                assert changed >= vc.CHANGED_VOXELS_FLOOR, (who, other, changed)
                least = changed if least is None else min(least, changed)
    return least


def _rescued(c):
    """the rays that only the atlas answers, per point, against the floor; 0 where the extent is the window"""
    same = c.ref.sizes() == c.window
    got = [p["rescued"] for p in c.trail]
    if same:
        assert got == [0] * len(got), got
    else:
        assert min(got) >= RESCUED_RAYS_FLOOR, got
    return got


@pytest.mark.parametrize("grid,bs,kw", CASES, ids=IDS)
def test_the_atlas_script_can_tell_every_merge_from_a_wrong_one(grid, bs, kw):
    c = qc.run_script(vc.AtlasCycle(grid, bs, **kw))
    assert tuple(p["label"] for p in c.trail) == qc.SCRIPT_POINTS and c.ref.seq == len(qc.SCRIPT_POINTS)
    by = {p["label"]: p for p in c.trail}
    assert by["A"]["W"] == c.first == vc.first_window(grid)
    for label in UNCHANGED:                                    # the same map merged again: every observed voxel is confirmed
        n = by[label]["n"]
        assert n["confirmed"] > 0 and n["confirmed"] + n["uninformative"] + n["outside"] == np.prod(c.window), (label, n)
        assert "speculated" in [o[0] for o in by[label]["others"]], label
    follow = kw["follow"]
    least = _wrong_maps(c, equal=("E",), counts_only=() if follow else ("K",))
    volume = int(np.prod(c.window))
    if follow:
        assert all(by[k]["n"]["cleared"] > 0 for k in ("D", "F", "G", "J", "K")), [(k, by[k]["n"]["cleared"]) for k in "DFGJK"]
        seen_leaving = [(p["label"], p["n"]["cleared_observed"]) for p in c.trail if p["label"] != "K" and p["n"]["cleared_observed"] > 0]
        # two or more points before K taken over the following cases: a 64-voxel extent has 8 voxels to spare around an np2 window and
        # the script moves it further once before K (F: 10 in x; 582 or 1425 voxels); around a p2 window it has none (734 to 19,708)
        assert [k for k, _ in seen_leaving] == (["D", "F", "G", "J"] if grid == "p2" else ["F"]), seen_leaving
        assert by["K"]["n"]["cleared"] == 64 * 64 * 32 == c.ref.cls.size and by["K"]["n"]["cleared_observed"] >= 30000, by["K"]["n"]
        assert all(p["n"]["outside"] == 0 for p in c.trail)
        print(grid, bs, "cleared_observed", seen_leaving, "at K", by["K"]["n"]["cleared_observed"])
    else:
        partly = [(p["label"], p["n"]["outside"]) for p in c.trail if 0 < p["n"]["outside"] < volume]
        assert len(partly) >= 2 and [k for k, _ in partly] == ["F", "J"], partly
        n = by["K"]["n"]
        assert n["outside"] == volume and all(n[k] == 0 for k in va.COUNT_NAMES[:5]) and by["K"]["counts"]["seq"] == by["J"]["counts"]["seq"] + 1, n
        assert by["K"]["counts"]["observed"] == by["J"]["counts"]["observed"] > 0
        for p in c.trail:
            if p["n"]["outside"] < volume:                     # storage coordinate = world coordinate & (side - 1): the seam lies at world 0
                assert all(p["W"][k] < 0 < p["W"][k] + c.window[k] for k in (0, 1)), p["W"]
            assert p["E"] == c.ref.E
        print(grid, bs, "outside", partly)
    print(grid, bs, "least voxels a wrong map changes:", least, "rays only the atlas answers:", _rescued(c))


@pytest.mark.parametrize("bs", [1, 3])
def test_the_atlas_epoch_script_can_tell_every_merge_from_a_wrong_one(bs):
    """(the renumbering itself needs the library: the mirror's maps do not depend on the site)"""
    c = vc.AtlasCycle("np2", bs, **vc.FOLLOWING)
    c.P0("P0")
    qc.run_epoch_script(c, "combine")
    assert [p["label"] for p in c.trail] == ["after combine 3", "after scan 4", "after combine 4", "after scan 5", "after combine 5", "the end"]
    # on the one-slot ring the spare buffer holds the speculation of scan 5, not the map of combine 3 any more (888 voxels)
    least = _wrong_maps(c, unheld=(("after scan 5", "combine 3"),) if bs == 1 else ())
    for p in c.trail:
        assert (p["n"]["cleared"] > 0) == ("combine" in p["label"] or p["label"] == "the end"), p
    print("np2", bs, "epoch script: least voxels a wrong map changes:", least, "rays only the atlas answers:", _rescued(c))


@pytest.mark.parametrize("bs", [3, 4])
def test_the_first_call_behind_an_asynchronous_combine_can_tell_its_map_from_the_one_before(bs):
    c = vc.run_async_first_script(vc.AtlasCycle("np2", bs, **vc.FOLLOWING))
    assert [p["label"] for p in c.trail] == ["first", "second, pending", "second"] and c.trail[1]["n"]["cleared"] > 0
    assert [o[0] for o in c.trail[1]["others"]] == ["first"] and not c.trail[0]["others"]
    print("np2", bs, "asynchronous combine: least voxels the map before changes:", _wrong_maps(c), "rays only the atlas answers:", _rescued(c))


@pytest.mark.parametrize("bs", [1, 3])
def test_the_integrating_thread_can_tell_the_ten_maps_apart(bs):
    """the ten maps of query_cycle.thread_mirror merged in step order into a following 64 x 64 x 32 atlas: at every step, merging a
    neighbouring step's map instead -- the one before: a stale buffer; the one after: the spare buffer -- reports other counts and
    leaves at least 1000 voxels in another class (measured: 2089 to 18408); and the replay of tests/voxel_atlas_cycle.py holds its own
    referee's answers"""
    grid = "np2"
    maps, A, B = qc.thread_mirror(grid, bs)
    xr, zr, xy, zs = rr.GRIDS[grid]
    origins = [tuple(int(v) for v in m.W) for m in maps]
    assert len(set(origins)) == len(maps) == qc.THREAD_STEPS
    ref = va.VoxelAtlasRef(64, 32, xy, zs)
    least, rescued, kept = None, [], []
    for k, m in enumerate(maps):
        before = copy.deepcopy(ref)
        n = ref.integrate(m.state, origins[k])
        assert n["cleared"] > 0, (k, n)
        for j in (k - 1, k + 1):
            if 0 <= j < len(maps):
                wrong = copy.deepcopy(before)
                assert wrong.integrate(maps[j].state, origins[j]) != n, (k, j)
                changed = vc.world_difference(ref, wrong)
                assert changed >= vc.CHANGED_VOXELS_FLOOR, (k, j, changed)
                least = changed if least is None else min(least, changed)
        walked = va.atlas_walk(ref, (xr, xr, zr), A, B, unknown_blocks=True)
        rescued.append(vc.rays_rescued(rr.walk(m.state, m.W, grid, A, B, unknown_blocks=True)[0], walked[0]))
        if k in (0, 1, 2, 3, 9):                               # what a thread that saw these steps would have recorded ...
            kept.append((origins[k],) + ref.box() + (ref.E,) + walked)
    assert min(rescued) >= RESCUED_RAYS_FLOOR, rescued
    print(grid, bs, "least voxels a neighbouring map changes:", least, "rays only the atlas answers:", rescued)
    # ... is NOT what the replay of that subsequence gives: the recorded atlas had the steps in between merged too
    assert vc.replay(kept[:4], maps, grid, A, B) == [0, 1, 2, 3]
    with pytest.raises(AssertionError, match="integrate 4"):
        vc.replay(kept, maps, grid, A, B)
