"""The voxel atlas's change query at every point of the scan cycle (tests/voxel_changes_cycle.py has the cycle; tests/voxel_atlas_cycle.py the
atlas on the cycle; tests/query_cycle.py the rule, the mirror and the scripts): VoxelAtlas.changes() held with tolerance 0, all seven
parts, to the numpy referee of tests/voxel_changes_ref.py on the referee atlas of tests/voxel_atlas_ref.py, both fed ONLY from the CPU
oracle's maps -- never from the handle's read_dense(), which is what tests/test_voxel_changes.py feeds its referee with.
gvom_voxel_atlas_changes reads the live fused buffers as gvom_voxel_atlas_integrate does, so it is asked -- as the first call on the
handle -- after a scan that has not been combined, while combine_maps_async() is pending, after a combine that adopted the speculative
fusion of a one-slot ring, after a combine without a scan, after rejected scans, after combine_maps_device() and
combine_maps_occupancy(), on rings of 1 to 4 slots, with the voxel statistics on, after a jump that takes the window out of the extent,
across the tile-epoch renumbering, and from a second thread beside scans and combines.  It is asked twice per point, the second time
with a cap of 3 that cuts the clusters off, and must leave the atlas's counts and default box as they were.  Under two schedules: merged
at every point (the answer at B, C, "H pending", H and I is all zeros, where the spare buffer's speculation has hundreds of codes) and
merged at A, D, F and K only (the answer at G, "H pending", H and I is one product of thousands of codes, asked four times).  Where an
integrate follows, the call's totals equal the integrate's free_to_occupied and occupied_to_free (include/gvom_hip.h "voxel atlas
changes").  tests/test_voxel_changes_cycle_cpu.py holds, on the mirror alone, the conditions under which these tests can fail.

The cases are the smallest shapes at which each path exists: np2 and p2 are the cycle files' grids, 64 x 64 x 32 is the smallest legal
atlas, the fixed 128 x 128 x 64 extents are those of tests/test_voxel_atlas_cycle.py.  Rings of 3 and 4 slots make the asynchronous
combine at G take the second-stream branch.

THAT THESE TESTS CAN FAIL was tried on the MI355X, one run of this file each, with three one-line mutations of
gvom_voxel_atlas_calls.hip (not committed):
  a  current_map() hands out h->fused[h->cur ^ 1] (both fused buffers are allocated at creation for every ring size, so the mutant reads
     inside its allocations): all fourteen cases fail at their FIRST point -- A, "first", "after combine 3", the thread's answer 0 --
     already in origin_voxels, which is the other buffer's ((0, 0, 0) where it was never fused, the window of the combine before on the
     one-slot ring of the epoch script); the script stops there, so B was not reached.  (current_map() is integrate's too.)
  b  gvom_voxel_atlas_changes reads under the epoch before (P.epoch - 1): all fourteen fail at the first point whose answer has a code,
     with every part zero against the referee's -- D in all eight cases of run_script ([28, 186, 21] kept / marked / dropped expected
     on np2 ring 1), "second, pending", "after combine 4", the thread's answer for step 1.  A, B and C pass it: their answer is zeros
     and `outside` comes from the host.
  c  the call's own join_second_stream() taken out: all fourteen PASS, the asynchronous-first cases and G on rings of 3 and 4
     included.  As for integrate (tests/test_voxel_atlas_cycle.py): on np2 and p2 the fusion on the second stream is over before
     k_vchange_planes, behind the call's own memsets, starts.  These tests show that changes() answers for the map of the combine just
     begun with nothing in front of it; they do not show that the join is there.

Wall time on the MI355X (pytest --durations, one run):
the five cases of test_changes_at_every_point_of_the_cycle 0.35 to 0.57 s each (twenty-four changes(), twelve
window bundles, twelve integrates, twenty-five snapshots of counts and box, and the referees), the three of test_changes_against_a_lagging_memory 0.33 to 0.51 s, the two of
test_changes_across_the_epoch_renumbering 0.45 and 0.48 s (two ring sizes each), the two asynchronous-first cases 0.12 s each, the two
thread cases 0.19 and 0.20 s (101 answers, for the maps of steps 0 to 7 and 9); the file 5.9 s (tests/test_voxel_atlas_cycle.py: 4.9 s)."""
import os
import threading

import pytest

import query_cycle as qc
import voxel_atlas_cycle as vac
import voxel_changes_cycle as vcc
import voxel_changes_ref as vcr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST_LIB = os.path.join(ROOT, "g-vom_amd", "lib", "libgvom_hip_test.so")     # the production sources + the hooks of include/gvom_hip_test.h
CASES = [("np2", 1, False, vac.FOLLOWING), ("np2", 2, False, vac.fixed((70, 20, 30))), ("np2", 4, False, vac.FOLLOWING),
         ("p2", 1, True, vac.fixed((50, 10, 20))), ("p2", 3, True, vac.FOLLOWING)]       # tests/test_voxel_atlas_cycle.py CASES
LAGGING_CASES = [("np2", 1, False, vac.FOLLOWING), ("np2", 3, False, vac.fixed((70, 20, 30))), ("p2", 1, True, vac.fixed((50, 10, 20)))]


@pytest.fixture(scope="module")
def gvom():
    import gvom as mod
    rc, info = mod.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    return mod


def _script(c, integrates):
    """run_script on the ChangesCycle c, and what both schedules assert behind it"""
    qc.run_script(c)
    assert tuple(label for label, _, _ in c.points) == qc.SCRIPT_POINTS and c.asked == len(qc.SCRIPT_POINTS)
    g = c.g
    assert c.atlas.seq == c.ref.seq == integrates == c.atlas.counts()["seq"]
    if c.bs == 1:
        # as tests/test_voxel_atlas_cycle.py: the combines at A, D, F, G, J and K find a speculation to adopt; the calls in between
        # neither drop nor adopt one
        print(c.grid, c.bs, "adopted", g.get_tuning("eager_adopted"), "dropped", g.get_tuning("eager_dropped"))
        assert g.get_tuning("eager_adopted") >= 4 and g.get_tuning("eager_dropped") >= 1
    else:
        assert g.get_tuning("eager_adopted") == 0
    c.atlas.release()
    assert g.get_tuning("voxel_atlas") == 0


@pytest.mark.parametrize("grid,bs,stats,kw", CASES, ids=["np2-1-off-following", "np2-2-off-fixed", "np2-4-off-following", "p2-1-on-fixed", "p2-3-on-following"])
def test_changes_at_every_point_of_the_cycle(gvom, grid, bs, stats, kw):
    """the script P0 .. L of tests/query_cycle.py on a ChangesCycle that merges at every point: twenty-four changes(), twelve window
    bundles, twelve integrates"""
    _script(vcc.ChangesCycle(grid, bs, gvom, stats, **kw), len(qc.SCRIPT_POINTS))


@pytest.mark.parametrize("grid,bs,stats,kw", LAGGING_CASES, ids=["np2-1-off-following", "np2-3-off-fixed", "p2-1-on-fixed"])
def test_changes_against_a_lagging_memory(gvom, grid, bs, stats, kw):
    """the same script, merged at A, D, F and K only: G's map against the memory of F, asked at G, "H pending", H and I across a scan,
    the end of the asynchronous combine and two rejected scans; J's against the memory of F as well"""
    _script(vcc.ChangesCycle(grid, bs, gvom, stats, integrate_at=vcc.LAGGING, **kw), len(vcc.LAGGING))


@pytest.mark.parametrize("bs,stats", [(3, False), (4, True)])
def test_changes_is_the_first_call_behind_an_asynchronous_combine(gvom, bs, stats):
    """voxel_atlas_cycle.run_async_first_script: combine_maps_async() begins its fusion on the second stream and changes() is the next
    call on the handle -- no window query in between joins the streams for it.  It must wait for that fusion and answer for the new map,
    before .result(); the integrate behind it counts what it reported"""
    c = vac.run_async_first_script(vcc.ChangesCycle("np2", bs, gvom, stats, **vac.FOLLOWING))
    assert [label for label, _, _ in c.points] == ["first", "second, pending", "second"] and c.atlas.seq == 3
    assert c.g.get_tuning("eager_adopted") == 0


@pytest.mark.parametrize("site", ["combine", "scan"])
def test_changes_across_the_epoch_renumbering(gvom, site):
    """the test library's "epoch_bias" makes the tile-epoch renumbering -- which rewrites the fused map's tags -- happen inside a combine
    or inside a scan (query_cycle.EPOCHS_LEFT); the changes() behind it must read the rewritten tags under the new epoch: under the old
    one it would take every tile for unknown and report nothing where the referee has 813 to 3157 coded voxels"""
    for bs in (1, 3):
        c = vcc.ChangesCycle("np2", bs, gvom, False, _library=TEST_LIB, **vac.FOLLOWING)
        c.P0("P0")
        qc.run_epoch_script(c, site)
        assert len(c.points) == 6 and c.atlas.seq == c.ref.seq == 6 and c.asked == 6
        if bs == 1:                                               # the sign that the counter crossed where EPOCHS_LEFT says (tests/test_query_cycle.py)
            assert c.g.get_tuning("eager_adopted") == (6 if site == "combine" else 7) and c.g.get_tuning("eager_dropped") == 0


@pytest.mark.parametrize("bs", [1, 3])
def test_a_changes_thread_beside_scans_and_combines(gvom, bs):
    """query_cycle.thread_mirror's ten steps of scan and combine_maps() on the main thread, each held to the oracle; behind the combine
    of step 0 the main thread integrates once into a following 128 x 128 x 64 atlas and integrates no more.  A second thread calls
    changes() back to back, at most 100 times and once more when the main thread is done.  The product's origin names the map it
    answered for (the ten origins are distinct): all seven parts must equal the referee's product of that step against the memory of
    step 0 -- never a mixture, never the spare buffer --, the steps must not go back and must end at step 9.  Bounded, nothing retried:
    how many steps the thread got to see is printed, not required."""
    grid = "np2"
    maps, want = vcc.changes_thread_mirror(grid, bs)
    step_of = {tuple(int(v) for v in m.W): k for k, m in enumerate(maps)}
    assert len(step_of) == len(maps)
    g = gvom.Gvom(*qc.rr.params(grid, bs), voxel_statistics=False)
    atlas = g.create_voxel_atlas(vcc.THREAD_ATLAS["cells"], vcc.THREAD_ATLAS["levels"])
    done, kept, errors = threading.Event(), [], []

    def ask():
        with vcc.changes(atlas, *vcc.FIRST) as ch:
            kept.append((tuple(ch.origin_voxels), [ch.n_clusters, ch.marked_columns, ch.dropped], ch.copy_to_host()))

    def query():
        try:
            for _ in range(vcc.THREAD_CALLS):
                if done.is_set():
                    break
                ask()
            done.wait(60)
            ask()
        except BaseException as exc:                              # pragma: no cover
            errors.append(exc)

    t = threading.Thread(target=query)
    try:
        for k, m in enumerate(maps):
            g.process_pointcloud(qc.rr.cloud_of(grid, k), qc.rr.ego_of(grid, k))
            qc.hold_maps(g.combine_maps(), m, "step %d" % k)
            qc.hold_dense(g, gvom, m, "step %d" % k)
            if k == 0:
                assert atlas.integrate() is True                  # the memory every answer is against
                t.start()
    finally:
        done.set()
        if t.ident is not None:
            t.join(120)
    assert not t.is_alive() and not errors, errors
    assert 1 <= len(kept) <= vcc.THREAD_CALLS + 1 and atlas.counts()["seq"] == 1
    steps = []
    for i, (origin, info, got) in enumerate(kept):
        assert origin in step_of, "answer %d has an origin no map of the run has: %r" % (i, origin)
        k = step_of[origin]
        parts, want_info = want[k]
        bad = vcr.differing_parts(got, parts)
        assert not bad and info == want_info, "answer %d (origin of step %d): parts %r differ from the referee on that map; part 3 %r, referee %r; info %r, referee %r" % (
            i, k, bad, list(got[3]), list(parts[3]), info, want_info)
        steps.append(k)
    print("ring of %d: %d answers, steps %s" % (bs, len(kept), sorted(set(steps))))
    assert steps == sorted(steps) and steps[-1] == len(maps) - 1, steps
