"""The voxel atlas at every point of the scan cycle (tests/voxel_atlas_cycle.py has the cycle; tests/query_cycle.py the rule, the mirror
and the scripts): integrate(), box(), raycast(), score_viewpoints() and score_alignments() of a VoxelAtlas, each held with tolerance 0
to the numpy referee of tests/voxel_atlas_ref.py, which is fed ONLY from the CPU oracle's maps -- never from the handle's read_dense().
gvom_voxel_atlas_integrate reads the live fused buffers, so it is asked after a scan that has not been combined, while
combine_maps_async() is pending, after a combine that adopted the speculative fusion of a one-slot ring, after a combine without a
scan, after rejected scans, after combine_maps_device() and combine_maps_occupancy(), on rings of 1 to 4 slots, with the voxel
statistics on, after a jump that clears a following extent or leaves a fixed one behind, across the tile-epoch renumbering, and from a
second thread beside scans and combines.  The window queries of tests/test_query_cycle.py run at every point too: they must hold with
an atlas attached and integrates in between.  tests/test_voxel_atlas_cycle_cpu.py holds, on the mirror alone, the conditions under
which these tests can fail: merging the map a wrong answer would come from leaves at least 1000 voxels in another class.

The cases are the smallest shapes at which each path exists: 64 x 64 x 32 is the smallest legal atlas (on p2 exactly the window), the
fixed 128 x 128 x 64 extents hold the windows of A .. J across the storage seams at world 0, partly lose those of F and J and lie ten
windows from K's.  Rings of 3 and 4 slots make the asynchronous combine at G take the second-stream branch (the counting is in
tests/test_query_cycle.py's docstring).

test_integrate_is_the_first_call_behind_an_asynchronous_combine is this file's own: in the script the window queries come first at G
and join the second stream before the atlas is asked, so there integrate()'s own join is never the one that counts.  What that test
shows is that integrate() takes the map of the combine just begun with nothing in front of it.  It does not show that the join is
there: a library built without the join in gvom_voxel_atlas_integrate passed it three times on the MI355X -- on np2 the fusion is over
before the merge kernel, behind integrate()'s own memset and move launches, starts.  The same holds for the second thread, whose
combines are synchronous.  A library that merged the other fused buffer, or merged under the epoch before, failed at A in every case.

VoxelAtlas.extent_origin is set by integrate() from a second call into the library; beside combines on another thread it can name a
newer window than the merge used.  The thread test therefore takes the extent from its products (DeviceAtlasRays.extent_origin), which
the library fills under the same lock as the walk.

Wall time on the MI355X (pytest --durations, one run): the five cases of test_the_atlas_at_every_point_of_the_cycle 0.41 to 0.67 s each
(twelve window bundles, twelve integrates with nine atlas products each, and the referees), the two of
test_the_atlas_across_the_epoch_renumbering 0.52 and 0.54 s (two ring sizes each), the two asynchronous-first cases 0.14 s each, the two
thread cases 0.18 s each (41 integrates, replayed); the file 4.9 s."""
import os
import threading

import pytest

import query_cycle as qc
import voxel_atlas_cycle as vc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST_LIB = os.path.join(ROOT, "g-vom_amd", "lib", "libgvom_hip_test.so")     # the production sources + the hooks of include/gvom_hip_test.h
CASES = [("np2", 1, False, vc.FOLLOWING), ("np2", 2, False, vc.fixed((70, 20, 30))), ("np2", 4, False, vc.FOLLOWING),
         ("p2", 1, True, vc.fixed((50, 10, 20))), ("p2", 3, True, vc.FOLLOWING)]


@pytest.fixture(scope="module")
def gvom():
    import gvom as mod
    rc, info = mod.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    return mod


@pytest.mark.parametrize("grid,bs,stats,kw", CASES, ids=["np2-1-off-following", "np2-2-off-fixed", "np2-4-off-following", "p2-1-on-fixed", "p2-3-on-following"])
def test_the_atlas_at_every_point_of_the_cycle(gvom, grid, bs, stats, kw):
    """the script P0 .. L of tests/query_cycle.py on an AtlasCycle: twelve integrates, each followed by two boxes, the 512 rays under
    both flags, the viewpoints and two alignment boxes"""
    c = qc.run_script(vc.AtlasCycle(grid, bs, gvom, stats, **kw))
    assert tuple(label for label, _, _ in c.points) == qc.SCRIPT_POINTS
    g = c.g
    assert c.atlas.seq == c.ref.seq == len(qc.SCRIPT_POINTS) == c.atlas.counts()["seq"]
    if bs == 1:
        # as tests/test_query_cycle.py: the combines at A, D, F, G, J and K find a speculation to adopt; the integrates in between
        # neither drop nor adopt one
        print(grid, bs, "adopted", g.get_tuning("eager_adopted"), "dropped", g.get_tuning("eager_dropped"))
        assert g.get_tuning("eager_adopted") >= 4 and g.get_tuning("eager_dropped") >= 1
    else:
        assert g.get_tuning("eager_adopted") == 0
    c.atlas.release()
    assert g.get_tuning("voxel_atlas") == 0


@pytest.mark.parametrize("bs,stats", [(3, False), (4, True)])
def test_integrate_is_the_first_call_behind_an_asynchronous_combine(gvom, bs, stats):
    """voxel_atlas_cycle.run_async_first_script: combine_maps_async() begins its fusion on the second stream and integrate() is the
    next call on the handle -- no window query in between joins the streams for it.  The merge must wait for that fusion and take the
    new map: counts and box equal the referee's on the mirror's map of THIS combine, before .result()"""
    c = vc.run_async_first_script(vc.AtlasCycle("np2", bs, gvom, stats, **vc.FOLLOWING))
    assert [label for label, _, _ in c.points] == ["first", "second, pending", "second"] and c.atlas.seq == 3
    assert c.g.get_tuning("eager_adopted") == 0


@pytest.mark.parametrize("site", ["combine", "scan"])
def test_the_atlas_across_the_epoch_renumbering(gvom, site):
    """the test library's "epoch_bias" makes the tile-epoch renumbering -- which rewrites the fused map's tags -- happen inside a combine
    or inside a scan (query_cycle.EPOCHS_LEFT); the integrate behind it must read the rewritten tags under the new epoch: a merge under
    the old one would take every tile for stale and report the whole window uninformative"""
    for bs in (1, 3):
        c = vc.AtlasCycle("np2", bs, gvom, False, _library=TEST_LIB, **vc.FOLLOWING)
        c.P0("P0")
        qc.run_epoch_script(c, site)
        assert len(c.points) == 6 and c.atlas.seq == c.ref.seq == 6
        if bs == 1:                                               # the sign that the counter crossed where EPOCHS_LEFT says (tests/test_query_cycle.py)
            assert c.g.get_tuning("eager_adopted") == (6 if site == "combine" else 7) and c.g.get_tuning("eager_dropped") == 0


@pytest.mark.parametrize("bs", [1, 3])
def test_an_integrating_thread_beside_scans_and_combines(gvom, bs):
    """query_cycle.thread_mirror's ten steps of scan and combine_maps() on the main thread, each held to the oracle, while a second
    thread integrates, takes the default box and casts 512 rays, at most 40 times and once more when the main thread is done.  The
    box's origin is the window of the thread's own integrate and names the map it merged.  Afterwards exactly that subsequence of the
    mirror's maps is replayed into a VoxelAtlasRef: every recorded box and ray answer must equal the referee's at that point of the
    replay -- never a mixture, never the spare buffer --, the merged steps must not go back and must end at step 9.  Bounded, nothing
    retried: how many steps the thread got to see is printed, not required."""
    grid = "np2"
    maps, A, B = qc.thread_mirror(grid, bs)
    g = gvom.Gvom(*qc.rr.params(grid, bs), voxel_statistics=False)
    atlas = g.create_voxel_atlas(vc.FOLLOWING["cells"], vc.FOLLOWING["levels"])
    done, kept, errors = threading.Event(), [], []

    def ask():
        assert atlas.integrate() is True
        with atlas.box() as box, atlas.raycast(A, B, unknown_blocks=True) as rays:
            kept.append((tuple(box.origin_voxels),) + box.copy_to_host() + (tuple(rays.extent_origin),) + rays.copy_to_host())

    def query():
        try:
            for _ in range(vc.THREAD_INTEGRATES):
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
                t.start()                                         # (from the first combine on there is a map to merge)
    finally:
        done.set()
        if t.ident is not None:
            t.join(120)
    assert not t.is_alive() and not errors, errors
    assert 1 <= len(kept) <= vc.THREAD_INTEGRATES + 1 and atlas.counts()["seq"] == len(kept)
    steps = vc.replay(kept, maps, grid, A, B, vc.FOLLOWING["cells"], vc.FOLLOWING["levels"])
    print("ring of %d: %d integrates, steps %s" % (bs, len(kept), sorted(set(steps))))
    assert steps == sorted(steps) and steps[-1] == len(maps) - 1, steps
