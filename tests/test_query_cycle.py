"""The map queries at every point of the scan cycle (tests/query_cycle.py has the rule, the mirror, the query bundle and the scripts):
raycast, score_viewpoints, score_alignments, occupancy_grid_device / get_map_as_occupancy_grid and the dense read hook, each held to
its numpy referee on the CPU oracle's map with tolerance 0 -- after a scan that has not been combined, while combine_maps_async() is
pending, after a combine that adopted the speculative fusion of a one-slot ring, after a combine without a scan, after rejected scans,
after combine_maps_device() and combine_maps_occupancy(), after a jump of ten windows, across the tile-epoch renumbering, and from a
second thread beside scans and combines.  tests/test_query_cycle_cpu.py holds, on the oracle alone, the conditions under which these
tests can fail: between the map a point must answer for and the map a wrong answer would come from, at least 256 of the 512 rays, the
viewpoint gains and the alignment counts differ.

Which branch an asynchronous combine takes: gvom_combine_begin counts the filled ring slots and runs the fusion on the second stream
from three on.  No tuning value reports it.  It holds at G by counting: scans 0, 1, 2 and 6 have been accepted before G's scan 3, so
a ring of 3 or 4 holds 3 or 4 filled slots when G begins (and a ring of 1 or 2 cannot hold three).

Wall time on the MI355X (pytest --durations, one run): the five cases of test_queries_at_every_point_of_the_cycle 0.26 to 0.30 s
each (twelve bundles, seven referee maps and the oracle's nine combines), the two of test_queries_across_the_epoch_renumbering 0.36
and 0.38 s (two ring sizes each), the two of test_a_query_thread_beside_scans_and_combines 0.17 s each; the file 2.5 s.  The extended
tests/test_hip_parity.py::test_asynchronous_combine_with_several_scans_before_its_end takes 0.51 s."""
import os
import threading

import numpy as np
import pytest

import query_cycle as qc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST_LIB = os.path.join(ROOT, "g-vom_amd", "lib", "libgvom_hip_test.so")     # the production sources + the hooks of include/gvom_hip_test.h


@pytest.fixture(scope="module")
def gvom():
    import gvom as mod
    rc, info = mod.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    return mod


@pytest.mark.parametrize("grid,bs,stats", [("np2", 1, False), ("np2", 2, False), ("np2", 4, False), ("p2", 1, True), ("p2", 3, True)],
                         ids=["np2-1-off", "np2-2-off", "np2-4-off", "p2-1-on", "p2-3-on"])
def test_queries_at_every_point_of_the_cycle(gvom, grid, bs, stats):
    """the script P0 .. L of tests/query_cycle.py.  With the statistics on (p2) the speculation of a one-slot ring has a statistics
    half, and eager_launch waits for the previous merge before it rewrites the spare buffer."""
    c = qc.run_script(qc.Cycle(grid, bs, gvom, stats))
    assert tuple(label for label, _, _ in c.points) == qc.SCRIPT_POINTS
    g = c.g
    if bs == 1:
        # every scan of a one-slot ring speculates; the combines at A, D, F, G, J and K find a speculation to adopt, scan 2 (behind
        # scan 1) and the first rejected scan (behind scan 4) drop one
        print(grid, bs, "adopted", g.get_tuning("eager_adopted"), "dropped", g.get_tuning("eager_dropped"))
        assert g.get_tuning("eager_adopted") >= 4 and g.get_tuning("eager_dropped") >= 1
    else:
        assert g.get_tuning("eager_adopted") == 0


@pytest.mark.parametrize("site", ["combine", "scan"])
def test_queries_across_the_epoch_renumbering(gvom, site):
    """the test library's "epoch_bias" pushes the tile-epoch counter to its limit so that the renumbering -- which rewrites every
    live tag, the fused map's included -- happens inside a combine or inside a scan (query_cycle.EPOCHS_LEFT has the arithmetic for
    both ring sizes); Q after every scan and every combine around it, and products kept from before it"""
    for bs in (1, 3):
        c = qc.run_epoch_script(qc.Cycle("np2", bs, gvom, False, _library=TEST_LIB), site)
        assert len(c.points) == 6
        if bs == 1:
            # the sign that the counter crossed where EPOCHS_LEFT says: a renumbering inside a combine drops the speculation that
            # waits for it (6 of the 7 combines adopt one), a renumbering at the start of a scan meets none (all 7 do)
            assert c.g.get_tuning("eager_adopted") == (6 if site == "combine" else 7) and c.g.get_tuning("eager_dropped") == 0


@pytest.mark.parametrize("bs", [1, 3])
def test_a_query_thread_beside_scans_and_combines(gvom, bs):
    """ten steps of scan and combine_maps() on the main thread while a second thread casts the same 512 rays back to back, at most
    200 times and once more when the main thread is done.  Every answer must be the referee's on the oracle map that has the answer's
    origin -- never a mixture, never the spare buffer --, the origins must come in step order, and the mapper's own maps equal the
    oracle's at every step.  Bounded, nothing retried: how many maps the thread gets to see is printed, not required (on the
    MI355X, both ring sizes: 201 answers, for the maps of steps 0, 1, 2, 3 and 9 -- the 200 calls are over during step 3)."""
    grid = "np2"
    maps, A, B = qc.thread_mirror(grid, bs)
    want = [qc.rr.walk(m.state, m.W, grid, A, B, unknown_blocks=True) for m in maps]
    step_of = {tuple(m.W.tolist()): k for k, m in enumerate(maps)}
    assert len(step_of) == len(maps)
    g = gvom.Gvom(*qc.rr.params(grid, bs), voxel_statistics=False)
    done, kept, errors = threading.Event(), [], []

    def ask():
        with g.raycast(A, B, unknown_blocks=True) as rays:
            kept.append((rays.origin.copy(),) + rays.copy_to_host())

    def query():
        try:
            for _ in range(qc.THREAD_CALLS):
                if done.is_set():
                    break
                ask()
            done.wait(60)
            ask()
        except Exception as exc:                                  # pragma: no cover
            errors.append(exc)

    t = threading.Thread(target=query)
    try:
        for k, m in enumerate(maps):
            g.process_pointcloud(qc.rr.cloud_of(grid, k), qc.rr.ego_of(grid, k))
            qc.hold_maps(g.combine_maps(), m, "step %d" % k)
            qc.hold_dense(g, gvom, m, "step %d" % k)
            if k == 0:
                t.start()                                         # (from the first combine on there is a map to ask about)
    finally:
        done.set()
        if t.ident is not None:
            t.join(120)
    assert not t.is_alive() and not errors, errors
    steps = []
    for i, (origin, result, position) in enumerate(kept):
        key = tuple(origin.tolist())
        assert key in step_of, "answer %d has an origin no map of the run has: %r" % (i, origin)
        k = step_of[key]
        changed = qc.rays_changed((result, position), want[k])
        assert changed == 0, "answer %d (origin of step %d): %d of 512 rays differ from the referee on that map" % (i, k, changed)
        steps.append(k)
    print("ring of %d: %d answers, steps %s" % (bs, len(kept), sorted(set(steps))))
    assert steps == sorted(steps) and steps[-1] == len(maps) - 1, steps
