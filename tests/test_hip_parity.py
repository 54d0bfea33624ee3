"""Parity tests proper: the HIP path (g-vom_amd/gvom.py -> C ABI -> gfx950 kernels) against
  (1) the golden vectors recorded from the reference itself (tests/golden/f*.npz), and
  (2) the CPU oracle on seeded inputs up to BASELINE.json's full sizes (c1, c2, c3, 256^3),
plus size-independent properties (point-order invariance, count conservation).

Bar (BASELINE.json north_star): integer maps and per-voxel counts bit-exact; float maps
within 1e-5 (only log/atan2-derived values can differ from glibc, by ~1 ulp; everything
else is compared exactly)."""
import os

import numpy as np
import pytest

import scenarios
import synth
from parity import compare_cloud, compare_records, compare_statistics
from oracle import oracle

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST_LIB = os.path.join(ROOT, "g-vom_amd", "lib", "libgvom_hip_test.so")     # make -C g-vom_amd test-lib (built by __graft_entry__.build())


@pytest.fixture(scope="module")
def gvom_mod():
    """The product module, with ONE difference for these tests: `gvom_mod.Gvom` defaults to voxel_statistics=False -- the
    north-star path at every step (eager fusion of one-slot rings included), as in every round before the statistics became
    on-demand.  The class as a user gets it (statistics for as long as somebody reads them) is `gvom_mod.DefaultGvom`: the golden
    fixtures and the on-demand test run through it."""
    import types
    import gvom
    rc, info = gvom.Gvom.backend_info()
    assert rc == 0, "HIP backend unusable: %s" % info
    assert "gfx950" in info, info

    class NorthStarGvom(gvom.Gvom):
        def __init__(self, *p, **kw):
            kw.setdefault("voxel_statistics", False)
            super(NorthStarGvom, self).__init__(*p, **kw)
    ns = types.SimpleNamespace(**{k: v for k, v in vars(gvom).items() if not k.startswith("__")})
    ns.Gvom, ns.DefaultGvom = NorthStarGvom, gvom.Gvom
    return ns


@pytest.mark.parametrize("name", ["f1", "f2", "f3", "f4", "f5", "f6", "f7"])
def test_hip_reproduces_reference_golden(gvom_mod, name):
    path = os.path.join(G, name + ".npz")
    if not os.path.exists(path):
        pytest.skip("fixture %s not generated" % name)
    want = np.load(path)
    sc = scenarios.scenario_from_record(want)
    got = scenarios.run_and_record(gvom_mod.DefaultGvom, sc, record_debug=(name != "f7"))
    # (eigenvalue columns of the debug voxel cloud: on these fixtures the two algorithms -- the reference's two centred passes, this
    # library's raw moments + shift algebra -- agree to 2.3e-16 absolute, tools/stats_deviation.py; held to 1e-6 relative / 1e-9)
    assert compare_records(got, want, float_tol=1e-5, stats_rtol=1e-6, stats_atol=1e-9) > 5
    plain = scenarios.run_and_record(gvom_mod.Gvom, sc, record_debug=(name != "f7"))        # no statistics at any step
    assert compare_records(plain, want, float_tol=1e-5, skip=("debug_voxel_map",)) > 5 and not any(k.endswith("debug_voxel_map") for k in plain)
    # the DEFAULT constructor, no environment variable, the node's call pattern (gvom_ros.py:109, 115, 171-189: scan, combine,
    # the three debug reads): the per-voxel statistics run for as long as make_debug_voxel_map is called, so the unchanged
    # node gets the reference's debug voxel cloud from its first tick on
    if name != "f7":
        assert any(k.endswith("debug_voxel_map") for k in got) == any(k.endswith("debug_voxel_map") for k in want.files)


@pytest.mark.parametrize("name", ["f1", "f2", "f3", "f4", "f5", "f6"])
def test_hip_voxel_statistics_match_reference_golden(gvom_mod, name):
    """Opt-in per-voxel statistics: make_debug_voxel_map against the rows the
    reference produced (sorted by voxel; f64 atomic accumulation order is unspecified on both sides; on these small fixtures the
    eigenvalue columns agree to 2.3e-16 and are held to 1e-6 relative / 1e-9 absolute -- the full-size comparisons against the oracle
    keep 1e-4 / 2e-5), everything else as in the default configuration."""
    want = np.load(os.path.join(G, name + ".npz"))
    sc = scenarios.scenario_from_record(want)
    got = scenarios.run_and_record(lambda *p: gvom_mod.Gvom(*p, voxel_statistics=True), sc)
    assert compare_records(got, want, float_tol=1e-5, stats_rtol=1e-6, stats_atol=1e-9) > 5
    assert any(k.endswith("debug_voxel_map") for k in got) == any(k.endswith("debug_voxel_map") for k in want.files)


def test_voxel_statistics_run_on_demand(gvom_mod):
    """voxel_statistics=None (the default): the reference's per-voxel path runs from the first scan on and for as long as somebody
    reads it (the unchanged node calls make_debug_voxel_map every tick, gvom_ros.py:171) -- golden F1-F6 above hold that form to
    the reference's rows.  Here the other half: a caller that never asks stops paying at the fourth unread combine (the scans then take
    the north-star path: eager fusion on this one-slot ring); a later make_debug_voxel_map() returns None once -- which the node
    tolerates, gvom_ros.py:172 -- and switches the statistics on again for the scans that follow; the cloud is back once the
    ring has been replaced.  Its position / solid-factor / hit columns are exact at every moment (they do not depend on the
    statistics); the eigenvalue columns restart from the ring.  voxel_statistics=False never produces a cloud.  The returned
    maps never depend on any of it."""
    params = (0.4, 0.2, 32, 16, 1, 0.5, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
    rng = np.random.default_rng(77)
    auto, always, never = gvom_mod.DefaultGvom(*params), gvom_mod.Gvom(*params, voxel_statistics=True), gvom_mod.Gvom(*params, voxel_statistics=False)
    import stats_demand_ref
    mirror = stats_demand_ref.DemandOracle(*params)             # the rule in plain Python (tests/test_stats_on_demand.py holds it at length)

    def step(k, read):
        ego = (0.3 * k, -0.2 * k, 0.02 * k)
        pc = np.stack([rng.uniform(-5, 5, 4000) + ego[0], rng.uniform(-5, 5, 4000) + ego[1], rng.normal(-0.8, 0.3, 4000)], 1).astype(np.float32)
        outs = []
        for g in (auto, always, never):
            g.process_pointcloud(pc, ego)
            outs.append(g.combine_maps())
        mirror.process_pointcloud(pc.copy(), ego)
        mirror.combine_maps()
        for o in outs[1:]:
            for a, b in zip(outs[0], o):
                assert np.array_equal(a, b)
        if not read:
            return None
        a = auto.make_debug_voxel_map()
        assert mirror.read() == (a is not None), k
        return a, always.make_debug_voxel_map(), never.make_debug_voxel_map()

    def same_cloud(a, b, eigen):
        a, b = a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))], b[np.lexsort((b[:, 2], b[:, 1], b[:, 0]))]
        assert a.shape == b.shape and np.array_equal(a[:, :5], b[:, :5])
        if eigen:
            np.testing.assert_allclose(a[:, 5:], b[:, 5:], rtol=1e-4, atol=2e-5)

    for k in range(3):                                          # the node's pattern: read after every combine
        a, w, n = step(k, True)
        assert n is None and a is not None and w is not None
        same_cloud(a, w, True)
    # (one-slot ring: with or without statistics the scan's second kernel is the eager encode-and-fuse, and the statistics' own
    # merge -- k_fuse_stats -- is enqueued with the scan as well; the combines adopt both)
    assert auto.get_tuning("eager_adopted") == 3 and always.get_tuning("eager_adopted") == 3
    for k in range(3, 9):                                       # nobody asks: off at the fourth unread combine (number 6)
        step(k, False)
    assert auto.get_tuning("eager_adopted") == 9 and always.get_tuning("eager_adopted") == 9 and never.get_tuning("eager_adopted") == 9
    a, w, n = step(9, True)
    assert a is None and w is not None and n is None            # the read that switches them on again finds nothing
    a, w, n = step(10, True)                                    # one-slot ring: replaced by the next scan
    assert a is not None and n is None
    same_cloud(a, w, False)
    compare_statistics(auto, mirror, what="restarted, step 10: ")      # means, covariances, counts, eigenvalues: restarted from the ring
    a, w, n = step(11, True)
    same_cloud(a, w, False)
    compare_statistics(auto, mirror, what="restarted, step 11: ")


def test_hip_voxel_statistics_match_oracle_c2(gvom_mod):
    """Statistics at full c2 size over 3 scans with a moving sensor and buffer=2 (ring slots in
    float64, previous fused map in float32, as in the reference)."""
    params, scans = synth.config_inputs("c2", n_scans=3)
    params = params[:4] + (2,) + params[5:]
    steps = []
    for s in scans:
        steps += [("scan",) + s, ("combine",)]
    sc = {"params": params, "steps": steps}
    want = scenarios.run_and_record(lambda *p: oracle.OracleGvom(*p, voxel_statistics=True), sc)
    got = scenarios.run_and_record(lambda *p: gvom_mod.Gvom(*p, voxel_statistics=True), sc)
    # (measured, tools/stats_deviation.py c2: max |d| 3.7e-8 over 175,000 eigenvalue entries, 99.9 % of them below 1e-16 -- held to the
    # north star's 1e-5 relative, 1e-7 absolute)
    assert compare_records(got, want, float_tol=1e-5, stats_rtol=1e-5, stats_atol=1e-7) > 20


def test_reference_statistics_attributes(gvom_mod):
    """SURVEY App. B.12 attributes that exist on the reference object when the statistics path runs:
    metrics_buffer[slot] (float64 (C,10)), combined_metrics / last_combined_metrics (float32 (Cc,10)) and
    voxels_eigenvalues (float32 (Cc,3), set by make_debug_voxel_map) -- compared with the oracle's, rows
    in voxel order on both sides (row order is unspecified in the reference, gvom.py:964,1158).
    Counts exact; means / covariances to float-atomic-order tolerance."""
    params = (0.4, 0.2, 32, 16, 2, 0.5, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
    rng = np.random.default_rng(12)
    g, w = gvom_mod.Gvom(*params, voxel_statistics=True), oracle.OracleGvom(*params, voxel_statistics=True)
    assert gvom_mod.Gvom(*params).combined_metrics is None
    for k in range(3):
        ego = (0.5 * k, -0.3 * k, 0.05 * k)
        pc = np.stack([rng.uniform(-5, 5, 6000) + ego[0], rng.uniform(-5, 5, 6000) + ego[1], rng.normal(-0.8, 0.3, 6000)], 1)
        g.process_pointcloud(pc, ego); w.process_pointcloud(pc.copy(), ego)
        g.combine_maps(); w.combine_maps()
        assert w.make_debug_voxel_map() is not None and g.make_debug_voxel_map() is not None
        slot = w.last_buffer_index

        def voxel_order(index_map, arr):
            im = np.asarray(index_map)
            return np.asarray(arr)[im[im >= 0]]
        wm = voxel_order(w.index_buffer[slot], w.metrics_buffer[slot])
        gm = g.metrics_buffer[slot].copy_to_host()
        assert gm.dtype == np.float64 and gm.shape == wm.shape
        assert np.array_equal(gm[:, 9], wm[:, 9])
        np.testing.assert_allclose(gm, wm, rtol=1e-9, atol=1e-9)
        wc = voxel_order(w.combined_index_map, w.combined_metrics)
        gc_ = g.combined_metrics.copy_to_host()
        assert gc_.dtype == np.float32 and gc_.shape == wc.shape
        assert np.array_equal(gc_[:, 9], wc[:, 9])
        np.testing.assert_allclose(gc_, wc, rtol=1e-4, atol=1e-5)
        we = voxel_order(w.combined_index_map, w.voxels_eigenvalues)
        ge = g.voxels_eigenvalues.copy_to_host()
        assert ge.dtype == np.float32 and ge.shape == we.shape
        np.testing.assert_allclose(ge, we, rtol=1e-3, atol=2e-5)
        assert np.array_equal(g.last_combined_metrics.copy_to_host(), gc_)


@pytest.mark.parametrize("site", ["combine", "scan"])
def test_tile_epoch_renumbering_before_the_counter_wraps(gvom_mod, site):
    """Tile epochs are 32-bit and advance twice per step (2^32 = ~3 days at 7.7 kHz).  Before the counter
    can wrap, every live map is re-tagged with a small epoch and all other tags are zeroed: pushed to
    just below the limit, a run with ring wrap + previous-map carry continues to match the oracle."""
    params = (0.4, 0.2, 32, 16, 3, 0.5, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
    rng = np.random.default_rng(4)
    # "epoch_bias" is a TEST HOOK: it exists in lib/libgvom_hip_test.so (the production sources + include/gvom_hip_test.h's three
    # hooks), not in the production library, which refuses the name
    with pytest.raises(gvom_mod.GvomBackendError):
        gvom_mod.DefaultGvom(*params).set_tuning("epoch_bias", 1)
    g, w = gvom_mod.Gvom(*params, _library=TEST_LIB), oracle.OracleGvom(*params)
    for k in range(12):
        if k == 4:
            # 8 epochs used so far; the threshold is crossed by the next combine / the scan after it
            g.set_tuning("epoch_bias", 0xFFFFFF00 - 2 * 4 - (3 if site == "combine" else 2))
        ego = (0.45 * k, -0.3 * k, 0.04 * k)
        pc = np.stack([rng.uniform(-5, 5, 3000) + ego[0], rng.uniform(-5, 5, 3000) + ego[1], rng.normal(-0.8, 0.3, 3000)], 1)
        g.process_pointcloud(pc, ego); w.process_pointcloud(pc.copy(), ego)
        a, b = g.combine_maps(), w.combine_maps()
        for i in (0, 1, 2, 4):
            assert np.array_equal(a[i], b[i]), (k, i)
        assert np.allclose(a[3], b[3], rtol=0, atol=1e-5)
        assert g.combined_cell_count_cpu == w.combined_cell_count_cpu
        gd = g.read_dense(gvom_mod.GVOM_WHICH_FUSED)
        wd = scenarios.dense_from_compact(w.combined_index_map, w.combined_hit_count, w.combined_total_count, w.combined_min_height)
        for j in range(4):
            assert np.array_equal(np.asarray(wd[j]), gd[j]), (k, j)


def test_returned_arrays_in_c_order_and_the_reference_objects_attributes(gvom_mod):
    """combine_maps returns Fortran-ordered VIEWS of the pinned memory the GPU wrote (the node flattens them with order='F',
    gvom_ros.py:141-162: a no-copy reshape); the reference returns C-contiguous copies (gvom.py:352-354).  Gvom(..., c_order=True)
    returns those: same values, dtypes and [x, y] indexing, C-contiguous, their own memory.  And the reference object's remaining
    attributes (gvom.py:54, 65-67, 94, 96) exist on a live mapper."""
    import threading
    params = (0.4, 0.2, 48, 16, 2, 0.5, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
    rng = np.random.default_rng(3)
    f, c = gvom_mod.Gvom(*params), gvom_mod.Gvom(*params, c_order=True)
    for k in range(3):
        ego = (0.5 * k, -0.3 * k, 0.02 * k)
        pc = np.stack([rng.uniform(-8, 8, 5000) + ego[0], rng.uniform(-8, 8, 5000) + ego[1], rng.normal(-0.8, 0.3, 5000)], 1)
        f.process_pointcloud(pc, ego); c.process_pointcloud(pc, ego)
        a, b = f.combine_maps(), c.combine_maps()
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)
        for m in b[1:]:
            assert m.flags["C_CONTIGUOUS"] and m.flags["OWNDATA"]
        for m in a[1:]:
            assert m.flags["F_CONTIGUOUS"] and np.shares_memory(np.reshape(m, -1, order="F"), m)     # the node's flatten: a view
        assert np.array_equal(np.reshape(a[1], -1, order="F"), np.reshape(b[1], -1, order="F"))
    assert len(f.semaphores) == params[4] and all(isinstance(sm, type(threading.Semaphore())) for sm in f.semaphores)
    assert isinstance(f.ego_semaphore, type(threading.Semaphore())) and f.blocks == -(-f.voxel_count // f.threads_per_block)
    assert np.array_equal(f.metrics.copy_to_host(), np.array([[3, 2]]))


def test_asynchronous_combine_overlapped_with_the_next_scan(gvom_mod):
    """combine_maps_async(): the next scan is processed while the maps of the pending combine are still
    being computed / stored (k_map2d on the second stream).  Every result equals the synchronous
    mapper's, over a moving window with ring wrap; misuse is refused."""
    params = (0.4, 0.2, 64, 32, 3, 0.5, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
    rng = np.random.default_rng(11)
    a, b = gvom_mod.Gvom(*params), gvom_mod.Gvom(*params)
    assert b.combine_maps_async().result() is None                 # empty ring
    pending, want = None, None
    for k in range(10):
        ego = (0.45 * k, -0.3 * k, 0.04 * k)
        pc = np.stack([rng.uniform(-11, 11, 20000) + ego[0], rng.uniform(-11, 11, 20000) + ego[1],
                       rng.normal(-0.8, 0.4, 20000)], 1).astype(np.float32)
        a.process_pointcloud(pc, ego)
        b.process_pointcloud(pc, ego)                              # runs while combine k-1 is pending
        if pending is not None:
            got = pending.result()
            assert pending.result() is got                         # idempotent
            for i in range(5):
                assert np.array_equal(got[i], want[i]), (k, i)
        want = a.combine_maps()
        pending = b.combine_maps_async()
        with pytest.raises(Exception):
            b.combine_maps()                                       # one combine at a time
        with pytest.raises(Exception):
            b.combine_maps_async()
    got = pending.result()
    for i in range(5):
        assert np.array_equal(got[i], want[i])
    assert b.combined_cell_count_cpu == a.combined_cell_count_cpu
    ad, bd = a.read_dense(gvom_mod.GVOM_WHICH_FUSED), b.read_dense(gvom_mod.GVOM_WHICH_FUSED)
    for j in range(4):
        assert np.array_equal(ad[j], bd[j])
    # after the pending combine is ended the synchronous call works again
    assert b.combine_maps() is not None
    # ... and a handle dropped without result() ends its combine
    dropped = b.combine_maps_async()
    del dropped
    assert b.combine_maps() is not None
    # the occupancy form (int8 grids): asynchronous == synchronous
    for _ in range(3):
        a.combine_maps()                                           # b has combined three times more (the previous map enters a combine)
    want_occ = a.combine_maps_occupancy(40, -8, 0)
    got_occ = b.combine_maps_occupancy_async(40, -8, 0).result()
    for i in range(6):
        assert np.array_equal(got_occ[i], want_occ[i]), i


def test_asynchronous_combine_with_several_scans_before_its_end(gvom_mod):
    """with three or more filled slots the asynchronous combine runs its FUSION on the second stream
    too.  The first scan after combine_maps_async() goes into the spare slot, but its commit makes the ring's
    oldest slot -- a source of the fusion in flight -- the next spare one, and the SECOND scan writes it.  A long
    ring (40 slots of a 256 x 256 x 64 grid: a fusion of several hundred microseconds) and tiny clouds (a scan
    of a few tens) make that overlap certain; the main stream must wait for the fusion before it touches the
    slot, and the read hooks before they read the fused map.  Everything equals the synchronous mapper's.
    The product calls read the fused map too: in rounds 2 to 5 raycast, occupancy_grid_device and score_alignments are issued on
    both mappers -- on the asynchronous one while its fusion is in flight, each kind once as the FIRST call behind
    combine_maps_async() (the call that has to join the second stream; round 3 keeps the read hook first) -- and their products
    must be bit-identical.  Two schedules of the same kernels are compared here; tests/test_query_cycle.py holds the same calls to
    their referees on small maps."""
    params = (0.2, 0.2, 256, 64, 40, 0.5, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
    rng = np.random.default_rng(21)
    # 512 segments and 2,048 returns inside the window of every round (the egos of rounds 0 .. 5 lie within 3 m of (11, -7, 0.5);
    # the window is 51.2 m wide and 12.8 m high), 16 candidate poses; a generator of their own: the clouds' stay as they were
    qrng = np.random.default_rng(77)
    centre = np.array([10.0, -6.0, 0.5])
    seg_a, seg_b = ((centre + qrng.uniform(-1, 1, (512, 3)) * (20.0, 20.0, 4.5)).astype(np.float32) for _ in range(2))
    returns = (centre + qrng.uniform(-1, 1, (2048, 3)) * (20.0, 20.0, 2.0)).astype(np.float32)
    poses = np.tile(np.identity(4), (16, 1, 1))
    poses[:, :3, 3] = qrng.uniform(-0.6, 0.6, (16, 3)) * (1.0, 1.0, 0.2)
    calls = {"raycast": lambda g: g.raycast(seg_a, seg_b, unknown_blocks=True),
             "occupancy": lambda g: g.occupancy_grid_device(),
             "alignments": lambda g: g.score_alignments(returns, poses, dilate=1)}
    first = {2: "raycast", 3: "raycast", 4: "occupancy", 5: "alignments"}

    def products(g, rnd):
        """the three products of mapper g as bytes, the kind `first[rnd]` first"""
        out = {}
        for kind in [first[rnd]] + [k for k in sorted(calls) if k != first[rnd]]:
            with calls[kind](g) as p:
                parts = p.copy_to_host()
                parts = parts if isinstance(parts, tuple) else (parts,)
                out[kind] = [a.tobytes() for a in parts] + ([p.origin.tobytes()] if kind != "occupancy" else [])
        return out

    def cloud(k, n):
        ego = (0.21 * k, -0.13 * k, 0.01 * k)
        return np.stack([rng.uniform(-20, 20, n) + ego[0], rng.uniform(-20, 20, n) + ego[1],
                         rng.normal(-0.9, 0.5, n)], 1).astype(np.float32), ego
    a, b = gvom_mod.Gvom(*params), gvom_mod.Gvom(*params)
    k = 0
    for _ in range(42):                                              # fill the ring and wrap once: big clouds
        pc, ego = cloud(k, 30000); k += 1
        a.process_pointcloud(pc, ego); b.process_pointcloud(pc, ego)
    for rnd in range(6):
        want = a.combine_maps()
        pending = b.combine_maps_async()
        if rnd == 3:                                                 # a read hook while the fusion is in flight
            ad, bd = a.read_dense(gvom_mod.GVOM_WHICH_FUSED), b.read_dense(gvom_mod.GVOM_WHICH_FUSED)
            for j in range(4):
                assert np.array_equal(ad[j], bd[j]), ("fused map read during the combine", j)
        if rnd in first:                                             # the product calls while the fusion is in flight
            bp, ap = products(b, rnd), products(a, rnd)
            for kind in sorted(calls):
                assert ap[kind] == bp[kind], ("round %d: the %s product differs between the two mappers" % (rnd, kind))
            assert np.frombuffer(bp["occupancy"][0], np.uint8).sum() > 10000 and len(set(bp["raycast"][0])) > 4
        for _ in range(3 + rnd % 2):                                 # several tiny scans before the combine is ended
            pc, ego = cloud(k, 300); k += 1
            a.process_pointcloud(pc, ego); b.process_pointcloud(pc, ego)
        got = pending.result()
        for i in range(5):
            assert np.array_equal(got[i], want[i]), (rnd, i)
        assert a.combined_cell_count_cpu == b.combined_cell_count_cpu
    ad, bd = a.read_dense(gvom_mod.GVOM_WHICH_FUSED), b.read_dense(gvom_mod.GVOM_WHICH_FUSED)
    for j in range(4):
        assert np.array_equal(ad[j], bd[j]), j
    for slot in (0, 17, 39):
        ad, bd = a.read_dense(slot), b.read_dense(slot)
        for j in range(4):
            assert np.array_equal(ad[j], bd[j]), (slot, j)


@pytest.mark.parametrize("buffer_size", [3, 1])
def test_scans_from_a_second_thread_while_a_combine_waits(gvom_mod, buffer_size):
    """The ROS node calls process_pointcloud and combine_maps from two callback threads
    (gvom_ros.py:44-51).  combine_maps waits for its maps with the handle released, so scans keep being
    accepted; no call is lost, nothing deadlocks, and once both threads are done the map is the one a
    sequential run of the same scans gives (the fusion only depends on the scans in the ring).
    buffer_size 1: the eager fusion's speculations are adopted or dropped as the two threads' calls happen to
    interleave (a scan entering while a combine waits, a combine entering while a scan waits for its trace)."""
    import threading
    params = (0.4, 0.2, 64, 32, buffer_size, 0.5, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
    rng = np.random.default_rng(12)
    scans = []
    for k in range(40):
        ego = (0.1 * k, 0.0, 0.0)
        scans.append((np.stack([rng.uniform(-11, 11, 20000) + ego[0], rng.uniform(-11, 11, 20000),
                                rng.normal(-0.8, 0.4, 20000)], 1).astype(np.float32), ego))
    g, ref = gvom_mod.Gvom(*params), gvom_mod.Gvom(*params)
    combines, errors = [0], []

    def scanner():
        try:
            for pc, ego in scans:
                g.process_pointcloud(pc, ego)
        except Exception as exc:                                      # pragma: no cover
            errors.append(exc)

    def combiner():
        try:
            while t1.is_alive():
                if g.combine_maps() is not None:
                    combines[0] += 1
        except Exception as exc:                                      # pragma: no cover
            errors.append(exc)

    t1 = threading.Thread(target=scanner); t2 = threading.Thread(target=combiner)
    t1.start(); t2.start(); t1.join(60); t2.join(60)
    assert not t1.is_alive() and not t2.is_alive() and not errors, errors
    assert combines[0] > 0
    if buffer_size == 1:
        assert g.get_tuning("eager_adopted") + g.get_tuning("eager_dropped") > 0
        # a quiet epilogue on both mappers: scan, combine, combine -- the first adopts a speculation, the second re-fuses the slot
        g.combine_maps()
    for pc, ego in scans:
        ref.process_pointcloud(pc, ego)
    # the previous fused map enters a combine (gvom.py:972-997), so only ring contents are compared
    for slot in range(params[4]):
        a, b = g.read_dense(slot), ref.read_dense(slot)
        for j in range(4):
            assert np.array_equal(a[j], b[j]), (slot, j)


@pytest.mark.parametrize("grid", [(64, 32), (30, 20)])
def test_free_counts_stop_before_they_wrap_into_row_indices(gvom_mod, grid):
    """The voxels next to the sensor are passed by a good part of all rays, and the fused map carries its
    predecessor's free counts along (gvom.py:996): ~25,000 passes per combine reach 2^31 within 90,000 combines
    (c3's 262 k-point scans in a ring of 8: within ~1000).  An int32 that wraps becomes a
    non-negative state, i.e. a row index, for every reader (the reference's does, and then indexes out of
    bounds).  Here the count stops at 2^30: the voxel stays free, the maps stay what they were, nothing faults.
    (Both fusion kernels: xy % 4 == 0 and not.)"""
    xy, zs = grid
    params = (0.4, 0.2, xy, zs, 1, 0.5, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
    rng = np.random.default_rng(3)
    n = 200000
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
    pc = (d * rng.uniform(2.0, 0.19 * xy, (n, 1)) * np.array([1, 1, 0.15])).astype(np.float32)
    g = gvom_mod.Gvom(*params)
    g.process_pointcloud(pc, (0.0, 0.0, 0.0))
    for k in range(200):
        out = g.combine_maps()
    early = [m.copy() for m in out]                                   # (the previous map's carry-over has settled by now)
    for k in range(100000):                                           # the busiest voxels: ~25 k x 100,000 = 2.5e9 > 2^31
        out = g.combine_maps()
    state = g.read_dense(gvom_mod.GVOM_WHICH_FUSED)[0]
    assert state.min() == -(1 << 30)                                   # the busiest voxels sit on the floor ...
    busy = state == -(1 << 30)
    assert 0 < busy.sum() < 64
    # ... and every voxel that was free after two combines still is (no count turned into a row)
    g2 = gvom_mod.Gvom(*params)
    g2.process_pointcloud(pc, (0.0, 0.0, 0.0)); g2.combine_maps(); g2.combine_maps()
    s2 = g2.read_dense(gvom_mod.GVOM_WHICH_FUSED)[0]
    assert np.array_equal(state >= 0, s2 >= 0) and np.array_equal(state == -1, s2 == -1)
    for i in (1, 2, 4):
        assert np.array_equal(out[i], early[i]), i


def test_cloud_sizes_swing_by_orders_of_magnitude(gvom_mod):
    """5 ... 300,000 returns from scan to scan (float32 and float64, host arrays): the grow-only buffers are
    re-allocated while earlier scans sit in the ring; an empty cloud in between; everything equals the oracle."""
    params = (0.4, 0.2, 64, 32, 4, 0.5, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
    rng = np.random.default_rng(21)
    steps = []
    for k, n in enumerate([100, 50000, 5, 0, 300000, 17, 120000, 1, 64, 65, 4096, 250000]):
        ego = (0.3 * k, -0.1 * k, 0.0)
        pc = np.stack([rng.uniform(-11, 11, n) + ego[0], rng.uniform(-11, 11, n) + ego[1], rng.normal(-0.8, 0.4, n)], 1)
        steps += [("scan", pc.astype(np.float32 if k % 3 else np.float64), ego, None), ("combine",)]
    got, want = _run_both(gvom_mod, params, steps, record_debug=False)
    assert compare_records(got, want, float_tol=1e-5) > 50


def test_huge_jumps_of_the_window(gvom_mod):
    """The ego jumps by tens of kilometres and to 3e8 m (window origin beyond 2^30 voxels: the literal float64
    voxel lookup) and back, with a ring of 3 and float64 clouds: every slot of the ring falls out of the window and
    comes back; everything equals the oracle."""
    params = (0.4, 0.2, 32, 16, 3, 0.5, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
    rng = np.random.default_rng(9)
    egos = [(0, 0, 0), (0.5, 0.2, 0.0), (5e4, -3e4, 10.0), (5e4 + 0.3, -3e4, 10.0), (3.2e8, 1.1e8, -50.0),
            (3.2e8 + 0.4, 1.1e8, -50.0), (-7.7e8, 2.0e8, 0.0), (0, 0, 0), (0.3, 0, 0)]
    steps = []
    for ego in egos:
        pc = np.stack([rng.uniform(-5, 5, 4000) + ego[0], rng.uniform(-5, 5, 4000) + ego[1],
                       rng.normal(-0.8, 0.3, 4000) + ego[2]], 1)
        steps += [("scan", pc, ego, None), ("combine",)]
    got, want = _run_both(gvom_mod, params, steps)
    assert compare_records(got, want, float_tol=1e-5) > 100


def test_returned_arrays_outlive_the_mapper(gvom_mod):
    """combine_maps' arrays are views of a pinned buffer: they stay valid after the Gvom is gone, and the
    buffer is released when the last of them is collected (no leak per orphaned result)."""
    import gc
    params, scans = synth.config_inputs("c2")
    g = gvom_mod.Gvom(*params)
    pc, ego, tf = scans[0]
    g.process_pointcloud(pc, ego, tf)
    out = g.combine_maps()
    pool = g._out_pool
    keep = [np.array(o, copy=True) for o in out]
    del g
    gc.collect()
    assert pool.closed and pool.free == []
    for a, b in zip(out, keep):
        assert np.array_equal(a, b)
    del out, a
    gc.collect()
    assert pool.free == []                   # given back after the mapper's death: freed, not pooled


def _run_both(gvom_mod, params, steps, record_debug=True):
    sc = {"params": params, "steps": steps}
    want = scenarios.run_and_record(oracle.OracleGvom, sc, record_debug=record_debug)
    got = scenarios.run_and_record(gvom_mod.Gvom, sc, record_debug=record_debug)
    return got, want


def _random_steps(seed, n_scans, n_pts, half_xy, half_z, dtype, with_tf, step=0.7):
    rng = np.random.default_rng(seed)
    steps = []
    for k in range(n_scans):
        ego = (step * k + rng.uniform(-.2, .2), -0.4 * step * k + rng.uniform(-.2, .2),
               0.1 * k + rng.uniform(-.1, .1))
        pc = np.stack([rng.uniform(-half_xy, half_xy, n_pts) + ego[0],
                       rng.uniform(-half_xy, half_xy, n_pts) + ego[1],
                       rng.normal(-0.8, 0.5 * half_z, n_pts) + ego[2]], axis=1).astype(dtype)
        tf = None
        if with_tf:
            tf = scenarios.rot_z(0.05 * (k + 1), (0.01 * k, -0.02, 0.005))
        steps.append(("scan", pc, ego, tf))
        steps.append(("combine",))
    return steps


@pytest.mark.parametrize("case", [
    # (xy, zs, buffer, n_scans, n_pts, dtype, with_tf)
    (64, 32, 1, 1, 50000, np.float64, False),      # c1 shape
    (64, 32, 3, 5, 20000, np.float32, True),       # ring wrap + previous-map carry + transform
    (50, 13, 2, 4, 8000, np.float64, True),        # sizes not multiples of 4/8/64 (scalar encode path)
    (33, 7, 4, 6, 3000, np.float32, False),
    (128, 16, 2, 3, 30000, np.float32, False),
])
def test_hip_matches_oracle_random(gvom_mod, case):
    xy, zs, buf, n_scans, n_pts, dtype, with_tf = case
    params = (0.4, 0.2, xy, zs, buf, 0.8, 0.5, 0.5, 0.3, 2.0, 2.0, 1.0, 1, 1)
    steps = _random_steps(hash(case[:5]) % 1000, n_scans, n_pts, xy * 0.4 * 0.55, zs * 0.2 * 0.5,
                          dtype, with_tf)
    got, want = _run_both(gvom_mod, params, steps)
    assert compare_records(got, want, float_tol=1e-5) > 10


def test_hip_matches_oracle_c1(gvom_mod):
    params, scans = synth.config_inputs("c1")
    steps = [("scan",) + scans[0], ("combine",)]
    got, want = _run_both(gvom_mod, params, steps)
    assert compare_records(got, want, float_tol=1e-5) > 10


def test_hip_matches_oracle_c2_full_size(gvom_mod):
    """BASELINE c2: 256x256x64 @0.2 m, OS1-64 131,072-point scan, buffer=1."""
    params, scans = synth.config_inputs("c2")
    steps = [("scan",) + scans[0], ("combine",), ("combine",)]
    got, want = _run_both(gvom_mod, params, steps, record_debug=False)
    assert compare_records(got, want, float_tol=1e-5) > 10


def _stream_against_oracle(gvom_mod, params, scans, dense_at, threads=16):
    """scan + combine per element of `scans`, HIP and oracle side by side: the returned maps are compared
    after EVERY step (ints exact, roughness 1e-5), the newest ring slot and the fused map densely at
    the steps in `dense_at` (keeps memory bounded at 256^3).  The oracle runs its all-core build (held
    to the reference's vectors by tests/test_oracle_golden.py)."""
    oracle.use_all_cores(True, threads=threads)
    try:
        g, want = gvom_mod.Gvom(*params), oracle.OracleGvom(*params)
        for k, (pc, ego, tf) in enumerate(scans):
            g.process_pointcloud(pc, ego, tf)
            want.process_pointcloud(pc, ego, tf)
            a, b = g.combine_maps(), want.combine_maps()
            assert np.array_equal(a[0], b[0])
            for i in (1, 2, 4):
                assert np.array_equal(a[i], b[i]), "step %d map %d differs" % (k, i)
            assert np.allclose(a[3], b[3], rtol=0, atol=1e-5), "step %d roughness" % k
            assert g.combined_cell_count_cpu == want.combined_cell_count_cpu
            assert (g.buffer_index, g.last_buffer_index) == (want.buffer_index, want.last_buffer_index)
            if k in dense_at:
                slot = want.last_buffer_index
                ws = scenarios.dense_from_compact(want.index_buffer[slot], want.hit_count_buffer[slot],
                                                  want.total_count_buffer[slot], want.min_height_buffer[slot])
                gs = g.read_dense(slot)
                wf = scenarios.dense_from_compact(want.combined_index_map, want.combined_hit_count,
                                                  want.combined_total_count, want.combined_min_height)
                gf = g.read_dense(gvom_mod.GVOM_WHICH_FUSED)
                for got_d, want_d, what in ((gs, ws, "slot"), (gf, wf, "fused")):
                    for j, nm in enumerate(("state", "hit", "total", "minh")):
                        assert np.array_equal(np.asarray(want_d[j]), got_d[j]), "step %d %s %s" % (k, what, nm)
    finally:
        oracle.use_all_cores(False)


def test_hip_matches_oracle_c3_ring_fills_wraps_and_evicts(gvom_mod):
    """BASELINE c3 at full size: OS1-128 262,144-point scans, buffer=8, combine after every scan, sensor
    moving 0.2 m per scan -- all 8 poses PLUS 4 more: the ring fills (scan 8 = the steady state
    BASELINE.md asks for), wraps and evicts four slots (gvom.py:163-175, 198-216, 238-274)."""
    params, scans = synth.config_inputs("c3", n_scans=12)
    _stream_against_oracle(gvom_mod, params, scans, dense_at=(7, 11))


def test_hip_matches_oracle_m256b8_ring(gvom_mod):
    """BASELINE row "M", second half (a bench.py config): 256^3 voxels, buffer=8, 11 moving scans (the
    ring wraps and evicts three slots)."""
    params, scans = synth.config_inputs("m256b8", n_scans=11)
    _stream_against_oracle(gvom_mod, params, scans, dense_at=(8, 10))


def test_hip_matches_oracle_metric_grid_256cubed(gvom_mod):
    """The headline metric grid: 256^3 voxels @0.2 m with the c2 cloud."""
    params, scans = synth.config_inputs("m256")
    steps = [("scan",) + scans[0], ("combine",)]
    got, want = _run_both(gvom_mod, params, steps, record_debug=False)
    assert compare_records(got, want, float_tol=1e-5) > 10


def test_point_order_invariance_and_conservation(gvom_mod):
    """Size-independent properties at full c2 size: shuffling the cloud changes nothing
    (integer atomics commute), sum(total) >= sum(hit) == points inside the grid that pass the
    min-distance test, visibility is 0/1."""
    params, scans = synth.config_inputs("c2")
    pc, ego, _ = scans[0]
    a = gvom_mod.Gvom(*params); b = gvom_mod.Gvom(*params)
    a.process_pointcloud(pc, ego)
    perm = np.random.default_rng(0).permutation(pc.shape[0])
    b.process_pointcloud(np.ascontiguousarray(pc[perm]), ego)
    da, db = a.read_dense(0), b.read_dense(0)
    for k in range(4):
        assert np.array_equal(da[k], db[k])
    state, hit, total, minh, origin, cells = da
    assert cells == int((state >= 0).sum()) == int((hit > 0).sum())
    st = a.scan_stats()
    assert st["sum_hit"] == int(hit.sum()) and st["cells"] == cells
    free_total = int((-state[state < -1].astype(np.int64) - 1).sum())
    assert st["sum_total"] == int(total.sum()) + free_total >= st["sum_hit"]
    d2 = (pc.astype(np.float32) ** 2).sum(1)
    assert st["sum_hit"] <= int((d2 >= 1.0).sum())
    oa, ob = a.combine_maps(), b.combine_maps()
    for x, y in zip(oa, ob):
        assert np.array_equal(x, y)
    assert set(np.unique(oa[4])) <= {0, 1}


def test_rejected_scans_leave_ring_untouched(gvom_mod, capsys):
    g = gvom_mod.Gvom(0.4, 0.4, 16, 8, 2, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
    assert g.combine_maps() is None
    assert "[WARNING] The map buffer is empty, nothing will happen!" in capsys.readouterr().out
    rng = np.random.default_rng(0)
    pc = np.stack([rng.uniform(-3, 3, 300), rng.uniform(-3, 3, 300), rng.uniform(-1.5, .5, 300)], 1)
    g.process_pointcloud(pc, (0, 0, 0), np.eye(4))
    before = g.read_dense(0)
    g.process_pointcloud(np.zeros((0, 3)), (0, 0, 0))
    assert "[WARNING] Processing an empty pointcloud, nothing will happen!" in capsys.readouterr().out
    g.process_pointcloud(np.full((5, 3), 400.0), (0.1, 0, 0))
    assert "[WARNING] The pointcloud points don't overlap with any voxels, nothing will happen!" \
        in capsys.readouterr().out
    assert g.buffer_index == 1 and g.last_buffer_index == 0
    after = g.read_dense(0)
    for k in range(4):
        assert np.array_equal(before[k], after[k])
    assert g.read_dense(1) is None
    out = g.combine_maps()
    assert [o.dtype for o in out] == [np.float64, np.int32, np.int32, np.float64, np.int32]
    assert np.count_nonzero(out[1]) == 207 and out[4].sum() == 250          # SURVEY App. C smoke
    assert out[3].min() == pytest.approx(-7.333893209065674, abs=1e-5)


def test_strided_and_extra_column_clouds(gvom_mod):
    """(N,4) float32 rows (x,y,z,intensity) and non-contiguous views must equal the packed cloud."""
    params = (0.4, 0.2, 32, 16, 1, 0.5, 0.5, 0.5, 0.3, 2.0, 2.0, 1.0, 1, 1)
    rng = np.random.default_rng(9)
    base = rng.uniform(-5, 5, (4000, 3)).astype(np.float32); base[:, 2] *= 0.2
    xyzi = np.concatenate([base, rng.uniform(0, 1, (4000, 1)).astype(np.float32)], axis=1)
    outs = []
    for pc in (base, xyzi, np.asfortranarray(base), xyzi[:, :3]):
        g = gvom_mod.Gvom(*params)
        g.process_pointcloud(pc, (0.2, 0.1, 0.0))
        outs.append(g.read_dense(0))
    for o in outs[1:]:
        for k in range(4):
            assert np.array_equal(outs[0][k], o[k])


def test_hip_matches_oracle_c4_at_baseline_settings(gvom_mod):
    """BASELINE c4 as BASELINE.md section 3 states it, on one GPU: 512 x 512 x 128 voxels (33.5 M), buffer=4, the
    1,048,576-point cloud of four interleaved OS1-128-shaped sensors, SEVEN scans with a moving ego and a combine
    after each -- the ring fills at scan 4, wraps at scan 5 and evicts three slots (gvom.py:163-175, 198-274).
    Returned maps, cell counts and ring indices against the all-core oracle at every step; the newest slot and
    the fused map densely at the wrap step and at the end."""
    params, scans = synth.config_inputs("c4", n_scans=7)
    assert params[2:5] == (512, 128, 4) and scans[0][0].shape[0] == 1048576
    _stream_against_oracle(gvom_mod, params, scans, dense_at=(4, 6))


def _free_ram_gb():
    try:
        with open("/proc/meminfo") as f:
            for line in f:
                if line.startswith("MemAvailable:"):
                    return int(line.split()[1]) / 1048576.0
    except OSError:
        pass
    return 0.0


def test_hip_matches_oracle_c5_one_tick(gvom_mod):
    """BASELINE c5's real tick against the oracle ("feasible for one or two ticks on the 128-core box"):
    1024 x 1024 x 128 voxels (134 M), buffer=8, the 4,194,304-point cloud of 16 interleaved sensors; one scan and
    one combine.  Compared with the all-core oracle: the four returned maps, the fused cell count, sum(hit) and
    sum(total) of the scan, and the newest ring slot densely (state classes, hit, total, min-height: 4 x 537 MB per
    side, hence the memory gate).  The six-tick moving-window properties are in the test below."""
    if _free_ram_gb() < 24.0:
        pytest.skip("needs 24 GB of free host memory for the dense compare at 134 M voxels")
    params, scans = synth.config_inputs("c5", n_scans=1)
    pc, ego, tf = scans[0]
    assert params[2:5] == (1024, 128, 8) and pc.shape[0] == 4194304
    oracle.use_all_cores(True, threads=32)
    try:
        g, want = gvom_mod.Gvom(*params), oracle.OracleGvom(*params)
        g.process_pointcloud(pc, ego, tf)
        want.process_pointcloud(pc, ego, tf)
        a, b = g.combine_maps(), want.combine_maps()
        assert np.array_equal(a[0], b[0])
        for i in (1, 2, 4):
            assert np.array_equal(a[i], b[i]), "map %d differs" % i
        assert np.allclose(a[3], b[3], rtol=0, atol=1e-5)
        assert g.combined_cell_count_cpu == want.combined_cell_count_cpu
        slot = want.last_buffer_index
        ws = scenarios.dense_from_compact(want.index_buffer[slot], want.hit_count_buffer[slot],
                                          want.total_count_buffer[slot], want.min_height_buffer[slot])
        gs = g.read_dense(slot)
        for j, nm in enumerate(("state", "hit", "total", "minh")):
            assert np.array_equal(np.asarray(ws[j]), gs[j]), "slot " + nm
        st = g.scan_stats()
        assert st["sum_hit"] == int(np.asarray(ws[1], np.int64).sum())
        free_total = int((-np.asarray(ws[0])[np.asarray(ws[0]) < -1].astype(np.int64) - 1).sum())
        assert st["sum_total"] == int(np.asarray(ws[2], np.int64).sum()) + free_total
    finally:
        oracle.use_all_cores(False)


def test_concurrent_scan_and_combine_threads(gvom_mod):
    """gvom_ros.py calls process_pointcloud from lidar threads while a timer thread calls
    combine_maps (README.md:49).  Hammer one handle from three threads; every combine must return
    a self-consistent tuple, and the final state must equal a serial replay of the same scans
    (commit order is the order in which process_pointcloud calls returned)."""
    import threading
    params = (0.4, 0.2, 64, 32, 4) + synth.REF_TAIL
    rng = np.random.default_rng(3)
    clouds = [np.stack([rng.uniform(-10, 10, 20000), rng.uniform(-10, 10, 20000),
                        rng.normal(-0.8, 0.6, 20000)], 1).astype(np.float32) for _ in range(6)]
    g = gvom_mod.Gvom(*params)
    order, lock, errors = [], threading.Lock(), []

    def lidar(ids):
        try:
            for i in ids:
                with lock:                       # serialise call+record so the commit order is known
                    g.process_pointcloud(clouds[i], (0.0, 0.0, 0.0))
                    order.append(i)
        except Exception as e:                   # pragma: no cover
            errors.append(e)

    def timer():
        try:
            for _ in range(20):
                out = g.combine_maps()
                if out is not None:
                    assert out[1].shape == (64, 64) and set(np.unique(out[4])) <= {0, 1}
        except Exception as e:                   # pragma: no cover
            errors.append(e)

    ts = [threading.Thread(target=lidar, args=([0, 2, 4],)), threading.Thread(target=lidar, args=([1, 3, 5],)),
          threading.Thread(target=timer)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    ref = gvom_mod.Gvom(*params)
    for i in order:
        ref.process_pointcloud(clouds[i], (0.0, 0.0, 0.0))
    for slot in range(4):
        a, b = g.read_dense(slot), ref.read_dense(slot)
        assert (a is None) == (b is None)
        if a is not None:
            for k in range(4):
                assert np.array_equal(a[k], b[k])


def test_trace_exact_zero_and_tiny_negative_coordinates(gvom_mod):
    """k_trace looks voxels up with integer arithmetic; the reference's floor((f64)p - origin) rounds
    a coordinate just below zero UP (gvom.py:1121-1133).  Sensor exactly at the world origin with
    rays whose off-axis slopes are 0, +-1e-17 and +-1e-30 (what sin(pi) gives a lidar driver)."""
    params = (0.2, 0.2, 64, 32, 2) + synth.REF_TAIL
    rng = np.random.default_rng(11)
    base = []
    for r in (2.0, 3.7, 5.1):
        for t in (0.0, 1e-17, -1e-17, 1e-30, -1e-30, 1e-9, -1e-9):
            base += [(r, t, 0.3), (-r, t, -0.2), (t, r, 0.1), (t, -r, t), (r, r * t, t), (-r, -r, t)]
    pc = np.asarray(base, dtype=np.float64)
    pc = np.concatenate([pc, rng.uniform(-6, 6, (3000, 3)) * np.array([1, 1, 0.3])])
    steps = [("scan", pc, (0.0, 0.0, 0.0), None), ("combine",),
             ("scan", pc.astype(np.float32), (-1e-12, 1e-20, -0.0), None), ("combine",)]
    got, want = _run_both(gvom_mod, params, steps)
    assert compare_records(got, want, float_tol=1e-5) > 20


def test_trace_far_origin_uses_f64_lookup(gvom_mod):
    """|origin| >= 2^30 voxels: the integer voxel lookup is not used (gvom_capi.hip selects the
    f64 variant); results still match the oracle."""
    params = (0.2, 0.2, 64, 32, 1) + synth.REF_TAIL
    ego = (2.5e8, -2.5e8, 3.0)
    rng = np.random.default_rng(5)
    pc = rng.uniform(-5, 5, (4000, 3)) * np.array([1, 1, 0.3]) + np.asarray(ego)
    steps = [("scan", pc, ego, None), ("combine",)]
    got, want = _run_both(gvom_mod, params, steps)
    assert compare_records(got, want, float_tol=1e-5) > 10


@pytest.mark.parametrize("res", [(0.2, 0.2), (0.4, 0.2), (0.1, 0.1), (1.0 / 3.0, 0.07), (0.25, 0.5), (1.0, 1.0), (0.3, 0.15), (0.123456789, 0.987654321)])
def test_division_by_the_resolution_through_the_verified_reciprocal(gvom_mod, res):
    """k_trace divides every float32 coordinate by xy_resolution / z_resolution (gvom.py:1072-1080, 1101-1103).  The library does
    it with the host's r = RN(1 / d) and two fused multiply-adds (q = x r; e = fma(-q, d, x); fma(e, r, q)) after gvom_create
    has checked on the host that this IS the IEEE quotient for all 2^23 float32 significands -- the rounding depends on nothing
    else -- and with the divide otherwise ("fastdiv" knob 0: always the divide).  Both forms and the oracle (which divides) on
    clouds that sit on the edges: returns on voxel faces (quotients that are integers, or one ulp off), huge, tiny, denormal,
    zero, negative-zero and non-finite coordinates, an ego off the origin; float64 clouds take the divide in either setting."""
    xy_res, z_res = res
    params = (xy_res, z_res, 48, 24, 1, 0.0, 0.5, 0.5, 0.3, 2.0, 2.0, 1.0, 1, 1)
    rng = np.random.default_rng(int(xy_res * 1e6) + 17)
    half = np.array([24 * xy_res, 24 * xy_res, 12 * z_res])
    steps = []
    for k in range(3):
        ego = tuple(float(v) for v in rng.uniform(-2, 2, 3) * np.array([1, 1, 0.1]))
        n = 20000
        body = rng.uniform(-1.3, 1.3, (n, 3)) * half + np.array(ego)
        faces = np.round(rng.uniform(-1, 1, (4000, 3)) * half / np.array([xy_res, xy_res, z_res])) * np.array([xy_res, xy_res, z_res])
        near = faces * (1.0 + rng.choice([-1, 1], (4000, 1)) * 2.0 ** -rng.integers(18, 25, (4000, 1)))   # an ulp or so off a face
        odd = np.array([[0.0, 0.0, 0.0], [-0.0, 0.0, -0.0], [1e-42, -1e-42, 1e-45], [3e38, 1.0, 1.0], [-3e38, 3e38, -3e38],
                        [np.inf, 0.5, 0.5], [0.5, -np.inf, 0.5], [1e-20, 1e-30, -1e-38]])   # (NaN returns: test_non_finite_returns_have_no_effect)
        pc = np.concatenate([body, faces, near, odd], 0).astype(np.float32 if k < 2 else np.float64)
        steps += [("scan", pc, ego, None), ("combine",)]
    sc = {"params": params, "steps": steps}
    want = scenarios.run_and_record(oracle.OracleGvom, sc)
    made = []

    def knob(v):
        def make(*p):
            g = gvom_mod.Gvom(*p, voxel_statistics=False)
            g.set_tuning("fastdiv", v)
            made.append(g)
            return g
        return make
    recs = [scenarios.run_and_record(knob(v), sc) for v in (-1, 0)]
    with np.errstate(invalid="ignore"):
        for got in recs:
            assert compare_records(got, want, float_tol=1e-5) > 10
    for key in recs[0]:
        a, b = np.asarray(recs[0][key]), np.asarray(recs[1][key])
        assert a.shape == b.shape and (np.array_equal(a, b, equal_nan=True) if a.dtype.kind in "fiub" else True), key
    # every resolution of this list passes the host's check (it is a property of the divisor; 1.0 trivially so)
    assert made[0].get_tuning("fastdiv") == 3 and made[1].get_tuning("fastdiv") == 0


def test_trace_tuning_knobs_leave_results_unchanged(gvom_mod):
    """k_trace splits every ray into step segments handled by different waves (set-up + replay of the
    earlier steps + the segment's own steps); the segment count, the flush period of a wave's LDS line
    cache, the dispatch row of the endpoint blocks and the waves' issue priorities are performance knobs
    (gvom_set_tuning) and must leave bit-identical scan slots.  segs=1 is the unsegmented walk, segs=9 / period=1 the extremes."""
    params, scans = synth.config_inputs("c2", n_scans=2)
    ref = None
    # (+ prio: steps per issue-priority level of a wave's remaining work; 0 = the hardware's default arbitration)
    for segs, period, ep_row, prio in ((0, 0, -2, -1), (1, 12, 0, 0), (2, 1, 1, 8), (3, 32, 3, 1), (6, 12, 6, 0), (9, 5, 4, 3),
                                       (5, 16, -1, 100), (1, 7, -1, 8)):
        g = gvom_mod.Gvom(*params)
        g.set_tuning("segs", segs); g.set_tuning("period", period); g.set_tuning("ep_row", ep_row); g.set_tuning("prio", prio)
        slots = []
        for pc, ego, tf in scans:
            g.process_pointcloud(pc, ego, tf)
            b = g.last_buffer_index
            slots.append(scenarios.dense_from_compact(scenarios.host(g.index_buffer[b]), scenarios.host(g.hit_count_buffer[b]),
                                                      scenarios.host(g.total_count_buffer[b]), scenarios.host(g.min_height_buffer[b])))
        if ref is None:
            ref = slots
        else:
            for a, b_ in zip(ref, slots):
                for x, y in zip(a, b_):
                    assert np.array_equal(x, y), "segs %d / period %d / ep_row %d / prio %d differs" % (segs, period, ep_row, prio)


def test_sub_cloud_interleave_leaves_results_unchanged(gvom_mod):
    """gvom_set_tuning("interleave", K): lane l of bundle b traces return (p mod K) * (n / K) + p / K, p = 64 b + l -- the K
    sub-clouds of a multi-sensor cloud side by side in one wave.  A permutation of who traces which return: scan slots are
    bit-identical for every K (a K that does not divide n, is no power of two or exceeds 64 is ignored), with and without the
    other knobs, for float64 clouds with a transform, and for the cloud it is meant for (4 sensors interleaved in azimuth)."""
    params, scans = synth.config_inputs("c2", n_scans=2)
    ragged = [(pc[:-37], ego, tf) for pc, ego, tf in scans]                  # n = 131,035 = 5 * 73 * 359: only K = 1 divides it
    f64 = [(pc.astype(np.float64), ego, scenarios.rot_z(0.01, (0.1, 0.0, 0.0))) for pc, ego, tf in scans]
    p4, multi = synth.config_inputs("c4", n_scans=1)
    p4 = (0.4, 0.4, 128, 32) + p4[4:]                                        # the 4-sensor cloud in a grid the test can densify
    for prm, clouds, settings in ((params, scans, ((1, 0), (2, 0), (4, 12), (16, 16), (64, 5), (3, 0), (128, 0))),
                                  (params, ragged, ((1, 0), (4, 0), (64, 0))),
                                  (params, f64, ((1, 0), (8, 0))),
                                  (p4, multi, ((1, 0), (4, 0), (16, 12)))):
        ref = None
        for K, period in settings:
            g = gvom_mod.Gvom(*prm)
            g.set_tuning("interleave", K); g.set_tuning("period", period)
            slots = []
            for pc, ego, tf in clouds:
                g.process_pointcloud(pc, ego, tf)
                b = g.last_buffer_index
                slots.append(scenarios.dense_from_compact(scenarios.host(g.index_buffer[b]), scenarios.host(g.hit_count_buffer[b]),
                                                          scenarios.host(g.total_count_buffer[b]), scenarios.host(g.min_height_buffer[b])))
            maps = g.combine_maps()
            if ref is None:
                ref = (slots, maps)
            else:
                for a, b_ in zip(ref[0], slots):
                    for x, y in zip(a, b_):
                        assert np.array_equal(x, y), "interleave %d / period %d differs" % (K, period)
                for x, y in zip(ref[1], maps):
                    assert np.array_equal(x, y), "interleave %d: returned maps differ" % K


def test_layout_probe_finds_interleaved_sensors_and_nothing_else(gvom_mod):
    """Automatic interleave (the default): a one-wave probe kernel in front of k_trace looks at the second cloud of a length (and
    every 32nd after it) and the NEXT clouds of as many returns are traced accordingly (clouds whose length changes from scan to
    scan are not looked at for sub-clouds).  It must find the 4 sensors of the c4 cloud (and the sensor groups of a 16-sensor one), must not find
    structure in a single sensor's scan or in random points, forgets its answer when the cloud's length changes -- and whatever
    it answers, the slots equal those of a mapper with the interleave switched off."""
    p4, multi = synth.config_inputs("c4", n_scans=2)
    p4 = (0.4, 0.4, 128, 32) + p4[4:]
    pc2, single = synth.config_inputs("c2", n_scans=2)
    rnd = [(synth.uniform_cloud(65536, 7 + k, (-20, 20), (-20, 20), (-3, 3), np.float32), (0.1 * k, 0.0, 0.0), None) for k in range(2)]
    f64tf = [(pc.astype(np.float64), ego, scenarios.rot_z(0.3, (0.0, 0.0, 0.0))) for pc, ego, tf in multi]
    for prm, clouds, want in ((p4, multi, 4), (pc2, single, 1), (p4, rnd, 1), (p4, f64tf, 4)):
        g, off = gvom_mod.Gvom(*prm), gvom_mod.Gvom(*prm)
        off.set_tuning("interleave", 1)
        used = []
        for pc, ego, tf in clouds + [clouds[0], (clouds[0][0][:-64], clouds[0][1], clouds[0][2])]:
            for m in (g, off):
                m.process_pointcloud(pc, ego, tf)
            used.append(g.get_tuning("interleave"))
            assert off.get_tuning("interleave") == 1
            a, b = [scenarios.dense_from_compact(*[scenarios.host(getattr(m, n)[m.last_buffer_index]) for n in
                    ("index_buffer", "hit_count_buffer", "total_count_buffer", "min_height_buffer")]) for m in (g, off)]
            for x, y in zip(a, b):
                assert np.array_equal(x, y)
        # first cloud: nothing known; second (the same length: stable, the probe runs in front of it); third: the probe's answer;
        # fourth (another length): forgotten
        assert used == [1, 1, want, 1], (used, want)


@pytest.mark.parametrize("pct", [10, 25, 40])
def test_layout_probe_is_stable_on_the_clouds_a_real_node_delivers(gvom_mod, pct):
    """synth m256_d*: an OS1-64-like sensor with non-uniform beam elevations and staggered beam columns, 10 / 25 / 40 % of its
    returns removed BEFORE the call (what ros_numpy's xyz array is, gvom_ros.py:108), the length changing with every scan.  The
    layout probe (every 8th scan of a stream of changing lengths) must keep ONE verdict for the stream -- the survivors are still in
    beam-major order, which the trace takes as it is: no directional sort, no sub-cloud interleave, and above all no flapping
    between modes on consecutive scans (each flip would change the trace's cost by a factor; results never change).  Not a
    timing test.  The maps of the stream equal those of the same clouds traced in forced directional order."""
    params, scans = synth.config_inputs("m256_d%d" % pct, n_scans=12)
    params = params[:3] + (64,) + params[4:]                   # (a flatter grid: the same rays, a quicker test)
    g, f = gvom_mod.Gvom(*params), gvom_mod.Gvom(*params)
    f.set_tuning("dirsort", 2)
    assert len({pc.shape[0] for pc, _, _ in scans}) > 6
    modes, ilv = [], []
    for k in range(60):
        pc, ego, tf = scans[k % len(scans)]
        g.process_pointcloud(pc, ego, tf); f.process_pointcloud(pc, ego, tf)
        modes.append(g.get_tuning("dirsort")); ilv.append(g.get_tuning("interleave"))
        if k % 6 == 5:
            for a, b in zip(g.combine_maps(), f.combine_maps()):
                assert np.array_equal(a, b)
    assert f.get_tuning("dirsort") == 2
    assert sum(1 for a, b in zip(modes, modes[1:]) if a != b) == 0 and modes[-1] == 0, modes
    assert set(ilv) == {1}, ilv


def test_directional_order_of_unordered_clouds_leaves_results_unchanged(gvom_mod):
    """Clouds in no spatial order (BASELINE c1: uniformly random points) are traced in DIRECTIONAL order: a counting sort by
    direction bin seen from the sensor (k_dirbin_*: 6 cube faces x 16 x 16 cells, or 256 elevation rows x 32 azimuth sectors for
    clouds whose bundles are vertical fans) in front of k_trace, so that a wave's 64 rays share accumulator lines --
    gvom_set_tuning("dirsort", 1 | 2) forces a mode, -1 forbids it, 0 (default) takes the layout probe's verdict on the previous
    cloud of the same length.  A permutation of who traces which return: scan slots, fused maps and
    returned maps are bit-identical with and without it -- random clouds, float64 + transform, ragged lengths, non-finite and
    far-away returns, clouds below the sort's minimum, a one-slot ring (eager fusion) and a ring of three; and the probe
    finds c1's cloud scattered and a lidar's scan ordered."""
    params1, scans1 = synth.config_inputs("c1")
    rng = np.random.default_rng(4)
    c1 = scans1[0][0]
    odd = np.concatenate([c1[:12345].astype(np.float32), np.array([[np.nan, 0, 0], [np.inf, 1, 1], [1e9, -1e9, 3.0], [0.3, -0.2, 0.1]], np.float32)], 0)
    tiny = c1[:100].astype(np.float32)
    cases = [(params1, [(c1, scans1[0][1], None), (c1[::-1].copy(), (0.7, -0.2, 0.1), scenarios.rot_z(0.2, (0.1, 0.0, 0.0))), (odd, (0.3, -0.2, 0.1), None), (tiny, (0.3, -0.2, 0.1), None)]),
             (params1[:4] + (3,) + params1[5:], [(c1[:30000].astype(np.float32), (0.2 * k, 0.1 * k, 0.0), None) for k in range(4)])]
    for params, clouds in cases:
        rec = {}
        for mode in (-1, 1, 2):                             # off / cube cells / elevation rows
            g = gvom_mod.Gvom(*params)
            g.set_tuning("dirsort", mode)
            out = []
            for pc, ego, tf in clouds:
                g.process_pointcloud(pc, ego, tf)
                assert g.get_tuning("dirsort") == (mode if mode > 0 and pc.shape[0] >= 256 else 0)
                b = g.last_buffer_index
                out.append(scenarios.dense_from_compact(scenarios.host(g.index_buffer[b]), scenarios.host(g.hit_count_buffer[b]),
                                                        scenarios.host(g.total_count_buffer[b]), scenarios.host(g.min_height_buffer[b])))
                out.append(g.combine_maps())
                out.append(g.read_dense(gvom_mod.GVOM_WHICH_FUSED))
            rec[mode] = out
        for other in (1, 2):
            for a, b in zip(rec[-1], rec[other]):
                for x, y in zip(a, b):
                    assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)
    # the probe: c1's cloud is scattered (the third scan of that length runs sorted), an OS1-64 scan is not
    g = gvom_mod.Gvom(*params1)
    seen = []
    for k in range(4):
        g.process_pointcloud(c1, scans1[0][1]); seen.append(g.get_tuning("dirsort"))
    assert seen[0] == 0 and seen[-1] == 1, seen
    # a stream of unordered clouds whose length changes every scan (invalid returns dropped) is probed every 8th scan and sorted too
    gv = gvom_mod.Gvom(*params1)
    seen = []
    for k in range(20):
        gv.process_pointcloud(c1[:45000 + 137 * k], scans1[0][1]); seen.append(gv.get_tuning("dirsort"))
    assert seen[0] == 0 and seen[-1] == 1 and sum(seen) >= 8, seen
    p2, lidar = synth.config_inputs("c2", n_scans=1)
    g2 = gvom_mod.Gvom(*p2)
    for k in range(4):
        g2.process_pointcloud(*lidar[0])
        assert g2.get_tuning("dirsort") == 0
    # ... and the SAME scan in azimuth-major ("firing") order -- every beam of one azimuth behind one another, a bundle a vertical
    # fan -- is re-ordered as well, with the beam-major scan's maps
    pc, ego, tf = lidar[0]
    firing = np.ascontiguousarray(pc.reshape(64, 2048, 3).transpose(1, 0, 2).reshape(-1, 3))
    g3 = gvom_mod.Gvom(*p2)
    seen = []
    for k in range(4):
        g3.process_pointcloud(firing, ego, tf); seen.append(g3.get_tuning("dirsort"))
    assert seen[0] == 0 and seen[-1] == 2, seen             # (elevation rows: the beam-major fans come back)
    a, b = g2.combine_maps(), g3.combine_maps()
    for i in range(5):
        assert np.array_equal(a[i], b[i], equal_nan=True), i


@pytest.mark.parametrize("occ_params", [(50, -10, 0), (12.5, -6.0, 1.5)])
def test_combine_maps_occupancy_matches_node_postprocessing(gvom_mod, occ_params):
    """combine_maps_occupancy() == the ROS node's numpy post-processing
    (gvom_ros.py:141-165, restated in oracle.ros_occupancy_grids) of combine_maps()'s result, bit for
    bit, while the map state advances identically (previous-map carry over three combines)."""
    params, scans = synth.config_inputs("c2", n_scans=3)
    params = params[:4] + (2,) + params[5:]
    a, b = gvom_mod.Gvom(*params), gvom_mod.Gvom(*params)
    assert b.combine_maps_occupancy(*occ_params) is None
    for pc, ego, tf in scans:
        a.process_pointcloud(pc, ego, tf)
        b.process_pointcloud(pc, ego, tf)
        maps = a.combine_maps()
        got = b.combine_maps_occupancy(*occ_params)
        want = oracle.ros_occupancy_grids(maps, *occ_params)
        assert np.array_equal(got[0], maps[0])
        for name, g, w in zip(("hard", "soft", "certainty", "negative", "roughness"), got[1:], want):
            assert g.dtype == np.int8 and g.shape == w.shape
            assert np.array_equal(g, w), "%s grid differs in %d cells" % (name, int(np.sum(g != w)))
    assert a.combined_cell_count_cpu == b.combined_cell_count_cpu
    # a small odd-sized grid with a transform as well
    params2 = (0.4, 0.2, 50, 13, 2, 0.8, 0.5, 0.5, 0.3, 2.0, 2.0, 1.0, 1, 1)
    a, b = gvom_mod.Gvom(*params2), gvom_mod.Gvom(*params2)
    for st in _random_steps(3, 3, 6000, 50 * 0.4 * 0.55, 13 * 0.2 * 0.5, np.float64, True):
        if st[0] == "scan":
            a.process_pointcloud(*st[1:]); b.process_pointcloud(*st[1:])
        else:
            maps = a.combine_maps()
            got = b.combine_maps_occupancy(*occ_params)
            for g, w in zip(got[1:], oracle.ros_occupancy_grids(maps, *occ_params)):
                assert np.array_equal(g, w)


@pytest.mark.parametrize("name", ["f3", "f4", "f5"])
def test_combine_maps_occupancy_matches_the_reference_node_golden(gvom_mod, name):
    """combine_maps_occupancy() against what the reference's own ROS node published (tests/golden/ros_f3.npz, recorded
    from the unmodified VoxelMapper.cb_timer, gvom_ros.py:113-165) for the scenarios F3 / F4 / F5: the HIP mapper
    replays the scenario's scans and every combine must hand back the node's five int8 grids, under the node's
    default parameters and under a second set (two mappers: a combine advances the map)."""
    ros = np.load(os.path.join(G, "ros_f3.npz"))
    sc = scenarios.scenario_from_record(np.load(os.path.join(G, name + ".npz")))
    for p in ros["param_sets"]:
        thr = (float(ros[p + "_density_threshold"]), float(ros[p + "_min_roughness"]), float(ros[p + "_max_roughness"]))
        g = gvom_mod.Gvom(*sc["params"])
        checked = 0
        for k, st in enumerate(sc["steps"]):
            if st[0] == "scan":
                g.process_pointcloud(*st[1:])
                continue
            got = g.combine_maps_occupancy(*thr)
            tag = "%s_s%d" % (name, k)
            if got is None:
                assert tag not in ros["tags"]
                continue
            assert np.array_equal(got[0][:2], ros["%s_%s_origin_xy" % (p, tag)])
            for short, a in zip(("hard", "soft", "certainty", "negative", "roughness"), got[1:]):
                w = ros["%s_%s_%s" % (p, tag, short)]
                assert a.dtype == np.int8 and np.array_equal(a, w), (p, tag, short, int(np.sum(a != w)))
            checked += 1
        assert checked >= 1


def test_c_entry_combine_maps_fills_caller_buffers_row_major(gvom_mod):
    """include/gvom_hip.h gvom_combine_maps(): the plain C entry a non-Python host binds (caller-owned
    buffers, maps in row-major [x][y] order -- k_map2d's transposing variant) returns the same maps as
    Gvom.combine_maps() (pinned zero-copy buffers, column-major variant), which the tests above hold
    to the golden vectors and the oracle; a grid whose size is no multiple of the 32 x 8 tile as well."""
    import ctypes
    for params, n_pts in (((0.2, 0.2, 128, 32, 2, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1), 40000),
                          ((0.4, 0.2, 50, 13, 2, 0.8, 0.5, 0.5, 0.3, 2.0, 2.0, 1.0, 1, 1), 6000)):
        xy = params[2]
        a, b = gvom_mod.Gvom(*params), gvom_mod.Gvom(*params)
        L = b._lib
        for st in _random_steps(5, 3, n_pts, xy * params[0] * 0.55, params[3] * params[1] * 0.5, np.float32, True):
            if st[0] == "scan":
                a.process_pointcloud(*st[1:]); b.process_pointcloud(*st[1:])
                continue
            want = a.combine_maps()
            origin = np.full(3, np.nan)
            pos = np.full((xy, xy), -7, np.int32); neg = np.full((xy, xy), -7, np.int32)
            vis = np.full((xy, xy), -7, np.int32); rough = np.full((xy, xy), np.nan)
            rc = L.gvom_combine_maps(b._h, origin.ctypes.data_as(ctypes.c_void_p), pos.ctypes.data_as(ctypes.c_void_p),
                                     neg.ctypes.data_as(ctypes.c_void_p), rough.ctypes.data_as(ctypes.c_void_p),
                                     vis.ctypes.data_as(ctypes.c_void_p))
            assert rc == gvom_mod.GVOM_OK
            assert np.array_equal(origin, want[0])
            for name, g, w in (("positive", pos, want[1]), ("negative", neg, want[2]), ("visibility", vis, want[4])):
                assert np.array_equal(g, w), "%s differs in %d cells" % (name, int(np.sum(g != w)))
            assert np.array_equal(rough, want[3]), "roughness differs"
        assert a.combined_cell_count_cpu == b.combined_cell_count_cpu


def test_output_buffers_of_the_callers_own_must_be_coherent_pinned_memory(gvom_mod):
    """gvom_combine_maps_into with a buffer that is not from gvom_output_buffer_alloc: accepted iff it is coherent, device-mapped
    pinned memory (the completion flag is only ordered behind the maps for write-through stores, include/gvom_hip.h)
    -- a non-coherent pinned buffer and plain host memory are refused with GVOM_ERR_INVALID and a message, nothing is launched
    into them, and the mapper goes on working."""
    import ctypes
    rt = ctypes.CDLL("libamdhip64.so")
    rt.hipHostMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_uint]
    rt.hipHostFree.argtypes = [ctypes.c_void_p]
    params = (0.4, 0.2, 32, 16, 1, 0.5, 0.5, 0.5, 0.3, 2.0, 2.0, 1.0, 1, 1)
    g = gvom_mod.Gvom(*params)
    rng = np.random.default_rng(3)
    pc = np.stack([rng.uniform(-5, 5, 3000), rng.uniform(-5, 5, 3000), rng.normal(-0.6, 0.2, 3000)], 1).astype(np.float32)
    g.process_pointcloud(pc, (0.0, 0.0, 0.0))
    want = g.combine_maps()
    n2 = 32 * 32
    origin = (ctypes.c_double * 3)()
    good, bad = ctypes.c_void_p(), ctypes.c_void_p()
    assert rt.hipHostMalloc(ctypes.byref(good), n2 * 20, 0x2 | 0x40000000) == 0            # mapped | coherent
    assert rt.hipHostMalloc(ctypes.byref(bad), n2 * 20, 0x2 | 0x80000000) == 0             # mapped | NON-coherent
    plain = np.zeros(n2 * 20, np.uint8)
    try:
        g.process_pointcloud(pc, (0.0, 0.0, 0.0))
        assert g._lib.gvom_combine_maps_into(g._h, origin, bad) == gvom_mod.GVOM_ERR_INVALID
        assert b"coherent" in g._lib.gvom_last_error(g._h)
        assert g._lib.gvom_combine_maps_into(g._h, origin, plain.ctypes.data_as(ctypes.c_void_p)) == gvom_mod.GVOM_ERR_INVALID
        assert g._lib.gvom_combine_maps_into(g._h, origin, good) == gvom_mod.GVOM_OK      # (the refused calls changed nothing)
        pos = np.ctypeslib.as_array(ctypes.cast(good, ctypes.POINTER(ctypes.c_int32)), (n2,)).reshape(32, 32).T
        again = g.combine_maps()
        assert int(pos.sum()) > 0 and again is not None
    finally:
        g._check(g._lib.gvom_sync(g._h))
        rt.hipHostFree(good); rt.hipHostFree(bad)
    assert want is not None


def _pointcloud2_bytes(xyz32, point_step, offsets, seed):
    """Packed PointCloud2 data: x, y, z float32 at `offsets`, the other bytes random (intensity, ring,
    timestamps ...), a few records with NaN / inf coordinates as real drivers emit."""
    rng = np.random.default_rng(seed)
    n = xyz32.shape[0]
    raw = rng.integers(0, 256, (n, point_step), dtype=np.uint8)
    pts = xyz32.copy()
    bad = rng.choice(n, size=max(3, n // 200), replace=False)
    pts[bad[0::3], 0] = np.nan; pts[bad[1::3], 1] = np.inf; pts[bad[2::3], 2] = -np.inf
    for k, off in enumerate(offsets):
        raw[:, off:off + 4] = pts[:, k:k + 1].copy().view(np.uint8)
    return raw.tobytes()


@pytest.mark.parametrize("layout", [(16, (0, 4, 8)), (48, (0, 4, 8)), (32, (12, 4, 20))])
def test_pointcloud2_ingest_matches_ros_numpy_path(gvom_mod, layout):
    """process_pointcloud2(raw PointCloud2 bytes) == process_pointcloud(
    ros_numpy.pointcloud2_to_xyz_array(msg)) -- the float64 array without the non-finite records,
    restated in oracle.pointcloud2_to_xyz_array -- on the HIP path AND against the CPU oracle;
    with the node's tf matrix (quaternion + translation, gvom_ros.py:93-105)."""
    point_step, offs = layout
    params = (0.4, 0.2, 64, 32, 2) + synth.REF_TAIL
    tf = gvom_mod.transform_from_translation_rotation((0.3, -0.2, 0.1), (0.01, -0.02, 0.38, 0.92))
    assert np.allclose(tf[:3, :3] @ tf[:3, :3].T, np.eye(3), atol=1e-12) and tf[3].tolist() == [0, 0, 0, 1]
    g2, g1, want = gvom_mod.Gvom(*params), gvom_mod.Gvom(*params), oracle.OracleGvom(*params)
    rng = np.random.default_rng(17)
    for k in range(3):
        ego = (0.5 * k, -0.3 * k, 0.05 * k)
        xyz = (rng.uniform(-12, 12, (20000, 3)) * np.array([1, 1, 0.25])).astype(np.float32)
        data = _pointcloud2_bytes(xyz, point_step, offs, 100 + k)
        pc = oracle.pointcloud2_to_xyz_array(data, xyz.shape[0], point_step, offs)
        assert pc.dtype == np.float64 and pc.shape[0] < xyz.shape[0]
        g2.process_pointcloud2(data, xyz.shape[0], point_step, offs, ego, tf)
        g1.process_pointcloud(pc, ego, tf)
        want.process_pointcloud(pc, ego, tf)
        b = g2.last_buffer_index
        slot = lambda g: scenarios.dense_from_compact(*[scenarios.host(x) for x in (
            g.index_buffer[b], g.hit_count_buffer[b], g.total_count_buffer[b], g.min_height_buffer[b])])
        for u, v in zip(slot(g2), slot(g1)):
            assert np.array_equal(u, v)
        m2, m1, mo = g2.combine_maps(), g1.combine_maps(), want.combine_maps()
        for u, v, w in zip(m2, m1, mo):
            assert np.array_equal(u, v)
            assert np.allclose(u, w, rtol=0, atol=1e-5)
        assert np.array_equal(m2[1], mo[1]) and np.array_equal(m2[2], mo[2]) and np.array_equal(m2[4], mo[4])


def test_c5_full_size_properties(gvom_mod):
    """BASELINE c5's grid and cloud on one GPU (1024x1024x128 = 134 M voxels, 4,194,304 points from
    16 interleaved OS1-128-shaped sensors): too large for the CPU oracle, so size-independent
    properties -- point-order invariance of every per-voxel count and every returned map, count
    conservation, and agreement of the PointCloud2 ingest (f64 computation) with the same cloud
    passed as float64."""
    params = (0.2, 0.2, 1024, 128, 1) + synth.REF_TAIL     # (one slot: this test is about one scan's invariants)
    scene = synth.make_scene(2, extent=90.0)
    ego = (0.4, -0.2, 0.0)
    pc = np.concatenate([synth.lidar_scan(scene, beams=128, sensor=ego, yaw=2 * np.pi / 2048 * r / 16, noise_seed=r)
                         for r in range(16)], axis=0)
    assert pc.shape[0] == 4194304 and pc.dtype == np.float32
    a, b = gvom_mod.Gvom(*params), gvom_mod.Gvom(*params)
    a.process_pointcloud(pc, ego)
    b.process_pointcloud(np.ascontiguousarray(pc[np.random.default_rng(1).permutation(pc.shape[0])]), ego)
    da, db = a.read_dense(0), b.read_dense(0)
    for k in range(4):
        assert np.array_equal(da[k], db[k])
    state, hit, total, minh, origin, cells = da
    del db
    st = a.scan_stats()
    assert cells == int((state >= 0).sum()) == int((hit > 0).sum()) == st["cells"]
    assert st["sum_hit"] == int(hit.sum())
    free_total = int((-state[state < -1].astype(np.int64) - 1).sum())
    assert st["sum_total"] == int(total.sum()) + free_total >= st["sum_hit"] > 1000000
    oa, ob = a.combine_maps(), b.combine_maps()
    for x, y in zip(oa, ob):
        assert np.array_equal(x, y)
    assert set(np.unique(oa[4])) <= {0, 1} and oa[4].sum() > 10000
    del a, b, da, state, hit, total, minh
    # PointCloud2 ingest at full size == the float64 cloud (what ros_numpy would hand over)
    c, d = gvom_mod.Gvom(*params), gvom_mod.Gvom(*params)
    c.process_pointcloud2(pc.tobytes(), pc.shape[0], 12, (0, 4, 8), ego)
    d.process_pointcloud(pc.astype(np.float64), ego)
    for x, y in zip(c.combine_maps(), d.combine_maps()):
        assert np.array_equal(x, y)
    assert c.scan_stats() == d.scan_stats()


def test_c5_moving_window_buffer4_and_sharded_equal_unsharded(gvom_mod):
    """BASELINE c5 (1024 x 1024 x 128, 4,194,304 returns per tick) with buffer=4 over 6 ticks of a moving
    window -- the ring wraps and evicts, tile epochs and slots are reused at 134 M voxels (too large for
    the CPU oracle): (i) point-order invariance of every returned map at every tick and of the fused map
    at the end; (ii) the map sharded over 8 ranks (threads on this GPU, 16 sensors -> 2 per rank) returns
    the same maps as the unsharded handle at every tick."""
    from shard_threads import run_ranks
    params = (0.2, 0.2, 1024, 128, 4) + synth.REF_TAIL
    scene = synth.make_scene(2, extent=90.0)
    W = 8
    ticks = []
    for k in range(6):
        ego = (0.4 + 0.3 * k, -0.2 - 0.25 * k, 0.02 * k)
        sens = [synth.lidar_scan(scene, beams=128, sensor=ego, yaw=2 * np.pi / 2048 * r / 16, noise_seed=50 * k + r)
                for r in range(16)]
        ticks.append((sens, ego))
    a, b = gvom_mod.Gvom(*params), gvom_mod.Gvom(*params)
    want = []
    for k, (sens, ego) in enumerate(ticks):
        pc = np.concatenate(sens, axis=0)
        a.process_pointcloud(pc, ego)
        b.process_pointcloud(np.ascontiguousarray(pc[np.random.default_rng(k).permutation(pc.shape[0])]), ego)
        oa, ob = a.combine_maps(), b.combine_maps()
        for x, y in zip(oa, ob):
            assert np.array_equal(x, y), "tick %d: point order changed a returned map" % k
        assert a.combined_cell_count_cpu == b.combined_cell_count_cpu
        want.append(([np.array(x, copy=True) for x in oa], a.combined_cell_count_cpu, a.buffer_index))
        del pc, oa, ob
    assert want[-1][2] == 6 % 4
    da, db = a.read_dense(gvom_mod.GVOM_WHICH_FUSED), b.read_dense(gvom_mod.GVOM_WHICH_FUSED)
    for j in range(4):
        assert np.array_equal(da[j], db[j])
    assert int((da[0] >= 0).sum()) == want[-1][1]
    del a, b, da, db

    def body(r, sh):
        for (sens, ego), (wout, wcnt, wbuf) in zip(ticks, want):
            sh.process_pointcloud(np.concatenate(sens[2 * r:2 * r + 2], axis=0), ego)
            got = sh.combine_maps()
            for x, y in zip(got, wout):
                assert np.array_equal(x, y)
            assert sh.combined_cell_count_cpu == wcnt and sh.b.g.buffer_index == wbuf
        return True

    assert run_ranks(W, params, body) == [True] * W


def test_non_finite_returns_have_no_effect(gvom_mod):
    """One contract for NaN / +-inf on BOTH entry points: a return with a non-finite coordinate (ros_numpy
    drops them before the reference sees the cloud, gvom_ros.py:108) has no effect on the map.
    process_pointcloud with such rows == the same cloud without them == the oracle on the clean cloud;
    float32 and float64, with and without a transform."""
    params = (0.2, 0.2, 64, 32, 2) + synth.REF_TAIL
    rng = np.random.default_rng(77)
    for dtype, with_tf in ((np.float32, False), (np.float64, True), (np.float32, True), (np.float64, False)):
        clean = (rng.uniform(-6, 6, (5000, 3)) * np.array([1, 1, 0.3])).astype(dtype)
        dirty = np.repeat(clean, 2, axis=0)
        bad = np.array([np.nan, np.inf, -np.inf], dtype)
        for i in range(clean.shape[0]):                   # every second row gets one or more non-finite fields
            row = dirty[2 * i + 1]
            row[rng.integers(0, 3)] = bad[rng.integers(0, 3)]
            if i % 5 == 0:
                row[:] = bad[rng.integers(0, 3)]
        tf = scenarios.rot_z(0.3, (0.2, -0.1, 0.05)) if with_tf else None
        ego = (0.11, -0.07, 0.02)
        gd, gc, want = gvom_mod.Gvom(*params), gvom_mod.Gvom(*params), oracle.OracleGvom(*params)
        for k in range(3):
            gd.process_pointcloud(dirty, ego, tf); gc.process_pointcloud(clean, ego, tf)
            want.process_pointcloud(clean.copy(), ego, tf)
            od, oc, ow = gd.combine_maps(), gc.combine_maps(), want.combine_maps()
            for i in (0, 1, 2, 4):
                assert np.array_equal(od[i], oc[i]) and np.array_equal(od[i], ow[i])
            assert np.array_equal(od[3], oc[3]) and np.allclose(od[3], ow[3], rtol=0, atol=1e-5)
            sd, sc_ = gd.read_dense(gd.last_buffer_index), gc.read_dense(gc.last_buffer_index)
            for j in range(4):
                assert np.array_equal(sd[j], sc_[j])
    # a cloud of ONLY non-finite returns is rejected like one that misses the grid (gvom.py:148-150)
    g = gvom_mod.Gvom(*params)
    g.process_pointcloud(np.full((100, 3), np.nan, np.float32), (0, 0, 0))
    assert g.combine_maps() is None and g.buffer_index == 0


@pytest.mark.parametrize("grid", [(32, 300, 2), (16, 1024, 3), (24, 513, 1)])
def test_tall_grids_use_the_generic_fusion_kernel(gvom_mod, grid):
    """z_size in (256, 1024]: chunks of more than 16 levels, i.e. the generic k_fuse<false> (per-wave static
    row ranges, liveness per level, column tail) -- no other test launches it.  Moving window, buffer > 1."""
    xy, zs, buf = grid
    params = (0.4, 0.05, xy, zs, buf, 0.5, 0.5, 0.5, 0.3, 2.0, 2.0, 1.0, 1, 1)
    rng = np.random.default_rng(zs)
    steps = []
    for k in range(4):
        ego = (0.9 * k, -0.5 * k, 0.3 * k)
        n = 6000
        pc = np.stack([rng.uniform(-0.2 * xy, 0.2 * xy, n) + ego[0], rng.uniform(-0.2 * xy, 0.2 * xy, n) + ego[1],
                       rng.uniform(-0.024 * zs, 0.024 * zs, n) + ego[2]], axis=1).astype(np.float32 if k % 2 else np.float64)
        steps += [("scan", pc, ego, None), ("combine",)]
    got, want = _run_both(gvom_mod, params, steps, record_debug=False)
    assert compare_records(got, want, float_tol=1e-5) > 20


@pytest.mark.parametrize("grid", [(64, 32, 1), (64, 64, 1), (128, 256, 1), (32, 512, 1), (64, 128, 3), (48, 16, 1)])
def test_one_slot_fusion_kernel_against_the_oracle_and_the_general_kernel(gvom_mod, grid):
    """k_fuse1: the fusion of ONE ring slot (+ the previous fused map) -- every combine of a buffer_size = 1 mapper and the
    first combine of any ring.  Grids of 2 ... 32 sixteen-level chunks (2, 4 and 8 waves per column block, 1, 2 and 4 chunks
    per wave), a moving window with decaying previous-map voxels, float32 and float64 scans; a ring of 3 takes it for its first
    combine only.  Compared with the oracle (returned maps, cell counts, the fused map densely) AND with the same mapper sent
    through the general kernel (gvom_set_tuning("fuse1", 1)): bit-identical."""
    xy, zs, buf = grid
    params = (0.4, 0.1 if zs > 100 else 0.2, xy, zs, buf, 0.5, 0.5, 0.5, 0.3, 2.0, 2.0, 1.0, 1, 1)
    rng = np.random.default_rng(xy * 7 + zs)
    g, g4, w = gvom_mod.Gvom(*params), gvom_mod.Gvom(*params), oracle.OracleGvom(*params)
    g4.set_tuning("fuse1", 1)
    for k in range(7):
        ego = (0.5 * k, -0.3 * k, 0.05 * k)
        n = 9000
        ground = np.stack([rng.uniform(-0.2 * xy, 0.2 * xy, n) + ego[0], rng.uniform(-0.2 * xy, 0.2 * xy, n) + ego[1],
                           rng.normal(-0.8, 0.15, n) + ego[2]], axis=1)
        # (returns that come and go: voxels of the previous map that the new scan sees through, gvom.py:992)
        wall = np.stack([np.full(600, 3.0 + 0.4 * (k % 2)) + ego[0], rng.uniform(-2, 2, 600) + ego[1], rng.uniform(-0.8, 1.0, 600) + ego[2]], axis=1)
        pc = np.concatenate([ground, wall], 0).astype(np.float32 if k % 2 else np.float64)
        for m in (g, g4, w):
            m.process_pointcloud(pc.copy(), ego)
        a, a4, b = g.combine_maps(), g4.combine_maps(), w.combine_maps()
        for i in range(5):
            assert np.array_equal(a[i], a4[i], equal_nan=True), (k, i)
        for i in (0, 1, 2, 4):
            assert np.array_equal(a[i], b[i]), (k, i)
        assert np.allclose(a[3], b[3], rtol=0, atol=1e-5)
        assert g.combined_cell_count_cpu == g4.combined_cell_count_cpu == w.combined_cell_count_cpu, k
    gd, gd4 = g.read_dense(gvom_mod.GVOM_WHICH_FUSED), g4.read_dense(gvom_mod.GVOM_WHICH_FUSED)
    wd = scenarios.dense_from_compact(w.combined_index_map, w.combined_hit_count, w.combined_total_count, w.combined_min_height)
    for j in range(4):
        assert np.array_equal(gd[j], gd4[j]) and np.array_equal(np.asarray(wd[j]), gd[j]), j


@pytest.mark.parametrize("grid", [(64, 32), (32, 8), (128, 256), (48, 20), (16, 4), (64, 70)])
def test_eager_fusion_of_one_slot_rings_equals_the_two_pass_form_and_the_oracle(gvom_mod, grid):
    """Eager fusion (buffer_size = 1): the scan launches k_encfuse behind k_trace -- slot encoding AND its fusion with the
    previous map in one pass over the accumulators, into spare buffers -- and combine_maps adopts the result iff nothing
    changed in between; otherwise the combine fuses the encoded slot with k_fuse1 as before.  Every call order must give the
    reference's results: a scan behind a scan (speculation dropped, the slot still correctly encoded), two combines behind one
    scan (the second re-fuses the slot), rejected scans (no return in the grid: ring untouched, but the ego moves), debug
    reads between a scan and its combine (they show the LAST combine's maps), a moving window with decaying voxels.  The
    mapper with the automatic policy, one forced eager, one with eager off and the oracle are recorded step by step (scan
    slots, fused maps densely, all 2-D maps, counts, debug maps) and compared; z sizes that are no multiple of the kernel's
    4-level groups and grids of a single column block included."""
    xy, zs = grid
    params = (0.4, 0.2, xy, zs, 1, 0.5, 0.5, 0.5, 0.3, 2.0, 2.0, 1.0, 1, 1)
    rng = np.random.default_rng(xy * 13 + zs)

    def cloud(k, ego, dtype):
        n = 6000
        ground = np.stack([rng.uniform(-0.18 * xy, 0.18 * xy, n) + ego[0], rng.uniform(-0.18 * xy, 0.18 * xy, n) + ego[1],
                           rng.normal(-0.5, 0.12, n) + ego[2]], axis=1)
        wall = np.stack([np.full(500, 2.6 + 0.4 * (k % 2)) + ego[0], rng.uniform(-2, 2, 500) + ego[1], rng.uniform(-0.6, 0.6, 500) + ego[2]], axis=1)
        return np.concatenate([ground, wall], 0).astype(dtype)
    far = np.full((50, 3), 1.0e4)                               # no return in the grid: rejected (gvom.py:148-150)
    steps, k = [], 0
    for kind in "sc sc ssc cc s rc sc rsc c ssssc sc sc".replace(" ", ""):
        if kind == "c":
            steps.append(("combine",))
            continue
        ego = (0.45 * k, -0.25 * k, 0.04 * k)
        steps.append(("scan", far if kind == "r" else cloud(k, ego, np.float32 if k % 2 else np.float64), ego,
                      scenarios.rot_z(0.01 * k, (0.0, 0.0, 0.0)) if k % 3 == 0 and kind != "r" else None))
        k += 1
    sc = {"params": params, "steps": steps}

    def knob(v):
        def make(*p):
            g = gvom_mod.Gvom(*p, voxel_statistics=False)       # (statistics on demand would keep the first combines off the eager path)
            g.set_tuning("eager", v)
            made.append(g)
            return g
        return make
    made = []
    want = scenarios.run_and_record(oracle.OracleGvom, sc)
    recs = [scenarios.run_and_record(knob(v), sc) for v in (-1, 1, 0)]
    for got in recs:
        assert compare_records(got, want, float_tol=1e-5) > 50
    for key in recs[2]:                                         # eager on / off: bit-identical, floats included
        for other in recs[:2]:
            a, b = np.asarray(recs[2][key]), np.asarray(other[key])
            assert a.shape == b.shape and (np.array_equal(a, b, equal_nan=True) if a.dtype.kind in "fiub" else True), key
    auto, forced, off = made
    n_comb = sum(1 for st in steps if st[0] == "combine")
    assert off.get_tuning("eager_adopted") == 0 and off.get_tuning("eager_dropped") == 0
    assert 0 < forced.get_tuning("eager_adopted") < n_comb and forced.get_tuning("eager_dropped") > 0
    # the automatic policy stops speculating after three wasted fusions in a row ("ssssc") and comes back
    assert 0 < auto.get_tuning("eager_adopted") <= forced.get_tuning("eager_adopted")
    assert auto.get_tuning("eager_dropped") <= forced.get_tuning("eager_dropped")


@pytest.mark.parametrize("zs", [16, 32, 70])
def test_eager_fusion_shape_knob_numbers_its_rows_inside_what_was_allocated(gvom_mod, zs):
    """gvom_set_tuning("encfuse", 1..3): fewer waves per column block.  A wave numbers its fused rows from
    (block * waves + wave) * iterations * 256, and waves' * ceil(z / 4 waves') can EXCEED the default shape's product
    (z 16: 4 x 1 against 3 x 2; z 32: 4 x 2 against 3 x 3) -- the row buffer is sized from the shape that is launched
    (it was sized from the default one and k_encfuse wrote past its end).  Dense scans (most voxels occupied near
    the sensor, so high row numbers are really written), a moving window, every shape against the default and the oracle."""
    xy = 64
    params = (0.4, 0.2, xy, zs, 1, 0.5, 0.5, 0.5, 0.3, 2.0, 2.0, 1.0, 1, 1)
    rng = np.random.default_rng(900 + zs)
    steps = []
    for k in range(4):
        ego = (0.45 * k, -0.25 * k, 0.04 * k)
        n = 60000
        pc = np.stack([rng.uniform(-0.19 * xy, 0.19 * xy, n) + ego[0], rng.uniform(-0.19 * xy, 0.19 * xy, n) + ego[1],
                       rng.uniform(-0.09 * zs, 0.09 * zs, n) + ego[2]], axis=1).astype(np.float32)
        steps += [("scan", pc, ego, None), ("combine",)]
    sc = {"params": params, "steps": steps}
    want = scenarios.run_and_record(oracle.OracleGvom, sc)

    def knob(v):
        def make(*p):
            g = gvom_mod.Gvom(*p, voxel_statistics=False)
            g.set_tuning("eager", 1)
            g.set_tuning("encfuse", v)
            made.append(g)
            return g
        return make
    made = []
    recs = [scenarios.run_and_record(knob(v), sc) for v in (0, 1, 2, 3, 16 + 3)]
    for got in recs:
        assert compare_records(got, want, float_tol=1e-5) > 20
    for key in recs[0]:
        for other in recs[1:]:
            a, b = np.asarray(recs[0][key]), np.asarray(other[key])
            assert a.shape == b.shape and (np.array_equal(a, b, equal_nan=True) if a.dtype.kind in "fiub" else True), key
    assert all(g.get_tuning("eager_adopted") == 4 for g in made)


@pytest.mark.parametrize("grid", [(32, 16, 20), (30, 12, 24), (16, 300, 18), (32, 16, 40)])
def test_long_rings_read_their_descriptors_from_memory(gvom_mod, grid):
    """More than 17 fusion sources (ring slots + previous map) no longer fit the kernel arguments: the
    descriptors then come from device memory (the MEM instantiations of k_fuse4 / k_fuse).  The ring fills
    beyond 17 slots, wraps (the 40-slot one does not) and the window moves; xy % 4 != 0 and a tall grid take
    the generic kernels."""
    xy, zs, buf = grid
    params = (0.4, 0.2 if zs < 100 else 0.05, xy, zs, buf, 0.5, 0.5, 0.5, 0.3, 2.0, 2.0, 1.0, 1, 1)
    rng = np.random.default_rng(xy * 1000 + buf)
    g, w = gvom_mod.Gvom(*params), oracle.OracleGvom(*params)
    n_scans = 26
    for k in range(n_scans):
        ego = (0.25 * k, -0.15 * k, 0.02 * k)
        n = 1500
        pc = np.stack([rng.uniform(-0.2 * xy, 0.2 * xy, n) + ego[0], rng.uniform(-0.2 * xy, 0.2 * xy, n) + ego[1],
                       rng.normal(-0.5, 0.3, n) + ego[2]], axis=1).astype(np.float32)
        g.process_pointcloud(pc, ego); w.process_pointcloud(pc.copy(), ego)
        if k >= 16 or k % 5 == 0:
            a, b = g.combine_maps(), w.combine_maps()
            for i in (0, 1, 2, 4):
                assert np.array_equal(a[i], b[i]), (k, i)
            assert np.allclose(a[3], b[3], rtol=0, atol=1e-5)
            assert g.combined_cell_count_cpu == w.combined_cell_count_cpu, k
    gd = g.read_dense(gvom_mod.GVOM_WHICH_FUSED)
    wd = scenarios.dense_from_compact(w.combined_index_map, w.combined_hit_count, w.combined_total_count, w.combined_min_height)
    for j in range(4):
        assert np.array_equal(np.asarray(wd[j]), gd[j]), j


def test_cuda_f32_sqrt_flag(gvom_mod):
    """numba_cuda_typing=True (GVOM_FLAG_NUMBA_CUDA_TYPING; its name before round 6: cuda_f32_sqrt): the types Numba infers for
    a real CUDA device where they differ from the simulator's -- profiles/numba_cuda_typing.txt, generated by
    tests/golden/numba_typing_probe.py from Numba 0.54.1's own type inference (CUDA typing context) over the unmodified
    reference: ray_length = math.sqrt(float32) -> float32 (gvom.py:1109), slope / ray_length in float32 (:1112-1114), the loop
    bound from that float32 (:1127); every other difference in the table is value-neutral.  The simulator -- and therefore the
    fixtures and the default -- takes the float64 square root.  Two returns, found by search, whose rays mark different
    voxels under the two typings; the HIP path follows the oracle in both modes, on them, on a random cloud and on the 40 seeds
    of the edge-case fuzz (this mode has no reference-generated VECTOR: the simulator cannot produce one, and no CUDA device is
    here -- what is pinned is the typing table)."""
    params = (0.2, 0.2, 64, 32, 1, 0.5, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
    ego = (0.013, -0.027, 0.004)
    rays = np.array([[4.66099739074707, -5.127684116363525, -0.5784711241722107],
                     [4.96124792098999, 4.209757328033447, 0.7061797380447388]], np.float32)
    rng = np.random.default_rng(9)
    cloud = np.concatenate([rays, (rng.uniform(-6, 6, (20000, 3)) * np.array([1, 1, 0.3])).astype(np.float32)])
    dense = {}
    for flag in (False, True):
        for pc, tag in ((rays, "rays"), (cloud, "cloud")):
            g = gvom_mod.Gvom(*params, numba_cuda_typing=flag)
            w = oracle.OracleGvom(*params, numba_cuda_typing=flag)
            g.process_pointcloud(pc, ego); w.process_pointcloud(pc.copy(), ego)
            gd = g.read_dense(0)
            wd = scenarios.dense_from_compact(w.index_buffer[0], w.hit_count_buffer[0], w.total_count_buffer[0], w.min_height_buffer[0])
            for j in range(4):
                assert np.array_equal(np.asarray(wd[j]), gd[j]), (flag, tag, j)
            dense[(flag, tag)] = gd[0].copy()
    assert not np.array_equal(dense[(False, "rays")], dense[(True, "rays")])
    assert gvom_mod.Gvom(*params, cuda_f32_sqrt=True).read_dense(0) is None                        # (the old keyword still binds)
    differ = 0
    for seed in range(40):
        fparams, steps = _fuzz_case(1000 + seed)
        sc = {"params": fparams, "steps": steps}
        want = scenarios.run_and_record(lambda *p: oracle.OracleGvom(*p, numba_cuda_typing=True), sc)
        got = scenarios.run_and_record(lambda *p: gvom_mod.Gvom(*p, numba_cuda_typing=True), sc)
        assert compare_records(got, want, float_tol=1e-5) > 3, seed
        plain = scenarios.run_and_record(oracle.OracleGvom, sc)
        differ += any(k in plain and not np.array_equal(np.asarray(plain[k]), np.asarray(want[k]), equal_nan=True)
                      for k in want if k.endswith(("slot_total", "fused_total")))
    print("numba_cuda_typing: %d of 40 fuzz seeds mark other voxels than the simulator's typing" % differ)


def test_long_run_moving_window_matches_oracle(gvom_mod):
    """600 scan+combine steps with a random-walking sensor (the robot-centred window shifts ~170
    voxels in x and y and wraps the toroidal storage several times; ring slots and tile epochs are
    reused hundreds of times): every 25th step, and the last, must match the oracle bit for bit
    (ints) / 1e-5 (floats)."""
    params = (0.4, 0.2, 48, 24, 3, 0.8, 0.5, 0.5, 0.3, 2.0, 2.0, 1.0, 1, 1)
    g, want = gvom_mod.Gvom(*params), oracle.OracleGvom(*params)
    rng = np.random.default_rng(2024)
    ego = np.zeros(3)
    heading = 0.0
    checked = 0
    for k in range(600):
        heading += rng.normal(0, 0.15)
        ego = ego + np.array([0.32 * np.cos(heading) + 0.1, 0.32 * np.sin(heading) + 0.12, rng.normal(0, 0.02)])
        n = int(rng.integers(1500, 4000))
        pc = np.stack([rng.uniform(-9, 9, n) + ego[0], rng.uniform(-9, 9, n) + ego[1],
                       rng.normal(-0.9, 0.6, n) + ego[2]], axis=1).astype(np.float32 if k % 2 else np.float64)
        tf = scenarios.rot_z(0.01 * (k % 7), (0.0, 0.0, 0.0)) if k % 3 == 0 else None
        e = tuple(float(v) for v in ego)
        g.process_pointcloud(pc, e, tf)
        want.process_pointcloud(pc, e, tf)
        a, b = g.combine_maps(), want.combine_maps()
        if k % 25 == 24 or k == 599:
            assert np.array_equal(a[0], b[0])
            for i in (1, 2, 4):
                assert np.array_equal(a[i], b[i]), "step %d map %d differs" % (k, i)
            assert np.allclose(a[3], b[3], rtol=0, atol=1e-5)
            assert g.combined_cell_count_cpu == want.combined_cell_count_cpu
            checked += 1
    assert checked == 24 and abs(ego[0]) + abs(ego[1]) > 40.0


def _fuzz_case(seed):
    """A random small configuration and call sequence with the inputs that sit on the edges of the
    algorithm: returns on voxel faces and grid corners, axis-parallel rays, returns at the sensor
    (zero-length rays), duplicates, far outliers, empty clouds, exact-integer and negative egos."""
    rng = np.random.default_rng(seed)
    xy_res = float(rng.choice([0.1, 0.25, 0.4, 1.0])); z_res = float(rng.choice([0.1, 0.2, 0.5]))
    xy = int(rng.integers(4, 71)); zs = int(rng.integers(1, 41)); buf = int(rng.integers(1, 5))
    params = (xy_res, z_res, xy, zs, buf, float(rng.choice([0.0, 0.5, 2.0])),
              float(rng.uniform(0.1, 1.0)), float(rng.uniform(0.1, 1.0)), float(rng.uniform(0.1, 0.6)),
              float(rng.uniform(0.5, 3.0)), float(rng.uniform(0.0, 5.0)), float(rng.uniform(0.0, 2.0)), 1, 1)
    half = np.array([xy * xy_res, xy * xy_res, zs * z_res]) * 0.5
    steps = []
    ego = np.round(rng.uniform(-3, 3, 3), int(rng.integers(0, 3)))          # often exact integers
    for k in range(int(rng.integers(1, 7))):
        ego = ego + np.round(rng.uniform(-1.5, 1.5, 3) * np.array([1, 1, 0.1]), int(rng.integers(0, 3)))
        n = int(rng.choice([0, 1, 7, 300, 3000]))
        parts = [rng.uniform(-1.2, 1.2, (n, 3)) * half + ego]
        if n:
            m = max(1, n // 6)
            grid = np.round(rng.uniform(-1, 1, (m, 3)) * half / np.array([xy_res, xy_res, z_res])) * np.array([xy_res, xy_res, z_res])
            parts.append(grid + np.floor(ego / np.array([xy_res, xy_res, z_res])) * np.array([xy_res, xy_res, z_res]))   # on voxel faces
            ax = np.zeros((m, 3)); ax[np.arange(m), rng.integers(0, 3, m)] = rng.uniform(-1, 1, m) * half.min()
            parts.append(ax + ego)                                            # axis-parallel rays
            parts.append(np.repeat(ego[None], 3, 0))                          # zero-length rays
            parts.append(parts[0][:m])                                        # duplicates
            parts.append(rng.uniform(-40, 40, (3, 3)) * half + ego)           # far outside the grid
        pc = np.concatenate(parts, 0).astype(rng.choice([np.float32, np.float64]))
        tf = scenarios.rot_z(float(rng.uniform(-0.2, 0.2)), tuple(rng.uniform(-0.1, 0.1, 3))) if rng.random() < 0.4 else None
        steps.append(("scan", pc, tuple(float(v) for v in ego), tf))
        if rng.random() < 0.7:
            steps.append(("combine",))
    steps.append(("combine",))
    return params, steps


@pytest.mark.parametrize("seed", range(40))
def test_fuzz_small_configurations_match_oracle(gvom_mod, seed):
    params, steps = _fuzz_case(1000 + seed)
    got, want = _run_both(gvom_mod, params, steps)
    assert compare_records(got, want, float_tol=1e-5) > 3


# ---- per-voxel statistics against the oracle on every fusion route ------------------------------------------------------------
# gvom_get_tuning("fuse_kernel"): the kernel of the last fusion, as the library launched it (include/gvom_hip.h)
FUSE1, FUSE4_2, FUSE4_4, FUSE_SHORT, FUSE_TALL, ENCFUSE, DESCS_MEM = 1, 2, 3, 4, 5, 6, 16


def _stats_hip(gvom_mod, **kw):
    return lambda *p: gvom_mod.Gvom(*p, voxel_statistics=True, **kw)


def _stats_oracle(**kw):
    return lambda *p: oracle.OracleGvom(*p, voxel_statistics=True, **kw)


def _same_maps(a, b, what):
    assert (a is None) == (b is None), what
    if a is None:
        return
    for i in (0, 1, 2, 4):
        assert np.array_equal(a[i], b[i]), "%s: map %d differs" % (what, i)
    assert np.allclose(a[3], b[3], rtol=0, atol=1e-5), what + ": roughness"


def _stats_steps(gvom_mod, params, steps, route=None, make_hip=None, make_oracle=None, what=""):
    """Drives a HIP mapper and the oracle, both with voxel_statistics, through `steps` (("scan", cloud, ego, tf) / ("combine",)):
    after every combine the returned maps (ints exact, roughness 1e-5), the fused cell count and ALL the statistics
    (parity.compare_statistics).  route(k, filled, has_prev) -> the "fuse_kernel" the combine of step k must report (None:
    not asserted).  Returns (hip mapper, oracle mapper, number of combines checked)."""
    g = (make_hip or _stats_hip(gvom_mod))(*params)
    w = (make_oracle or _stats_oracle())(*params)
    checked, has_prev = 0, False
    for k, step in enumerate(steps):
        tag = "%s step %d" % (what, k)
        if step[0] == "scan":
            _, pc, ego, tf = step
            g.process_pointcloud(pc, ego, tf)
            w.process_pointcloud(np.array(pc, copy=True), ego, tf)
            continue
        a, b = g.combine_maps(), w.combine_maps()
        _same_maps(a, b, tag)
        if b is None:
            continue
        assert g.combined_cell_count_cpu == w.combined_cell_count_cpu, tag
        if route is not None:
            filled = sum(o is not None for o in w.origin_buffer)
            want_route = route(k, filled, has_prev)
            if want_route is not None:
                assert g.get_tuning("fuse_kernel") == want_route, (tag, filled, g.get_tuning("fuse_kernel"), want_route)
        compare_statistics(g, w, what=tag + ": ")
        checked += 1
        has_prev = True
    return g, w, checked


def _surface_steps(seed, xy, zs, xy_res, z_res, n_scans, n_pts=4000, dtype=np.float32, with_tf=False, move=(0.45, -0.3, 0.04)):
    """scan + combine per pose of a moving sensor over a rolling surface with posts on it (voxels with many returns, with few,
    with one; flat, thin and round neighbourhoods)"""
    rng = np.random.default_rng(seed)
    half = 0.5 * xy * xy_res * 0.9
    steps = []
    for k in range(n_scans):
        ego = (move[0] * k, move[1] * k, move[2] * k)
        x = rng.uniform(-half, half, n_pts) + ego[0]
        y = rng.uniform(-half, half, n_pts) + ego[1]
        z = 0.3 * np.sin(0.8 * x) + 0.2 * np.cos(0.5 * y) - 0.8 + rng.normal(0, 0.03, n_pts)
        posts = rng.uniform(-half, half, (6, 2)) + np.array(ego[:2])
        m = n_pts // 8
        j = rng.integers(0, 6, m)
        x[:m], y[:m] = posts[j, 0] + rng.normal(0, 0.02, m), posts[j, 1] + rng.normal(0, 0.02, m)
        z[:m] = rng.uniform(-0.8, min(1.2, 0.45 * zs * z_res), m)
        pc = np.stack([x, y, z], axis=1).astype(dtype)
        tf = scenarios.rot_z(0.03 * (k + 1), (0.02 * k, -0.01, 0.003)) if with_tf else None
        steps += [("scan", pc, ego, tf), ("combine",)]
    return steps


def _route_by_slots(filled, has_prev, mem_above=17):
    r = FUSE1 if filled == 1 else (FUSE4_2 if filled == 2 else FUSE4_4)
    return r | (DESCS_MEM if filled + has_prev > mem_above else 0)


_ROUTES = {
    # name: (xy, zs, buffer, z_res, n_scans, route(k, filled, has_prev))
    "encfuse_64x32": (64, 32, 1, 0.2, 7, lambda k, f, p: ENCFUSE),
    "encfuse_48x20": (48, 20, 1, 0.2, 7, lambda k, f, p: ENCFUSE),          # z_size % 4 != 0
    "fuse1_36x32": (36, 32, 1, 0.2, 7, lambda k, f, p: FUSE1),              # xy_size % 16 != 0: no eager fusion
    "fuse4x2_64x32": (64, 32, 2, 0.2, 7, lambda k, f, p: _route_by_slots(f, p)),
    "fuse4x4_64x32_b3": (64, 32, 3, 0.2, 7, lambda k, f, p: _route_by_slots(f, p)),
    "fuse4x4_64x32_b4": (64, 32, 4, 0.2, 8, lambda k, f, p: _route_by_slots(f, p)),
    "fuse_short_50x13": (50, 13, 3, 0.2, 7, lambda k, f, p: FUSE_SHORT),     # xy_size % 4 != 0, 13-level chunks
    "fuse_tall_16x300": (16, 300, 2, 0.05, 7, lambda k, f, p: FUSE_TALL),    # 19-level chunks
    "descs_mem_32x16": (32, 16, 20, 0.2, 26, lambda k, f, p: _route_by_slots(f, p)),
    "descs_mem_30x12": (30, 12, 18, 0.2, 26, lambda k, f, p: FUSE_SHORT | (DESCS_MEM if f + p > 17 else 0)),
}


@pytest.mark.parametrize("name", sorted(_ROUTES))
def test_voxel_statistics_match_oracle_on_every_fusion_route(gvom_mod, name):
    """The per-voxel statistics (k_stats, k_stats_gather, k_fuse_stats, k_voxel_cloud) against the oracle after EVERY combine of
    a moving window, on each fusion kernel the library has -- the adopted eager k_encfuse (its merge reads the previous map
    through the link table), k_fuse1, k_fuse4<2>, k_fuse4<4>, k_fuse with short and with tall chunks, and the descriptors read
    from memory (more than 17 sources) -- as the library reports it launched them.  The rings fill, wrap and evict."""
    xy, zs, buf, z_res, n_scans, route = _ROUTES[name]
    params = (0.4, z_res, xy, zs, buf, 0.5, 0.5, 0.5, 0.3, 2.0, 2.0, 1.0, 1, 1)
    n_pts = 1500 if n_scans > 20 else 4000
    steps = _surface_steps(xy * 100 + zs + buf, xy, zs, 0.4, z_res, n_scans, n_pts, move=(0.25, -0.15, 0.02) if n_scans > 20 else (0.45, -0.3, 0.04))
    g, _, checked = _stats_steps(gvom_mod, params, steps, route=route, what=name)
    assert checked == n_scans
    if name.startswith("encfuse"):
        assert g.get_tuning("eager_adopted") == n_scans


@pytest.mark.parametrize("site", ["combine", "scan"])
def test_voxel_statistics_across_the_tile_epoch_renumbering(gvom_mod, site):
    """test_tile_epoch_renumbering_before_the_counter_wraps with the statistics on: the statistics' sources are found by their
    tile epochs too (k_stats' direct form, k_stats_gather's neighbours, k_fuse_stats' slots and previous map)."""
    params = (0.4, 0.2, 32, 16, 3, 0.5, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
    steps = _surface_steps(4, 32, 16, 0.4, 0.2, 12, 3000)
    seen = []

    def hip(*p):
        g = gvom_mod.Gvom(*p, voxel_statistics=True, _library=TEST_LIB)
        seen.append(g)
        return g

    def route(k, f, p):
        if k == 7:                  # (behind the combine of scan 3: 8 epochs used so far; the threshold is crossed by the next combine / scan)
            seen[0].set_tuning("epoch_bias", 0xFFFFFF00 - 2 * 4 - (3 if site == "combine" else 2))
        return _route_by_slots(f, p)
    _, _, checked = _stats_steps(gvom_mod, params, steps, route=route, make_hip=hip, what="epoch " + site)
    assert checked == 12


def test_voxel_statistics_with_numba_cuda_typing(gvom_mod):
    """numba_cuda_typing=True (float32 ray lengths) with the statistics on, both sides."""
    params = (0.2, 0.2, 64, 32, 2, 0.5, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
    steps = _surface_steps(31, 64, 32, 0.2, 0.2, 6)
    _, _, checked = _stats_steps(gvom_mod, params, steps, route=lambda k, f, p: _route_by_slots(f, p),
                                 make_hip=_stats_hip(gvom_mod, numba_cuda_typing=True),
                                 make_oracle=_stats_oracle(numba_cuda_typing=True), what="numba typing")
    assert checked == 6


def test_voxel_statistics_of_float64_transformed_and_strided_clouds(gvom_mod):
    """float64 clouds with a 4x4 transform, then float32 (N, 4) rows with an extra column, a Fortran-ordered cloud and a
    strided view, one per scan (k_stats<double> / k_stats<float> and the cloud strides of the statistics' pass)."""
    params = (0.4, 0.2, 64, 32, 2, 0.5, 0.5, 0.5, 0.3, 2.0, 2.0, 1.0, 1, 1)
    steps = _surface_steps(5, 64, 32, 0.4, 0.2, 8, dtype=np.float64, with_tf=True)
    rng = np.random.default_rng(6)
    for k in range(4, 8):
        _, pc, ego, _ = steps[2 * k]
        pc32 = pc.astype(np.float32)
        xyzi = np.concatenate([pc32, rng.uniform(0, 1, (pc32.shape[0], 1)).astype(np.float32)], axis=1)
        pc_k = (xyzi, np.asfortranarray(pc32), xyzi[:, :3], pc32[::-1])[k - 4]
        steps[2 * k] = ("scan", pc_k, ego, None)
    _, _, checked = _stats_steps(gvom_mod, params, steps, route=lambda k, f, p: _route_by_slots(f, p), what="dtype/stride")
    assert checked == 8


def test_voxel_statistics_at_the_grid_border_inside_min_distance_and_of_empty_scans(gvom_mod):
    """Returns OUTSIDE the grid whose neighbourhood reaches border voxels (the direct form of k_stats), returns inside
    min_distance (no statistics), an empty scan and a scan the map rejects (no return near the grid) between the others."""
    xy, zs, xy_res, z_res = 48, 16, 0.4, 0.2
    params = (xy_res, z_res, xy, zs, 3, 1.0, 0.5, 0.5, 0.3, 2.0, 2.0, 1.0, 1, 1)
    rng = np.random.default_rng(8)
    steps = []
    for k in range(8):
        ego = (0.37 * k, -0.21 * k, 0.03 * k)
        lo = (np.floor(np.array(ego) / np.array([xy_res, xy_res, z_res]) - np.array([xy, xy, zs]) / 2) * np.array([xy_res, xy_res, z_res]))
        hi = lo + np.array([xy * xy_res, xy * xy_res, zs * z_res])
        n = 3000
        pc = np.stack([rng.uniform(lo[0], hi[0], n), rng.uniform(lo[1], hi[1], n), rng.normal(-0.6, 0.3, n) + ego[2]], 1)
        band = []
        for ax in range(3):                                       # just outside each face, within one voxel of it
            for side in (lo, hi):
                b = np.stack([rng.uniform(lo[0], hi[0], 300), rng.uniform(lo[1], hi[1], 300), rng.uniform(lo[2], hi[2], 300)], 1)
                res = (xy_res, xy_res, z_res)[ax]
                b[:, ax] = side[ax] + (rng.uniform(0.02, 0.98, 300) * res if side is hi else -rng.uniform(0.02, 0.98, 300) * res)
                band.append(b)
        corner = hi + rng.uniform(0.01, 0.3, (50, 3)) * np.array([xy_res, xy_res, z_res])
        near = np.array(ego) + rng.normal(0, 0.3, (200, 3))       # mostly inside min_distance (1.0 m)
        pc = np.concatenate([pc] + band + [corner, near], 0).astype(np.float32 if k % 2 else np.float64)
        if k == 3:
            pc = pc[:0]                                            # empty scan
        if k == 5:
            pc = pc + 900.0                                        # no return reaches the grid: rejected
        steps += [("scan", pc, ego, None), ("combine",)]
    _, _, checked = _stats_steps(gvom_mod, params, steps, route=lambda k, f, p: _route_by_slots(f, p), what="border")
    assert checked == 8


@pytest.mark.parametrize("dist", [(0, 0), (1, 0), (0, 2), (2, 1), (3, 2)])
def test_voxel_statistics_neighbourhood_sizes(gvom_mod, dist):
    """(xy_eigen_dist, z_eigen_dist) other than (1, 1): the neighbourhood arithmetic of k_stats' direct form and of k_stats_gather
    (wx = 2 xy_e + 1, nb = wx^2 (2 z_e + 1), the offset decode, the shifted moments) over a moving window, ring of 2."""
    params = (0.4, 0.2, 64, 32, 2, 0.5, 0.5, 0.5, 0.3, 2.0, 2.0, 1.0) + dist
    steps = _surface_steps(40 + 7 * dist[0] + dist[1], 64, 32, 0.4, 0.2, 6)
    _, _, checked = _stats_steps(gvom_mod, params, steps, route=lambda k, f, p: _route_by_slots(f, p), what="dist %r" % (dist,))
    assert checked == 6


def test_voxel_statistics_of_degenerate_voxels(gvom_mod):
    """(0, 0) neighbourhoods (each voxel's own returns only) built to hold exactly one return (all covariances zero: the
    eigen-solver's p1 == 0 branch), two returns, three collinear returns (along an axis: p1 == 0 again; and oblique), four
    coplanar returns (horizontal and vertical planes), exact duplicates, and returns on voxel faces / corners (in-voxel
    position exactly 0) -- scanned three times from poses a whole voxel apart and merged over a ring of 2."""
    xy_res, z_res, xy, zs = 0.5, 0.25, 32, 16
    params = (xy_res, z_res, xy, zs, 2, 0.5, 0.5, 0.5, 0.3, 2.0, 2.0, 1.0, 0, 0)
    res = np.array([xy_res, xy_res, z_res])
    voxels = {
        (20, 20, 8): [(0.5, 0.5, 0.5)],
        (22, 20, 8): [(0.2, 0.3, 0.4), (0.7, 0.1, 0.9)],
        (24, 20, 8): [(0.1, 0.5, 0.5), (0.5, 0.5, 0.5), (0.9, 0.5, 0.5)],
        (26, 20, 8): [(0.1, 0.1, 0.1), (0.2, 0.3, 0.4), (0.3, 0.5, 0.7)],
        (28, 20, 8): [(0.1, 0.1, 0.5), (0.9, 0.1, 0.5), (0.1, 0.9, 0.5), (0.9, 0.9, 0.5)],
        (20, 23, 9): [(0.25, 0.1, 0.1), (0.25, 0.9, 0.1), (0.25, 0.1, 0.9), (0.25, 0.9, 0.9)],
        (22, 23, 9): [(0.3, 0.6, 0.2)] * 5,
        (24, 23, 9): [(0.0, 0.0, 0.0)],
        (26, 23, 9): [(0.0, 0.5, 0.5), (0.0, 0.25, 0.75), (0.5, 0.0, 0.0)],
        (28, 23, 7): [(0.0, 0.0, 0.0)] * 3 + [(0.5, 0.5, 0.5)],
        (8, 9, 8): [(0.5, 0.5, 0.5), (0.5, 0.5, 0.5), (0.25, 0.75, 0.5)],
    }
    steps = []
    for k, ego in enumerate([(0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (0.5, 0.5, 0.25)]):
        pts = [(np.array(v) - np.array([16, 16, 8]) + np.array(f)) * res for v, fs in voxels.items() for f in fs]
        pc = np.array(pts, np.float64)
        steps += [("scan", pc if k != 1 else pc.astype(np.float32), ego, None), ("combine",)]
    g, w, checked = _stats_steps(gvom_mod, params, steps, what="degenerate")
    assert checked == 3
    counts = np.asarray(w.metrics_buffer[w.last_buffer_index])[:, 9]
    assert sorted(np.unique(counts).tolist()) == [1.0, 2.0, 3.0, 4.0, 5.0]


def _device_clouds(scans):
    """the clouds in HBM (hipMalloc'd; bench.py's feed): [(pointer, n, dtype, ego, tf)], and a function that frees them"""
    import ctypes
    rt = ctypes.CDLL("libamdhip64.so")
    rt.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    rt.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    rt.hipFree.argtypes = [ctypes.c_void_p]
    out = []
    for pc, ego, tf in scans:
        pc = np.ascontiguousarray(pc)
        p = ctypes.c_void_p()
        assert rt.hipMalloc(ctypes.byref(p), pc.nbytes) == 0
        out.append((p, pc.shape[0], pc.dtype, ego, tf))
        assert rt.hipMemcpy(p, pc.ctypes.data_as(ctypes.c_void_p), pc.nbytes, 1) == 0
    assert rt.hipDeviceSynchronize() == 0
    return out, lambda: [rt.hipFree(d[0]) for d in out]


@pytest.mark.parametrize("stats", [True, False])
def test_bench_sequence_m256_matches_oracle_every_step(gvom_mod, stats):
    """The exact sequence bench.py times: the m256 grid (256^3 @0.2 m, buffer 1), its 8 moving poses of the 131,072-return
    scan, each fed from HBM through process_pointcloud_device and combined, every step against the all-core oracle.
    stats=True: the default constructor read by the node's debug call after every combine (statistics on demand) against the
    oracle's statistics, every combine an adopted eager fusion.  stats=False: the north-star path, returned maps every step
    plus the newest ring slot and the fused map densely at steps 1 and 7."""
    params, scans = synth.config_inputs("m256", n_scans=8)
    assert params[2:5] == (256, 256, 1) and len(scans) == 8
    dev, free = _device_clouds(scans)
    oracle.use_all_cores(True, threads=16)
    try:
        g = gvom_mod.DefaultGvom(*params) if stats else gvom_mod.Gvom(*params)
        w = oracle.OracleGvom(*params, voxel_statistics=stats)
        for k, ((d, n, dt, ego, tf), (pc, _, _)) in enumerate(zip(dev, scans)):
            g.process_pointcloud_device(d.value, n, dt, ego, tf)
            w.process_pointcloud(pc, ego, tf)
            a, b = g.combine_maps(), w.combine_maps()
            _same_maps(a, b, "m256 step %d" % k)
            assert g.combined_cell_count_cpu == w.combined_cell_count_cpu
            assert (g.buffer_index, g.last_buffer_index) == (w.buffer_index, w.last_buffer_index)
            assert g.get_tuning("fuse_kernel") == ENCFUSE, k
            if stats:
                compare_statistics(g, w, what="m256 step %d: " % k)
            elif k in (1, 7):
                slot = w.last_buffer_index
                ws = scenarios.dense_from_compact(w.index_buffer[slot], w.hit_count_buffer[slot], w.total_count_buffer[slot], w.min_height_buffer[slot])
                wf = scenarios.dense_from_compact(w.combined_index_map, w.combined_hit_count, w.combined_total_count, w.combined_min_height)
                for got_d, want_d, what in ((g.read_dense(slot), ws, "slot"), (g.read_dense(gvom_mod.GVOM_WHICH_FUSED), wf, "fused")):
                    for j, nm in enumerate(("state", "hit", "total", "minh")):
                        assert np.array_equal(np.asarray(want_d[j]), got_d[j]), "step %d %s %s" % (k, what, nm)
        assert g.get_tuning("eager_adopted") == 8
        del g
    finally:
        oracle.use_all_cores(False)
        free()


@pytest.mark.parametrize("cfg", ["c3", "c4", "c5"])
def test_voxel_statistics_match_oracle_at_full_size(gvom_mod, cfg):
    """Statistics on both sides at BASELINE sizes: c3 (OS1-128 scans, buffer 8) over 12 scans -- the ring fills, wraps and evicts
    four slots; c4 at its BASELINE settings (512 x 512 x 128, buffer 4, 1,048,576 returns) over 3 scans; one c5 tick (1024 x
    1024 x 128, 4,194,304 returns: k_fuse_stats at its 8,192-workgroup cap, k_voxel_cloud in many grid-stride passes)."""
    n_scans = {"c3": 12, "c4": 3, "c5": 1}[cfg]
    if cfg == "c5" and _free_ram_gb() < 24.0:
        pytest.skip("needs 24 GB of free host memory at 134 M voxels")
    params, scans = synth.config_inputs(cfg, n_scans=n_scans)
    steps = []
    for pc, ego, tf in scans:
        steps += [("scan", pc, ego, tf), ("combine",)]
    oracle.use_all_cores(True, threads=16)
    try:
        _, _, checked = _stats_steps(gvom_mod, params, steps, what=cfg)
    finally:
        oracle.use_all_cores(False)
    assert checked == n_scans


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_voxel_statistics_match_oracle(world):
    """The slab-sharded statistics (thread ranks on one GPU; only the direct form of k_stats: a neighbour's moments may live on
    another rank) against the ORACLE, not only against the unsharded handle: the ranks' debug voxel clouds together are the
    oracle's cloud (positions, hit counts exact, solid factors 1e-6, eigenvalue columns to parity.STATS_TOL["cloud"])."""
    import contextlib
    import io
    from shard_threads import run_ranks
    params = (0.2, 0.2, 64, 32, 2, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
    scene = synth.make_scene(2, extent=5.5)
    steps = []
    for k in range(5):
        ego = (0.5 * k, -0.35 * k, 0.04 * k)
        shares = [synth.lidar_scan(scene, beams=16, azimuths=512, sensor=ego, yaw=0.002 * r, noise_seed=10 * k + r, dtype=np.float32)[:8192 - 701 * r]
                  for r in range(world)]
        steps.append((shares, ego))
    w = oracle.OracleGvom(*params, voxel_statistics=True)
    want = []
    for shares, ego in steps:
        w.process_pointcloud(np.concatenate(shares, 0), ego)
        want.append((w.combine_maps(), w.make_debug_voxel_map()))

    def body(r, sh):
        parts = []
        for (shares, ego), (wmaps, _) in zip(steps, want):
            sh.process_pointcloud(shares[r], ego)
            got = sh.combine_maps()
            _same_maps(got, wmaps, "rank %d" % r)
            parts.append(np.array(sh.make_debug_voxel_map(), copy=True))
        return parts

    with contextlib.redirect_stdout(io.StringIO()):
        parts = run_ranks(world, params, body, voxel_statistics=True)
    for k, (_, wcloud) in enumerate(want):
        compare_cloud(np.concatenate([parts[r][k] for r in range(world)], 0), wcloud, what="%d ranks step %d: " % (world, k))


@pytest.mark.parametrize("seed", range(24))
def test_fuzz_voxel_statistics_match_oracle(gvom_mod, seed):
    """The edge-case fuzz (_fuzz_case, fresh seeds) with the statistics on both sides, (xy_eigen_dist, z_eigen_dist) drawn from
    {0, 1, 2}^2, and every third seed snapped to the shapes the eager fusion takes (buffer 1, xy_size % 16 == 0, z_size >= 4)."""
    params, steps = _fuzz_case(3000 + seed)
    rng = np.random.default_rng(5000 + seed)
    params = params[:12] + (int(rng.integers(0, 3)), int(rng.integers(0, 3)))
    if seed % 3 == 0:
        params = params[:2] + (16 * max(1, min(4, round(params[2] / 16))), max(4, params[3]), 1) + params[5:]
    _stats_steps(gvom_mod, params, steps, what="seed %d" % seed)
