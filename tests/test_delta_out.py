"""combine_maps() stores only the runs of the returned maps that changed (k_map2d's DELTA form, include/gvom_hip.h
"ONLY WHAT CHANGED IS STORED"): a run of 32 cells in x that is default now and was default the last time the library wrote the
same pinned buffer does not cross the host link again.  What the caller reads must not depend on it.

Every comparison is against the same calls on a twin mapper with set_tuning("delta_out", 0) -- bit for bit -- or against the CPU
oracle (int maps exact, roughness to 1e-5, the tolerance of the parity suite: log / atan2 may differ from glibc in the last ulp).
Small grids: 64 x 64 x 32 is 2 x 8 of k_map2d's 32 x 8 tiles; 50 x 50 has partial tiles in both axes and takes the generic fusion."""
import gc

import numpy as np
import pytest

import gvom
from oracle import oracle

pytestmark = pytest.mark.gpu

RES, ZRES = 0.4, 0.2
MAPS = (("positive", 0), ("negative", 0), ("roughness", -1.0), ("visibility", 0))     # out[1 + i], its default


def params(xy=64, ring=1):
    return (RES, ZRES, xy, 32, ring, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)


def ground(seed, ego, radius=5.0, n=5000):
    """returns on a rough ground disc around the ego: most of the window stays empty"""
    rng = np.random.default_rng(seed)
    r, a = radius * np.sqrt(rng.uniform(0.07, 1.0, n)), rng.uniform(0, 2 * np.pi, n)
    x, y = ego[0] + r * np.cos(a), ego[1] + r * np.sin(a)
    z = -0.8 + 0.15 * np.sin(1.3 * x) * np.cos(0.9 * y) + rng.normal(0, 0.02, n)
    return np.stack([x, y, z], axis=1).astype(np.float32)


def block(seed, centre, n=400):
    """an obstacle: returns in a 0.3 m column from the ground up to 0.6 m above it"""
    rng = np.random.default_rng(seed)
    return np.stack([centre[0] + rng.uniform(-0.15, 0.15, n), centre[1] + rng.uniform(-0.15, 0.15, n),
                     rng.uniform(-0.8, -0.2, n)], axis=1).astype(np.float32)


def far_ring(ego, n=2048):
    """a sweep without a return inside the window: every ray ends 60 m out (free space only, no height anywhere)"""
    a = 2 * np.pi * np.arange(n) / n
    return np.stack([ego[0] + 60 * np.cos(a), ego[1] + 60 * np.sin(a), ego[2] - 2.0 + 0 * a], axis=1).astype(np.float32)


def moving_window(xy):
    """12 (cloud, ego): the window shifts by +1 / -1 / 0 cells in x and in y between scans; an obstacle near the +x edge, outside
    the rows the ground disc reaches, is seen by the first two scans and leaves the window when it has moved 3 cells in -x"""
    dx = (0, -1, -1, -1, -1, -1, 0, +1, +1, 0, -1, +1)
    dy = (0, +1, 0, -1, -1, 0, +1, +1, 0, -1, 0, +1)
    cx, cy = np.cumsum(dx), np.cumsum(dy)
    obstacle = (RES * (xy // 2 - 3) + 0.2, RES * (xy // 2 - 10) + 0.2)
    scans = []
    for k in range(12):
        ego = (RES * cx[k] + 0.13, RES * cy[k] + 0.13, 0.0)
        pc = ground(k, ego, radius=RES * xy / 5.0)
        if k < 2:
            pc = np.concatenate([pc, block(100 + k, obstacle)], 0)
        scans.append((pc, ego))
    return scans


def same_bits(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def default_runs(a, default):
    """a[x, y] -> bool[ceil(xy / 32), xy]: run (x // 32, y) holds only the default"""
    xy = a.shape[0]
    return np.stack([(a[x0:x0 + 32] == default).all(axis=0) for x0 in range(0, xy, 32)])


def assert_oracle(got, want):
    assert np.array_equal(got[0], want[0])
    for i in (1, 2, 4):
        assert got[i].dtype == np.int32 and np.array_equal(got[i], want[i]), MAPS[i - 1][0]
    assert np.allclose(got[3], want[3], rtol=0, atol=1e-5), "roughness"


def record_bits(g, out):
    rec = g.output_record(out[1])
    assert rec is not None, "the buffer has no content record"
    return rec


def twins(prm):
    g1, g0 = gvom.Gvom(*prm), gvom.Gvom(*prm)
    g0.set_tuning("delta_out", 0)
    assert g1.get_tuning("delta_out") == 1 and g0.get_tuning("delta_out") == 0
    return g1, g0


@pytest.mark.parametrize("xy,ring", [(64, 1), (64, 3), (50, 1)])
def test_window_in_motion(xy, ring):
    g1, g0 = twins(params(xy, ring))
    ref = oracle.OracleGvom(*params(xy, ring))
    prev_runs, gone, gen, skipped = None, 0, None, 0
    for k, (pc, ego) in enumerate(moving_window(xy)):
        for g in (g1, g0, ref):
            g.process_pointcloud(pc.copy(), ego)
        out1, out0 = g1.combine_maps(), g0.combine_maps()
        assert same_bits(out1, out0), "step %d differs from delta_out=0" % k
        assert_oracle(out0, ref.combine_maps())
        bits, g_now = record_bits(g1, out1)
        assert gen is None or g_now == gen, "step %d: the record restarted (the buffer was not recycled?)" % k
        gen = g_now
        assert g0.output_record(out0[1]) is None
        runs = [default_runs(out0[1 + i], d) for i, (_, d) in enumerate(MAPS)]
        # the record says "non-default" exactly for the runs that are: every map's set bits = its non-default runs
        assert int(np.unpackbits(bits).sum()) == sum(int((~r).sum()) for r in runs)
        if prev_runs is not None:
            gone += sum(int((~p & r).sum()) for p, r in zip(prev_runs, runs))
            skipped += sum(int((p & r).sum()) for p, r in zip(prev_runs, runs))
        prev_runs = runs
        del out1, out0                                      # one recycled buffer per mapper
    assert gone > 0, "no run went from non-default back to default: the scene does not test that"
    assert skipped > 0, "no run was ever skippable: the scene does not test the mechanism"
    assert g1.get_tuning("output_records") == 1 and g0.get_tuning("output_records") == 0


def test_poisoned_buffer_and_a_second_buffer():
    g1, g0 = twins(params())
    scans = moving_window(64)

    def step(k):
        for g in (g1, g0):
            g.process_pointcloud(scans[k][0].copy(), scans[k][1])

    step(0)
    out1, out0 = g1.combine_maps(), g0.combine_maps()
    assert same_bits(out1, out0)
    _, gen = record_bits(g1, out1)
    for a in (out1[1], out1[2], out1[4]):
        a.fill(0x5A5A5A5A)
    out1[3].T.view(np.uint64)[...] = 0x5A5A5A5A5A5A5A5A
    g1.forget(out1[3])
    assert g1.get_tuning("output_records") == 0
    poisoned = out1[1].__array_interface__["data"][0]
    del out1, out0, a
    step(1)
    out1, out0 = g1.combine_maps(), g0.combine_maps()
    assert out1[1].__array_interface__["data"][0] == poisoned, "the poisoned buffer did not come back"
    assert same_bits(out1, out0), "a forgotten buffer must be stored in full"
    assert record_bits(g1, out1)[1] != gen                  # (its record started over)
    # the previous result is held: the next combine gets a buffer the library has never written
    step(2)
    held = out1
    second = g1.combine_maps()
    ref2 = g0.combine_maps()
    assert not np.shares_memory(held[1], second[1])
    assert same_bits(second, ref2)
    assert same_bits(held, out0), "the held result changed"
    assert g1.get_tuning("output_records") == 2
    # ... and both buffers keep working, whichever the pool hands out
    del held, second, out1, out0, ref2
    for k in (3, 4, 5):
        step(k)
        a, b = g1.combine_maps(), g0.combine_maps()
        assert same_bits(a, b), "step %d" % k
        del a, b


def test_interleaved_entry_points():
    g1, g0 = twins(params())
    for k, (pc, ego) in enumerate(moving_window(64)):
        for g in (g1, g0):
            g.process_pointcloud(pc.copy(), ego)
        kind = k % 3
        if kind == 0:
            a, b = g1.combine_maps(), g0.combine_maps()
        elif kind == 1:                                     # the int8 grids go into the same pooled block: its record must go
            a, b = g1.combine_maps_occupancy(), g0.combine_maps_occupancy()
        else:
            a, b = g1.combine_maps_async().result(), g0.combine_maps_async().result()
        assert same_bits(a, b), "step %d (%s)" % (k, ("combine_maps", "combine_maps_occupancy", "combine_maps_async")[kind])
        if kind == 1:
            assert g1.get_tuning("output_records") == 0
        del a, b
    # the same with the knob toggled in between: a record never survives a combine that did not use it
    for k, (pc, ego) in enumerate(moving_window(64)[:6]):
        for g in (g1, g0):
            g.process_pointcloud(pc.copy(), ego)
        g1.set_tuning("delta_out", 0 if k in (2, 3) else 1)
        a, b = g1.combine_maps(), g0.combine_maps()
        assert same_bits(a, b), "toggle step %d" % k
        del a, b


def empty_scan_steps():
    """a full scan; a sweep without a return in the window (the reference REJECTS such a scan, gvom.py:148-150: the map stays); the
    emptiest scan it accepts -- 50 returns in one voxel -- in a window 500 m away, where nothing of the old map is left; a full one"""
    ego, ego_far = (0.13, 0.13, 0.0), (500.0 + 0.13, 0.13, 0.0)
    rng = np.random.default_rng(7)
    speck = (np.array([ego_far[0] + 3.0, ego_far[1] + 1.0, -0.7]) + rng.uniform(-0.05, 0.05, (50, 3))).astype(np.float32)
    return [(ground(0, ego, radius=11.0, n=20000), ego), (far_ring(ego), ego), (speck, ego_far), (ground(1, ego_far), ego_far)]


def test_empty_scan_after_a_full_one():
    # robot_radius 0: the reference gives every cell within robot_radius of the ego a height (gvom.py:531-533), scan or no scan
    prm = params()[:10] + (0.0,) + params()[11:]
    g1, g0 = twins(prm)
    ref = oracle.OracleGvom(*prm)
    for k, (pc, ego) in enumerate(empty_scan_steps()):
        for g in (g1, g0, ref):
            g.process_pointcloud(pc.copy(), ego)
        out1, out0, want = g1.combine_maps(), g0.combine_maps(), ref.combine_maps()
        assert_oracle(out1, want)
        assert same_bits(out1, out0)
        bits, _ = record_bits(g1, out1)
        nondefault = [int((want[1 + i] != d).sum()) for i, (_, d) in enumerate(MAPS)]
        runs = sum(int((~default_runs(want[1 + i], d)).sum()) for i, (_, d) in enumerate(MAPS) if i != 2)
        runs += int((~default_runs(out0[3], -1.0)).sum())   # (roughness: the library's own values, held to the oracle's above)
        assert int(np.unpackbits(bits).sum()) == runs
        if k == 2:
            # every run has gone back to default but the one visible cell's and what hangs on it (an accepted scan has a voxel,
            # a voxel a height)
            assert nondefault[3] == 1 and sum(nondefault) <= 2 and runs <= 2, nondefault
        else:
            assert min(nondefault[2:]) > 100 and runs > 20
        del out1, out0


def test_two_mappers_in_one_process():
    a1, a0 = twins(params(64, 1))
    b1, b0 = twins(params(50, 2))
    sa, sb = moving_window(64), moving_window(50)
    for k in range(8):
        for g in (a1, a0):
            g.process_pointcloud(sa[k][0].copy(), sa[k][1])
        for g in (b1, b0):
            g.process_pointcloud(sb[11 - k][0].copy(), sb[11 - k][1])
        oa, ob = a1.combine_maps(), b1.combine_maps()
        assert same_bits(oa, a0.combine_maps()), "mapper A, step %d" % k
        assert same_bits(ob, b0.combine_maps()), "mapper B, step %d" % k
        assert a1.get_tuning("output_records") == 1 and b1.get_tuning("output_records") == 1
        del oa, ob
        gc.collect()
