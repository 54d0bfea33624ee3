"""Pins the CPU oracle against end-to-end golden vectors recorded from the reference
(tests/golden/f*.npz).  Every recorded per-slot dense accumulator,
fused map, internal 2-D map and returned map must be reproduced: ints bit-exact, floats
exactly except log/atan2-derived maps (1e-9: same glibc on both sides)."""
import os

import numpy as np
import pytest

import scenarios
from parity import compare_records
from oracle import oracle

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["f1", "f2", "f3", "f4", "f5", "f6", "f7"]


@pytest.fixture(params=["one_thread", "all_cores"])
def oracle_build(request):
    """the oracle's two builds of the same source: one thread, and OpenMP on all host cores
    (bench.py's cpu_baseline times both); both are held to the reference's vectors"""
    n = oracle.use_all_cores(request.param == "all_cores", threads=8 if request.param == "all_cores" else None)
    assert n >= 1
    yield request.param
    oracle.use_all_cores(False)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_reference(name, capsys, oracle_build):
    path = os.path.join(G, name + ".npz")
    if not os.path.exists(path):
        pytest.skip("fixture %s not generated yet" % name)
    want = np.load(path)
    sc = scenarios.scenario_from_record(want)
    # F1..F6 also pin the optional per-voxel statistics (debug voxel cloud: eigenvalues of the
    # merged covariances); the oracle restates the reference's two-pass f64 accumulation in the
    # same order, so it agrees to float32 rounding (one-thread build only: the statistics passes
    # are not parallelised)
    stats = name != "f7" and oracle_build == "one_thread"
    got = scenarios.run_and_record(lambda *p: oracle.OracleGvom(*p, voxel_statistics=stats), sc,
                                   record_debug=(name != "f7"))
    n = compare_records(got, want, float_tol=1e-9, stats_rtol=2e-6, stats_atol=1e-7,
                        skip=() if stats or name == "f7" else ("debug_voxel_map",))      # (this build runs without them)
    assert n > 5
    if stats:
        assert any(k.endswith("debug_voxel_map") for k in got)


def test_warning_strings_and_return_types(capsys):
    g = oracle.OracleGvom(0.4, 0.4, 16, 8, 2, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
    assert g.combine_maps() is None
    assert "[WARNING] The map buffer is empty, nothing will happen!" in capsys.readouterr().out
    assert g.process_pointcloud(np.zeros((0, 3)), (0, 0, 0)) is None
    assert "[WARNING] Processing an empty pointcloud, nothing will happen!" in capsys.readouterr().out
    g.process_pointcloud(np.full((4, 3), 500.0), (0, 0, 0))
    assert "[WARNING] The pointcloud points don't overlap with any voxels, nothing will happen!" \
        in capsys.readouterr().out
    assert g.buffer_index == 0
    rng = np.random.default_rng(0)
    pc = np.stack([rng.uniform(-3, 3, 300), rng.uniform(-3, 3, 300), rng.uniform(-1.5, .5, 300)], 1)
    g.process_pointcloud(pc, (0, 0, 0), np.eye(4))
    out = g.combine_maps()
    assert [o.dtype for o in out] == [np.float64, np.int32, np.int32, np.float64, np.int32]
    assert [o.shape for o in out] == [(3,), (16, 16), (16, 16), (16, 16), (16, 16)]
    # SURVEY Appendix C end-to-end smoke values
    assert np.allclose(out[0], [-3.2, -3.2, -1.6])
    assert np.count_nonzero(out[1]) == 207 and np.count_nonzero(out[2]) == 0
    assert out[4].sum() == 250
    assert out[3].min() == pytest.approx(-7.333893209065674, abs=1e-9)


ROS_SHORT = ("hard", "soft", "certainty", "negative", "roughness")


def test_ros_postprocessing_matches_the_reference_node():
    """SURVEY 8f rank 3, pinned by the reference itself: tests/golden/ros_f3.npz holds what the
    UNMODIFIED VoxelMapper.cb_timer (reference gvom_ros.py:113-165, imported with stand-ins for the ROS packages:
    tests/golden/make_ros_golden.py) published for recorded combine_maps() tuples -- the reference's own outputs of
    F3 / F4 / F5 and one tuple that walks the value ranges -- under the node's default parameters and under a
    second set (density 12.5, roughness -6 .. 1.5).  oracle.ros_occupancy_grids must reproduce every int8 array."""
    rec = np.load(os.path.join(G, "ros_f3.npz"))
    n = 0
    for p in rec["param_sets"]:
        thr = (float(rec[p + "_density_threshold"]), float(rec[p + "_min_roughness"]), float(rec[p + "_max_roughness"]))
        for tag in rec["tags"]:
            tup = tuple(rec["in_%s_%s" % (tag, f)] for f in ("origin_world", "positive", "negative", "roughness", "visibility"))
            got = oracle.ros_occupancy_grids(tup, *thr)
            for short, g in zip(ROS_SHORT, got):
                w = rec["%s_%s_%s" % (p, tag, short)]
                assert g.dtype == np.int8 and np.array_equal(g, w), (p, tag, short, int(np.sum(g != w)))
                n += 1
            assert np.array_equal(rec["%s_%s_all_certainty" % (p, tag)], got[2])          # gvom_ros.py:152-153: one array, two topics
            assert np.array_equal(rec["%s_%s_origin_xy" % (p, tag)], tup[0][:2])          # gvom_ros.py:137-138
    assert n == 2 * 7 * 5
