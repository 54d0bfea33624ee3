"""Multi-origin scans, the part that needs no GPU: gvom.column_origins against the formula of include/gvom_hip.h, the header and
the binding, and the referee of tests/test_multi_origin.py (tests/multi_origin_ref.py) held to the oracle it is built from."""
import inspect
import os
import re

import numpy as np
import pytest

import gvom
import multi_origin_ref as mo
import scenarios
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_column_origins_is_the_formula():
    W = 7
    rng = np.random.default_rng(5)
    cols = np.tile(np.eye(4), (W, 1, 1))
    cols[:, :3, :] = rng.normal(size=(W, 3, 4))
    tf = np.eye(4)
    tf[:3, :] = rng.normal(size=(3, 4))
    got = gvom.column_origins(cols, tf)
    assert got.shape == (W, 3) and got.dtype == np.float64
    for w in range(W):
        t0, t1, t2 = cols[w, 0, 3], cols[w, 1, 3], cols[w, 2, 3]
        for k in range(3):
            assert got[w, k] == ((t0 * tf[k, 0] + t1 * tf[k, 1]) + t2 * tf[k, 2]) + tf[k, 3]
    plain = gvom.column_origins(cols)
    assert np.array_equal(plain, cols[:, :3, 3]) and plain.flags.c_contiguous
    assert np.array_equal(gvom.column_origins(cols[:, :3, :], tf), got)           # [W, 3, 4] poses
    for bad in (np.zeros((W, 4)), np.zeros((W, 2, 4)), np.zeros((W, 4, 3))):
        with pytest.raises(ValueError):
            gvom.column_origins(bad)
    with pytest.raises(ValueError):
        gvom.column_origins(cols, np.eye(3))


def test_header_declares_and_binding_binds_the_entry_points():
    header = open(os.path.join(ROOT, "include", "gvom_hip.h")).read()
    bound = {name: args for name, _, args in gvom.ABI}
    for name, nargs in (("gvom_process_pointcloud_origins", 11), ("gvom_process_range_image_origins", 9)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, name + " is not declared in include/gvom_hip.h"
        assert len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == nargs
        assert name in bound and len(bound[name]) == nargs
    assert re.search(r"#define\s+GVOM_ABI_VERSION\s+10\b", header) and gvom.ABI_VERSION == 10
    assert "multi_origin" in header
    for meth in ("process_pointcloud_origins", "process_pointcloud_origins_device", "process_range_image_origins",
                 "process_range_image_origins_device"):
        assert callable(getattr(gvom.Gvom, meth))
    # the range-image form takes what the plain call takes, and the plain calls keep their signatures
    for plain, form in (("process_range_image", "process_range_image_origins"),
                        ("process_range_image_device", "process_range_image_origins_device")):
        assert list(inspect.signature(getattr(gvom.Gvom, plain)).parameters) == list(inspect.signature(getattr(gvom.Gvom, form)).parameters)
    assert list(inspect.signature(gvom.Gvom.process_range_image).parameters)[1:] == [
        "ranges", "ego_position", "transform", "column_transforms", "cloud_dtype"]


def test_binding_checks_arguments_before_the_library_is_touched():
    g = object.__new__(gvom.Gvom)                                   # no handle: a check that reached the library would fail differently
    pc = np.zeros((10, 3), np.float32)
    for origins in (np.zeros((0, 3)), np.zeros((65537, 3)), np.array([[0.0, np.nan, 0.0]]), np.zeros((4, 2))):
        with pytest.raises(ValueError):
            g.process_pointcloud_origins(pc, origins, (0, 0, 0))
        with pytest.raises(ValueError):
            g.process_pointcloud_origins_device(0, 10, np.float32, origins, (0, 0, 0))
    for index in (np.full(10, 2), np.full(10, -1), np.zeros(9, np.int64)):
        with pytest.raises(ValueError):
            g.process_pointcloud_origins(pc, np.zeros((2, 3)), (0, 0, 0), origin_index=index)
    with pytest.raises(ValueError):
        g.process_range_image_origins(np.zeros((2, 4), np.uint16), (0, 0, 0))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_referee_reduces_to_the_oracle_for_one_origin(dtype):
    prm = mo.params("p2", 2)
    a, b = mo.MultiOriginOracle(*prm, voxel_statistics=True), oracle.OracleGvom(*prm, voxel_statistics=True)
    for k in range(2):
        pc, _, _, ego, tf = mo.scan_inputs("p2", k, dtype)
        a.process_pointcloud_origins(pc, [ego], ego, tf)
        b.process_pointcloud(pc, ego, tf)
        slot = b.last_buffer_index
        assert a.last_buffer_index == slot and a.last_scan_updates == b.last_scan_updates
        for name in ("index_buffer", "hit_count_buffer", "total_count_buffer", "min_height_buffer", "origin_buffer", "metrics_buffer"):
            assert np.array_equal(getattr(a, name)[slot], getattr(b, name)[slot]), name
        for u, v in zip(a.combine_maps(), b.combine_maps()):
            assert np.array_equal(u, v)


@pytest.mark.parametrize("grid", sorted(mo.GRIDS))
def test_inputs_can_tell_a_scan_that_ignores_the_origins(grid):
    """what tests/test_multi_origin.py relies on, under the oracle alone: enough returns in the grid, enough per origin, the
    out-of-window origin adds endpoints only, the return that is its own origin takes no step, `hit` is the single-origin
    scan's and `total` is not"""
    prm = mo.params(grid, 2)
    ref = mo.MultiOriginOracle(*prm)
    for k in range(3):
        dtype = np.float32 if k != 1 else np.float64
        pc, origins, index, ego, tf = mo.scan_inputs(grid, k, dtype)
        assert pc.dtype == dtype and origins.shape == (mo.K, 3) and np.bincount(index).min() >= 1000
        world = pc if tf is None else mo.apply_transform(pc, tf)
        assert np.array_equal(origins[4], world[np.nonzero((world == origins[4].astype(dtype)).all(axis=1))[0][0]].astype(np.float64))
        ref.process_pointcloud_origins(pc, origins, ego, tf, index)
        assert ref.last_scan_points_in_grid >= 0.2 * mo.N
        slot = ref.last_buffer_index
        hit = scenarios.dense_from_compact(ref.index_buffer[slot], ref.hit_count_buffer[slot], ref.total_count_buffer[slot],
                                           ref.min_height_buffer[slot])[1]
        # origin 3 lies outside the window: every add of its fifth is an endpoint's (hit and total: two adds per endpoint)
        sub = world[index == 3]
        ends = oracle.point_2_map(prm[0], prm[1], prm[2], prm[3], ref.min_distance, sub, ego,
                                  ref.origin_buffer[slot])[0].sum()
        assert 0 < ref.adds_per_origin[3] <= 2 * ends
        single = mo.single_origin_total(prm, pc, ego, tf)
        assert int((ref.last_tmp_total != single).sum()) > 1000
        assert hit.sum() == ref.last_scan_points_in_grid
