"""Multi-origin scans on the GPU (Gvom.process_pointcloud_origins / process_range_image_origins): return
i traced from origins[index[i]] instead of from the ego.  The referee is the unmodified CPU oracle, one orc_point_2_map call per
origin onto the same arrays (tests/multi_origin_ref.py): integers exact, roughness within the 1e-5 every comparison with glibc
uses.  Inputs: 8,192 returns, five origins -- the ego, the window's edge region, a few decimetres off, outside the window, one
of its own returns -- on the smallest grid of each kind of step body."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import multi_origin_ref as mo
import parity
import scenarios
import synth
from oracle import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gvom_mod():
    import gvom
    rc, info = gvom.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    return gvom


def _make(gvom_mod, prm, **kw):
    kw.setdefault("voxel_statistics", False)
    return gvom_mod.Gvom(*prm, **kw)


def _same_maps(a, b, what):
    assert (a is None) == (b is None), what
    if a is None:
        return
    for k, (u, v) in enumerate(zip(a, b)):
        assert np.array_equal(np.asarray(u), np.asarray(v)), "%s: returned map %d differs" % (what, k)


def _same_dense(a, b, what):
    assert (a is None) == (b is None), what
    for k, name in enumerate(("state", "hit", "total", "min-height", "origin")):
        assert np.array_equal(a[k], b[k]), "%s: %s differs in %d places" % (what, name, int(np.sum(a[k] != b[k])))


def _slot_against_referee(g, ref, what):
    slot = ref.last_buffer_index
    assert (g.buffer_index, g.last_buffer_index) == (ref.buffer_index, slot), what
    want = scenarios.dense_from_compact(ref.index_buffer[slot], ref.hit_count_buffer[slot], ref.total_count_buffer[slot],
                                        ref.min_height_buffer[slot])
    got = g.read_dense(slot)
    for j, name in enumerate(("state", "hit", "total", "min-height")):
        assert np.array_equal(np.asarray(want[j]), got[j]), "%s: slot %s differs in %d voxels" % (
            what, name, int(np.sum(np.asarray(want[j]) != got[j])))
    st = g.scan_stats()
    assert st["cells"] == len(ref.hit_count_buffer[slot]), what
    assert st["sum_hit"] == int(ref.hit_count_buffer[slot].sum(dtype=np.int64)), what
    # (ray passes of the free voxels included: the referee's whole `total` array, as orc_point_2_map left it)
    assert st["sum_total"] == int(ref.last_tmp_total.sum(dtype=np.int64)), what


def _maps_against_referee(g, ref, got, want, what):
    assert got is not None and want is not None, what
    assert np.array_equal(got[0], want[0]), what
    for j in (1, 2, 4):                                          # positive, negative, visibility: integers
        assert np.array_equal(got[j], want[j]), "%s: integer map %d differs from the referee" % (what, j)
    assert np.allclose(got[3], want[3], rtol=0, atol=1e-5), what + ": roughness"
    assert g.combined_cell_count_cpu == ref.combined_cell_count_cpu, what


# (grid, ring slots, eager knob, cloud dtype of scans 0 and 2; scan 1 takes the other one)
PIPELINE = [("p2", 2, None, np.float32), ("np2", 2, None, np.float64), ("tall", 2, None, np.float32),
            ("p2", 1, 1, np.float64), ("p2", 1, 0, np.float32), ("np2", 1, 1, np.float32), ("np2", 1, 0, np.float64),
            ("tall", 1, 1, np.float64), ("tall", 1, 0, np.float32)]


@pytest.mark.parametrize("grid,B,eager,dtype", PIPELINE,
                         ids=["%s-B%d-%s-%s" % (g, b, "auto" if e is None else "eager%d" % e, np.dtype(d).name) for g, b, e, d in PIPELINE])
def test_pipeline_against_the_referee(gvom_mod, grid, B, eager, dtype):
    """three scans + a combine after each: the ring slot (state, hit, total, min-height) and scan_stats after every scan, the
    returned maps and the cell count after every combine.  B = 1 is the eager k_encfuse route, forced on and forced off.  Fails
    on a build that ignores the origins: the referee's `total` is asserted to differ from the single-origin scan's."""
    prm = mo.params(grid, B)
    g, ref = _make(gvom_mod, prm), mo.MultiOriginOracle(*prm)
    assert g.get_tuning("multi_origin") == 1
    if eager is not None:
        g.set_tuning("eager", eager)
    other = np.float64 if dtype == np.float32 else np.float32
    for k in range(3):
        pc, origins, index, ego, tf = mo.scan_inputs(grid, k, dtype if k != 1 else other)
        # scan 2 hands no index over: i % K (the referee gets the same rule)
        use = index if k != 2 else None
        assert g.process_pointcloud_origins(pc, origins, ego, tf, use) is None
        ref.process_pointcloud_origins(pc, origins, ego, tf, use)
        what = "%s B=%d scan %d" % (grid, B, k)
        # the input can tell, and no test hides behind an empty grid
        assert ref.last_scan_points_in_grid >= 0.2 * mo.N, what
        assert np.bincount(index if use is not None else np.arange(mo.N) % mo.K).min() >= 1000
        assert int((ref.last_tmp_total != mo.single_origin_total(prm, pc, ego, tf)).sum()) > 1000, what
        assert g.get_tuning("multi_origin_ran") == 1 and g.get_tuning("interleave") == 1 and g.get_tuning("dirsort") == 0
        _slot_against_referee(g, ref, what)
        _maps_against_referee(g, ref, g.combine_maps(), ref.combine_maps(), what.replace("scan", "combine"))
    if eager == 1:
        assert g.get_tuning("eager_adopted") == 3
    if eager == 0:
        assert g.get_tuning("eager_adopted") == 0


@pytest.mark.parametrize("stats", [False, True], ids=["plain", "statistics"])
@pytest.mark.parametrize("grid", ["p2", "np2"])
def test_one_origin_at_the_ego_is_process_pointcloud(gvom_mod, grid, stats):
    """K = 1, origins = [ego]: bit for bit the single-origin call on a second handle.  With statistics the debug voxel cloud has
    the same rows: positions, solid factor and hit counts exactly; the eigenvalue columns come out of float atomics whose order
    differs from run to run of the SAME call, so they are held to the bound two runs of process_pointcloud are held to
    (parity.STATS_TOL["cloud"]) -- the statistics never see an origin."""
    prm = mo.params(grid, 2)
    a, b = _make(gvom_mod, prm, voxel_statistics=stats), _make(gvom_mod, prm, voxel_statistics=stats)
    for k in range(3):
        pc, _, _, ego, tf = mo.scan_inputs(grid, k, np.float32 if k != 1 else np.float64)
        a.process_pointcloud_origins(pc, [ego], ego, tf, None if k else np.zeros(mo.N, np.uint16))
        b.process_pointcloud(pc, ego, tf)
        assert a.get_tuning("multi_origin_ran") == 1 and b.get_tuning("multi_origin_ran") == 0
        _same_dense(a.read_dense(a.last_buffer_index), b.read_dense(b.last_buffer_index), "scan %d" % k)
        assert a.scan_stats() == b.scan_stats()
        _same_maps(a.combine_maps(), b.combine_maps(), "combine %d" % k)
        if stats:
            ca, cb = parity.compare_cloud(a.make_debug_voxel_map(), b.make_debug_voxel_map(), what="combine %d: " % k)
            assert ca.shape[0] > 1000 and np.array_equal(ca[:, :5], cb[:, :5])


@pytest.mark.parametrize("grid", ["p2", "np2"])
def test_knobs_never_change_a_result(gvom_mod, grid):
    prm = mo.params(grid, 2)
    pc, origins, index, ego, tf = mo.scan_inputs(grid, 1, np.float32)

    def run(knob=None, value=None):
        g = _make(gvom_mod, prm)
        if knob:
            g.set_tuning(knob, value)
        g.process_pointcloud_origins(pc, origins, ego, tf, index)
        out = (g.read_dense(0), g.combine_maps(), g.get_tuning("segs"), g.get_tuning("interleave"), g.get_tuning("dirsort"))
        return out
    base = run()
    assert base[0][5] > 1000
    for knob, value in (("dirsort", -1), ("dirsort", 1), ("dirsort", 2), ("interleave", 1), ("interleave", 4), ("segs", 1),
                        ("segs", 9), ("fastdiv", 0)):
        got = run(knob, value)
        what = "%s %s=%d" % (grid, knob, value)
        _same_dense(got[0], base[0], what)
        _same_maps(got[1], base[1], what)
        # what actually ran: a forced order the route cannot honour is ignored
        assert got[3] == 1 and got[4] == 0, what
        if knob == "segs":                                       # (9 is capped by the rays' longest possible walk, never below the default)
            assert got[2] == 1 if value == 1 else base[2] <= got[2] <= 9, what


@pytest.mark.parametrize("with_tf", [False, True], ids=["no-transform", "transform"])
@pytest.mark.parametrize("cloud_dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("range_dtype", [np.uint16, np.float32], ids=["u16", "rf32"])
def test_range_image_traced_from_its_columns(gvom_mod, range_dtype, cloud_dtype, with_tf):
    """A: the image through process_range_image_origins; B: its cloud through process_pointcloud_origins with column_origins();
    the referee: the same.  C: the plain process_range_image -- on a handle whose previous scan was traced from the columns --
    against D, a handle that never heard of origins: today's call, bit for bit."""
    prm = mo.params("p2", 2)
    H, W = 16, 512
    scene = synth.make_scene(2, extent=10.0)
    el = np.linspace(-24.0, 3.0, H)
    scale = 0.001 if range_dtype == np.uint16 else 1.0
    A, B, C, D = (_make(gvom_mod, prm) for _ in range(4))
    ref = mo.MultiOriginOracle(*prm)
    for k in range(2):
        sensor = (0.5 * k, -0.3 * k, 0.05 * k)
        raw, dirs, offs = synth.range_image_scan(scene, H, W, sensor, 0.0, k, range_dtype, dropout=0.1, elevations_deg=el)
        if k == 0:
            for h in (A, C, D):
                h.set_sensor_model(dirs, offs, scale, 0.8, 45.0)
        tf = gvom_mod.transform_from_translation_rotation(sensor, (0.01, -0.02, 0.05 * k, 1.0)) if with_tf else None
        ego = sensor if with_tf else (0.7, 0.0, 0.0)             # (without a transform the sweep is around the world origin)
        cols = mo.column_poses(W, k)
        full = gvom_mod.unproject_range_image(raw, dirs, offs, scale, 0.8, 45.0, cols, cloud_dtype)
        O = gvom_mod.column_origins(cols, tf)
        assert O.shape == (W, 3) and np.ptp(O[:, 0]) > 1.2        # several voxels of 0.4 m
        assert A.process_range_image_origins(raw, ego, tf, cols, cloud_dtype) is None
        B.process_pointcloud_origins(full, O, ego, tf)
        kept = ~np.isnan(full[:, 0])
        ref.process_pointcloud_origins(full[kept], O, ego, tf, (np.arange(H * W) % W)[kept])
        what = "sweep %d" % k
        assert A.get_tuning("multi_origin_ran") == 1
        _same_dense(A.read_dense(A.last_buffer_index), B.read_dense(B.last_buffer_index), what + " A/B")
        assert A.scan_stats() == B.scan_stats()
        _slot_against_referee(A, ref, what)
        ma, mb = A.combine_maps(), B.combine_maps()
        _same_maps(ma, mb, what + " A/B")
        _maps_against_referee(A, ref, ma, ref.combine_maps(), what)
        if k == 1:                                               # (rejected or not, the route has run on C before its plain call)
            C.process_range_image_origins(np.zeros_like(raw), ego, tf, cols, cloud_dtype)
            assert C.get_tuning("multi_origin_ran") == 1
        C.process_range_image(raw, ego, tf, cols, cloud_dtype)
        D.process_range_image(raw, ego, tf, cols, cloud_dtype)
        assert C.get_tuning("multi_origin_ran") == 0
        _same_dense(C.read_dense(C.last_buffer_index), D.read_dense(D.last_buffer_index), what + " C/D")
        _same_maps(C.combine_maps(), D.combine_maps(), what + " C/D")
        # the columns' rays are not the ego's
        assert not np.array_equal(A.read_dense(A.last_buffer_index)[2], C.read_dense(C.last_buffer_index)[2])
    assert ref.combined_cell_count_cpu > 1000


def test_device_cloud_and_index_guard_through_torch():
    """torch holds cloud and index in HBM: a fresh child process that imports torch BEFORE the library is loaded (one HIP runtime
    per process, as tests/test_range_image.py does it)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_multi_origin_torch.py"), "device_index_guard"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "CASE OK device_index_guard" in r.stdout, r.stdout[-4000:]


def test_argument_errors_leave_the_ring_untouched(gvom_mod):
    prm = mo.params("p2", 2)
    g = _make(gvom_mod, prm)
    pc, origins, index, ego, tf = mo.scan_inputs("p2", 0, np.float32)
    lib, cego = gvom_mod.load_library(), (ctypes.c_double * 3)(*ego)
    p = pc.ctypes.data_as(ctypes.c_void_p)
    big = np.zeros((65537, 3))
    nan = origins.copy(); nan[2, 1] = np.nan
    bad_index = index.copy(); bad_index[4000] = mo.K
    ok_idx = index.ctypes.data_as(ctypes.c_void_p)

    def call(o, K, idx):
        return lib.gvom_process_pointcloud_origins(g._h, p, 0, mo.N, 12, 0, o.ctypes.data_as(ctypes.c_void_p), K, idx, cego, None)
    INVALID = gvom_mod.GVOM_ERR_INVALID
    assert call(origins, 0, ok_idx) == INVALID
    assert call(big, 65537, None) == INVALID
    assert call(nan, mo.K, ok_idx) == INVALID
    assert call(origins, mo.K, bad_index.ctypes.data_as(ctypes.c_void_p)) == INVALID
    assert lib.gvom_process_pointcloud_origins(g._h, p, 0, mo.N, 12, 0, None, mo.K, ok_idx, cego, None) == INVALID
    # ... and the binding's own checks
    for o, idx in ((np.zeros((0, 3)), None), (big, None), (nan, index), (origins, bad_index)):
        with pytest.raises(ValueError):
            g.process_pointcloud_origins(pc, o, ego, tf, idx)
    raw, dirs, offs = synth.range_image_scan(synth.make_scene(2, extent=10.0), 16, 512, (0.0, 0.0, 0.0), 0.0, 0, np.uint16,
                                             elevations_deg=np.linspace(-24.0, 3.0, 16))
    g.set_sensor_model(dirs, offs)
    with pytest.raises(ValueError):
        g.process_range_image_origins(raw, (0, 0, 0))
    assert lib.gvom_process_range_image_origins(g._h, raw.ctypes.data_as(ctypes.c_void_p), 0, 0, 1024, None, 0, cego, None) == INVALID
    assert g.buffer_index == 0 and g.read_dense(0) is None and g.combine_maps() is None
    # a sharded handle refuses both forms
    s = gvom_mod.Gvom(*prm, _shard=(0, 1))
    with pytest.raises(ValueError) as e:
        s.process_pointcloud_origins(pc, origins, ego, tf, index)
    assert "sharded" in str(e.value)
    s.set_sensor_model(dirs, offs)
    with pytest.raises(ValueError) as e:
        s.process_range_image_origins(raw, (0, 0, 0), column_transforms=mo.column_poses(512, 0))
    assert "sharded" in str(e.value)
    # and the handle still scans
    g.process_pointcloud_origins(pc, origins, ego, tf, index)
    assert g.buffer_index == 1 and g.combine_maps() is not None
