"""Range-image ingest on the GPU (Gvom.set_sensor_model / process_range_image / process_range_image_device): by definition the
scan of the cloud gvom.unproject_range_image computes on the CPU, so every comparison with that cloud's own scan is EXACT; the
referee is the CPU oracle fed with the same cloud (integer maps exact, roughness within the 1e-5 every comparison with glibc
uses: ocml's log / atan2 in the 2-D stage)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import synth
from oracle import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = (0.4, 0.2, 64, 32, 2) + synth.REF_TAIL
SCALE = {np.uint16: 0.001, np.uint32: 0.001, np.float32: 1.0}


@pytest.fixture(scope="module")
def gvom_mod():
    import gvom
    rc, info = gvom.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    return gvom


def _make(gvom_mod, params, **kw):
    kw.setdefault("voxel_statistics", False)
    return gvom_mod.Gvom(*params, **kw)


def _same_maps(a, b, what):
    assert (a is None) == (b is None), what
    if a is None:
        return
    for k, (u, v) in enumerate(zip(a, b)):
        assert np.array_equal(np.asarray(u), np.asarray(v)), "%s: returned map %d differs" % (what, k)


def _same_dense(a, b, what):
    for k, name in enumerate(("state", "hit", "total", "min-height")):
        assert np.array_equal(a[k], b[k]), "%s: %s differs" % (what, name)
    assert np.array_equal(a[4], b[4]), what


def _column_poses(W, k):
    """the sensor's motion during sweep k: a slow yaw and a drift along x and z, one 4x4 per column"""
    out = np.zeros((W, 4, 4))
    t = np.arange(W) / W
    a = 0.03 * t + 0.01 * k
    out[:, 0, 0] = np.cos(a); out[:, 0, 1] = -np.sin(a); out[:, 1, 0] = np.sin(a); out[:, 1, 1] = np.cos(a)
    out[:, 2, 2] = 1.0; out[:, 3, 3] = 1.0
    out[:, 0, 3] = 0.4 * t; out[:, 2, 3] = -0.05 * t
    return out


@pytest.mark.parametrize("posed", [False, True], ids=["one-pose", "column-poses"])
@pytest.mark.parametrize("cloud_dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("range_dtype", [np.uint16, np.uint32, np.float32], ids=["u16", "u32", "rf32"])
def test_range_image_equals_its_cloud_small_grid(gvom_mod, range_dtype, cloud_dtype, posed):
    """A: the image; B: its cloud with the invalid pixels dropped (what a node hands over today); C: its cloud with the NaN rows
    kept; the oracle: B's cloud.  Ring slot after every scan, every returned map after every combine."""
    H, W = 16, 512
    scene = synth.make_scene(2, extent=10.0)
    el = np.linspace(-24.0, 3.0, H)                              # (mostly below the horizon: most rays have a return)
    A, B, C = (_make(gvom_mod, SMALL) for _ in range(3))
    ref = oracle.OracleGvom(*SMALL)
    scale = SCALE[range_dtype]
    invalid = pixels = 0
    for k in range(3):
        sensor = (0.5 * k, -0.3 * k, 0.05 * k)
        raw, dirs, offs = synth.range_image_scan(scene, H, W, sensor, 0.0, k, range_dtype, dropout=0.1, elevations_deg=el)
        assert raw.dtype == range_dtype and np.abs(offs).max() > 0.01
        tf = gvom_mod.transform_from_translation_rotation(sensor, (0.01, -0.02, 0.05 * k, 1.0))     # node-style: quaternion + translation
        cols = _column_poses(W, k) if posed else None
        gate = (0.8, 45.0)
        if k == 0:
            A.set_sensor_model(dirs, offs, scale, *gate)
            assert A.get_tuning("range_image") == 1 and B.get_tuning("range_image") == 0
        full = gvom_mod.unproject_range_image(raw, dirs, offs, scale, gate[0], gate[1], cols, cloud_dtype)
        kept = gvom_mod.unproject_range_image(raw, dirs, offs, scale, gate[0], gate[1], cols, cloud_dtype, drop_invalid=True)
        assert full.dtype == cloud_dtype and full.shape == (H * W, 3) and kept.shape[0] == int((~np.isnan(full[:, 0])).sum())
        invalid += int(np.isnan(full[:, 0]).sum()); pixels += H * W
        assert A.process_range_image(raw, sensor, tf, cols, cloud_dtype) is None
        B.process_pointcloud(kept, sensor, tf)
        C.process_pointcloud(full, sensor, tf)
        ref.process_pointcloud(kept, sensor, tf)
        assert A.buffer_index == B.buffer_index == C.buffer_index == ref.buffer_index
        slot = A.last_buffer_index
        da, db, dc = A.read_dense(slot), B.read_dense(slot), C.read_dense(slot)
        _same_dense(da, db, "scan %d A/B" % k)
        _same_dense(da, dc, "scan %d A/C" % k)
        sa, sc = A.scan_stats(), C.scan_stats()
        assert sa == sc and sa["points"] == H * W
        ma, mb, mc, mo = A.combine_maps(), B.combine_maps(), C.combine_maps(), ref.combine_maps()
        _same_maps(ma, mb, "combine %d A/B" % k)
        _same_maps(ma, mc, "combine %d A/C" % k)
        assert np.array_equal(ma[0], mo[0])
        for j in (1, 2, 4):                                      # positive, negative, visibility: integers
            assert np.array_equal(ma[j], mo[j]), "combine %d: integer map %d differs from the referee" % (k, j)
        assert np.allclose(ma[3], mo[3], rtol=0, atol=1e-5)
        assert A.combined_cell_count_cpu == ref.combined_cell_count_cpu
    # the input is neither clean nor empty
    assert 0.05 < invalid / pixels < 0.40, invalid / pixels
    assert ref.combined_cell_count_cpu > 1000


def test_range_image_m256_full_size(gvom_mod):
    """256^3, 64 x 2048 pixels of uint32 millimetres, a quarter of them dropped, the bench's 8 poses, buffer 1: every returned map,
    the fused map at the end, the eager path undisturbed, the scan statistics of the NaN-carrying cloud."""
    params = synth.CONFIGS["m256"][0]
    assert params[2:5] == (256, 256, 1)
    scene = synth.make_scene(2)
    A, B, C = (_make(gvom_mod, params) for _ in range(3))
    for k in range(8):
        sensor = (0.2 * k, 0.0, 0.0)
        raw, dirs, offs = synth.range_image_scan(scene, 64, 2048, sensor, 0.0, k, np.uint32, dropout=0.25)
        assert raw.shape == (64, 2048) and raw.dtype == np.uint32
        if k == 0:
            A.set_sensor_model(dirs, offs, 0.001)
        tf = synth.sensor_transform(sensor)
        full = gvom_mod.unproject_range_image(raw, dirs, offs, 0.001, 0.0, float("inf"), None, np.float32)
        kept = full[~np.isnan(full[:, 0])]
        assert 20000 < kept.shape[0] < 0.75 * 131072
        A.process_range_image(raw, sensor, tf)
        B.process_pointcloud(kept, sensor, tf)
        C.process_pointcloud(full, sensor, tf)
        assert A.scan_stats() == C.scan_stats()
        _same_maps(A.combine_maps(), B.combine_maps(), "m256 step %d" % k)
        C.combine_maps()
    _same_dense(A.read_dense(gvom_mod.GVOM_WHICH_FUSED), B.read_dense(gvom_mod.GVOM_WHICH_FUSED), "fused map")
    assert A.read_dense(gvom_mod.GVOM_WHICH_FUSED)[5] > 10000
    assert A.get_tuning("eager_adopted") == 8 and B.get_tuning("eager_adopted") == 8


def _torch_case(name):
    """torch uploads the image: a fresh child process that imports torch BEFORE the library is loaded (one HIP runtime per
    process, as tests/test_device_maps.py does it)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_range_image_torch.py"), name],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "CASE OK " + name in r.stdout, r.stdout[-4000:]


def test_device_images_with_padded_rows_through_torch():
    _torch_case("device_input")


def test_contract_errors_and_warnings(gvom_mod, capsys):
    g = _make(gvom_mod, SMALL)
    scene = synth.make_scene(2, extent=10.0)
    raw, dirs, offs = synth.range_image_scan(scene, 16, 512, (0.0, 0.0, 0.0), 0.0, 0, np.uint16, elevations_deg=np.linspace(-24.0, 3.0, 16))
    assert g.get_tuning("range_image") == 0
    with pytest.raises(gvom_mod.GvomBackendError) as e:           # GVOM_ERR_INVALID: no model
        g.process_range_image(raw, (0, 0, 0))
    assert "(-1)" in str(e.value) and "sensor model" in str(e.value)
    g.set_sensor_model(dirs, offs)
    assert g.get_tuning("range_image") == 1
    for bad in (raw[:, :256], raw[:8], raw.astype(np.int32), raw.astype(np.float64), raw[:, ::2], raw.reshape(-1)):
        with pytest.raises(ValueError):
            g.process_range_image(bad, (0, 0, 0))
    with pytest.raises(ValueError):
        g.process_range_image(raw, (0, 0, 0), column_transforms=np.zeros((16, 4, 4)))
    with pytest.raises(ValueError):
        g.set_sensor_model(dirs, offs[:8])
    with pytest.raises(ValueError):
        g.set_sensor_model(dirs, offs, range_scale=0.0)
    # the C entry point itself: a row stride shorter than a row, one that is no multiple of the element, a bad type
    lib, ego = gvom_mod.load_library(), (ctypes.c_double * 3)(0, 0, 0)
    p = raw.ctypes.data_as(ctypes.c_void_p)
    for rdt, stride, cdt in ((0, 1022, 0), (0, 1025, 0), (3, 1024, 0), (0, 1024, 2), (1, 1024, 0)):
        assert lib.gvom_process_range_image(g._h, p, 0, rdt, stride, None, cdt, ego, None) == gvom_mod.GVOM_ERR_INVALID
    assert g.buffer_index == 0 and g.combine_maps() is None
    capsys.readouterr()
    # an image without a return: the reference's warning, nothing enters the ring
    g.process_range_image(np.zeros_like(raw), (0, 0, 0))
    assert "don't overlap with any voxels" in capsys.readouterr().out
    assert g.buffer_index == 0 and g.combine_maps() is None
    # and it still scans
    g.process_range_image(raw, (0, 0, 0))
    assert g.buffer_index == 1 and g.combine_maps() is not None
    # sharded handles refuse
    s = gvom_mod.Gvom(*SMALL, _shard=(0, 1))
    s.set_sensor_model(dirs, offs)
    with pytest.raises(gvom_mod.GvomBackendError) as e:
        s.process_range_image(raw, (0, 0, 0))
    assert "(-1)" in str(e.value) and "sharded" in str(e.value)


def test_model_replaced_between_scans(gvom_mod):
    """two sensors of different shapes in turn on one handle == their two clouds; replacing a model many times allocates nothing
    new once it has been as large as it gets"""
    scene = synth.make_scene(2, extent=10.0)
    A, B = _make(gvom_mod, SMALL), _make(gvom_mod, SMALL)
    shapes = ((16, 512, np.uint16, 0.001), (8, 300, np.float32, 1.0))           # (a width that is no multiple of the workgroup's 256 pixels)
    for k in range(4):
        H, W, rdt, scale = shapes[k & 1]
        sensor = (0.3 * k, 0.2 * k, 0.0)
        raw, dirs, offs = synth.range_image_scan(scene, H, W, sensor, 0.0, k, rdt, dropout=0.1, elevations_deg=np.linspace(-24.0, 3.0, H))
        A.set_sensor_model(dirs, offs if k < 2 else None, scale)
        assert A.get_tuning("range_image") == 1
        tf = synth.sensor_transform(sensor)
        A.process_range_image(raw, sensor, tf)
        B.process_pointcloud(gvom_mod.unproject_range_image(raw, dirs, offs if k < 2 else None, scale, drop_invalid=True), sensor, tf)
        _same_dense(A.read_dense(A.last_buffer_index), B.read_dense(B.last_buffer_index), "scan %d" % k)
        _same_maps(A.combine_maps(), B.combine_maps(), "combine %d" % k)
    rt = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)

    def free_bytes():
        assert rt.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value
    H, W, rdt, scale = shapes[0]
    raw, dirs, offs = synth.range_image_scan(scene, H, W, (0.0, 0.0, 0.0), 0.0, 9, rdt, elevations_deg=np.linspace(-24.0, 3.0, H))
    A.set_sensor_model(dirs, offs, scale)
    import gc
    gc.collect()                                              # (mappers of earlier tests go now, not during the loop)
    before = free_bytes()
    for k in range(200):
        A.set_sensor_model(dirs * (1.0 if k & 1 else -1.0), offs, scale)
        assert A.get_tuning("range_image") == 1
    # a model of 16 x 512 pixels is 393 KB: 200 leaked copies would take 78 MB or more.  Free memory is a number of the whole
    # device, so the test is one-sided and leaves 32 MB for whatever else lives there
    assert before - free_bytes() < (32 << 20)
    A.process_range_image(raw, (0.0, 0.0, 0.0))
    B.process_pointcloud(gvom_mod.unproject_range_image(raw, dirs, offs, scale), (0.0, 0.0, 0.0))
    _same_maps(A.combine_maps(), B.combine_maps(), "after the replacements")


def test_cloud_route_is_untouched_by_a_model(gvom_mod):
    scene = synth.make_scene(2, extent=10.0)
    raw, dirs, offs = synth.range_image_scan(scene, 16, 512, (0.0, 0.0, 0.0), 0.0, 0, np.uint16, elevations_deg=np.linspace(-24.0, 3.0, 16))
    A, B = _make(gvom_mod, SMALL), _make(gvom_mod, SMALL)
    A.set_sensor_model(dirs, offs)
    pc = synth.lidar_scan(scene, 16, 512, (0.1, 0.0, 0.0), elevations_deg=np.linspace(-24.0, 3.0, 16))
    A.process_pointcloud(pc, (0.1, 0.0, 0.0))
    B.process_pointcloud(pc, (0.1, 0.0, 0.0))
    _same_dense(A.read_dense(0), B.read_dense(0), "cloud route")
    assert A.scan_stats() == B.scan_stats()
    _same_maps(A.combine_maps(), B.combine_maps(), "cloud route")
