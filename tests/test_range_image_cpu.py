"""Range-image ingest, the part that needs no GPU: known answers for gvom.unproject_range_image -- the numpy restatement of the
arithmetic include/gvom_hip.h lays down for gvom_process_range_image, and what the GPU tests compare the kernel with -- the
synthetic range images of synth.range_image_scan, and the binding's argument checks."""
import ctypes
import inspect

import numpy as np
import pytest

import gvom
import synth

NAN = np.nan


def _dirs(H, W):
    """distinct, exactly representable directions (not unit length: the arithmetic does not care)"""
    d = np.zeros((H, W, 3))
    for h in range(H):
        for w in range(W):
            d[h, w] = (1.0 + h, 0.5 * w, -0.25 * (h + w))
    return d


def test_two_by_three_image_by_hand():
    raw = np.array([[1000, 0, 2000], [500, 4000, 65535]], np.uint16)
    d = _dirs(2, 3)
    o = np.zeros((2, 3, 3))
    o[1, 0] = (0.125, -0.25, 0.5)                               # offsets are added AFTER the multiply
    got = gvom.unproject_range_image(raw, d, o, 0.001, 0.0, float("inf"), None, np.float64)
    assert got.shape == (6, 3) and got.dtype == np.float64 and got.flags.c_contiguous
    r = lambda v: np.float64(v) * np.float64(0.001)
    want = np.array([[r(1000) * 1.0, r(1000) * 0.0, r(1000) * -0.0],
                     [NAN, NAN, NAN],                           # raw 0: no return
                     [r(2000) * 1.0, r(2000) * 1.0, r(2000) * -0.5],
                     [r(500) * 2.0 + 0.125, r(500) * 0.0 - 0.25, r(500) * -0.25 + 0.5],
                     [r(4000) * 2.0, r(4000) * 0.5, r(4000) * -0.5],
                     [r(65535) * 2.0, r(65535) * 1.0, r(65535) * -0.75]])
    assert np.array_equal(got, want, equal_nan=True)
    assert got[5, 0] == 65535 * 0.001 * 2.0 and abs(got[5, 0] - 131.07) < 1e-12     # the largest uint16 at millimetre scale


def test_range_gate_is_inclusive_and_drop_invalid_keeps_order():
    raw = np.array([[999, 1000, 1001, 0, 3000, 3001]], np.uint32)
    d = np.zeros((1, 6, 3)); d[..., 0] = 1.0
    lo, hi = np.float64(1000) * 0.001, np.float64(3000) * 0.001
    full = gvom.unproject_range_image(raw, d, None, 0.001, lo, hi, None, np.float64)
    assert np.isnan(full[:, 0]).tolist() == [True, False, False, True, False, True]
    kept = gvom.unproject_range_image(raw, d, None, 0.001, lo, hi, None, np.float64, drop_invalid=True)
    assert kept[:, 0].tolist() == [lo, np.float64(1001) * 0.001, hi] and kept.shape == (3, 3)
    assert np.array_equal(kept, full[~np.isnan(full[:, 0])])


def test_float32_ranges_inf_nan_zero_and_negative_are_invalid():
    raw = np.array([[1.5, np.inf, np.nan, 0.0, -0.0, -2.0, 3.25]], np.float32)
    d = np.zeros((1, 7, 3)); d[..., 2] = 1.0
    got = gvom.unproject_range_image(raw, d, None, 1.0, 0.0, float("inf"), None, np.float32)
    assert got.dtype == np.float32
    assert np.isnan(got[:, 2]).tolist() == [False, True, True, True, True, True, False]
    assert got[0].tolist() == [0.0, 0.0, 1.5] and got[6].tolist() == [0.0, 0.0, 3.25]


def test_column_poses_translation_and_quarter_turn():
    raw = np.array([[2000, 2000], [4000, 4000]], np.uint16)
    d = np.zeros((2, 2, 3)); d[..., 0] = 1.0                     # every beam along +x
    o = np.zeros((2, 2, 3)); o[..., 2] = 0.5
    shift = np.eye(4); shift[:3, 3] = (10.0, -20.0, 30.0)        # column 0: a pure translation
    yaw = np.array([[0.0, -1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])   # column 1: +90 degrees
    got = gvom.unproject_range_image(raw, d, o, 0.001, 0.0, float("inf"), np.stack([shift, yaw]), np.float64)
    assert got.tolist() == [[12.0, -20.0, 30.5], [0.0, 2.0, 0.5], [14.0, -20.0, 30.5], [0.0, 4.0, 0.5]]
    same = gvom.unproject_range_image(raw, d, o, 0.001, 0.0, float("inf"), np.stack([shift, yaw])[:, :3, :], np.float64)   # [W, 3, 4]
    assert np.array_equal(got, same)


def test_float32_rounding_happens_once_at_the_end():
    """One pixel whose p is exactly half-way between two float32 values: rounded to float32 BEFORE the pose (a cloud unprojected
    on the host in float32, then transformed) it goes to the even neighbour 1.0 and the pose's shift of 2^-30 is then lost as
    well; carried in float64 to the end, the shift decides the tie upwards."""
    px = 1.0 + 2.0 ** -24                                        # = 16777217 * 2^-24 exactly, half an ulp(float32) above 1
    assert np.float64(16777217) * np.float64(2.0 ** -24) == px
    raw = np.array([[16777217]], np.uint32)
    d = np.array([[[1.0, 0.0, 0.0]]])
    pose = np.eye(4)[None].copy(); pose[0, 0, 3] = 2.0 ** -30
    assert np.float32(px) == np.float32(1.0)                                                     # the tie goes to even
    early = np.float32(np.float64(np.float32(px)) + 2.0 ** -30)
    assert early == np.float32(1.0)
    got = gvom.unproject_range_image(raw, d, None, 2.0 ** -24, 0.0, float("inf"), pose, np.float32)
    assert got.dtype == np.float32 and got[0, 0] == np.float32(1.0 + 2.0 ** -23) and got[0, 0] != early
    assert got[0, 1] == 0.0 and got[0, 2] == 0.0
    # the float64 cloud keeps the sum itself
    assert gvom.unproject_range_image(raw, d, None, 2.0 ** -24, 0.0, float("inf"), pose, np.float64)[0, 0] == px + 2.0 ** -30


def test_restatement_spells_the_pose_out():
    """the normative order of operations, not a matrix product of unspecified summation order"""
    src = inspect.getsource(gvom.unproject_range_image)
    assert "einsum" not in src and " @ " not in src and "np.dot" not in src and "matmul" not in src
    rng = np.random.default_rng(5)
    raw = rng.integers(1, 60000, (4, 8)).astype(np.uint32)
    d, o = rng.normal(size=(4, 8, 3)), rng.normal(scale=0.03, size=(4, 8, 3))
    C = rng.normal(size=(8, 3, 4))
    got = gvom.unproject_range_image(raw, d, o, 0.001, 0.0, float("inf"), C, np.float64)
    for h in range(4):
        for w in range(8):
            r = float(raw[h, w]) * 0.001
            p = [r * d[h, w, k] + o[h, w, k] for k in range(3)]
            q = [((p[0] * C[w, k, 0] + p[1] * C[w, k, 1]) + p[2] * C[w, k, 2]) + C[w, k, 3] for k in range(3)]
            assert got[h * 8 + w].tolist() == q


def test_bad_arguments_raise_value_errors():
    d = _dirs(2, 3)
    ok = np.ones((2, 3), np.uint16)
    for bad in (np.ones((2, 3), np.int32), np.ones((2, 3), np.float64), np.ones((2, 3), np.uint8)):
        with pytest.raises(ValueError):
            gvom.unproject_range_image(bad, d, None, 0.001, 0.0, 1.0, None, np.float32)
    with pytest.raises(ValueError):
        gvom.unproject_range_image(np.ones(6, np.uint16), d, None, 0.001, 0.0, 1.0, None, np.float32)
    with pytest.raises(ValueError):
        gvom.unproject_range_image(ok, _dirs(3, 2), None, 0.001, 0.0, 1.0, None, np.float32)
    with pytest.raises(ValueError):
        gvom.unproject_range_image(ok, d, np.zeros((2, 3)), 0.001, 0.0, 1.0, None, np.float32)
    with pytest.raises(ValueError):
        gvom.unproject_range_image(ok, d, None, 0.001, 0.0, 1.0, np.zeros((2, 4, 4)), np.float32)     # W poses, not H
    with pytest.raises(ValueError):
        gvom.unproject_range_image(ok, d, None, 0.001, 0.0, 1.0, None, np.float16)


def test_binding_declares_the_two_entry_points():
    abi = {name: (res, args) for name, res, args in gvom.ABI}
    res, args = abi["gvom_sensor_model_set"]
    assert res is ctypes.c_int and len(args) == 8 and args[5:] == [ctypes.c_double] * 3
    res, args = abi["gvom_process_range_image"]
    assert res is ctypes.c_int and len(args) == 9 and args[4] is ctypes.c_int64
    assert (gvom.RANGE_U16, gvom.RANGE_U32, gvom.RANGE_F32) == (0, 1, 2)
    L = gvom.load_library()
    assert hasattr(L, "gvom_sensor_model_set") and hasattr(L, "gvom_process_range_image")
    assert L.gvom_abi_version() == 10 == gvom.ABI_VERSION                  # additions: the version stays
    for m in ("set_sensor_model", "process_range_image", "process_range_image_device"):
        assert callable(getattr(gvom.Gvom, m))
    sig = inspect.signature(gvom.Gvom.process_range_image)
    assert list(sig.parameters)[1:] == ["ranges", "ego_position", "transform", "column_transforms", "cloud_dtype"]
    # a null handle is refused before anything touches a device
    assert L.gvom_sensor_model_set(None, 1, 1, None, None, 0.001, 0.0, 1.0) == gvom.GVOM_ERR_INVALID
    assert L.gvom_process_range_image(None, None, 0, 0, 2, None, 0, None, None) == gvom.GVOM_ERR_INVALID


def test_synthetic_range_images():
    scene = synth.make_scene(2)
    a = synth.range_image_scan(scene, 16, 256, (0.2, 0.0, 0.0), 0.0, 3, np.uint16, dropout=0.2)
    b = synth.range_image_scan(scene, 16, 256, (0.2, 0.0, 0.0), 0.0, 3, np.uint16, dropout=0.2)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)                                           # seeded
    raw, d, o = a
    assert raw.shape == (16, 256) and raw.dtype == np.uint16 and d.shape == o.shape == (16, 256, 3)
    assert np.allclose(np.linalg.norm(d, axis=2), 1.0, atol=1e-12)
    assert 0.01 < np.abs(o).max() < 0.06 and np.abs(o[..., 2]).min() > 0.03   # a few centimetres, none of them zero in z
    whole = synth.range_image_scan(scene, 16, 256, (0.2, 0.0, 0.0), 0.0, 3, np.uint16)[0]
    assert 0.15 < ((raw == 0) & (whole != 0)).sum() / (whole != 0).sum() < 0.25     # the dropout takes its share of the returns there are
    assert np.array_equal(raw[raw != 0], whole[raw != 0])
    # the image is the sweep lidar_scan(frame="sensor") ray-casts: without offsets, every valid pixel within half a millimetre
    el, azo = synth.os1_like_elevations(16), synth.os1_like_azimuth_offsets(16)
    cloud = synth.lidar_scan(scene, 16, 256, (0.2, 0.0, 0.0), 0.0, 3, np.float64, "sensor", el, azo)
    pts = gvom.unproject_range_image(whole, d, None, 0.001, 0.0, float("inf"), None, np.float64)
    v = ~np.isnan(pts[:, 0])
    assert v.sum() > 1000 and np.abs(pts[v] - cloud[v]).max() < 0.00051
    f = synth.range_image_scan(scene, 16, 256, (0.2, 0.0, 0.0), 0.0, 3, np.float32)[0]
    assert f.dtype == np.float32 and np.array_equal(f == 0, whole == 0) and np.abs(f[f != 0] - whole[f != 0] * 0.001).max() < 0.00051
    # the existing generators are untouched by the new one
    p1, s1 = synth.config_inputs("c2")
    assert s1[0][0].shape == (131072, 3)
