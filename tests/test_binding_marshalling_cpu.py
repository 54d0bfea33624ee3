"""What the binding (g-vom_amd/gvom.py, and the two scan routes of gvom_sharded.py) hands to the library, checked without a GPU
and without the library: a Gvom made with __new__ (no handle), whose `_lib` is a stand-in that notes every call -- the entry
point's name and its arguments, pointed-to values read AT CALL TIME -- and returns 0.

  - every scan route refuses a transform that is not 4x4 before it calls anything (the library reads tf[0..11]);
  - every scan route passes the expected entry point n, stride, dtype code, on_device flag, ego and the transform's 16 doubles in
    row-major order, whatever the memory order and dtype the caller's matrix had;
  - the [x, y] window maps of clearance_of, cost_to_go_of and score_rollouts_of: what each caller checks and what it lets through;
  - the combine routes: one pinned buffer per call from one place, and the views of it (shapes, strides, dtypes, offsets) from
    _combine_into, combine_maps_occupancy and _PendingMaps.result."""
import ctypes
import re
import warnings

import numpy as np
import pytest

import gvom
import gvom_sharded

XY = 6                                              # window of the handle-less mapper (cells a side)
EGO = (1.5, -2.25, 3.0)
TF = np.arange(16, dtype=np.float64).reshape(4, 4) + 0.5          # not symmetric; exact in float32
TF_GIVEN = np.asfortranarray(TF.astype(np.float32))               # as a caller might hold it: float32, column-major
assert not TF_GIVEN.flags["C_CONTIGUOUS"]

# arguments the stand-in reads through their pointers when the call is made: entry point -> {argument index: (element type, count)}
PEEK = {
    "gvom_process_pointcloud": {6: (ctypes.c_double, 16)},
    "gvom_process_pointcloud_device": {6: (ctypes.c_double, 16)},
    "gvom_process_pointcloud_origins": {10: (ctypes.c_double, 16)},
    "gvom_process_pointcloud2": {9: (ctypes.c_double, 16)},
    "gvom_process_range_image": {8: (ctypes.c_double, 16)},
    "gvom_process_range_image_origins": {8: (ctypes.c_double, 16)},
    "gvom_shard_scan_local": {7: (ctypes.c_double, 16)},
    "gvom_comm_process_pointcloud": {8: (ctypes.c_double, 16)},
    "gvom_clearance": {2: (ctypes.c_int32, XY * XY), 3: (ctypes.c_int32, XY * XY)},
    "gvom_cost_to_go": {3: (ctypes.c_int32, XY * XY)},
    "gvom_score_rollouts": {2: (ctypes.c_uint16, XY * XY), 3: (ctypes.c_int32, XY * XY)},
}
# where a scan entry point takes what: (n, stride, dtype code, on_device, ego, transform); None = it has no such argument
SCAN_ARGS = {
    "gvom_process_pointcloud": (2, 3, 4, None, 5, 6),
    "gvom_process_pointcloud_device": (2, 3, 4, None, 5, 6),
    "gvom_process_pointcloud_origins": (3, 4, 5, 2, 9, 10),
    "gvom_process_pointcloud2": (2, 3, 7, None, 8, 9),
    "gvom_process_range_image": (None, 4, 6, 2, 7, 8),
    "gvom_process_range_image_origins": (None, 4, 6, 2, 7, 8),
    "gvom_shard_scan_local": (3, 4, 5, 2, 6, 7),
    "gvom_comm_process_pointcloud": (4, 5, 6, 3, 7, 8),
}


def _plain(a):
    """a ctypes argument as plain Python: arrays as tuples, pointers as addresses, by-reference arguments by name"""
    if isinstance(a, ctypes.Array):
        return tuple(a)
    if isinstance(a, ctypes._SimpleCData):
        return a.value
    if a is None or isinstance(a, (int, float, bytes)):
        return a
    return type(a).__name__                         # (ctypes.byref's CArgObject, a Structure)


class RecordingLib(object):
    """Stands in for the loaded library: every attribute is a function that notes (name, arguments) in `.calls` and returns 0.
    gvom_output_buffer_alloc hands out host memory of `buffer_bytes` (kept in `.buffers`, filled with a byte pattern), and
    gvom_device_product_export an address."""

    def __init__(self, buffer_bytes=0):
        self.calls, self.buffers, self._bytes = [], [], buffer_bytes

    def __getattr__(self, name):
        def entry(*args):
            noted = [_plain(a) for a in args]
            for k, (ctype, count) in PEEK.get(name, {}).items():
                if noted[k] is not None:
                    noted[k] = tuple((ctype * count).from_address(noted[k]))
            self.calls.append((name, tuple(noted)))
            if name == "gvom_output_buffer_alloc":
                buf = (np.arange(self._bytes) % 251).astype(np.uint8)
                self.buffers.append(buf)
                args[1]._obj.value = buf.ctypes.data
            elif name == "gvom_device_product_export":
                args[4]._obj.value = 4096           # some address and no dimensions: enough for the views of a product
            return 0
        return entry

    def named(self, name):
        return [args for n, args in self.calls if n == name]


def make_gvom(sensor_shape=None):
    g = gvom.Gvom.__new__(gvom.Gvom)                # no handle, no library
    g._lib, g._h = RecordingLib(XY * XY * 20), None
    g.xy_size, g.xy_resolution = XY, 0.5
    g._out_pool = gvom._OutputPool()
    g.ego_position = [0, 0, 0]
    if sensor_shape is not None:
        g._sensor_shape = sensor_shape
    return g


def make_backend(world=2):
    b = gvom_sharded.HipShardBackend.__new__(gvom_sharded.HipShardBackend)
    b.g = make_gvom()
    b.lib, b.h, b.rank, b.world, b.dtype_code = b.g._lib, None, 0, world, 0
    return b


def make_comm(lib):
    c = gvom_sharded.RcclComm.__new__(gvom_sharded.RcclComm)
    c.lib, c.c, c.rank, c.world = lib, None, 0, 2
    return c


# ---- the scan routes ----
def _cloud(dtype):
    return (np.arange(15).reshape(5, 3) * 0.25).astype(dtype)


RANGES = np.array([[1000, 0, 3000], [4000, 5000, 6000]], np.uint16)       # 2 x 3, the model's shape
ORIGINS = np.array([[0.0, 0.0, 1.0], [0.5, 0.0, 1.0]])
COLUMNS = np.tile(np.identity(4), (3, 1, 1))


def _scan_routes():
    """(id, entry point, expected (n, stride, code, on_device), the memory the cloud lies in or None, make() -> the object the
    route is called on, call(object, transform))"""
    routes = []
    sensor = lambda: make_gvom((2, 3))
    for dt, stride, code in ((np.float32, 12, 0), (np.float64, 24, 1)):
        pc = _cloud(dt)
        at = pc.ctypes.data                         # stands in for a device address: the stand-in never follows it
        offsets = (0, stride // 3, 2 * stride // 3)
        for name, entry, on_device, make, call in (
                ("process_pointcloud", "gvom_process_pointcloud", None, make_gvom,
                 lambda g, tf, pc=pc: g.process_pointcloud(pc, EGO, tf)),
                ("process_pointcloud_device", "gvom_process_pointcloud_device", None, make_gvom,
                 lambda g, tf, at=at, dt=dt: g.process_pointcloud_device(at, 5, dt, EGO, tf)),
                ("process_pointcloud_origins", "gvom_process_pointcloud_origins", 0, make_gvom,
                 lambda g, tf, pc=pc: g.process_pointcloud_origins(pc, ORIGINS, EGO, tf)),
                ("process_pointcloud_origins_device", "gvom_process_pointcloud_origins", 1, make_gvom,
                 lambda g, tf, at=at, dt=dt: g.process_pointcloud_origins_device(at, 5, dt, ORIGINS, EGO, tf)),
                ("process_pointcloud2", "gvom_process_pointcloud2", None, make_gvom,
                 lambda g, tf, pc=pc, dt=dt, stride=stride, offsets=offsets: g.process_pointcloud2(pc.tobytes(), 5, stride, offsets, EGO, tf, dt)),
                ("scan_local", "gvom_shard_scan_local", 0, make_backend,
                 lambda b, tf, pc=pc: b.scan_local(pc, EGO, tf)),
                ("scan_local-device", "gvom_shard_scan_local", 1, make_backend,
                 lambda b, tf, at=at, dt=dt: b.scan_local((at, 5, dt), EGO, tf)),
                ("scan_native", "gvom_comm_process_pointcloud", 0, make_backend,
                 lambda b, tf, pc=pc: make_comm(b.lib).scan_native(b, pc, EGO, tf)),
                ("scan_native-device", "gvom_comm_process_pointcloud", 1, make_backend,
                 lambda b, tf, at=at, dt=dt: make_comm(b.lib).scan_native(b, (at, 5, dt), EGO, tf))):
            source = None if name == "process_pointcloud2" else pc          # (its bytes are a copy)
            routes.append(("%s-%s" % (name, np.dtype(dt).name), entry, (5, stride, code, on_device), source, make, call))
    # range images: stride = the bytes of a row (3 x uint16), code = the dtype code of the cloud they are unprojected to
    for name, entry in (("process_range_image", "gvom_process_range_image"), ("process_range_image_origins", "gvom_process_range_image_origins")):
        routes.append((name, entry, (None, 6, 0, 0), RANGES, sensor,
                       lambda g, tf, name=name: getattr(g, name)(RANGES, EGO, tf, COLUMNS)))
        routes.append((name + "_device", entry, (None, 6, 0, 1), RANGES, sensor,
                       lambda g, tf, name=name: getattr(g, name + "_device")(RANGES.ctypes.data, np.uint16, EGO, tf, COLUMNS)))
    return routes


def _lib_of(obj):
    return obj.lib if isinstance(obj, gvom_sharded.HipShardBackend) else obj._lib


SCAN_ROUTES = _scan_routes()
_IDS = [r[0] for r in SCAN_ROUTES]


@pytest.mark.parametrize("route", SCAN_ROUTES, ids=_IDS)
def test_a_transform_that_is_not_4x4_is_refused_before_any_library_call(route):
    make, call = route[4:]
    for shape in ((3, 3), (3, 4), (16,), (4, 4, 1)):
        obj = make()
        with pytest.raises(ValueError, match="4x4"):
            call(obj, np.ones(shape))
        assert _lib_of(obj).calls == []


@pytest.mark.parametrize("route", SCAN_ROUTES, ids=_IDS)
def test_scan_routes_hand_over_cloud_frame_and_row_major_transform(route):
    _, entry, (n, stride, code, on_device), source, make, call = route
    i_n, i_stride, i_code, i_dev, i_ego, i_tf = SCAN_ARGS[entry]
    obj = make()
    call(obj, TF_GIVEN)
    lib = _lib_of(obj)
    assert [name for name, _ in lib.calls] == [entry]
    args = lib.calls[0][1]
    if i_n is not None:
        assert args[i_n] == n
    assert args[i_stride] == stride and args[i_code] == code
    if i_dev is not None:
        assert args[i_dev] == on_device
    assert args[i_ego] == EGO
    assert args[i_tf] == tuple(TF.ravel())                          # 16 doubles, row-major
    if source is not None:
        assert source.ctypes.data in args                           # the caller's memory itself: a well-formed cloud is not copied
    g = obj.g if isinstance(obj, gvom_sharded.HipShardBackend) else obj
    assert g.ego_position is EGO
    # no transform: a null pointer
    obj = make()
    call(obj, None)
    assert _lib_of(obj).calls[0][0] == entry and _lib_of(obj).calls[0][1][i_tf] is None


def test_device_cloud_code_and_stride():
    assert gvom._device_cloud(np.float32) == (0, 12) and gvom._device_cloud(np.dtype("float32")) == (0, 12)
    assert gvom._device_cloud(np.float64) == (1, 24) and gvom._device_cloud("float64") == (1, 24)
    assert gvom._device_cloud(np.float32, 32) == (0, 32) and gvom._device_cloud(np.float64, 40) == (1, 40)
    g = make_gvom()
    assert g.process_pointcloud_device(4096, 7, np.float32, EGO, None, row_stride_bytes=16) == 0      # the code, not None
    assert g._lib.calls[0][1][1:5] == (4096, 7, 16, 0)
    assert g.process_pointcloud_origins_device(4096, 7, np.float64, ORIGINS, EGO, origin_index_ptr=8192) == 0
    a = g._lib.calls[1][1]
    assert a[1:6] == (4096, 1, 7, 24, 1) and a[7] == 2 and a[8] == 8192
    assert make_gvom().process_pointcloud(_cloud(np.float32), EGO) is None


def test_scan_warnings_keep_their_texts(capsys):
    gvom._warn_scan(gvom.GVOM_OK)
    assert capsys.readouterr().out == ""
    gvom._warn_scan(gvom.GVOM_EMPTY_CLOUD)
    assert capsys.readouterr().out == "[WARNING] Processing an empty pointcloud, nothing will happen!\n"
    gvom._warn_scan(gvom.GVOM_NO_OVERLAP)
    assert capsys.readouterr().out == "[WARNING] The pointcloud points don't overlap with any voxels, nothing will happen!\n"
    gvom._warn_empty_ring()
    assert capsys.readouterr().out == "[WARNING] The map buffer is empty, nothing will happen!\n"


# ---- window maps ----
GOOD = np.arange(XY * XY).reshape(XY, XY)           # C order: the binding turns it x fastest
POSES = np.zeros((2, 3, 3), np.float32)


def _bad_maps():
    """one wrong shape, one non-finite, one fractional and one out-of-range [x, y] map"""
    nan = GOOD.astype(np.float64)
    nan[1, 2] = np.nan
    frac = GOOD.astype(np.float64)
    frac[3, 0] = 0.5
    big = GOOD.astype(np.int64)
    big[2, 2] = 2 ** 40
    return {"shape": np.zeros((XY, XY + 1), np.int32), "finite": nan, "whole": frac, "range": big}


def test_clearance_of_checks_the_shape_and_casts_the_rest():
    bad = _bad_maps()
    for which in ("positive", "negative"):
        g = make_gvom()
        with pytest.raises(ValueError, match=r"%s must have shape \(6, 6\), got \(6, 7\)" % which):
            g.clearance_of(bad["shape"], None) if which == "positive" else g.clearance_of(GOOD, bad["shape"])
        assert g._lib.calls == []
    with pytest.raises(ValueError, match="positive must be an array"):
        make_gvom().clearance_of(None)
    for kind in ("finite", "whole", "range"):       # no such check on this route: the map is cast to int32 and goes to the library
        g = make_gvom()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")         # (numpy's note about casting a NaN)
            g.clearance_of(bad[kind], bad[kind])
        assert len(g._lib.named("gvom_clearance")) == 1
    g = make_gvom()
    g.clearance_of(GOOD)
    args = g._lib.named("gvom_clearance")[0]
    assert args[1] == -1 and args[2] == tuple(GOOD.ravel(order="F")) and args[3] is None and args[4] == 0
    g = make_gvom()
    g.clearance_of(GOOD, GOOD.T.astype(np.float64))
    assert g._lib.named("gvom_clearance")[0][3] == tuple(GOOD.T.ravel(order="F"))


def test_cost_to_go_of_holds_its_map_to_whole_numbers_in_range():
    bad = _bad_maps()
    messages = {"shape": r"cost must have shape \(6, 6\), got \(6, 7\)", "finite": "cost must be finite",
                "whole": "cost must hold whole numbers", "range": re.escape("cost must lie in 0 .. 65535 (0 = blocked)")}
    for kind, message in messages.items():
        g = make_gvom()
        with pytest.raises(ValueError, match=message):
            g.cost_to_go_of(bad[kind], [(1, 1)])
        assert g._lib.calls == []
    for edge in (-1, 65536):
        m = GOOD.copy()
        m[0, 0] = edge
        with pytest.raises(ValueError, match=messages["range"]):
            make_gvom().cost_to_go_of(m, [(1, 1)])
    with pytest.raises(ValueError, match=r"cost must have shape \(6, 6\), got \(\)"):
        make_gvom().cost_to_go_of(None, [(1, 1)])
    with pytest.raises(ValueError, match="cost must hold whole numbers"):
        make_gvom().cost_to_go_of(GOOD.astype(bool), [(1, 1)])
    g = make_gvom()
    m = GOOD.astype(np.float64)
    m[0, 0] = 65535.0
    g.cost_to_go_of(m, [(1, 1)])
    assert g._lib.named("gvom_cost_to_go")[0][3] == tuple(int(v) for v in m.ravel(order="F"))


def test_score_rollouts_of_holds_both_maps_to_whole_numbers_in_range():
    bad = _bad_maps()
    for name, lo, hi in (("cell_cost", 0, 65535), ("cost_to_go", -2 ** 31, 2 ** 31 - 1)):
        messages = {"shape": r"%s must have shape \(6, 6\), got \(6, 7\)" % name, "finite": "%s must be finite" % name,
                    "whole": "%s must hold whole numbers" % name, "range": r"%s must lie in %d \.\. %d$" % (name, lo, hi)}
        for kind, message in messages.items():
            g = make_gvom()
            with pytest.raises(ValueError, match=message):
                g.score_rollouts_of(bad[kind], POSES) if name == "cell_cost" else g.score_rollouts_of(GOOD, POSES, bad[kind])
            assert g._lib.calls == []
    with pytest.raises(ValueError, match="cell_cost must be an array"):
        make_gvom().score_rollouts_of(None, POSES)
    with pytest.raises(ValueError, match=r"cell_cost must lie in 0 \.\. 65535$"):
        make_gvom().score_rollouts_of(GOOD - 1, POSES)
    g = make_gvom()
    g.score_rollouts_of(GOOD, POSES)
    args = g._lib.named("gvom_score_rollouts")[0]
    assert args[1] == -1 and args[2] == tuple(GOOD.ravel(order="F")) and args[3] is None
    g = make_gvom()
    field = (GOOD.T * -1000).astype(np.float32)
    g.score_rollouts_of(GOOD, POSES, field)
    assert g._lib.named("gvom_score_rollouts")[0][3] == tuple(int(v) for v in field.ravel(order="F"))


# ---- the combine routes ----
def _offset(view, lib):
    return view.__array_interface__["data"][0] - lib.buffers[-1].ctypes.data


def _check_maps(out, lib):
    n2 = XY * XY
    origin, positive, negative, roughness, visibility = out
    assert origin.shape == (3,) and origin.dtype == np.float64
    for view, dtype, offset in ((positive, np.int32, 0), (negative, np.int32, 4 * n2), (visibility, np.int32, 8 * n2),
                                (roughness, np.float64, 12 * n2)):
        item = np.dtype(dtype).itemsize
        assert view.shape == (XY, XY) and view.dtype == dtype and view.strides == (item, item * XY)       # [x, y], x fastest
        assert _offset(view, lib) == offset
        assert view.tobytes(order="F") == lib.buffers[-1][offset:offset + item * n2].tobytes()             # the buffer itself
        assert view.flags.writeable


def _check_grids(out, lib):
    n2 = XY * XY
    assert len(out) == 6 and out[0].shape == (3,) and out[0].dtype == np.float64
    for k, grid in enumerate(out[1:]):
        assert grid.shape == (n2,) and grid.dtype == np.int8 and grid.strides == (1,) and _offset(grid, lib) == k * n2
        assert grid.tobytes() == lib.buffers[-1][k * n2:(k + 1) * n2].tobytes()


def test_combine_into_returns_views_of_one_pinned_buffer():
    g = make_gvom()
    lib = g._lib
    rc, out = g._combine_into(lib.gvom_combine_maps_into)
    assert rc == gvom.GVOM_OK
    assert [n for n, _ in lib.calls] == ["gvom_output_buffer_alloc", "gvom_combine_maps_into"]
    assert lib.calls[1][1][2] == lib.buffers[0].ctypes.data
    _check_maps(out, lib)
    g._c_order = False
    _check_maps(g.combine_maps(), lib)              # the first call's arrays are alive: a second buffer
    assert len(lib.buffers) == 2
    del out
    out = g.combine_maps()                          # ... dropped: its buffer comes back from the pool, nothing is allocated
    assert len(lib.buffers) == 2 and len(lib.named("gvom_output_buffer_alloc")) == 2
    assert lib.named("gvom_combine_maps_into")[-1][2] == lib.buffers[0].ctypes.data


def test_combine_into_passes_a_refusal_on():
    g = make_gvom()
    assert g._combine_into(lambda h, origin, ptr: gvom.GVOM_EMPTY_BUFFER) == (gvom.GVOM_EMPTY_BUFFER, None)
    assert len(g._out_pool.free) == 1               # the buffer went back


def test_pending_maps_result_builds_the_same_views():
    g = make_gvom()
    lib = g._lib
    pending = g.combine_maps_async()
    assert lib.named("gvom_combine_begin") == [(None, lib.buffers[0].ctypes.data, None)]
    assert lib.named("gvom_combine_end") == []
    out = pending.result()
    assert len(lib.named("gvom_combine_end")) == 1
    _check_maps(out, lib)
    assert pending.result() is out and len(lib.named("gvom_combine_end")) == 1


def test_occupancy_combines_return_five_int8_grids():
    g = make_gvom()
    lib = g._lib
    out = g.combine_maps_occupancy(40, -8, 1)
    assert lib.named("gvom_combine_occupancy_into")[0][2:] == (lib.buffers[0].ctypes.data, 40.0, -8.0, 1.0)
    _check_grids(out, lib)
    pending = g.combine_maps_occupancy_async(40, -8, 1)
    assert lib.named("gvom_combine_begin") == [(None, lib.buffers[1].ctypes.data, (40.0, -8.0, 1.0))]
    _check_grids(pending.result(), lib)


def test_an_empty_ring_warns_once_per_call_and_returns_nothing(capsys):
    g = make_gvom()
    empty = type("EmptyRing", (RecordingLib,), {})(XY * XY * 20)
    real = RecordingLib.__getattr__

    def entry_or_empty(self, name):
        f = real(self, name)
        if name in ("gvom_combine_maps_into", "gvom_combine_maps_device", "gvom_combine_begin", "gvom_combine_occupancy_into"):
            return lambda *a: (f(*a), gvom.GVOM_EMPTY_BUFFER)[1]
        return f
    type(empty).__getattr__ = entry_or_empty
    g._lib, g._c_order = empty, False
    text = "[WARNING] The map buffer is empty, nothing will happen!\n"
    for call in (g.combine_maps, g.combine_maps_device, g.combine_maps_occupancy):
        assert call() is None
        assert capsys.readouterr().out == text
    for call in (g.combine_maps_async, g.combine_maps_occupancy_async):
        pending = call()
        assert capsys.readouterr().out == text
        assert pending.result() is None
    assert empty.named("gvom_combine_end") == []
    assert len(empty.buffers) == 1                  # every refused call gave its buffer back
