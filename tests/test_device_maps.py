"""Device-resident maps (Gvom.combine_maps_device): the nine maps of a combine left in HBM as a map set and handed to a GPU
consumer through DLPack with stream ordering and no host wait.  Held to the golden fixtures, bit-identical to the host
routes, interleaved with them, zero-copy through torch, reuse ordered behind the consumer's reads, lifetime and errors."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
for _p in (os.path.join(ROOT, "g-vom_amd"), os.path.join(ROOT, "tests"), G):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import scenarios  # noqa: E402
import synth  # noqa: E402
from parity import compare_records  # noqa: E402

pytestmark = pytest.mark.gpu

MAP_ATTRS = ("height_map", "inferred_height_map", "x_slope_map", "y_slope_map", "guessed_height_delta")


@pytest.fixture(scope="module")
def gvom():
    import gvom as mod
    rc, info = mod.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    return mod


def _device_route_class(gvom):
    class DeviceRouteGvom(gvom.Gvom):
        """combine_maps through combine_maps_device; the 2-D attributes from the same map set."""

        def __init__(self, *p, **kw):
            super(DeviceRouteGvom, self).__init__(*p, **kw)
            self._set = None

        def combine_maps(self):
            m = self.combine_maps_device()
            if m is None:
                return None
            if self._set is not None:
                self._set.release()
            self._set = m
            return (m.origin, m.positive.copy_to_host(), m.negative.copy_to_host(), m.roughness.copy_to_host(),
                    m.visibility.copy_to_host())

    for attr, dev in [(a, a) for a in MAP_ATTRS] + [("roughness_map", "roughness")]:
        setattr(DeviceRouteGvom, attr, property(lambda self, dev=dev: getattr(self._set, dev) if self._set is not None else None))
    return DeviceRouteGvom


@pytest.mark.parametrize("name", ["f1", "f2", "f3", "f4", "f5", "f6"])
def test_device_route_reproduces_reference_golden(gvom, name):
    want = np.load(os.path.join(G, name + ".npz"))
    sc = scenarios.scenario_from_record(want)
    got = scenarios.run_and_record(_device_route_class(gvom), sc)
    assert compare_records(got, want, float_tol=1e-5, stats_rtol=1e-6, stats_atol=1e-9) > 5


def _host_maps(g, out):
    origin, pos, neg, rough, vis = out
    return [np.asarray(origin), pos, neg, vis, rough] + [getattr(g, a).copy_to_host() for a in MAP_ATTRS]


def _device_maps(m):
    return [m.origin] + [getattr(m, n).copy_to_host() for n in ("positive", "negative", "visibility", "roughness") + MAP_ATTRS]


def _assert_same(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k, x.dtype, y.dtype, x.shape, y.shape)
        assert np.array_equal(x, y), "%s: map %d differs in %d cells" % (what, k, int(np.sum(x != y)))


def _pair(gvom, params, scans, **kw):
    """Two handles fed the same scans: one combines through combine_maps(), one through combine_maps_device()."""
    h, d = gvom.Gvom(*params, **kw), gvom.Gvom(*params, **kw)
    for k, (pc, ego, tf) in enumerate(scans):
        h.process_pointcloud(pc, ego, tf)
        d.process_pointcloud(pc, ego, tf)
        want = _host_maps(h, h.combine_maps())
        m = d.combine_maps_device()
        assert m is not None
        assert d.combined_cell_count_cpu == h.combined_cell_count_cpu, k
        _assert_same(_device_maps(m), want, "step %d" % k)
        m.release()
    return h, d


def test_device_route_bit_identical_m256_eager(gvom):
    params, scans = synth.config_inputs("m256", n_scans=8)
    assert params[4] == 1
    h, d = _pair(gvom, params, scans, voxel_statistics=False)
    assert d.get_tuning("eager_adopted") > 0 and d.get_tuning("eager_adopted") == h.get_tuning("eager_adopted")


def test_device_route_bit_identical_c3_ring_fills_wraps_evicts(gvom):
    params, scans = synth.config_inputs("c3", n_scans=10)
    assert params[4] == 8
    _pair(gvom, params, scans)


@pytest.mark.parametrize("xy,zs", [(30, 20), (16, 4)])
def test_device_route_bit_identical_odd_grids(gvom, xy, zs):
    rng = np.random.default_rng(xy * 100 + zs)
    params = (0.4, 0.2, xy, zs, 2, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
    half = 0.4 * xy / 2
    scans = []
    for k in range(4):
        ego = (0.4 * k, -0.3 * k, 0.0)
        pc = np.stack([rng.uniform(-half, half, 3000) + ego[0], rng.uniform(-half, half, 3000) + ego[1],
                       rng.normal(-0.8, 0.5, 3000)], axis=1)
        scans.append((pc, ego, scenarios.rot_z(0.03 * k, (0.0, 0.0, 0.0))))
    _pair(gvom, params, scans)


def test_device_route_interleaves_with_host_routes(gvom):
    params, scans = synth.config_inputs("c2", n_scans=1)
    pc0, _, _ = scans[0]
    a, b = gvom.Gvom(*params), gvom.Gvom(*params)
    for k in range(6):
        ego = (0.3 * k, 0.1 * k, 0.0)
        pc = pc0 + np.asarray(ego, pc0.dtype)
        a.process_pointcloud(pc, ego)
        b.process_pointcloud(pc, ego)
        want = b.combine_maps()
        if k % 3 == 0:
            got = a.combine_maps()
        elif k % 3 == 1:
            m = a.combine_maps_device()
            got = (m.origin, m.positive.copy_to_host(), m.negative.copy_to_host(), m.roughness.copy_to_host(),
                   m.visibility.copy_to_host())
            m.release()
        else:
            got = a.combine_maps_async().result()
        _assert_same(list(got), list(want), "step %d" % k)
        assert a.combined_cell_count_cpu == b.combined_cell_count_cpu


def _torch_case(name):
    """The torch consumer cases run in a fresh child process that imports torch BEFORE the library is loaded: libgvom_hip.so
    then binds to the HIP runtime torch carries (one runtime per process).  This process has long
    loaded the library against the system runtime."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_device_maps_torch.py"), name],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "CASE OK " + name in r.stdout, r.stdout[-4000:]


def test_dlpack_zero_copy_through_torch():
    """versioned and legacy capsules: device, dtype, shape, strides, the exported address, the values; unconsumed capsules and
    the copy / cross-device requests"""
    _torch_case("zero_copy")


def test_reuse_waits_for_the_consumers_reads():
    """a slow consumer on its own stream drops its tensor at once; three more combines without a host sync do not overwrite
    what it has still to read"""
    _torch_case("reuse_waits")


def test_pool_stays_small_and_caps_at_eight():
    _torch_case("pool")


def test_exported_tensor_outlives_the_mapper():
    _torch_case("outlives")


def test_empty_ring_sharded_handle_and_bad_arguments(gvom, capsys):
    import ctypes
    params, scans = synth.config_inputs("m256")
    g = gvom.Gvom(*params, voxel_statistics=False)
    assert g.combine_maps_device() is None
    assert "[WARNING] The map buffer is empty, nothing will happen!" in capsys.readouterr().out
    g.process_pointcloud(*scans[0])
    m = g.combine_maps_device()
    p, st = ctypes.c_void_p(), (ctypes.c_int64 * 2)()
    for which in (-1, 9):
        with pytest.raises(gvom.GvomBackendError):
            g._check(g._lib.gvom_device_map_export(g._h, m.set_id, which, None, ctypes.byref(p), st))
    with pytest.raises(gvom.GvomBackendError):
        g._check(g._lib.gvom_device_map_export(g._h, m.set_id, 0, None, None, st))
    old = m
    old.release()
    g.process_pointcloud(*scans[0])
    g.combine_maps_device().release()                    # the unheld set went back to the pool: its id is stale
    with pytest.raises(gvom.GvomBackendError):
        old.height_map.copy_to_host()
    with pytest.raises(gvom.GvomBackendError):
        g._check(g._lib.gvom_device_map_release(g._h, 10 ** 9, None))
    sharded = gvom.Gvom(*((0.2, 0.2, 64, 32, 1) + params[5:]), voxel_statistics=False, _shard=(0, 2))
    with pytest.raises(gvom.GvomBackendError):
        sharded.combine_maps_device()
