"""Device-resident 3-D products (Gvom.occupancy_grid_device, voxel_cloud_device, height_cloud_device,
inferred_height_cloud_device): the occupancy grid (k_occupancy) and the debug clouds left in HBM as product sets and handed to a
GPU consumer through DLPack.  Held to the golden fixtures, bit-identical to the host forms, the occupancy grid to the oracle at
full size; snapshots, torch consumers, lifetime, no-data and error cases.  CPU: the ABI and k_occupancy's registers."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
for _p in (ROOT, os.path.join(ROOT, "g-vom_amd"), os.path.join(ROOT, "tests"), G):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import scenarios  # noqa: E402
import synth  # noqa: E402
from parity import compare_records  # noqa: E402

gpu = pytest.mark.gpu
NEW_SYMBOLS = ("gvom_device_product", "gvom_device_product_export", "gvom_device_product_release", "gvom_device_product_dlpack",
               "gvom_device_product_copy")


@pytest.fixture(scope="module")
def gvom():
    import gvom as mod
    rc, info = mod.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    return mod


# ---- CPU: header, library and binding; the kernel's registers ------------------------------------------------------------
def test_abi_10_and_the_five_product_symbols():
    import gvom as mod
    header = open(os.path.join(ROOT, "include", "gvom_hip.h")).read()
    assert int(re.search(r"#define\s+GVOM_ABI_VERSION\s+(\d+)", header).group(1)) == 10
    assert mod.ABI_VERSION == 10 and mod.load_library().gvom_abi_version() == 10
    L = ctypes.CDLL(mod.library_path())
    bound = {n for n, _, _ in mod.ABI}
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in bound, name
    for word, value in (("GVOM_PRODUCT_OCCUPANCY", mod.PRODUCT_OCCUPANCY), ("GVOM_PRODUCT_VOXEL_CLOUD", mod.PRODUCT_VOXEL_CLOUD),
                        ("GVOM_PRODUCT_HEIGHT_CLOUD", mod.PRODUCT_HEIGHT_CLOUD),
                        ("GVOM_PRODUCT_INFERRED_HEIGHT_CLOUD", mod.PRODUCT_INFERRED_HEIGHT_CLOUD)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % word, header).group(1)) == value
    for m in ("occupancy_grid_device", "voxel_cloud_device", "height_cloud_device", "inferred_height_cloud_device"):
        assert callable(getattr(mod.Gvom, m))


def test_k_occupancy_uses_no_scratch_and_fits_four_waves_per_simd():
    """512 VGPRs per SIMD lane: 4 waves need <= 128 each.  Both forms of the dead-column handling and the z_size % 4 fallback."""
    import gvom as mod
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    if not os.path.exists(os.path.join(kernel_regs.LLVM, "clang-offload-bundler")):
        pytest.skip("no ROCm LLVM tools")
    kernels = kernel_regs.kernels(mod.library_path())
    occ = {k: v for k, v in kernels.items() if "k_occupancy" in k}
    assert len(occ) == 3, sorted(kernels)
    for k, v in occ.items():
        assert v["scratch"] == 0, (k, v)
        assert v["vgpr"] <= 128, (k, v)


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def _product_route_class(gvom):
    class ProductRouteGvom(gvom.Gvom):
        """The four debug reads through the device products and copy_to_host()."""

        def get_map_as_occupancy_grid(self):
            a = self.occupancy_grid_device()
            if a is None:
                raise AttributeError("'NoneType' object has no attribute 'copy_to_host'")
            with a:
                return a.copy_to_host().astype(bool)

        def make_debug_voxel_map(self):
            c = self.voxel_cloud_device()
            if c is None:
                return None
            with c:
                return c.copy_to_host()

        def make_debug_height_map(self):
            a = self.height_cloud_device()
            if a is None:
                return None
            with a:
                return a.copy_to_host()

        def make_debug_inferred_height_map(self):
            a = self.inferred_height_cloud_device()
            if a is None:
                return None
            with a:
                return a.copy_to_host()

    return ProductRouteGvom


@gpu
@pytest.mark.parametrize("name", ["f1", "f2", "f3", "f4", "f5", "f6"])
def test_product_route_reproduces_reference_golden(gvom, name):
    want = np.load(os.path.join(G, name + ".npz"))
    sc = scenarios.scenario_from_record(want)
    got = scenarios.run_and_record(_product_route_class(gvom), sc)
    assert any(k.endswith("_occupancy") for k in got) and any(k.endswith("_debug_height_map") for k in got)
    assert compare_records(got, want, float_tol=1e-5, stats_rtol=1e-6, stats_atol=1e-9) > 5


def _voxel_order(g, rows):
    """Permutation that sorts voxel-cloud rows into voxel order (the rows carry their world coordinates, gvom.py:462-466)."""
    st = g._state()
    x = np.rint(rows[:, 0].astype(np.float64) / g.xy_resolution - st.combined_origin[0]).astype(np.int64)
    y = np.rint(rows[:, 1].astype(np.float64) / g.xy_resolution - st.combined_origin[1]).astype(np.int64)
    z = np.rint(rows[:, 2].astype(np.float64) / g.z_resolution - st.combined_origin[2]).astype(np.int64)
    key = x + y * g.xy_size + z * g.xy_size * g.xy_size
    assert np.unique(key).shape[0] == key.shape[0]
    return np.argsort(key, kind="stable")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_against_host_forms(g, what, voxel=True):
    occ = g.occupancy_grid_device()
    assert occ.shape == (g.xy_size, g.xy_size, g.z_size) and occ.dtype == np.uint8
    got = occ.copy_to_host()
    want = g.get_map_as_occupancy_grid()
    assert got.dtype == np.uint8 and got.flags.c_contiguous and got.max() <= 1
    assert np.array_equal(got.astype(bool), want), "%s: occupancy differs in %d voxels" % (what, int(np.sum(got.astype(bool) != want)))
    assert int(got.sum()) == g.combined_cell_count_cpu, what
    occ.release()
    for dev, host, cols in ((g.height_cloud_device, g.make_debug_height_map, 7),
                            (g.inferred_height_cloud_device, g.make_debug_inferred_height_map, 3)):
        with dev() as a:
            assert a.shape == (g.xy_size * g.xy_size, cols) and a.dtype == np.float32
            assert np.array_equal(_bits(a.copy_to_host()), _bits(host())), (what, cols)
    if voxel:
        cloud = g.voxel_cloud_device()
        want_rows = g.make_debug_voxel_map()
        assert (cloud is None) == (want_rows is None), what
        if cloud is not None:
            n = int(cloud.count.copy_to_host()[0])
            assert n == want_rows.shape[0] == g.combined_cell_count_cpu, what
            rows, eig = cloud.copy_to_host(), cloud.eigenvalues_to_host()
            assert rows.shape == (n, 8) and eig.shape == (n, 3) and rows.dtype == eig.dtype == np.float32
            o = _voxel_order(g, rows)
            assert np.array_equal(_bits(rows[o]), _bits(want_rows[_voxel_order(g, want_rows)])), what
            assert np.array_equal(_bits(eig[o]), _bits(g.voxels_eigenvalues.copy_to_host())), what
            assert np.array_equal(_bits(rows[:, 7]), _bits(eig[:, 2]))          # (column 7 is the smallest eigenvalue: row for row)
            cloud.release()
    return got


def _run(gvom, params, scans, voxel=True, **kw):
    g = gvom.Gvom(*params, **kw)
    for k, (pc, ego, tf) in enumerate(scans):
        g.process_pointcloud(pc, ego, tf)
        assert g.combine_maps() is not None
        _check_against_host_forms(g, "step %d" % k, voxel)
    return g


@gpu
def test_products_bit_identical_m256_eager(gvom):
    params, scans = synth.config_inputs("m256", n_scans=8)
    assert params[4] == 1
    g = _run(gvom, params, scans, voxel=False, voxel_statistics=False)
    assert g.get_tuning("eager_adopted") > 0


@gpu
def test_products_bit_identical_c3_ring_fills_wraps_evicts(gvom):
    params, scans = synth.config_inputs("c3", n_scans=10)
    assert params[4] == 8
    _run(gvom, params, scans)


def _small_scans(xy, zs, n=4):
    rng = np.random.default_rng(xy * 100 + zs)
    half = 0.4 * xy / 2
    scans = []
    for k in range(n):
        ego = (0.4 * k, -0.3 * k, 0.0)
        pc = np.stack([rng.uniform(-half, half, 3000) + ego[0], rng.uniform(-half, half, 3000) + ego[1],
                       rng.normal(-0.8, 0.5, 3000)], axis=1)
        scans.append((pc, ego, scenarios.rot_z(0.03 * k, (0.0, 0.0, 0.0))))
    return scans


@gpu
@pytest.mark.parametrize("xy,zs", [(30, 20), (16, 4), (30, 18), (72, 133)])
def test_products_bit_identical_odd_grids(gvom, xy, zs):
    """(30, 18) and (72, 133): z_size % 4 != 0, the plain form of k_occupancy"""
    params = (0.4, 0.2, xy, zs, 2, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
    _run(gvom, params, _small_scans(xy, zs))


@gpu
@pytest.mark.parametrize("name", ["m256", "c3"])
def test_both_dead_column_forms_write_the_same_grid(gvom, name):
    params, scans = synth.config_inputs(name, n_scans=3)
    g = gvom.Gvom(*params, voxel_statistics=False)
    for pc, ego, tf in scans:
        g.process_pointcloud(pc, ego, tf)
        g.combine_maps()
    grids = []
    for clear in (0, 1, 0):
        g.set_tuning("occupancy_clear", clear)
        with g.occupancy_grid_device() as a:
            grids.append(a.copy_to_host())
    assert np.array_equal(grids[0], grids[1]) and np.array_equal(grids[0], grids[2])
    assert int(grids[0].sum()) == g.combined_cell_count_cpu > 0


@gpu
@pytest.mark.parametrize("name", ["m256", "c4"])
def test_occupancy_matches_the_oracle_at_full_size(gvom, name):
    from oracle import oracle
    params, scans = synth.config_inputs(name, n_scans=1)
    g, o = gvom.Gvom(*params, voxel_statistics=False), oracle.OracleGvom(*params)
    for m in (g, o):
        m.process_pointcloud(*scans[0])
        assert m.combine_maps() is not None
    want = np.asarray(o.get_map_as_occupancy_grid())
    with g.occupancy_grid_device() as a:
        got = a.copy_to_host()
    assert got.shape == want.shape
    assert np.array_equal(got.astype(bool), want.astype(bool)), int(np.sum(got.astype(bool) != want.astype(bool)))
    assert int(got.sum()) == g.combined_cell_count_cpu == int(want.sum())
    assert np.array_equal(g.get_map_as_occupancy_grid(), want.astype(bool))


@gpu
def test_products_are_snapshots(gvom):
    params, scans = synth.config_inputs("c3", n_scans=4)
    g = gvom.Gvom(*params)
    for pc, ego, tf in scans[:2]:
        g.process_pointcloud(pc, ego, tf)
        g.combine_maps()
    prods = [g.occupancy_grid_device(), g.height_cloud_device(), g.inferred_height_cloud_device()]
    cloud = g.voxel_cloud_device()
    assert cloud is not None
    prods += [cloud.rows, cloud.eigenvalues, cloud.count]
    before = [p.copy_to_host() for p in prods]
    for k, (pc, ego, tf) in enumerate(scans[2:]):
        ego = (ego[0] + 3.0 * (k + 1), ego[1] - 2.0 * (k + 1), ego[2] + 0.4)       # the window moves in x, y and z
        g.process_pointcloud(pc + np.asarray(ego, pc.dtype), ego, tf)
        g.combine_maps()
    assert not np.array_equal(g.get_map_as_occupancy_grid(), before[0].astype(bool))
    after = [p.copy_to_host() for p in prods]
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    fresh = g.occupancy_grid_device()
    assert fresh.ptr != prods[0].ptr                       # the held product was not reused
    assert np.array_equal(fresh.copy_to_host().astype(bool), g.get_map_as_occupancy_grid())


def _torch_case(name):
    """One case per fresh child process that imports torch BEFORE the library is loaded (one HIP runtime in the process)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_device_products_torch.py"), name],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "CASE OK " + name in r.stdout, r.stdout[-4000:]


@gpu
def test_dlpack_zero_copy_through_torch():
    _torch_case("zero_copy")


@gpu
def test_consumer_reduces_the_grid_on_its_own_stream_while_the_mapper_goes_on():
    _torch_case("consumer_stream")


@gpu
def test_reuse_waits_for_the_consumers_release():
    _torch_case("reuse_waits")


@gpu
def test_product_pool_caps_per_kind_and_leaves_map_sets_alone():
    _torch_case("pool")


@gpu
def test_exported_tensors_outlive_the_product_object_and_the_mapper():
    _torch_case("outlives")


@gpu
def test_no_data_before_the_first_combine_and_without_statistics(gvom, capsys):
    params, scans = synth.config_inputs("c3", n_scans=6)
    g = gvom.Gvom(*params, voxel_statistics=False)
    for m in (g.occupancy_grid_device, g.voxel_cloud_device, g.height_cloud_device, g.inferred_height_cloud_device):
        assert m() is None
    assert capsys.readouterr().out.count("No data") == 3    # the host forms of the three clouds print it; the grid's raises
    g.process_pointcloud(*scans[0])
    for m in (g.occupancy_grid_device, g.voxel_cloud_device, g.height_cloud_device, g.inferred_height_cloud_device):
        assert m() is None                                   # a scan is not a combine
    g.combine_maps()
    assert g.voxel_cloud_device() is None                    # voxel_statistics=False: never
    assert g.occupancy_grid_device() is not None and g.height_cloud_device() is not None
    assert g.get_tuning("device_product_sets") == 2 and g.get_tuning("device_map_sets") == 0


@gpu
def test_device_cloud_reads_keep_on_demand_statistics_alive(gvom):
    """A default-constructor handle read ONLY through voxel_cloud_device(): three combines without a read would switch the
    statistics off; the device form counts as a read."""
    params, scans = synth.config_inputs("c3", n_scans=7)
    g, ref = gvom.Gvom(*params), gvom.Gvom(*params, voxel_statistics=True)
    for k, (pc, ego, tf) in enumerate(scans):
        for m in (g, ref):
            m.process_pointcloud(pc, ego, tf)
            m.combine_maps()
        cloud = g.voxel_cloud_device()
        assert cloud is not None, k
        rows, want = cloud.copy_to_host(), ref.make_debug_voxel_map()
        assert rows.shape == want.shape and rows.shape[0] == g.combined_cell_count_cpu
        assert np.array_equal(_bits(rows[_voxel_order(g, rows)]), _bits(want[_voxel_order(ref, want)])), k
        cloud.release()
    idle = gvom.Gvom(*params)                                # the same handle, nobody reading: they do go off
    for pc, ego, tf in scans[:5]:
        idle.process_pointcloud(pc, ego, tf)
        idle.combine_maps()
    assert idle.voxel_cloud_device() is None


@gpu
def test_voxel_cloud_cap_drops_rows_and_still_counts_them(gvom):
    params, scans = synth.config_inputs("c3", n_scans=1)
    g = gvom.Gvom(*params, voxel_statistics=True)
    g.process_pointcloud(*scans[0])
    g.combine_maps()
    n = g.combined_cell_count_cpu
    full = g.make_debug_voxel_map()
    with g.voxel_cloud_device(max_rows=100) as c:
        assert c.rows.shape == (100, 8) and c.eigenvalues.shape == (100, 3) and c.count.shape == (1,)
        assert int(c.count.copy_to_host()[0]) == n > 100
        rows = c.copy_to_host()
    assert rows.shape == (100, 8)
    have = {r.tobytes() for r in full}
    assert all(r.tobytes() in have for r in rows)


@gpu
def test_stale_ids_bad_parts_and_sharded_handles_are_errors(gvom):
    params, scans = synth.config_inputs("c3", n_scans=1)
    g = gvom.Gvom(*params, voxel_statistics=False)
    g.process_pointcloud(*scans[0])
    g.combine_maps()
    a = g.occupancy_grid_device()
    p, nd, sh, st = ctypes.c_void_p(), ctypes.c_int32(), (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()

    def export(pid, part):
        return g._check(g._lib.gvom_device_product_export(g._h, pid, part, None, ctypes.byref(p), ctypes.byref(nd), sh, st))
    for part in (-1, 1, 3):
        with pytest.raises(gvom.GvomBackendError, match="part index"):
            export(a.product_id, part)
    for pid in (-1, 0, 10 ** 9):
        with pytest.raises(gvom.GvomBackendError, match="unknown or stale device product id"):
            export(pid, 0)
        with pytest.raises(gvom.GvomBackendError, match="unknown or stale device product id"):
            g._check(g._lib.gvom_device_product_release(g._h, pid, None))
    with pytest.raises(gvom.GvomBackendError, match="unknown product kind"):
        g._device_product(9)
    old = a
    old.release()
    with pytest.raises(gvom.GvomBackendError, match="no live export"):
        g._check(g._lib.gvom_device_product_release(g._h, old.product_id, None))
    g.occupancy_grid_device().release()                      # the unheld product went back to the pool: its id is stale
    with pytest.raises(gvom.GvomBackendError, match="unknown or stale device product id"):
        old.copy_to_host()
    assert g.get_tuning("device_product_sets") == 1
    sharded = gvom.Gvom(*((0.2, 0.2, 64, 32, 1) + params[5:]), voxel_statistics=False, _shard=(0, 2))
    for kind in (1, 2, 3, 4):
        with pytest.raises(gvom.GvomBackendError, match="sharded handles are not supported"):
            sharded._device_product(kind)
