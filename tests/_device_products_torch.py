"""Child process of tests/test_device_products.py: the cases with a torch consumer.  torch is imported FIRST, so that
libgvom_hip.so binds to the HIP runtime torch carries (one runtime in the process).  python _device_products_torch.py CASE"""
import os
import sys

import torch

torch.cuda.init()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "g-vom_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import gc  # noqa: E402

import numpy as np  # noqa: E402

import gvom  # noqa: E402
import synth  # noqa: E402

TORCH_DTYPES = {np.dtype(np.uint8): torch.uint8, np.dtype(np.float32): torch.float32, np.dtype(np.int64): torch.int64}


def _mapper(name="m256", n_scans=1, combined=True, **kw):
    params, scans = synth.config_inputs(name, n_scans=n_scans)
    g = gvom.Gvom(*params, **kw)
    if combined:
        g.process_pointcloud(*scans[0])
        assert g.combine_maps() is not None
    return g, scans


def _contiguous_strides(shape):
    st, n = [], 1
    for d in reversed(shape):
        st.insert(0, n)
        n *= d
    return tuple(st)


def case_zero_copy():
    g, _ = _mapper("c3", voxel_statistics=True)
    map_sets = g.get_tuning("device_map_sets")
    cloud = g.voxel_cloud_device()
    arrays = [g.occupancy_grid_device(), g.height_cloud_device(), g.inferred_height_cloud_device(), cloud.rows, cloud.eigenvalues,
              cloud.count]
    n2, n = g.xy_size * g.xy_size, g.combined_cell_count_cpu
    assert [a.shape for a in arrays] == [(g.xy_size, g.xy_size, g.z_size), (n2, 7), (n2, 3), (n, 8), (n, 3), (1,)]
    for a in arrays:
        want = a.copy_to_host()
        assert a.__dlpack_device__() == (10, 0)
        stream = torch.cuda.current_stream().cuda_stream
        for t in (torch.from_dlpack(a), torch.from_dlpack(a.__dlpack__(stream=stream))):          # versioned, legacy capsule
            assert t.device == torch.device("cuda:0") and t.dtype == TORCH_DTYPES[a.dtype]
            assert tuple(t.shape) == a.shape and t.stride() == _contiguous_strides(a.shape) == a.strides
            assert t.is_contiguous() and t.data_ptr() == a.ptr
            assert np.array_equal(t.cpu().numpy(), want)
            del t
        cap = a.__dlpack__(max_version=(1, 0))               # never consumed: its destructor gives the export back
        del cap
        for kw in ({"copy": True}, {"dl_device": (1, 0)}):
            try:
                a.__dlpack__(**kw)
                raise AssertionError("accepted %r" % (kw,))
            except BufferError:
                pass
    assert int(torch.from_dlpack(arrays[0]).sum()) == n == int(torch.from_dlpack(cloud.count)[0])
    torch.cuda.synchronize()
    sets = g.get_tuning("device_product_sets")
    assert sets == 4
    for a in arrays:
        a.release()
    g.occupancy_grid_device().release()                      # every export came back: the sets are reused
    g.voxel_cloud_device().release()
    assert g.get_tuning("device_product_sets") == sets
    assert g.get_tuning("device_map_sets") == map_sets == 0


def case_consumer_stream():
    g, scans = _mapper("m256", n_scans=4, voxel_statistics=False)
    occ = g.occupancy_grid_device()
    want = occ.copy_to_host()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = torch.from_dlpack(occ)
        torch.cuda._sleep(100_000_000)                       # the consumer is slow; the mapper goes on meanwhile
        columns = t.sum(dim=2, dtype=torch.int32)            # occupied voxels per (x, y) column
        total = t.sum(dtype=torch.int64)
        del t
    for pc, ego, tf in scans[1:]:
        g.process_pointcloud(pc, ego, tf)
        m = g.combine_maps_device()
        g.occupancy_grid_device()                            # (unheld: the held product is never the one reused)
        m.release()
    side.synchronize()
    assert np.array_equal(columns.cpu().numpy(), want.sum(axis=2, dtype=np.int32))
    assert int(total) == int(want.sum()) > 0
    assert np.array_equal(occ.copy_to_host(), want)
    assert not np.array_equal(g.get_map_as_occupancy_grid(), want.astype(bool))


def case_reuse_waits():
    g, scans = _mapper("m256", n_scans=4, voxel_statistics=False)
    occ = g.occupancy_grid_device()
    want = occ.copy_to_host()
    ptr = occ.ptr
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = torch.from_dlpack(occ)
        torch.cuda._sleep(200_000_000)                       # the consumer is slow...
        clone = t.clone()
        del t                                                # ...and drops its tensor at once: the release is stream-ordered
    occ.release()
    del occ
    for pc, ego, tf in scans[1:]:                            # the set is free now: the next products reuse it
        g.process_pointcloud(pc, ego, tf)
        g.combine_maps()
        nxt = g.occupancy_grid_device()
        assert nxt.ptr == ptr
        nxt.release()
    assert g.get_tuning("device_product_sets") == 1
    side.synchronize()
    assert not np.array_equal(want.astype(bool), g.get_map_as_occupancy_grid())    # (the later products hold other grids)
    assert np.array_equal(clone.cpu().numpy(), want)


def case_pool():
    g, _ = _mapper("c3", voxel_statistics=False)
    m = g.combine_maps_device()
    map_sets = g.get_tuning("device_map_sets")
    assert map_sets == 1
    for k in range(30):
        t = torch.from_dlpack(g.occupancy_grid_device())
        s = int(t.sum())
        del t
        assert s == g.combined_cell_count_cpu
    assert 1 <= g.get_tuning("device_product_sets") <= 2
    held = [g.occupancy_grid_device() for _ in range(4)]
    assert len({a.ptr for a in held}) == 4
    try:
        g.occupancy_grid_device()
        raise AssertionError("a fifth occupancy set was handed out")
    except gvom.GvomBackendError as e:
        assert "all 4 device product sets of this kind" in str(e), e
    clouds = [g.height_cloud_device() for _ in range(4)]     # the cap is per kind
    try:
        g.height_cloud_device()
        raise AssertionError("a fifth height-cloud set was handed out")
    except gvom.GvomBackendError as e:
        assert "all 4 device product sets of this kind" in str(e), e
    assert g.get_tuning("device_product_sets") == 8
    for a in held + clouds:
        a.release()
    a = g.occupancy_grid_device()
    assert a is not None and g.get_tuning("device_product_sets") == 8
    assert int(a.copy_to_host().sum()) == g.combined_cell_count_cpu
    assert g.get_tuning("device_map_sets") == map_sets       # no product call touched the map sets
    m.release()


def case_outlives():
    g, _ = _mapper("c3", voxel_statistics=True)
    occ, cloud = g.occupancy_grid_device(), g.voxel_cloud_device()
    want, want_rows = occ.copy_to_host(), cloud.rows.copy_to_host()
    t, r = torch.from_dlpack(occ), torch.from_dlpack(cloud.rows)
    del occ, cloud                                           # the product objects go (their exports with them)...
    gc.collect()
    assert np.array_equal(t.cpu().numpy(), want)
    del g                                                    # ...and the mapper
    gc.collect()
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), want) and np.array_equal(r.cpu().numpy(), want_rows)
    del t, r                                                 # the last releases free the orphaned sets
    torch.cuda.synchronize()


if __name__ == "__main__":
    name = sys.argv[1]
    globals()["case_" + name]()
    print("CASE OK " + name)
