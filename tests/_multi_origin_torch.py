"""Child process of tests/test_multi_origin.py: a multi-origin scan whose cloud AND index a torch tensor holds in HBM.  torch is
imported FIRST, so that libgvom_hip.so binds to the HIP runtime torch carries (one runtime in the process).
python _multi_origin_torch.py CASE"""
import os
import sys

import torch

torch.cuda.init()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "g-vom_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np  # noqa: E402

import gvom  # noqa: E402
import multi_origin_ref as mo  # noqa: E402


def case_device_index_guard():
    """a device index cannot be checked by the host: entries K and 65535 make their returns vanish -- the result is the host
    route's with those returns removed -- and index = None on the device route is i % K"""
    for grid, dtype in (("p2", np.float32), ("np2", np.float64)):
        prm = mo.params(grid, 2)
        dev, host = gvom.Gvom(*prm, voxel_statistics=False), gvom.Gvom(*prm, voxel_statistics=False)
        for k in range(3):
            pc, origins, index, ego, tf = mo.scan_inputs(grid, k, dtype)
            bad = index.copy()
            rng = np.random.default_rng(k)
            gone = rng.choice(mo.N, 700, replace=False)
            bad[gone[:350]] = mo.K
            bad[gone[350:]] = 65535
            keep = np.ones(mo.N, bool)
            keep[gone] = False
            if k == 2:                                        # no index at all: i % K on both routes
                bad, keep = None, np.ones(mo.N, bool)
            tc = torch.from_numpy(pc).cuda()
            ti = None if bad is None else torch.from_numpy(bad.view(np.int16)).cuda()
            torch.cuda.synchronize()                          # the data is ready when the call is made
            rc = dev.process_pointcloud_origins_device(tc.data_ptr(), mo.N, dtype, origins, ego, tf, None if ti is None else ti.data_ptr())
            assert rc == 0, rc
            host.process_pointcloud_origins(pc[keep], origins, ego, tf, None if bad is None else index[keep])
            a, b = dev.read_dense(dev.last_buffer_index), host.read_dense(host.last_buffer_index)
            assert a[5] > 1000
            for u, v in zip(a[:5], b[:5]):
                assert np.array_equal(u, v), (grid, k)
            sa, sb = dev.scan_stats(), host.scan_stats()
            assert {n: sa[n] for n in ("cells", "sum_hit", "sum_total")} == {n: sb[n] for n in ("cells", "sum_hit", "sum_total")}
            for u, v in zip(dev.combine_maps(), host.combine_maps()):
                assert np.array_equal(np.asarray(u), np.asarray(v)), (grid, k)
            del tc, ti


if __name__ == "__main__":
    name = sys.argv[1]
    globals()["case_" + name]()
    print("CASE OK " + name)
