"""Child process of tests/test_frontier.py: the case with a torch consumer.  torch is imported FIRST, so that libgvom_hip.so binds
to the HIP runtime torch carries (one runtime in the process).  python _frontier_torch.py CASE"""
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

import frontier_ref as fr  # noqa: E402
import gvom  # noqa: E402

XY = 65
PARAMS = (0.4, 0.2, XY, 8, 1, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)


def case_consumer_stream():
    """a planner's choice on the GPU: the cheapest kept cluster, and how many cells the map gives it, on a side stream; the set is
    reused behind the consumer's reads"""
    g = gvom.Gvom(*PARAMS, voxel_statistics=False)
    name = "random_m2_cbig"
    c, vis, D, mc, _ = fr.patterns(XY)[name]
    cap = 256
    rows, sums, cmap, counts, _ = fr.product(c, vis, D, mc, cap)
    n = int(counts[0])
    assert 2 < n <= cap
    # the maps come from torch tensors: device addresses, cell (x, y) at [y * xy + x]
    tc, tv, td = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (c.view(np.int16), vis, D))
    torch.cuda.synchronize()                                   # (device inputs must be ready when the call is made)
    f = g.frontiers_of_device(tc.data_ptr(), tv.data_ptr(), td.data_ptr(), min_cells=mc, max_clusters=cap)
    ptr = f.clusters.ptr
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t_rows, t_sums, t_map, t_counts = (torch.from_dlpack(a) for a in (f.clusters, f.sums, f.cluster_map, f.counts))
        assert t_rows.dtype == torch.int32 and t_sums.dtype == torch.int64 and t_map.dtype == torch.int32 and t_counts.dtype == torch.int32
        assert tuple(t_rows.shape) == (cap, 8) and tuple(t_sums.shape) == (cap, 2) and tuple(t_counts.shape) == (4,)
        assert tuple(t_map.shape) == (XY, XY) and t_map.stride() == (1, XY) and t_map.data_ptr() == f.cluster_map.ptr
        kept = t_counts[0].clone()                             # (a view would hold the export)
        key = torch.where(torch.arange(cap, device="cuda") < kept, t_rows[:, 7].to(torch.int64), torch.full((cap,), 1 << 40, device="cuda"))
        pick = torch.argmin(key)
        cells_of_pick = (t_map == pick).sum()
        centroid = t_sums[pick].to(torch.float64) / t_rows[pick, 1]
        whole = t_map.clone()
        del t_rows, t_sums, t_map, t_counts                    # dropped at once: the releases are stream-ordered
    f.release()
    del f
    gc.collect()
    for _ in range(3):                                         # the next products reuse the set, behind the consumer's reads
        nxt = g.frontiers_of(np.ones((XY, XY), np.uint16), np.zeros((XY, XY), np.int32), max_clusters=cap)
        assert nxt.clusters.ptr == ptr and nxt.frontier_cells == 0
        nxt.release()
    assert g.get_tuning("device_product_sets") == 1
    side.synchronize()
    want = int(np.lexsort((np.arange(n), rows[:n, 7]))[0])
    assert int(pick) == want and int(cells_of_pick) == int(rows[want, 1])
    assert np.array_equal(centroid.cpu().numpy(), sums[want] / rows[want, 1])
    assert np.array_equal(whole.cpu().numpy().T, cmap)


if __name__ == "__main__":
    name = sys.argv[1]
    globals()["case_" + name]()
    print("CASE OK " + name)
