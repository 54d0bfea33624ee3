"""Child process of tests/test_clearance.py: the cases with a torch consumer.  torch is imported FIRST, so that libgvom_hip.so
binds to the HIP runtime torch carries (one runtime in the process).  python _clearance_torch.py CASE"""
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

import clearance_ref as cr  # noqa: E402
import gvom  # noqa: E402

XY, RES = 50, 0.4
PARAMS = (RES, 0.2, XY, 8, 1, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)


def _inputs():
    pos = cr.patterns(XY)["random_1"][0]
    d2 = cr.separable(cr.obstacle_mask(pos, None, 50))
    return pos, d2, cr.distance(d2, RES)


def case_zero_copy():
    g = gvom.Gvom(*PARAMS, voxel_statistics=False)
    pos, d2, dist = _inputs()
    c = g.clearance_of(pos)
    stream = torch.cuda.current_stream().cuda_stream
    for a, want, dtype in ((c.distance, dist, torch.float32), (c.squared_cells, d2, torch.int32)):
        assert a.__dlpack_device__() == (10, 0)
        for t in (torch.from_dlpack(a), torch.from_dlpack(a.__dlpack__(stream=stream))):           # versioned, legacy capsule
            assert t.device == torch.device("cuda:0") and t.dtype == dtype
            assert tuple(t.shape) == (XY, XY) and t.stride() == (1, XY) and t.data_ptr() == a.ptr
            got = t.cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))                       # [x, y] indexing, bit for bit
            del t
    # the planner's first question: which cells can the robot's centre not enter
    radius = 1.0
    blocked = torch.from_dlpack(c.distance) < radius
    assert np.array_equal(blocked.cpu().numpy(), dist < np.float32(radius)) and 0 < int(blocked.sum()) < XY * XY
    del blocked
    torch.cuda.synchronize()
    c.release()
    g.clearance_of(pos).release()                              # every export came back: the set is reused
    assert g.get_tuning("device_product_sets") == 1 and g.get_tuning("device_map_sets") == 0


def case_consumer_stream():
    g = gvom.Gvom(*PARAMS, voxel_statistics=False)
    pos, d2, dist = _inputs()
    c = g.clearance_of(pos)
    ptr = c.distance.ptr
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t, u = torch.from_dlpack(c.distance), torch.from_dlpack(c.squared_cells)
        nearest = torch.where(torch.isinf(t), torch.zeros_like(t), t).sum(dtype=torch.float64)
        total = u.sum(dtype=torch.int64)
        rows = u.min(dim=0).values                             # per y: the smallest squared distance of the row
        del t, u                                               # dropped at once: the releases are stream-ordered
    c.release()
    del c
    gc.collect()
    other = np.ascontiguousarray(pos[::-1])                    # the next products reuse the set, behind the consumer's reads
    for _ in range(3):
        nxt = g.clearance_of(other)
        assert nxt.distance.ptr == ptr
        nxt.release()
    assert g.get_tuning("device_product_sets") == 1
    side.synchronize()
    assert int(total) == int(d2.astype(np.int64).sum())
    assert np.array_equal(rows.cpu().numpy(), d2.min(axis=0))
    assert abs(float(nearest) - float(dist.astype(np.float64).sum())) < 1e-6 * float(dist.sum())
    with g.clearance_of(other) as last:
        got = last.copy_to_host()[1]
    assert np.array_equal(got, d2[::-1]) and not np.array_equal(got, d2)


if __name__ == "__main__":
    name = sys.argv[1]
    globals()["case_" + name]()
    print("CASE OK " + name)
