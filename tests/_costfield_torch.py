"""Child process of tests/test_costfield.py: the cases with a torch consumer.  torch is imported FIRST, so that libgvom_hip.so
binds to the HIP runtime torch carries (one runtime in the process).  python _costfield_torch.py CASE"""
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

import costfield_ref as cf  # noqa: E402
import gvom  # noqa: E402

XY = 50
PARAMS = (0.4, 0.2, XY, 8, 1, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)


def _inputs():
    c, goals, _ = cf.patterns(XY)["random"]
    D, d, _ = cf.expected(XY, "random")
    return c, goals, D, d


def case_zero_copy():
    g = gvom.Gvom(*PARAMS, voxel_statistics=False)
    c, goals, D, d = _inputs()
    # the cost map comes from a torch tensor: graded costs are the caller's to build on the GPU
    tc = torch.from_numpy(np.ascontiguousarray(np.asfortranarray(c).T)).cuda()         # cell (x, y) at [y * xy + x]
    torch.cuda.synchronize()                                   # (device inputs must be ready when the call is made)
    f = g.cost_to_go_of_device(tc.data_ptr(), goals)
    assert f.converged and f.reached == int((D != cf.UNREACHED).sum())
    stream = torch.cuda.current_stream().cuda_stream
    for a, want, dtype in ((f.cost, D, torch.int32), (f.direction, d, torch.uint8)):
        assert a.__dlpack_device__() == (10, 0)
        for t in (torch.from_dlpack(a), torch.from_dlpack(a.__dlpack__(stream=stream))):           # versioned, legacy capsule
            assert t.device == torch.device("cuda:0") and t.dtype == dtype
            assert tuple(t.shape) == (XY, XY) and t.stride() == (1, XY) and t.data_ptr() == a.ptr
            assert np.array_equal(t.cpu().numpy(), want)                                           # [x, y] indexing, exact
            del t
    # a sampling planner's terminal cost: the field at a batch of cells
    cost = torch.from_dlpack(f.cost)
    xs = torch.tensor([3, 17, 49, 0], device="cuda")
    ys = torch.tensor([4, 30, 0, 49], device="cuda")
    assert cost[xs, ys].cpu().tolist() == [int(D[3, 4]), int(D[17, 30]), int(D[49, 0]), int(D[0, 49])]
    del cost
    torch.cuda.synchronize()
    f.release()
    g.cost_to_go_of_device(tc.data_ptr(), goals).release()       # every export came back: the set is reused
    assert g.get_tuning("device_product_sets") == 1 and g.get_tuning("cost_to_go_allocations") == 2


def case_consumer_stream():
    g = gvom.Gvom(*PARAMS, voxel_statistics=False)
    c, goals, D, d = _inputs()
    f = g.cost_to_go_of(c, goals)
    ptr = f.cost.ptr
    reached = np.argwhere(D != cf.UNREACHED)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t, u = torch.from_dlpack(f.cost), torch.from_dlpack(f.direction)
        idx = torch.from_numpy(reached).cuda()
        steps = u[idx[:, 0], idx[:, 1]]                        # one gather: the first step from every reached cell
        total = torch.where(t == cf.UNREACHED, torch.zeros_like(t), t).sum(dtype=torch.int64)
        del t, u                                               # dropped at once: the releases are stream-ordered
    f.release()
    del f
    gc.collect()
    other = np.ascontiguousarray(c[::-1])                      # the next products reuse the set, behind the consumer's reads
    flipped = np.array([(XY - 1 - goals[0][0], goals[0][1])], np.int32)
    for _ in range(3):
        nxt = g.cost_to_go_of(other, flipped)
        assert nxt.cost.ptr == ptr
        nxt.release()
    assert g.get_tuning("device_product_sets") == 1
    side.synchronize()
    assert np.array_equal(steps.cpu().numpy(), d[reached[:, 0], reached[:, 1]])
    assert int(total) == int(D[D != cf.UNREACHED].astype(np.int64).sum())
    with g.cost_to_go_of(other, flipped) as last:
        got = last.copy_to_host()[0]
    assert np.array_equal(got, D[::-1]) and not np.array_equal(got, D)


if __name__ == "__main__":
    name = sys.argv[1]
    globals()["case_" + name]()
    print("CASE OK " + name)
