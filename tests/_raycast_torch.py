"""Child process of tests/test_raycast.py: the cases with a torch consumer.  torch is imported FIRST, so that libgvom_hip.so
binds to the HIP runtime torch carries (one runtime in the process).  python _raycast_torch.py CASE"""
import os
import sys

import torch

torch.cuda.init()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "g-vom_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import gc  # noqa: E402

import numpy as np  # noqa: E402

import gvom  # noqa: E402
import raycast_ref as rr  # noqa: E402

GRID = "np2"


def _map():
    g = rr.build_map(gvom.Gvom, GRID, 1, voxel_statistics=False)
    state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
    W = np.asarray(origin, np.float64)
    A, B, fam = rr.rays_of(GRID, state, W)
    return g, state, W, A, B


def _same(t, want):
    got = t.cpu().numpy()
    return np.array_equal(got.view(np.uint32), want.view(np.uint32))


def case_zero_copy():
    """both parts through torch.from_dlpack, versioned and legacy capsule, in place; the segments come from torch tensors"""
    g, state, W, A, B = _map()
    want = rr.walk(state, W, GRID, A, B, unknown_blocks=True, check_target=True)
    ta, tb = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    torch.cuda.synchronize()                                   # (device inputs must be ready when the call is made)
    rays = g.raycast_device(ta.data_ptr(), rr.N_RAYS, tb.data_ptr(), rr.N_RAYS, unknown_blocks=True, check_target=True)
    stream = torch.cuda.current_stream().cuda_stream
    for a, w, dtype, cols in ((rays.result, want[0], torch.int32, 4), (rays.position, want[1], torch.float32, 3)):
        assert a.__dlpack_device__() == (10, 0)
        for t in (torch.from_dlpack(a), torch.from_dlpack(a.__dlpack__(stream=stream))):
            assert t.device == torch.device("cuda:0") and t.dtype == dtype
            assert tuple(t.shape) == (rr.N_RAYS, cols) and t.stride() == (cols, 1) and t.data_ptr() == a.ptr
            assert _same(t, w)
            del t
    # the planner's question: which segments are free, and how far do the others get
    res = torch.from_dlpack(rays.result)
    free = res[:, 0] == gvom.RAY_CLEAR
    assert int(free.sum()) == int((want[0][:, 0] == rr.CLEAR).sum()) > 0
    assert int(res[~free, 1].sum()) == int(want[0][want[0][:, 0] != rr.CLEAR, 1].sum())
    del res, free
    torch.cuda.synchronize()
    rays.release()
    g.raycast_device(ta.data_ptr(), rr.N_RAYS, tb.data_ptr(), rr.N_RAYS).release()      # every export came back: the set is reused
    assert g.get_tuning("device_product_sets") == 1 and g.get_tuning("raycast_allocations") == 1


def case_consumer_stream():
    """a consumer on a stream of its own; the product's set is reused behind its reads"""
    g, state, W, A, B = _map()
    want = rr.walk(state, W, GRID, A, B)
    rays = g.raycast(A, B)
    ptr = rays.result.ptr
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        r, p = torch.from_dlpack(rays.result), torch.from_dlpack(rays.position)
        counts = torch.bincount(r[:, 0], minlength=5)
        steps = r[:, 1].sum(dtype=torch.int64)
        reach = torch.nan_to_num(p, nan=0.0).sum(dim=0, dtype=torch.float64)
        del r, p                                               # dropped at once: the releases are stream-ordered
    rays.release()
    del rays
    gc.collect()
    for _ in range(3):                                         # the next products reuse the set, behind the consumer's reads
        nxt = g.raycast(A[::-1].copy(), B[::-1].copy(), unknown_blocks=True)
        assert nxt.result.ptr == ptr
        nxt.release()
    assert g.get_tuning("device_product_sets") == 1
    side.synchronize()
    assert counts.cpu().numpy().tolist() == np.bincount(want[0][:, 0], minlength=5).tolist()
    assert int(steps) == int(want[0][:, 1].astype(np.int64).sum())
    ref = np.nan_to_num(want[1].astype(np.float64), nan=0.0).sum(axis=0)
    assert np.allclose(reach.cpu().numpy(), ref, rtol=1e-9, atol=1e-6)


if __name__ == "__main__":
    name = sys.argv[1]
    globals()["case_" + name]()
    print("CASE OK " + name)
