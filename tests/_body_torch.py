"""Child process of tests/test_body.py: the case with a torch consumer.  torch is imported FIRST, so that libgvom_hip.so binds to the
HIP runtime torch carries (one runtime in the process).  python _body_torch.py CASE"""
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
import body_ref as br  # noqa: E402

XY = 33
TAIL = (1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)              # the mapper's other parameters (nothing here scans)


def case_planner():
    """a sampling planner's tick: field, ground and poses made by torch, scored in place, the clearance taken through DLPack on a side
    stream (the product itself and its `.clearance`), the rollout with the widest least clearance chosen there; the tensors dropped, the
    mapper reuses the set behind the consumer's reads"""
    res, zres, zs, oc, _ = br.GRIDS[XY]
    g = gvom.Gvom(res, zres, XY, zs, 1, *TAIL, voxel_statistics=False)
    K, T = 40, 24
    q = br._case("planner", XY, "plane", 7, 12, K, T, seed=5, device=True, min_margin=-0.05, poses=br._hover_poses(XY, K, T, 9))
    want = br.score_case(q)
    g.set_footprint(q["table"])
    g.set_chassis(gvom.chassis(*q["chassis"][:4]))
    g.set_body(q["body"])
    tf = torch.from_numpy(q["field"]).cuda()
    tg = torch.from_numpy(np.ascontiguousarray(np.asfortranarray(q["g"]).T)).cuda()                # cell (x, y) at [y * xy + x]
    tp = torch.from_numpy(q["poses"]).cuda()
    torch.cuda.synchronize()                                   # (device inputs must be ready when the call is made)
    call = lambda: g.score_body_of_device(tf.data_ptr(), np.array(q["field_origin"]), tg.data_ptr(), tp.data_ptr(), K, T, origin=q["origin"],
                                          min_margin=q["min_margin"])
    r = call()
    ptr = r.summary.ptr
    assert r.__dlpack_device__() == (10, 0) and r.clearance.__dlpack_device__() == (10, 0)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        clr, summary, status = torch.from_dlpack(r), torch.from_dlpack(r.summary), torch.from_dlpack(r.status)
        assert clr.dtype == torch.float32 and tuple(clr.shape) == (K, T) and clr.stride() == (T, 1) and clr.data_ptr() == r.clearance.ptr
        assert summary.dtype == torch.int32 and tuple(summary.shape) == (K, 4) and summary.data_ptr() == ptr
        assert status.dtype == torch.uint8 and tuple(status.shape) == (K, T, 2) and status.stride() == (2 * T, 2, 1)
        through = summary[:, 0] == gvom.BODY_OK
        least = clr.amin(dim=1)
        best = torch.argmax(torch.where(through, least, torch.full_like(least, float("-inf"))))
        got = summary.clone(), clr.clone(), status.clone()
        del clr, summary, status, through, least               # dropped at once: the releases are stream-ordered
    r.release()
    del r
    gc.collect()
    allocs = g.get_tuning("body_allocations")
    for _ in range(3):                                         # every export came back: the next products reuse the set
        nxt = call()
        assert nxt.summary.ptr == ptr
        nxt.release()
    assert g.get_tuning("device_product_sets") == 1 and g.get_tuning("body_allocations") == allocs == 2   # the table and the product set
    side.synchronize()
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[2].cpu().numpy(), want[2])
    assert np.array_equal(got[1].cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    ok = want[0][:, 0] == br.OK
    assert ok.sum() >= 3 and (~ok).sum() >= 3, np.bincount(want[0][:, 0])
    want_least = np.where(ok, want[1].min(axis=1), -np.inf)
    assert int(best) == int(np.argmax(want_least)) and ok[int(best)]


if __name__ == "__main__":
    name = sys.argv[1]
    globals()["case_" + name]()
    print("CASE OK " + name)
