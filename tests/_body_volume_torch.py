"""Child process of tests/test_body_volume.py: the case with a torch consumer.  torch is imported FIRST, so that libgvom_hip.so binds to
the HIP runtime torch carries (one runtime in the process).  python _body_volume_torch.py CASE"""
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
import body_volume_ref as bv  # noqa: E402

TAIL = (1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)              # the mapper's other parameters (nothing here scans)


def case_consumer():
    """a planner's tick: field and ground made by torch, the volume computed in place, status, squeeze, clearance and counts taken through
    DLPack on a side stream (the product itself hands out `.status`), the share of passable states per heading computed there; the
    tensors dropped, the mapper reuses the set behind the consumer's reads"""
    q, want = bv.cases()[1], bv.expected()[1]                  # 33 cells, 7 headings, 64 spheres
    xy, H = q["xy"], len(q["cos_sin"])
    res, zres, zs, _, _ = bv.GRIDS[xy]
    g = gvom.Gvom(res, zres, xy, zs, 1, *TAIL, voxel_statistics=False)
    g.set_footprint(q["table"])
    g.set_chassis(gvom.chassis(*q["chassis"][:4]))
    g.set_body(q["body"])
    tf = torch.from_numpy(q["field"]).cuda()
    tg = torch.from_numpy(np.ascontiguousarray(np.asfortranarray(q["g"]).T)).cuda()                # cell (x, y) at [y * xy + x]
    torch.cuda.synchronize()                                   # (device inputs must be ready when the call is made)
    call = lambda: g.body_volume_of_device(tf.data_ptr(), np.array(q["field_origin"]), tg.data_ptr(), origin=q["origin"],
                                           min_margin=q["min_margin"], soft_margin=q["soft_margin"])
    v = call()
    ptr = v.status.ptr
    assert v.__dlpack_device__() == (10, 0) and v.clearance.__dlpack_device__() == (10, 0)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        status, squeeze, clr, counts = torch.from_dlpack(v), torch.from_dlpack(v.squeeze), torch.from_dlpack(v.clearance), torch.from_dlpack(v.counts)
        for t, dt, part in ((status, torch.uint8, v.status), (squeeze, torch.uint8, v.squeeze), (clr, torch.float32, v.clearance)):
            assert t.dtype == dt and tuple(t.shape) == (H, xy, xy) and t.stride() == (xy * xy, 1, xy) and t.data_ptr() == part.ptr
        assert status.data_ptr() == ptr and counts.dtype == torch.int32 and tuple(counts.shape) == (8,)
        passable = (status == gvom.BODY_OK).sum(dim=(1, 2))
        got = status.clone(), squeeze.clone(), clr.clone(), counts.clone(), passable.clone()
        del t, status, squeeze, clr, counts, passable          # dropped at once: the releases are stream-ordered
    v.release()
    del v
    gc.collect()
    allocs = g.get_tuning("body_volume_allocations")
    for _ in range(3):                                         # every export came back: the next products reuse the set
        nxt = call()
        assert nxt.status.ptr == ptr
        nxt.release()
    assert g.get_tuning("device_product_sets") == 1 and g.get_tuning("body_volume_allocations") == allocs == 1   # the product set
    side.synchronize()
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1]) and np.array_equal(got[3].cpu().numpy(), want[3])
    assert np.array_equal(np.ascontiguousarray(got[2].cpu().numpy()).view(np.uint32), np.ascontiguousarray(want[2]).view(np.uint32))
    assert np.array_equal(got[4].cpu().numpy(), (want[0] == bv.OK).sum(axis=(1, 2))) and (want[3][:3] > 0).all()


if __name__ == "__main__":
    name = sys.argv[1]
    globals()["case_" + name]()
    print("CASE OK " + name)
