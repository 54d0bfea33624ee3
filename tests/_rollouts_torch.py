"""Child process of tests/test_rollouts.py: the case with a torch consumer.  torch is imported FIRST, so that libgvom_hip.so binds
to the HIP runtime torch carries (one runtime in the process).  python _rollouts_torch.py CASE"""
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
import rollouts_ref as rr  # noqa: E402

XY = 64
PARAMS = (rr.RES[XY], 0.2, XY, 8, 1, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)


def case_planner():
    """a sampling planner's tick: poses made by torch, scored in place, both parts taken through DLPack on a side stream, the
    cheapest rollout chosen there; the tensors dropped, the mapper reuses the set behind the consumer's reads"""
    g = gvom.Gvom(*PARAMS, voxel_statistics=False)
    res, oc = rr.RES[XY], rr.ORIGIN_CELLS[XY]
    origin = (oc[0] * res, oc[1] * res)
    table = gvom.rectangle_footprint(0.9, 0.4, 0.4, res, headings=16)
    g.set_footprint(table)
    c = rr.cost_map(XY, "random", seed=9, zeros=0.01)
    D = rr.field_of(c)
    K, T = 300, 24
    poses = rr.arc_poses(K, T, XY, res, oc, 31, spread=8.0, centre=(XY // 2, XY // 2))
    want_summary, want_cost, _ = rr.score(c, poses, table, res, oc, D)
    tc = torch.from_numpy(np.ascontiguousarray(np.asfortranarray(c).T).view(np.int16)).cuda()      # cell (x, y) at [y * xy + x]
    tD = torch.from_numpy(np.ascontiguousarray(np.asfortranarray(D).T)).cuda()
    tp = torch.from_numpy(poses).cuda()
    torch.cuda.synchronize()                                   # (device inputs must be ready when the call is made)
    r = g.score_rollouts_of_device(tc.data_ptr(), tp.data_ptr(), K, T, cost_to_go_ptr=tD.data_ptr(), origin=origin)
    ptr = r.summary.ptr
    assert r.summary.__dlpack_device__() == (10, 0)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        summary, cost = torch.from_dlpack(r.summary), torch.from_dlpack(r.pose_cost)
        assert summary.dtype == torch.int32 and tuple(summary.shape) == (K, 4) and summary.stride() == (4, 1) and summary.data_ptr() == ptr
        assert cost.dtype == torch.uint16 and tuple(cost.shape) == (K, T) and cost.stride() == (T, 1) and cost.data_ptr() == r.pose_cost.ptr
        clear = (summary[:, 0] == gvom.ROLLOUT_CLEAR) & (summary[:, 3] != gvom.CTG_UNREACHED)
        total = summary[:, 2].to(torch.int64) + summary[:, 3].to(torch.int64)
        best = torch.argmin(torch.where(clear, total, torch.full_like(total, 2 ** 62)))
        got_summary, got_cost = summary.clone(), cost.view(torch.int16).clone()
        del summary, cost, clear, total                        # dropped at once: the releases are stream-ordered
    r.release()
    del r
    gc.collect()
    for _ in range(3):                                         # every export came back: the next products reuse the set
        nxt = g.score_rollouts_of_device(tc.data_ptr(), tp.data_ptr(), K, T, origin=origin)
        assert nxt.summary.ptr == ptr
        nxt.release()
    assert g.get_tuning("device_product_sets") == 1 and g.get_tuning("rollout_allocations") == 1
    side.synchronize()
    assert np.array_equal(got_summary.cpu().numpy(), want_summary)
    assert np.array_equal(got_cost.cpu().numpy().view(np.uint16), want_cost)
    ok = (want_summary[:, 0] == rr.CLEAR) & (want_summary[:, 3] != rr.UNREACHED)
    assert ok.sum() >= 5 and (~ok).sum() >= 5
    want_total = np.where(ok, want_summary[:, 2].astype(np.int64) + want_summary[:, 3], 2 ** 62)
    assert int(best) == int(np.argmin(want_total)) and ok[int(best)]


if __name__ == "__main__":
    name = sys.argv[1]
    globals()["case_" + name]()
    print("CASE OK " + name)
