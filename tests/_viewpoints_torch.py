"""Child process of tests/test_viewpoints.py: the case with a torch consumer.  torch is imported FIRST, so that libgvom_hip.so binds
to the HIP runtime torch carries (one runtime in the process).  python _viewpoints_torch.py CASE"""
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
import viewpoint_ref as vr  # noqa: E402

GRID = "np2"


def case_consumer_stream():
    """an explorer's choice on the GPU: the pose with the largest gain per visit among those in free space, on a side stream; the
    poses come from a torch tensor, and the set is reused behind the consumer's reads"""
    g = rr.build_map(gvom.Gvom, GRID, 1, voxel_statistics=False)
    state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
    W = np.asarray(origin, np.float64)
    d, o = vr.model("m8x64")
    poses, r = vr.viewpoints_of(GRID, state, W, 33), vr.max_range_of(GRID, "third")
    want_rows, want_best = vr.product(state, W, GRID, d, o, poses, r)
    g.set_sensor_model(d, o)
    tp = torch.from_numpy(vr.rows34(poses)).cuda()
    torch.cuda.synchronize()                                   # (device inputs must be ready when the call is made)
    v = g.score_viewpoints_device(tp.data_ptr(), 33, r)
    ptr = v.rows.ptr
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert v.rows.__dlpack_device__() == (10, 0)
        t_rows, t_best = torch.from_dlpack(v.rows), torch.from_dlpack(v.best)
        assert t_rows.dtype == torch.int32 and t_best.dtype == torch.int32
        assert tuple(t_rows.shape) == (33, 8) and t_rows.stride() == (8, 1) and tuple(t_best.shape) == (4,) and t_rows.data_ptr() == ptr
        free = t_rows[:, 0] == gvom.RAY_CLEAR
        gain = torch.where(free, t_rows[:, 1], torch.full((33,), -1, dtype=torch.int32, device="cuda"))
        pick = torch.argmax(gain)
        total = t_rows[:, 1:].sum(dim=0, dtype=torch.int64)
        best = t_best.clone()                                  # (a view would hold the export)
        del t_rows, t_best, free                               # dropped at once: the releases are stream-ordered
    v.release()
    del v
    gc.collect()
    for _ in range(3):                                         # the next products reuse the set, behind the consumer's reads
        nxt = g.score_viewpoints(poses[::-1].copy(), r, unknown_blocks=True)
        assert nxt.rows.ptr == ptr
        nxt.release()
    assert g.get_tuning("device_product_sets") == 1
    side.synchronize()
    assert best.cpu().numpy().tolist() == want_best.tolist()
    assert int(gain[pick]) == int(want_best[1]) and int(want_best[0]) >= 0
    assert total.cpu().numpy().tolist() == want_rows[:, 1:].astype(np.int64).sum(axis=0).tolist()


if __name__ == "__main__":
    name = sys.argv[1]
    globals()["case_" + name]()
    print("CASE OK " + name)
