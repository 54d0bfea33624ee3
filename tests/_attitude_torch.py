"""Child process of tests/test_attitude.py: the case with a torch consumer.  torch is imported FIRST, so that libgvom_hip.so binds
to the HIP runtime torch carries (one runtime in the process).  python _attitude_torch.py CASE"""
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
import attitude_ref as ar  # noqa: E402
import rollouts_ref as rr  # noqa: E402

XY = 64
PARAMS = (rr.RES[XY], 0.2, XY, 8, 1, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)


def case_planner():
    """a sampling planner's tick: ground and poses made by torch, scored in place, all three parts taken through DLPack on a side
    stream, the flattest fully traversable rollout chosen there; the tensors dropped, the mapper reuses the set behind the
    consumer's reads"""
    g = gvom.Gvom(*PARAMS, voxel_statistics=False)
    res, oc = rr.RES[XY], rr.ORIGIN_CELLS[XY]
    origin = (oc[0] * res, oc[1] * res)
    table = gvom.rectangle_footprint(0.9, 0.4, 0.4, res, headings=16)
    g.set_footprint(table)
    ch = ar.make_chassis(0.7, -0.2, 0.7, 0.3, max_pitch=np.float32(0.25), max_roll=np.float32(0.25), min_clearance=np.float32(0.1))
    c = gvom.chassis(ch.front_axle, ch.rear_axle, ch.track, ch.belly_height)
    c.max_pitch, c.max_roll, c.min_clearance = ch.max_pitch, ch.max_roll, ch.min_clearance
    g.set_chassis(c)
    i, j = np.meshgrid(np.arange(XY, dtype=np.float64), np.arange(XY, dtype=np.float64), indexing="ij")
    ground = 0.6 * np.sin(i * 0.13) * np.cos(j * 0.11) + np.random.default_rng(9).uniform(0.0, 0.04, (XY, XY))
    ground[np.random.default_rng(10).random((XY, XY)) < 0.01] = np.nan
    K, T = 300, 24
    poses = rr.arc_poses(K, T, XY, res, oc, 31, spread=8.0, centre=(XY // 2, XY // 2))
    want = ar.score(ground, poses, table, ch, g.cos_sin, res, oc)
    tg = torch.from_numpy(np.ascontiguousarray(np.asfortranarray(ground).T)).cuda()                # cell (x, y) at [y * xy + x]
    tp = torch.from_numpy(poses).cuda()
    torch.cuda.synchronize()                                   # (device inputs must be ready when the call is made)
    r = g.score_attitude_of_device(tg.data_ptr(), tp.data_ptr(), K, T, origin=origin)
    ptr = r.summary.ptr
    assert r.attitude.__dlpack_device__() == (10, 0)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        summary, att, status = torch.from_dlpack(r.summary), torch.from_dlpack(r.attitude), torch.from_dlpack(r.status)
        assert summary.dtype == torch.int32 and tuple(summary.shape) == (K, 5) and summary.stride() == (5, 1) and summary.data_ptr() == ptr
        assert att.dtype == torch.float32 and tuple(att.shape) == (K, T, 3) and att.stride() == (3 * T, 3, 1) and att.data_ptr() == r.attitude.ptr
        assert status.dtype == torch.uint8 and tuple(status.shape) == (K, T) and status.stride() == (T, 1) and status.data_ptr() == r.status.ptr
        through = summary[:, 0] == gvom.ATTITUDE_OK
        worst = att[..., :2].abs().amax(dim=(1, 2))
        best = torch.argmin(torch.where(through, worst, torch.full_like(worst, float("inf"))))
        got = summary.clone(), att.clone(), status.clone()
        del summary, att, status, through, worst               # dropped at once: the releases are stream-ordered
    r.release()
    del r
    gc.collect()
    for _ in range(3):                                         # every export came back: the next products reuse the set
        nxt = g.score_attitude_of_device(tg.data_ptr(), tp.data_ptr(), K, T, origin=origin)
        assert nxt.summary.ptr == ptr
        nxt.release()
    assert g.get_tuning("device_product_sets") == 1 and g.get_tuning("attitude_allocations") == 1
    side.synchronize()
    for a, b in zip(got, want):
        assert np.array_equal(a.cpu().numpy(), b)
    ok = want[0][:, 0] == ar.OK
    assert ok.sum() >= 5 and (~ok).sum() >= 5
    want_worst = np.where(ok, np.abs(want[1][..., :2]).max(axis=(1, 2)), np.inf)
    assert int(best) == int(np.argmin(want_worst)) and ok[int(best)]


if __name__ == "__main__":
    name = sys.argv[1]
    globals()["case_" + name]()
    print("CASE OK " + name)
