"""Child process of tests/test_attitude_volume.py: the case with a torch consumer.  torch is imported FIRST, so that libgvom_hip.so
binds to the HIP runtime torch carries (one runtime in the process).  python _attitude_volume_torch.py CASE"""
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
import attitude_volume_ref as av  # noqa: E402

XY = 64
RES = 0.4
PARAMS = (RES, 0.2, XY, 8, 1, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)


def case_consumer():
    """a planner's tick: the ground made by torch, the volume computed in place, status, tilt and counts taken through DLPack on a side
    stream, the share of drivable states per heading computed there; the tensors dropped, the mapper reuses the set behind the
    consumer's reads"""
    g = gvom.Gvom(*PARAMS, voxel_statistics=False)
    H = 16
    table = gvom.rectangle_footprint(0.9, 0.4, 0.4, RES, headings=H)
    g.set_footprint(table)
    ch = ar.make_chassis(0.7, -0.2, 0.7, 0.3, max_pitch=np.float32(0.25), max_roll=np.float32(0.25), min_clearance=np.float32(0.1))
    c = gvom.chassis(ch.front_axle, ch.rear_axle, ch.track, ch.belly_height)
    c.max_pitch, c.max_roll, c.min_clearance = ch.max_pitch, ch.max_roll, ch.min_clearance
    g.set_chassis(c)
    i, j = np.meshgrid(np.arange(XY, dtype=np.float64), np.arange(XY, dtype=np.float64), indexing="ij")
    ground = 0.6 * np.sin(i * 0.13) * np.cos(j * 0.11) + np.random.default_rng(9).uniform(0.0, 0.04, (XY, XY))
    ground[np.random.default_rng(10).random((XY, XY)) < 0.01] = np.nan
    want = av.volume(ground, table, ch, g.cos_sin, RES)
    tg = torch.from_numpy(np.ascontiguousarray(np.asfortranarray(ground).T)).cuda()                # cell (x, y) at [y * xy + x]
    torch.cuda.synchronize()                                   # (device inputs must be ready when the call is made)
    v = g.attitude_volume_of_device(tg.data_ptr())
    ptr = v.status.ptr
    assert v.__dlpack_device__() == (10, 0) and v.tilt.__dlpack_device__() == (10, 0)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        status, tilt, counts = torch.from_dlpack(v), torch.from_dlpack(v.tilt), torch.from_dlpack(v.counts)
        assert status.dtype == torch.uint8 and tuple(status.shape) == (H, XY, XY) and status.stride() == (XY * XY, 1, XY) and status.data_ptr() == ptr
        assert tilt.dtype == torch.uint8 and tuple(tilt.shape) == (H, XY, XY) and tilt.stride() == (XY * XY, 1, XY) and tilt.data_ptr() == v.tilt.ptr
        assert counts.dtype == torch.int32 and tuple(counts.shape) == (8,)
        drivable = (status == gvom.ATTITUDE_OK).sum(dim=(1, 2))
        got = status.clone(), tilt.clone(), counts.clone(), drivable.clone()
        del status, tilt, counts, drivable                     # dropped at once: the releases are stream-ordered
    v.release()
    del v
    gc.collect()
    for _ in range(3):                                         # every export came back: the next products reuse the set
        nxt = g.attitude_volume_of_device(tg.data_ptr())
        assert nxt.status.ptr == ptr
        nxt.release()
    assert g.get_tuning("device_product_sets") == 1 and g.get_tuning("attitude_volume_allocations") == 2      # the set and the table
    side.synchronize()
    for a, b in zip(got[:3], want):
        assert np.array_equal(a.cpu().numpy(), b)
    assert np.array_equal(got[3].cpu().numpy(), (want[0] == ar.OK).sum(axis=(1, 2)))
    assert (want[2][:6] > 0).sum() >= 4


if __name__ == "__main__":
    name = sys.argv[1]
    globals()["case_" + name]()
    print("CASE OK " + name)
