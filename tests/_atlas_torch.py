"""Child process of tests/test_atlas.py: the case with a torch consumer.  torch is imported FIRST, so that libgvom_hip.so binds to the
HIP runtime torch carries (one runtime in the process).  python _atlas_torch.py CASE"""
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

import atlas_ref as ar  # noqa: E402
import gvom  # noqa: E402

XY, A = 33, 64
PARAMS = (0.4, 0.2, XY, 8, 1, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)


def case_consumer_stream():
    """a planner on the GPU: how much of a remembered window is observed, and how old what it knows is, on a side stream; the sets
    come from torch tensors, and the recalled set is reused behind the consumer's reads"""
    g = gvom.Gvom(*PARAMS, voxel_statistics=False)
    a = g.create_atlas(A)
    ref = ar.AtlasRef(A, XY)
    origins, sets = ar.walk(XY, A), ar.scenario_sets(XY, A)
    for k in range(3):
        # [y][x] maps as torch tensors: device addresses, cell (x, y) at [y * xy + x]; the f64 maps travel as their bit patterns
        held = [torch.from_numpy(np.ascontiguousarray(m if m.dtype == np.int32 else m.view(np.int64))).cuda() for m in sets[k]]
        torch.cuda.synchronize()                               # (device inputs must be ready when the call is made)
        a.integrate_of_device([t.data_ptr() for t in held], origins[k])
        ref.integrate(sets[k], origins[k])
        assert a.counts() == ref.counts()                      # (waits: the tensors may go)
    want, stamp, counts = ref.recall(origins[0])
    m = a.recall(origin_cells=origins[0])
    ptr, sptr = m.visibility.ptr, m.stamps.ptr
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t_vis, t_h, t_stamp, t_counts = (torch.from_dlpack(x) for x in (m.visibility, m.height_map, m.stamps, m.recall_counts))
        assert t_vis.dtype == torch.int32 and t_h.dtype == torch.float64 and t_stamp.dtype == torch.int32 and t_counts.dtype == torch.int32
        assert tuple(t_vis.shape) == (XY, XY) and t_vis.stride() == (1, XY) and t_vis.data_ptr() == ptr
        assert tuple(t_stamp.shape) == (XY, XY) and t_stamp.stride() == (1, XY) and t_stamp.data_ptr() == sptr and tuple(t_counts.shape) == (4,)
        observed = (t_vis > 0).sum()
        newest = torch.where(t_vis > 0, t_stamp, torch.zeros_like(t_stamp)).max()
        bits_h = t_h.view(torch.int64).clone()
        whole, tally = t_stamp.clone(), t_counts.clone()
        del t_vis, t_h, t_stamp, t_counts                      # dropped at once: the releases are stream-ordered
    m.stamps.release()
    m.release()
    del m
    gc.collect()
    for _ in range(3):                                         # the next recalls reuse the sets, behind the consumer's reads
        nxt = a.recall(origin_cells=(10 ** 6, 0))              # far outside: every cell UNKNOWN
        assert nxt.visibility.ptr == ptr and nxt.stamps.ptr == sptr
        nxt.stamps.release()
        nxt.release()
    assert g.get_tuning("device_map_sets") == 1
    side.synchronize()
    assert int(observed) == int(counts[0]) == int((want[2] > 0).sum())
    assert int(newest) == int(np.where(want[2] > 0, stamp, 0).max()) >= 1
    assert np.array_equal(bits_h.cpu().numpy().T, want[4]) and np.array_equal(whole.cpu().numpy().T, stamp)
    assert np.array_equal(tally.cpu().numpy(), counts)


if __name__ == "__main__":
    name = sys.argv[1]
    globals()["case_" + name]()
    print("CASE OK " + name)
