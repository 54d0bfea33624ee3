"""Child process of tests/test_align.py: the case with a torch consumer.  torch is imported FIRST, so that libgvom_hip.so binds to
the HIP runtime torch carries (one runtime in the process).  python _align_torch.py CASE"""
import os
import sys

import torch

torch.cuda.init()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "g-vom_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np  # noqa: E402

import gvom  # noqa: E402
import align_ref as ar  # noqa: E402
import raycast_ref as rr  # noqa: E402

GRID = "np2"


def case_argmax():
    """part 0 through torch.from_dlpack, in place; the cloud and the candidates come from torch tensors; argmax of the score column
    is part 1's best index, and the counts are the referee's"""
    g = rr.build_map(gvom.Gvom, GRID, 1, voxel_statistics=False)
    state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
    W = np.asarray(origin, np.float64)
    cloud, M = ar.cloud_of(GRID), ar.candidates(GRID)
    want = ar.score(state, W, GRID, cloud, M, 1)
    tc, tm = torch.from_numpy(cloud).cuda(), torch.from_numpy(np.ascontiguousarray(M[:, :3, :])).cuda()
    torch.cuda.synchronize()                                   # (device inputs must be ready when the call is made)
    r = g.score_alignments_device(tc.data_ptr(), len(cloud), tm.data_ptr(), len(M), dilate=1)
    assert r.counts.__dlpack_device__() == (10, 0)
    stream = torch.cuda.current_stream().cuda_stream
    for t in (torch.from_dlpack(r.counts), torch.from_dlpack(r.counts.__dlpack__(stream=stream))):
        assert t.device == torch.device("cuda:0") and t.dtype == torch.int32
        assert tuple(t.shape) == (len(M), 6) and t.stride() == (6, 1) and t.data_ptr() == r.counts.ptr
        assert np.array_equal(t.cpu().numpy(), want[0])
        del t
    counts, best = torch.from_dlpack(r.counts), torch.from_dlpack(r.best)
    assert tuple(best.shape) == (4,) and best.dtype == torch.int32
    k = int(torch.argmax(counts[:, 0]))                        # (torch's argmax returns the first of the maxima on this build: checked below)
    assert counts[k, 0] == counts[:, 0].max() == best[1]
    first = int(torch.nonzero(counts[:, 0] == counts[:, 0].max())[0])
    assert first == int(best[0]) == int(want[1][0]) == ar.CENTRE and k in (first, ar.N_GRID)
    assert best.cpu().numpy().tolist() == want[1].tolist()
    assert int(counts[:, 1:].sum()) == len(M) * len(cloud)
    del counts, best
    torch.cuda.synchronize()
    r.release()
    g.score_alignments_device(tc.data_ptr(), len(cloud), tm.data_ptr(), len(M)).release()      # every export came back: the set is reused
    assert g.get_tuning("device_product_sets") == 1 and g.get_tuning("alignment_allocations") == 2


if __name__ == "__main__":
    name = sys.argv[1]
    globals()["case_" + name]()
    print("CASE OK " + name)
