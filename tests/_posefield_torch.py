"""Child process of tests/test_posefield.py: a torch consumer of a pose field.  torch is imported FIRST, so that libgvom_hip.so binds
to the HIP runtime torch carries (one runtime in the process).  python _posefield_torch.py"""
import os
import sys

import torch

torch.cuda.init()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "g-vom_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np  # noqa: E402

import gvom  # noqa: E402
import posefield_ref as ref  # noqa: E402
import rollouts_ref  # noqa: E402


def case_terminal_costs():
    """a sampling planner's terminal cost: the field gathered at the last poses of a batch of rollouts through gvom.pose_states"""
    i = [k for k, q in enumerate(ref.cases()) if q["name"] == "xy40 H16 car arcs random"][0]
    q = ref.cases()[i]
    xy, H, res = q["xy"], q["H"], ref.CAR_RES
    origin = (-7.5, 3.0)                                        # the window corner in world metres, a multiple of the resolution
    oc = (int(round(origin[0] / res)), int(round(origin[1] / res)))
    g = gvom.Gvom(res, 0.2, xy, 8, 1, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1, voxel_statistics=False)
    g.set_footprint(q["footprint"])
    g.set_primitives(q["table"])
    f = g.pose_field_of(q["c"], ref.goals_for_binding(q["goals"], H), origin=origin)
    C, D, A, _, info = ref.expected(i)
    assert f.converged and (f.reached, f.goals_seeded) == info
    stream = torch.cuda.current_stream().cuda_stream
    for a, want, dtype in ((f.cost, D, torch.int32), (f.action, A, torch.uint8)):
        assert a.__dlpack_device__() == (10, 0)
        for t in (torch.from_dlpack(a), torch.from_dlpack(a.__dlpack__(stream=stream))):           # versioned, legacy capsule
            assert t.device == torch.device("cuda:0") and t.dtype == dtype
            assert tuple(t.shape) == (H, xy, xy) and t.stride() == (xy * xy, 1, xy) and t.data_ptr() == a.ptr
            assert np.array_equal(t.cpu().numpy(), want)                                           # [h, x, y] indexing, exact
            del t
    poses = rollouts_ref.arc_poses(300, 12, xy, res, oc, seed=11)
    last = poses[:, -1]
    states, valid = gvom.pose_states(last, origin, res, H)
    inside = valid & (states[:, 0] >= 0) & (states[:, 0] < xy) & (states[:, 1] >= 0) & (states[:, 1] < xy)
    assert 50 < inside.sum() < len(last)
    cost = torch.from_dlpack(f.cost)
    s = torch.from_numpy(states[inside].astype(np.int64)).cuda()
    terminal = cost[s[:, 2], s[:, 0], s[:, 1]].cpu().numpy()
    cx, cy, h, _ = rollouts_ref.pose_frame(last, res, oc, H)
    assert np.array_equal(terminal, D[h[inside], cx[inside], cy[inside]])
    assert (terminal < ref.UNREACHED).any() and (terminal == ref.UNREACHED).any()
    del cost
    torch.cuda.synchronize()
    ptr = f.cost.ptr
    f.release()
    nxt = g.pose_field_of(q["c"], ref.goals_for_binding(q["goals"], H))      # every export came back: the set is reused
    assert nxt.cost.ptr == ptr and g.get_tuning("device_product_sets") == 1
    nxt.release()


if __name__ == "__main__":
    case_terminal_costs()
    print("CASE OK terminal_costs")
