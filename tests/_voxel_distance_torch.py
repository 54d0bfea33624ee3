"""Child process of tests/test_voxel_distance.py: the case with a torch consumer.  torch is imported FIRST, so that libgvom_hip.so binds
to the HIP runtime torch carries (one runtime in the process).  python _voxel_distance_torch.py"""
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
import voxel_atlas_ref as va  # noqa: E402
import voxel_distance_ref as vd  # noqa: E402

RES = (va.DRIVE_RES[0], va.DRIVE_RES[2])


def case():
    g = gvom.Gvom(*(va.DRIVE_PARAMS + (1,) + va.DRIVE_TAIL), voxel_statistics=False)
    atlas = g.create_voxel_atlas(va.DRIVE_A, va.DRIVE_Z)
    pc, ego = va.drive_scans()[0]
    g.process_pointcloud(pc, ego)
    g.combine_maps()
    assert atlas.integrate()
    f = atlas.distance_field(2.0)
    dist, counts = f.copy_to_host()
    xy, zs = va.DRIVE_XY, va.DRIVE_ZS
    assert f.__dlpack_device__() == (10, 0)
    stream = torch.cuda.current_stream().cuda_stream
    for t in (torch.from_dlpack(f), torch.from_dlpack(f.distance), torch.from_dlpack(f.distance.__dlpack__(stream=stream))):   # the field hands over .distance
        assert t.device == torch.device("cuda:0") and t.dtype == torch.float32
        assert tuple(t.shape) == (xy, xy, zs) and t.stride() == (xy * zs, zs, 1) and t.data_ptr() == f.distance.ptr
        assert vd.same_bits(t.cpu().numpy(), dist)
        del t
    # the planner's questions: where does a sphere of this radius fit, and do these body spheres fit
    radius = 0.6
    free = torch.from_dlpack(f.distance) >= radius
    assert np.array_equal(free.cpu().numpy(), dist >= np.float32(radius)) and 0 < int(free.sum()) < dist.size
    rng = np.random.default_rng(2)
    pts = ((np.array(f.origin_voxels) + rng.uniform(-4, [xy + 4, xy + 4, zs + 4], (4096, 3))) * np.array([RES[0], RES[0], RES[1]])).astype(np.float32)
    centres = torch.from_numpy(pts).cuda()
    torch.cuda.synchronize()                                 # the points are torch's: uploaded before the mapper's stream reads them
    s = f.sample_device(centres.data_ptr(), len(pts))
    clear = torch.from_dlpack(s.distance) >= radius          # NaN (outside the field) compares false: not known to be clear
    want, want_counts = vd.gather(dist, f.origin_voxels, RES, pts)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(clear.cpu().numpy(), want >= np.float32(radius)) and 0 < int(clear.sum()) < len(pts)
    assert np.array_equal(torch.from_dlpack(s.counts).cpu().numpy(), want_counts) and want_counts[0] < len(pts)
    # release() of the atlas, and of the mapper's views, with the field still exported: the tensor stays valid
    held = torch.from_dlpack(f.distance)
    f.release()
    s.release()
    atlas.release()
    assert g.get_tuning("voxel_atlas") == 0
    torch.cuda.synchronize()
    assert vd.same_bits(held.cpu().numpy(), dist)
    atlas = g.create_voxel_atlas(va.DRIVE_A, va.DRIVE_Z)     # a new atlas, new fields: never in the exported set
    assert atlas.integrate()
    with atlas.distance_field(0.4, unknown_blocks=True) as other:
        assert other.distance.ptr != held.data_ptr()
        other.copy_to_host()
    assert vd.same_bits(held.cpu().numpy(), dist)
    del held, free, clear
    torch.cuda.synchronize()


if __name__ == "__main__":
    case()
    print("CASE OK")
