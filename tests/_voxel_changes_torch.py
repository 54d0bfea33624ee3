"""Child process of tests/test_voxel_changes.py: the case with a torch consumer.  torch is imported FIRST, so that libgvom_hip.so binds to
the HIP runtime torch carries (one runtime in the process).  python _voxel_changes_torch.py CASE"""
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
import voxel_atlas_ref as va  # noqa: E402
import voxel_changes_ref as vc  # noqa: E402


def case_consumer():
    """the hand-placed scene; the codes, the column counts and the cluster map taken through DLPack on a side stream (the product itself
    hands out `.codes`), the changed voxels per column summed there; the tensors dropped, the mapper reuses the set behind the
    consumer's reads"""
    g = gvom.Gvom(*vc.scene_params(), voxel_statistics=False)
    atlas = g.create_voxel_atlas(va.DRIVE_A, va.DRIVE_Z)
    ref = va.VoxelAtlasRef(va.DRIVE_A, va.DRIVE_Z, va.DRIVE_XY, va.DRIVE_ZS)

    def dense(m):
        state, _, _, _, origin, _ = m.read_dense(gvom.GVOM_WHICH_FUSED)
        return state, tuple(int(v) for v in origin)

    def between(state, W):
        atlas.integrate()
        ref.integrate(state, W)
    state, W = vc.run_scene(g, dense, between)
    want, _ = vc.product(ref, state, W, 3, 2, 1024)
    xy, zs = va.DRIVE_XY, va.DRIVE_ZS
    ch = atlas.changes()
    ptr = ch.codes.ptr
    assert ch.__dlpack_device__() == (10, 0)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        codes, cols, cmap = torch.from_dlpack(ch), torch.from_dlpack(ch.column_counts), torch.from_dlpack(ch.cluster_map)
        assert codes.dtype == torch.uint8 and tuple(codes.shape) == (xy, xy, zs) and codes.stride() == (xy * zs, zs, 1) and codes.data_ptr() == ptr
        assert cols.dtype == torch.uint16 and tuple(cols.shape) == (2, xy, xy) and cols.stride() == (xy * xy, 1, xy)
        assert cmap.dtype == torch.int32 and tuple(cmap.shape) == (xy, xy) and cmap.stride() == (1, xy)
        per_column = (codes != 0).sum(dim=2)
        got = codes.clone(), cols.clone(), cmap.clone(), per_column.clone()
        del codes, cols, cmap, per_column                      # dropped at once: the releases are stream-ordered
    ch.release()
    del ch
    gc.collect()
    allocs = g.get_tuning("voxel_atlas_allocations")
    for _ in range(3):                                         # every export came back: the next products reuse the set
        nxt = atlas.changes()
        assert nxt.codes.ptr == ptr
        nxt.release()
    assert g.get_tuning("voxel_atlas_allocations") == allocs
    side.synchronize()
    assert np.array_equal(got[0].cpu().numpy(), want[5]) and np.array_equal(got[2].cpu().numpy(), want[2])
    assert np.array_equal(got[1].cpu().view(torch.int16).numpy().view(np.uint16), want[6])
    assert np.array_equal(got[3].cpu().numpy(), want[6].astype(np.int64).sum(axis=0)) and want[5].any()


if __name__ == "__main__":
    name = sys.argv[1]
    globals()["case_" + name]()
    print("CASE OK " + name)
