"""A mapper that is dropped gives its device memory back: every entry point that allocates on the handle is called once on a mapper
with a map atlas and a voxel atlas, the products are released, the mapper is dropped -- nine times over, and the device's free memory
(hipMemGetInfo) must not sink by 32 MB from the end of the first cycle to the end of the ninth.

What this can see: the large regions -- the map atlas's planes (64 MB), the atlas-sized work and inflation buffers of its cost_to_go
and frontiers, the voxel atlas's pairs, the viewpoints' bitmaps, the intermediates of the distance field and of the change query:
several MB each per cycle, so any one of them leaked eight times is past the margin.  What it cannot see: the window-sized stage
buffers, tables and pinned counters, a few hundred KB a cycle at most; those go by construction -- they are members of the owning
buffer types of g-vom_amd/csrc/gvom_host.h, which free what they hold when the handle is deleted.  Free memory is a figure of the
whole device, which others may be using, so the test is one-sided, with the margin tests/test_range_image.py leaves."""
import ctypes
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
XY, ZS, RES, ZRES = 64, 8, 0.4, 0.2
REST = (1, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
HEADINGS = 16
MARGIN = 32 << 20


def _cycle(gvom, rng):
    """one mapper's life: tables, both atlases, a scan and a combine, one small call of every entry point that allocates on the handle"""
    g = gvom.Gvom(RES, ZRES, XY, ZS, *REST, voxel_statistics=False)
    g.set_footprint(gvom.rectangle_footprint(0.5, 0.5, 0.4, RES, headings=HEADINGS))
    g.set_chassis(gvom.chassis(0.5, -0.3, 0.6, 0.3))
    g.set_body(np.array([[0.0, 0.0, 0.5, 0.1]], np.float32))
    g.set_primitives(gvom.arc_primitives(HEADINGS, 1.0, RES))
    dirs = np.zeros((4, 8, 3), np.float64)
    dirs[:, :, 0], dirs[:, :, 1] = 1.0, np.linspace(-0.5, 0.5, 8)[None, :]
    g.set_sensor_model(dirs)
    atlas = g.create_atlas(1024)                            # 64 bytes a cell: 64 MB of planes
    vatlas = g.create_voxel_atlas(1024, 64)
    pc = np.stack([rng.uniform(-8, 8, 4000), rng.uniform(-8, 8, 4000), rng.normal(-0.5, 0.2, 4000)], axis=1).astype(np.float32)
    g.process_pointcloud(pc, (0.0, 0.0, 0.0))
    maps = g.combine_maps_device()
    assert maps is not None
    made = [maps]

    def keep(p):
        assert p is not None
        made.append(p)
        return p
    # the host routes of the window's calls
    n2 = (XY, XY)
    cost = np.where(rng.random(n2) < 0.1, 0, rng.integers(1, 40, n2)).astype(np.int32)
    cost[:4, :4] = 1
    cost16, vis, ground = cost.astype(np.uint16), (rng.random(n2) < 0.6).astype(np.int32), np.zeros(n2, np.float64)
    field, B = np.ones((XY, XY, ZS), np.float32), np.array([0, 0, 0])
    poses = np.zeros((2, 3, 3), np.float32)
    poses[:, :, :2] = 0.5 * XY * RES
    keep(g.clearance_of(cost, None))
    ctg = keep(g.cost_to_go_of(cost, [(2, 2)]))
    keep(g.score_rollouts_of(cost16, poses))
    keep(g.score_attitude_of(ground, poses))
    keep(g.score_body_of(field, B, ground, poses))
    keep(g.frontiers_of(cost16, vis, cost_to_go=np.asarray(ctg.copy_to_host()[0])))
    keep(g.pose_field_of(cost, [(2, 2)]))
    keep(g.attitude_volume_of(ground))
    keep(g.body_volume_of(field, B, ground))
    # the walk queries of the window
    org, tgt = np.zeros((1, 3), np.float32), np.array([[3.0, 1.0, 0.0], [-2.0, 2.0, -0.4]], np.float32)
    views = gvom.viewpoint_poses(np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 0.0]]), np.array([0.0, 1.0]))
    tfs = np.stack([np.eye(4), np.eye(4)])
    tfs[1, 0, 3] = 0.4
    keep(g.raycast(org, tgt))
    keep(g.score_viewpoints(views, 4.0))
    keep(g.score_alignments(pc[:500], tfs))
    # the map atlas
    atlas.integrate(maps)
    afield = keep(atlas.cost_to_go([(0.0, 0.0)], inflation_radius=0.8))
    keep(afield.frontiers(min_cells=1))
    # the voxel atlas: the change query comes before the integrate that would merge the window
    keep(vatlas.changes())
    assert vatlas.integrate()
    keep(vatlas.raycast(org, tgt))
    keep(vatlas.score_viewpoints(views, 4.0))
    keep(vatlas.score_alignments(pc[:500], tfs))
    keep(vatlas.distance_field(1.0))
    keep(vatlas.changes())
    for p in made:
        p.release()
    del made, maps, ctg, afield, atlas, vatlas, g            # (the atlases are NOT released: the handle's end frees them)
    gc.collect()


def test_a_dropped_mapper_gives_its_memory_back():
    import gvom
    rc, info = gvom.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    rt = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)

    def free_bytes():
        assert rt.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value
    rng = np.random.default_rng(11)
    gc.collect()                                              # (mappers of earlier tests go now, not during the loop)
    _cycle(gvom, rng)                                         # warms the allocator
    before = free_bytes()
    for _ in range(8):
        _cycle(gvom, rng)
    drop = before - free_bytes()
    print("free memory sank by %.2f MB over eight cycles" % (drop / 2.0 ** 20))
    assert drop < MARGIN
