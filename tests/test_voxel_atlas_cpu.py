"""CPU side of the voxel atlas (include/gvom_hip.h "voxel atlas"): the referee of tests/voxel_atlas_ref.py held to tests/raycast_ref.py's
walk on window-sized extents (that one is pinned to the CPU referee of the whole pipeline), the census of the drive with that referee as
the mapper, the header / binding / library agreement, and what the binding refuses before it calls the library.  No GPU.

Census of the drive (17 scans, xy 64, z 8, resolutions 0.4 / 0.2, atlas 128 x 128 x 16), rings of 1 / 2 slots:
  flat drive, no extent move (an extent that holds every window): 28,330 known voxels; 6,965 / 6,866 occupied and 9,538 / 9,637 free
      voxels remembered outside the final window; 2,873 / 2,624 occupied -> free and 5,434 / 5,090 free -> occupied transitions
  climbing drive, following: first seen 31,632; free -> occupied 2,215 / 2,181; occupied -> free 755 / 732; confirmed 73,727 / 73,784;
      uninformative 448,727; cleared by the move 942,178, of those observed 15,587; it ends with 16,045 observed and 3,294 / 3,324
      occupied voxels.  The window of a following atlas never leaves the extent: count [5] is met by the fixed run (100,608 voxels), whose
      counts [6] and [7] stay 0 in turn -- "every count at least once over the drive" is held over the two runs together.
  the 3,072 rays of the remembered-space test under GVOM_RAY_UNKNOWN_BLOCKS: CLEAR / OCCUPIED / UNKNOWN / LEFT / INVALID 231 / 1,590 /
      1,123 / 64 / 64 (ring 2: 251 / 1,578 / 1,115 / 64 / 64); 289 / 310 stop OCCUPIED at a voxel outside the final window; 69 / 56, 243 /
      232 and 201 / 207 examine voxels on both sides of the storage seam of x, y and z."""
import ctypes
import os
import re

import numpy as np
import pytest

import atlas_ref
import gvom
import raycast_ref as rr
import voxel_atlas_ref as va
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = [(False, False), (True, False), (False, True), (True, True)]
SYMBOLS = ("gvom_voxel_atlas_configure", "gvom_voxel_atlas_integrate", "gvom_voxel_atlas_clear", "gvom_voxel_atlas_counts", "gvom_voxel_atlas_box",
           "gvom_voxel_atlas_raycast", "gvom_voxel_atlas_score_viewpoints")
OCCUPIED_OUTSIDE_FLOOR, STATUS_FLOOR, SEAM_FLOOR = 256, 32, 32


# ---- 1. the walk with explicit sizes equals the walk that is pinned to the CPU referee ---------------------------------------------------------
def test_the_walk_equals_raycast_refs_on_a_window_sized_extent():
    grid = "p2"
    xr, zr, xy, zs = rr.GRIDS[grid]
    g = rr.build_map(oracle.OracleGvom, grid, 1)
    state, W = np.asarray(g.combined_index_map).copy(), np.asarray(g.combined_origin, np.float64)
    A, B, fam = rr.rays_of(grid, state, W)
    for ub, ct in FLAGS:
        for one in (False, True):
            a = A[:1] if one else A
            want_r, want_p = rr.walk(state, W, grid, a, B, unknown_blocks=ub, check_target=ct)
            res, pos, vox = va.walk(state, W, (xy, xy, zs), (xr, xr, zr), a, B, unknown_blocks=ub, check_target=ct)
            assert np.array_equal(res, want_r[:, [0, 1, 3]]), (ub, ct, one)
            assert np.array_equal(pos.view(np.uint32), want_p.view(np.uint32)), (ub, ct, one)
            v = want_r[:, 2].astype(np.int64)
            decoded = np.stack([v % xy, v // xy % xy, v // (xy * xy)], axis=1) + W.astype(np.int64)
            assert np.array_equal(vox, np.where((v >= 0)[:, None], decoded, 0)), (ub, ct, one)
            if (ub, ct, one) == (True, False, False):
                assert min(rr.census(want_r)[0]) >= rr.STATUS_FLOOR            # every status is met


def test_classes_and_the_merge_rule_on_hand_written_voxels():
    assert list(va.classes([5, 0, -1, -2, -7, -2 ** 31])) == [2, 2, 0, 1, 1, 1]
    ref = va.VoxelAtlasRef(64, 2, 2, 1, follow=False, origin=(0, 0, 0))
    assert ref.integrate(np.array([3, -2, -1, -2], np.int32), (0, 0, 0)) == dict(
        first_seen=3, free_to_occupied=0, occupied_to_free=0, confirmed=0, uninformative=1, outside=0, cleared=0, cleared_observed=0)
    # occupied -> free, free -> occupied, a NEVER that keeps nothing, a NEVER over a known voxel (kept)
    n = ref.integrate(np.array([-2, 9, -1, -1], np.int32), (0, 0, 0))
    assert (n["occupied_to_free"], n["free_to_occupied"], n["uninformative"], n["confirmed"], n["first_seen"]) == (1, 1, 2, 0, 0)
    assert list(ref.cls[0, :2, :2].reshape(-1)) == [va.FREE, va.OCCUPIED, va.NEVER, va.FREE]
    n = ref.integrate(np.array([-3, 7, -2, -1], np.int32), (63, 0, 1))           # x: one column inside; z: the upper level
    assert n["outside"] == 2 and n["first_seen"] == 2 and ref.cls[1, 0, 63] == va.FREE and ref.cls[1, 1, 63] == va.FREE
    assert ref.counts()["observed"] == 5 and ref.counts()["occupied"] == 1 and ref.counts()["seq"] == 3
    box, counts = ref.box((62, -1, 0))
    assert box.shape == (2, 2, 1) and list(counts) == [0, 0, 2, 3] and box.sum() == 0        # (62, 0, 0) and (63, 0, 0) are NEVER; the row y = -1 lies outside
    box, counts = ref.box((0, 0, 0))
    assert list(box[:, :, 0].T.reshape(-1)) == [1, 2, 0, 1] and list(counts) == [1, 2, 0, 3]


@pytest.mark.parametrize("d", [(0, 0, 0), (3, 0, 0), (0, -5, 0), (0, 0, 2), (-7, 9, -1), (64, 0, 0), (1, 1, 4), (-63, 63, 3)])
def test_moves_clear_what_entered_and_count_what_left(d):
    rng = np.random.default_rng(3)
    ref = va.VoxelAtlasRef(64, 4, 16, 2, origin=(-10, 5, 1))
    ref.cls[:] = rng.integers(0, 3, ref.cls.shape)
    before = ref.cls.copy()
    E0 = ref.E
    cleared, observed = ref.move(tuple(E0[k] + d[k] for k in range(3)))
    z, y, x = np.indices(before.shape)
    new_world = np.stack([x + ref.E[0], y + ref.E[1], z + ref.E[2]], axis=-1)
    was = ((new_world >= np.array(E0)) & (new_world < np.array(E0) + np.array([64, 64, 4]))).all(axis=-1)      # voxels of the new extent that were in the old
    assert cleared == int((~was).sum()) and (ref.cls[~was] == va.NEVER).all()
    o = new_world[was] - np.array(E0)
    assert np.array_equal(ref.cls[was], before[o[:, 2], o[:, 1], o[:, 0]])
    assert observed == int((before != va.NEVER).sum() - (ref.cls != va.NEVER).sum())


# ---- 2. the census of the drive ----------------------------------------------------------------------------------------------------------------
def _drive(ring, scans, *refs):
    o = oracle.OracleGvom(*(va.DRIVE_PARAMS + (ring,) + va.DRIVE_TAIL))
    W = None
    for pc, ego in scans:
        o.process_pointcloud(pc, ego)
        o.combine_maps()
        W = tuple(int(v) for v in np.asarray(o.combined_origin))
        assert W == va.window_origin(ego)
        for ref in refs:
            ref.integrate(np.asarray(o.combined_index_map), W)
    return W, scans[-1][1]


@pytest.mark.parametrize("ring", [1, 2])
def test_the_flat_drive_ends_with_the_issues_census(ring):
    """the drive of tests/atlas_ref.py as it is, in an extent that holds every window (no move): the figures the issue gives"""
    ref = va.VoxelAtlasRef(256, 16, va.DRIVE_XY, va.DRIVE_ZS, follow=False, origin=(-64, -128, -12))
    W, _ = _drive(ring, atlas_ref.drive_scans(), ref)
    c = ref.counts()
    occ, free = len(va.remembered_outside(ref, W, va.OCCUPIED)), len(va.remembered_outside(ref, W, va.FREE))
    print(ring, ref.total, c, occ, free)
    assert ref.total["outside"] == 0 and c["observed"] == ref.total["first_seen"] == 28330
    assert 6866 <= occ <= 6965 and 9538 <= free <= 9637
    assert 2624 <= ref.total["occupied_to_free"] <= 2873 and 5090 <= ref.total["free_to_occupied"] <= 5434


@pytest.mark.parametrize("ring", [1, 2])
def test_census_of_the_climbing_drive(ring):
    follow = va.VoxelAtlasRef(va.DRIVE_A, va.DRIVE_Z, va.DRIVE_XY, va.DRIVE_ZS)
    fixed = va.VoxelAtlasRef(va.DRIVE_A, va.DRIVE_Z, va.DRIVE_XY, va.DRIVE_ZS, follow=False, origin=va.fixed_origin())
    scans = va.drive_scans()
    W, ego = _drive(ring, scans, follow, fixed)
    Ws = [va.window_origin(e) for _, e in scans]
    assert len(scans) == 17 and Ws[-1] == Ws[0] and max(w[2] for w in Ws) - Ws[0][2] >= atlas_ref.DRIVE_LEGS       # Ez moves, out and back
    assert max(abs(w[0] - Ws[0][0]) for w in Ws) > va.DRIVE_XY
    print(ring, follow.total, fixed.total, follow.counts())
    for k, name in enumerate(va.COUNT_NAMES[:8]):
        assert follow.total[name] + fixed.total[name] >= 1, name
    assert all(follow.total[name] >= 1 for name in va.COUNT_NAMES[:5] + ("cleared", "cleared_observed")) and fixed.total["outside"] >= 1
    # the ray set of the remembered-space test
    a, b = va.drive_rays(follow, W, ego)
    res, pos, vox, visits = va.atlas_walk(follow, va.DRIVE_RES, a, b, unknown_blocks=True, record=True)
    status = [int((res[:, 0] == k).sum()) for k in range(5)]
    w = vox.astype(np.int64) - np.array(W)
    outside = ~((w >= 0) & (w < np.array([va.DRIVE_XY, va.DRIVE_XY, va.DRIVE_ZS]))).all(axis=1)
    stops_outside = int(((res[:, 0] == va.HIT) & outside).sum())
    seams = va.seam_crossers(follow, visits, len(a))
    print(ring, len(a), status, stops_outside, seams)
    assert stops_outside >= OCCUPIED_OUTSIDE_FLOOR and min(status) >= STATUS_FLOOR and min(seams) >= SEAM_FLOOR
    # what was remembered there is what the walk met: an OCCUPIED stop is an occupied voxel of the atlas
    assert (follow.world_class(vox[res[:, 0] == va.HIT]) == va.OCCUPIED).all()
    # and the poses of the viewpoint test: 16 outside the window, 16 inside, all in the extent
    poses = va.drive_poses(follow, W, ego)
    assert poses.shape == (32, 4, 4)
    pv = np.floor(poses[:, :3, 3] / np.array(va.DRIVE_RES)).astype(np.int64)
    pw = pv - np.array(W)
    inside = ((pw >= 0) & (pw < np.array([va.DRIVE_XY, va.DRIVE_XY, va.DRIVE_ZS]))).all(axis=1)
    assert int(inside.sum()) == 16 and not inside[:16].any() and (follow.world_class(pv) == va.FREE).all()


# ---- 3. header, binding, library ------------------------------------------------------------------------------------------------------------------
def test_the_header_the_binding_and_the_library_agree():
    header = open(os.path.join(ROOT, "include", "gvom_hip.h")).read()
    for name, value in (("GVOM_PRODUCT_VOXEL_BOX", gvom.PRODUCT_VOXEL_BOX), ("GVOM_PRODUCT_VOXEL_ATLAS_RAYS", gvom.PRODUCT_VOXEL_ATLAS_RAYS),
                        ("GVOM_PRODUCT_VOXEL_ATLAS_VIEWPOINTS", gvom.PRODUCT_VOXEL_ATLAS_VIEWPOINTS), ("GVOM_VOXEL_NEVER", gvom.VOXEL_NEVER),
                        ("GVOM_VOXEL_FREE", gvom.VOXEL_FREE), ("GVOM_VOXEL_OCCUPIED", gvom.VOXEL_OCCUPIED)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1)) == value, name
    assert (gvom.PRODUCT_VOXEL_BOX, gvom.PRODUCT_VOXEL_ATLAS_RAYS, gvom.PRODUCT_VOXEL_ATLAS_VIEWPOINTS) == (32, 34, 36)
    assert int(re.search(r"#define\s+GVOM_ABI_VERSION\s+(\d+)", header).group(1)) == 10 == gvom.ABI_VERSION          # additions: the version stays
    section = header[header.index("--- voxel atlas"):header.index("--- one map sharded")]
    for word in ("VOXELS", "CLASS", "STORAGE", "EXTENT", "INTEGRATE", "MOVE", "MERGE", "COUNTS", "BOX", "RAYS", "VIEWPOINTS", "GVOM_NO_DATA",
                 "GVOM_ERR_INVALID", "GVOM_ERR_CAPACITY", "NOT PROVIDED", "time decay", "hit counts", "saving to disk", '"voxel_atlas"',
                 '"voxel_atlas_levels"', '"voxel_atlas_allocations"', "Kinds 31, 33 and 35 are not assigned"):
        assert word in section, word
    assert '"voxel atlas" below' in header[header.index("--- map atlas"):header.index("--- atlas fields")]           # 3-D memory: pointed to
    bound = {n: a for n, _, a in gvom.ABI}
    assert set(SYMBOLS) <= set(bound)
    L = ctypes.CDLL(gvom.library_path())
    for name in SYMBOLS:
        assert hasattr(L, name) and re.search(r"\bint %s\(gvom_t \*h" % name, section), name
    assert len(bound["gvom_voxel_atlas_raycast"]) == len(bound["gvom_raycast"]) and len(bound["gvom_voxel_atlas_score_viewpoints"]) == len(bound["gvom_score_viewpoints"])
    layout = open(os.path.join(ROOT, "g-vom_amd", "csrc", "gvom_setlayout.h")).read()
    for name in ("GVOM_PRODUCT_VOXEL_BOX", "GVOM_PRODUCT_VOXEL_ATLAS_RAYS", "GVOM_PRODUCT_VOXEL_ATLAS_VIEWPOINTS"):
        assert layout.count(name) >= 2, name
    assert gvom._PRODUCT_DTYPES[32] == (np.uint8, np.int32) and gvom._PRODUCT_DTYPES[34] == (np.int32, np.float32, np.int32)
    assert gvom._PRODUCT_DTYPES[36] == gvom._PRODUCT_DTYPES[gvom.PRODUCT_VIEWPOINTS] and issubclass(gvom.DeviceAtlasViewpoints, gvom.DeviceViewpoints)
    makefile = open(os.path.join(ROOT, "g-vom_amd", "Makefile")).read()
    assert " gvom_voxel_atlas " in makefile and " gvom_voxel_atlas_calls " in makefile


# ---- the binding without a GPU -------------------------------------------------------------------------------------------------------------------
class _Lib(object):
    """stands in for the loaded library: notes every call and returns 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, [tuple(a) if isinstance(a, ctypes.Array) else a for a in args]))
            if name == "gvom_get_state":
                st = args[1]._obj
                st.has_combined = 1
                st.combined_origin[0], st.combined_origin[1], st.combined_origin[2] = -32.0, 7.0, -4.0
            if name == "gvom_voxel_atlas_box":
                args[3][0], args[3][1], args[3][2] = 1, -2, 3
            if name == "gvom_device_product_export":
                args[4]._obj.value = 4096
            return 0
        return entry

    def named(self, name):
        return [a for n, a in self.calls if n == name]


def _mapper():
    g = gvom.Gvom.__new__(gvom.Gvom)
    g._lib, g._h, g._device = _Lib(), ctypes.c_void_p(1), 0
    g.xy_size, g.xy_resolution, g.z_size, g.z_resolution = 64, 0.4, 8, 0.2
    return g


def test_create_voxel_atlas_refuses_bad_sizes_and_origins_in_python():
    g = _mapper()
    for cells, levels in ((0, 8), (63, 8), (96, 8), (32, 8), (8192, 8), (64.5, 8), (128, 0), (128, 4), (128, 12), (128, 256), (128, 8.5), (4096, 512)):
        with pytest.raises(ValueError):
            g.create_voxel_atlas(cells, levels)
    with pytest.raises(ValueError):
        g.create_voxel_atlas(128, 16, follow=False)                            # a fixed atlas needs its corner
    for bad in ((0, 0), (0.5, 0, 0), (1 << 30, 0, 0), (0, -(1 << 30), 0)):
        with pytest.raises(ValueError):
            g.create_voxel_atlas(128, 16, follow=False, origin_voxels=np.array(bad))
    assert g._lib.calls == []
    a = g.create_voxel_atlas(128, 16, follow=False, origin_voxels=np.array([-5, 6, (1 << 30) - 1]))
    assert g._lib.named("gvom_voxel_atlas_configure") == [[g._h, 128, 16, gvom.ATLAS_FIXED, (-5, 6, (1 << 30) - 1)]]
    assert a.extent_origin == (-5, 6, (1 << 30) - 1) and a.seq == 0 and (a.cells, a.levels) == (128, 16)
    b = g.create_voxel_atlas(4096, 256)                                         # 2^32 voxels: the most
    assert g._lib.named("gvom_voxel_atlas_configure")[-1] == [g._h, 4096, 256, gvom.ATLAS_FOLLOW, None] and b.extent_origin == (0, 0, 0)


def test_integrate_follows_with_the_map_atlas_rule_and_box_takes_voxels_or_a_centre():
    g = _mapper()
    a = g.create_voxel_atlas(128, 16)
    assert a.integrate() is True and a.seq == 1
    assert a.extent_origin == (-32 + 32 - 64, 7 + 32 - 64, -4 + 4 - 8)          # W + floor(size / 2) - side / 2 per axis
    fixed = g.create_voxel_atlas(128, 16, follow=False, origin_voxels=np.array([1, 2, 3]))
    fixed.integrate()
    assert fixed.extent_origin == (1, 2, 3)
    box = a.box()
    assert g._lib.named("gvom_voxel_atlas_box")[-1][1] is None and box.origin_voxels == (1, -2, 3)
    a.box(origin_voxels=np.array([5, -6, 1 << 40]))                            # any integer origin
    assert g._lib.named("gvom_voxel_atlas_box")[-1][1] == (5, -6, 1 << 40)
    a.box(center=(0.13, -7.07, -0.6))                                          # floor(c / resolution - size / 2): the scan's own arithmetic
    assert g._lib.named("gvom_voxel_atlas_box")[-1][1] == (-32, -50, -7)
    for kw in (dict(origin_voxels=np.array([0, 0, 0]), center=(0, 0, 0)), dict(center=(0, 0)), dict(center=(0, np.nan, 0)), dict(origin_voxels=np.array([0, 0]))):
        with pytest.raises(ValueError):
            a.box(**kw)
    with pytest.raises(ValueError):
        a.raycast(np.zeros(3), np.zeros((0, 3)))
    with pytest.raises(ValueError):
        a.raycast(np.zeros((2, 3)), np.zeros((3, 3)))
    with pytest.raises(ValueError):
        a.score_viewpoints(np.zeros((1, 4, 4)), -1.0)
    with pytest.raises(TypeError):
        a.score_viewpoints(np.zeros((1, 4, 4), np.float32), 1.0)
    rays = a.raycast(np.zeros(3), np.ones((5, 3)), unknown_blocks=True, check_target=True)
    call = g._lib.named("gvom_voxel_atlas_raycast")[-1]
    assert call[2] == 1 and call[4] == 5 and call[5] == 0 and call[6] == 3 and isinstance(rays, gvom.DeviceAtlasRays)
    assert a.counts() == dict.fromkeys(gvom.VOXEL_ATLAS_COUNTS, 0) and len(gvom.VOXEL_ATLAS_COUNTS) == 11
    a.clear(); a.release()
    assert g._lib.named("gvom_voxel_atlas_clear") == [[g._h]] and g._lib.named("gvom_voxel_atlas_configure")[-1] == [g._h, 0, 0, 0, None]
