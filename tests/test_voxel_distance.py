"""Voxel distance fields on the GPU (gvom_voxel_atlas_distance_field, gvom_voxel_distance_sample: gvom_voxel_distance.hip;
VoxelAtlas.distance_field, DeviceDistanceField.sample) against the numpy referee of tests/voxel_distance_ref.py in its separable form --
which tests/test_voxel_distance_cpu.py holds to the literal definition and to scipy --, fed with the dense fused states the SAME handle
returns, as tests/test_voxel_atlas.py feeds its referee.  Tolerance 0: floats are compared through their bit patterns, +inf and NaN by
position.

  the drive        rings of 1 and 2, following; after integrates 4, 8, 12 and 17 the fields of five boxes (the current window, the first
                   window, half outside the extent, wholly outside it, the displaced one that is not aligned to the pair grid and lies
                   across the storage seams) at caps 0.4, 2.0 and 26.0 m, with and without the flag
  a fixed atlas    windows across the extent's edge, after the last integrate; and a cap whose halo is more than one 64-bit word
  rounding         xy 40, z 6, 0.3 / 0.2 m: a and b are not representable, fl64 decides which voxels are within the cap
  consistency      distance 0 exactly at the box's OCCUPIED (and, flagged, NEVER) voxels
  sample           voxel centres, faces, negative coordinates, outside the box, NaN and +-inf; host and device routes
  ordering         a field is a snapshot of the atlas at its own call, whatever is enqueued behind it
  housekeeping     error codes, no data, the budget, allocations, the pool; DLPack and release() with a field exported (a torch child)

The caps are the issue's.  In the arithmetic of the definition the halo of 26.0 m on this grid is 64 columns and 129 levels, not 65 and
130 (fl64(0.4 * 0.4) lies above 0.16: tests/test_voxel_distance_cpu.py): the z halo still runs off the extent, the x search still spans
two words on either side, and the fixed-atlas test adds 26.5 m (66 columns) so that a halo beyond one word is met as well.

Wall time on the MI355X (pytest --durations, one run): the six drive cases 0.07 to 0.93 s each (the referee's 129 x-offsets at 26.0 m),
the two fixed-atlas cases 0.37 s, the torch child 2.3 s, everything else below 0.1 s; the file 6.3 s."""
import copy
import ctypes
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import obstacle_scenes
import voxel_atlas_cycle as vc
import voxel_atlas_ref as va
import voxel_distance_ref as vd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GVOM_ERR_INVALID, GVOM_ERR_CAPACITY, GVOM_NO_DATA = -1, -4, 4
RES = (va.DRIVE_RES[0], va.DRIVE_RES[2])
CAPS = (0.4, 2.0, 26.0)
DISPLACED = (13, -29, 2)
AFTER = (3, 7, 11, 16)                                      # integrates 4, 8, 12 and 17


@pytest.fixture(scope="module")
def gvom():
    import gvom as mod
    rc, info = mod.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    return mod


def _hold_field(field, want, origin, cap, what):
    assert field is not None, what + ": no data"
    with field:
        assert tuple(field.origin_voxels) == tuple(int(v) for v in origin) and field.max_distance == cap, what
        dist, counts = field.copy_to_host()
    assert dist.dtype == np.float32 and dist.shape == want[0].shape and counts.dtype == np.int32, what
    if not vd.same_bits(dist, want[0]):
        bad = np.argwhere(dist.view(np.uint32) != want[0].view(np.uint32))
        raise AssertionError("%s: %d voxels differ, first %r: got %r, referee %r" % (what, len(bad), tuple(bad[0]), dist[tuple(bad[0])], want[0][tuple(bad[0])]))
    assert np.array_equal(counts, want[1]), "%s: counts %r, referee %r" % (what, counts.tolist(), want[1].tolist())
    return dist, counts


def _boxes(ref, W, first):
    return va.box_origins(ref, first) + [tuple(W[k] + DISPLACED[k] for k in range(3))]


def _drive(gvom, ring, follow, each=None):
    """the climbing drive of tests/test_voxel_atlas.py: a fresh mapper and atlas, the referee beside it fed from read_dense(); each(k, g,
    atlas, ref, W, first W) after every integrate"""
    g = gvom.Gvom(*(va.DRIVE_PARAMS + (ring,) + va.DRIVE_TAIL), voxel_statistics=False)
    kw = dict(follow=True) if follow else dict(follow=False, origin_voxels=np.array(va.fixed_origin()))
    atlas = g.create_voxel_atlas(va.DRIVE_A, va.DRIVE_Z, **kw)
    ref = va.VoxelAtlasRef(va.DRIVE_A, va.DRIVE_Z, va.DRIVE_XY, va.DRIVE_ZS, follow=follow, origin=(0, 0, 0) if follow else va.fixed_origin())
    first = W = None
    for k, (pc, ego) in enumerate(va.drive_scans()):
        g.process_pointcloud(pc, ego)
        g.combine_maps()
        state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
        W = tuple(int(v) for v in origin)
        first = first or W
        assert atlas.integrate() is True
        ref.integrate(state, W)
        if each:
            each(k, g, atlas, ref, W, first)
    return g, atlas, ref, W, first


def _hold_boxes(g, atlas, ref, boxes, caps, what):
    for j, origin in enumerate(boxes):
        for cap in caps:
            for ub in (False, True):
                want = vd.separable(ref, origin, cap, RES, unknown_blocks=ub)
                f = atlas.distance_field(cap, origin_voxels=None if j == 0 else np.array(origin), unknown_blocks=ub)
                _hold_field(f, want, origin, cap, "%s, box %d %r, cap %r, flag %d" % (what, j, origin, cap, ub))
                assert g.get_tuning("voxel_distance_halo_xy") == vd.halo(cap, RES[0]) and g.get_tuning("voxel_distance_halo_z") == vd.halo(cap, RES[1])
                if j == 3:                                  # wholly outside the extent
                    assert np.isinf(want[0]).all() if not ub else not want[0].any()


# ---- 1. the drive ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("ring", [1, 2])
def test_the_drive_fields_equal_the_referee(gvom, ring, cap):
    seen = []

    def each(k, g, atlas, ref, W, first):
        if k in AFTER:
            _hold_boxes(g, atlas, ref, _boxes(ref, W, first), (cap,), "ring %d, integrate %d" % (ring, k + 1))
            seen.append(k)
    g, atlas, ref, W, first = _drive(gvom, ring, True, each)
    assert tuple(seen) == AFTER and g.get_tuning("voxel_distance_field") == 1
    _hold_field(atlas.distance_field(cap, center=va.drive_scans()[-1][1]), vd.separable(ref, W, cap, RES), W, cap, "field by centre")


# ---- 2. a fixed atlas --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring", [1, 2])
def test_a_fixed_atlas_with_windows_across_the_extents_edge(gvom, ring):
    g, atlas, ref, W, first = _drive(gvom, ring, False)
    assert ref.total["outside"] >= 1                        # windows of the drive lay across the extent's edge
    _hold_boxes(g, atlas, ref, _boxes(ref, W, first), CAPS, "fixed, ring %d" % ring)
    assert vd.halo(26.5, RES[0]) == 66                      # more than one 64-bit word in x
    _hold_boxes(g, atlas, ref, [W, tuple(W[k] + DISPLACED[k] for k in range(3))], (26.5,), "fixed, ring %d" % ring)


# ---- 3. no power of two, resolutions that round ---------------------------------------------------------------------------------------------
def test_a_grid_that_is_no_power_of_two_whose_resolutions_round(gvom):
    xy, zs, res = 40, 6, (0.3, 0.2)
    g = gvom.Gvom(res[0], res[1], xy, zs, 1, *va.DRIVE_TAIL, voxel_statistics=False)
    ego = (1.7, -2.9, 0.3)
    g.process_pointcloud(obstacle_scenes.post_scene(3, xy, res[0], res[1], ego, n_posts=40, ground_pts=3000), ego)
    g.combine_maps()
    state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
    W = tuple(int(v) for v in origin)
    atlas = g.create_voxel_atlas(64, 8)
    ref = va.VoxelAtlasRef(64, 8, xy, zs)
    assert atlas.integrate() and ref.integrate(state, W)["outside"] == 0
    # a and b are rounded products; three columns are within 0.9 m and not within fl64(0.3 * 3)
    assert Fraction(0.3 * 0.3) != Fraction(0.3) ** 2 and Fraction(0.2 * 0.2) != Fraction(0.2) ** 2 and 0.3 * 3 < 0.9
    for cap in (0.3, 0.9, 1.0):
        for ub in (False, True):
            for origin in (W, (W[0] - 7, W[1] + 5, W[2] + 1), (ref.E[0] + 64 - 9, ref.E[1] - 11, ref.E[2] + 8 - 2)):
                want = vd.separable(ref, origin, cap, res, unknown_blocks=ub)
                f = atlas.distance_field(cap, origin_voxels=np.array(origin), unknown_blocks=ub)
                _hold_field(f, want, origin, cap, "0.3 / 0.2 m, cap %r, flag %d, box %r" % (cap, ub, origin))
                if origin == W:
                    print(cap, ub, vd.census(want[0]))
    want = vd.separable(ref, W, 1.0, res)[0]
    assert min(vd.census(want)) >= 100, vd.census(want)


# ---- 4. consistency with what exists -----------------------------------------------------------------------------------------------------------
def test_the_field_is_zero_exactly_where_the_box_is_occupied(gvom):
    g = gvom.Gvom(*(va.DRIVE_PARAMS + (1,) + va.DRIVE_TAIL), voxel_statistics=False)
    atlas = g.create_voxel_atlas(va.DRIVE_A, va.DRIVE_Z)
    pc, ego = va.drive_scans()[0]
    g.process_pointcloud(pc, ego)
    g.combine_maps()
    assert atlas.integrate()
    for origin in (None, np.array(va.window_origin(ego)) + np.array([40, -9, 3])):
        classes, box_counts = atlas.box(origin).copy_to_host()
        dist, counts = atlas.distance_field(2.0, origin_voxels=origin).copy_to_host()
        assert np.array_equal(dist == 0, classes == gvom.VOXEL_OCCUPIED) and counts[0] == box_counts[0] and (origin is not None or counts[0] > 0)
        assert counts[1] == np.isfinite(dist).sum() and counts[2] == box_counts[2] and counts[3] == box_counts[3] == 1
        dist, counts = atlas.distance_field(2.0, origin_voxels=origin, unknown_blocks=True).copy_to_host()
        assert np.array_equal(dist == 0, classes != gvom.VOXEL_FREE) and counts[0] == (classes != gvom.VOXEL_FREE).sum()
    with g.occupancy_grid_device() as occ:                   # and voxel for voxel with the occupancy grid of the same map
        dist = atlas.distance_field(2.0).distance.copy_to_host()
        assert np.array_equal(dist == 0, occ.copy_to_host() == 1)


# ---- 5. sample -----------------------------------------------------------------------------------------------------------------------------------
class _Hip(object):
    def __init__(self):
        self.rt = ctypes.CDLL("libamdhip64.so")
        self.rt.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.rt.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.rt.hipFree.argtypes = [ctypes.c_void_p]
        self.held = []

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = ctypes.c_void_p()
        assert self.rt.hipMalloc(ctypes.byref(p), a.nbytes) == 0
        assert self.rt.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0           # host to device, blocking
        self.held.append(p)
        return p.value

    def free(self):
        for p in self.held:
            self.rt.hipFree(p)
        self.held = []


@pytest.fixture(scope="module")
def hip():
    h = _Hip()
    yield h
    h.free()


@pytest.fixture(scope="module")
def driven(gvom):
    """the following atlas of a one-slot ring after the drive: (mapper, atlas, referee, final W, first W)"""
    return _drive(gvom, 1, True)


def _sample_points(origin, shape, res):
    """float32 [n, 3]: voxel centres, faces (k * resolution and the float32 just below it), points outside the box on every side,
    non-finite coordinates.  The drive's windows lie at negative coordinates on every axis."""
    r = np.array([res[0], res[0], res[1]], np.float64)
    lo = np.array(origin, np.int64)
    rng = np.random.default_rng(11)
    v = lo + rng.integers(0, np.array(shape), (1500, 3))
    centres = ((v + 0.5) * r).astype(np.float32)
    faces = (v[:600] * r).astype(np.float32)
    below = np.nextafter(faces, np.float32(-np.inf))
    mixed = faces.copy()
    mixed[:, 1] = centres[:600, 1]                           # a face in x and z, a centre in y
    span = np.array(shape) * r
    outside = (lo * r + rng.uniform(-0.5, 1.5, (600, 3)) * span).astype(np.float32)
    bad = centres[:96].copy()
    bad[np.arange(96), np.arange(96) % 3] = np.array([np.nan, np.inf, -np.inf], np.float32)[(np.arange(96) // 3) % 3]
    edge = np.array([lo * r, (lo + np.array(shape)) * r, (lo + np.array(shape) - 1) * r], np.float64).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([centres, faces, below, mixed, outside, bad, edge]))


def test_samples_equal_a_gather_from_the_referees_field(driven, hip):
    g, atlas, ref, W, first = driven
    origin = tuple(W[k] + DISPLACED[k] for k in range(3))
    assert all(o < 0 for o in origin)                        # negative coordinates on every axis
    want_field = vd.separable(ref, origin, 2.0, RES)[0]
    pts = _sample_points(origin, want_field.shape, RES)
    want, want_counts = vd.gather(want_field, origin, RES, pts)
    print(len(pts), want_counts)
    assert want_counts[0] >= 3000 and want_counts[2] >= 50 and want_counts[1] < want_counts[0] < len(pts) and np.isnan(want[-99:-3]).all()
    field = atlas.distance_field(2.0, origin_voxels=np.array(origin))
    dev = hip.upload(pts)
    host, device = field.sample(pts), field.sample_device(dev, len(pts))
    field.release()                                          # the caller lets go of the field; the sample products are held
    del field
    atlas.distance_field(0.4, unknown_blocks=True).release()       # ... and the field's set is written again behind the gathers
    for s, what in ((host, "host route"), (device, "device route")):
        with s:
            got, counts = s.copy_to_host()
        assert got.dtype == np.float32 and got.shape == (len(pts),) and vd.same_bits(got, want), what
        assert np.array_equal(counts, want_counts), (what, counts, want_counts)
    one = atlas.distance_field(2.0, origin_voxels=np.array(origin)).sample(pts[:1])
    assert vd.same_bits(one.distance.copy_to_host(), want[:1]) and one.counts.copy_to_host()[3] == 1


# ---- 6. ordering ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", [1, 3])
def test_a_field_is_a_snapshot_of_its_own_moment(gvom, bs):
    """integrate(), distance_field() without a wait, then the next scan, an asynchronous combine and its integrate are enqueued before
    the first field is read back: the first field equals the referee's state of its own moment, the second the next.  The referee is
    fed from the CPU oracle's mirror (tests/voxel_atlas_cycle.py)"""
    c = vc.AtlasCycle("np2", bs, gvom, False, **vc.FOLLOWING)
    res = (c.res[0], c.res[2])
    c.scan(0)
    c.combine("sync", "A")
    _, W1, _, _ = c.merge("A")
    fields = [(c.atlas.distance_field(2.0, unknown_blocks=ub), ub) for ub in (False, True)]
    then = copy.deepcopy(c.ref)
    c.scan(1)
    c.combine("async", "B")
    W2 = tuple(int(v) for v in c.cur.W)
    assert c.atlas.integrate() is True                       # behind the fusion on the second stream; no wait in between
    c.ref.integrate(c.cur.state, W2)
    later = [(c.atlas.distance_field(2.0), False)]            # (four products of the kind are held at most)
    old_box = c.atlas.distance_field(2.0, origin_voxels=np.array(W1))
    assert W1 != W2
    for f, ub in fields:
        _hold_field(f, vd.separable(then, W1, 2.0, res, unknown_blocks=ub), W1, 2.0, "the field before the next integrate, flag %d" % ub)
    later.append((c.atlas.distance_field(2.0, unknown_blocks=True), True))
    for f, ub in later:
        _hold_field(f, vd.separable(c.ref, W2, 2.0, res, unknown_blocks=ub), W2, 2.0, "the field after it, flag %d" % ub)
    now, before = vd.separable(c.ref, W1, 2.0, res), vd.separable(then, W1, 2.0, res)
    assert not vd.same_bits(now[0], before[0])               # the second integrate changed what the first box reads
    _hold_field(old_box, now, W1, 2.0, "the first box, after the next integrate")
    c.finish("B")


# ---- 7. housekeeping -----------------------------------------------------------------------------------------------------------------------------
def test_errors_no_data_and_the_budget(gvom):
    g = gvom.Gvom(0.4, 0.2, 128, 16, 1, *va.DRIVE_TAIL, voxel_statistics=False)
    L, h = g._lib, g._h
    pid, out3 = ctypes.c_int64(-1), (ctypes.c_int64 * 3)()
    pts = np.zeros((8, 3), np.float32)
    pp = pts.ctypes.data_as(ctypes.c_void_p)

    def err():
        return L.gvom_last_error(h)

    def field(origin=None, cap=2.0, flags=0, out=pid):
        return L.gvom_voxel_atlas_distance_field(h, origin, cap, flags, ctypes.byref(out) if out is not None else None, out3)

    def sample(fid, p=pp, n=8, out=pid):
        return L.gvom_voxel_distance_sample(h, fid, p, n, 0, ctypes.byref(out) if out is not None else None)
    assert g.get_tuning("voxel_distance_field") == 1 and g.get_tuning("voxel_distance_mb") == 256
    assert field() == GVOM_ERR_INVALID and b"no voxel atlas" in err() and pid.value == -1
    atlas = g.create_voxel_atlas(128, 16)
    zero = (ctypes.c_int64 * 3)(0, 0, 0)
    assert field() == GVOM_NO_DATA and field(zero) == GVOM_NO_DATA and atlas.distance_field(2.0) is None      # before the first combine
    pc, ego = va.drive_scans()[0]
    g.process_pointcloud(pc, ego)
    g.combine_maps()
    assert field() == GVOM_NO_DATA and atlas.distance_field(2.0) is None      # a NULL origin before the first integrate
    assert field(zero) == 0 and pid.value > 0
    assert atlas.integrate() and field() == 0 and pid.value > 0
    fid = pid.value
    for cap in (float("nan"), float("inf"), -float("inf"), 0.0, -2.0):
        assert field(cap=cap) == GVOM_ERR_INVALID and b"max_distance" in err() and pid.value == -1, cap
    assert field(flags=2) == GVOM_ERR_INVALID and field(flags=-1) == GVOM_ERR_INVALID and b"flag" in err()
    assert field(out=None) == GVOM_ERR_INVALID
    assert field(cap=1e4) == GVOM_ERR_CAPACITY and b"32767" in err()          # 25,000 columns
    assert field(cap=1e200) == GVOM_ERR_CAPACITY
    assert field(cap=0.01) == 0                                               # below a voxel: legal in C (0 or +inf), refused in Python
    with pytest.raises(ValueError):
        atlas.distance_field(0.01)
    # the sample call
    assert field() == 0
    fid = pid.value
    assert sample(fid) == 0 and pid.value > 0
    sid = pid.value
    assert sample(fid, n=0) == GVOM_ERR_INVALID and sample(fid, p=None) == GVOM_ERR_INVALID and sample(fid, out=None) == GVOM_ERR_INVALID
    assert sample(fid, n=(1 << 26) + 1) == GVOM_ERR_CAPACITY and b"2^26" in err()
    for bad in (-1, 0, fid + 1000, sid):                                      # no product, a stale id, a product of another kind
        assert sample(bad) == GVOM_ERR_INVALID and b"distance field" in err(), bad
    with atlas.box() as box:
        assert sample(box.product_id) == GVOM_ERR_INVALID
    for kind in (39, 40, 41, 42):
        assert L.gvom_device_product(h, kind, 0, ctypes.byref(pid)) == GVOM_ERR_INVALID
    # the budget: 128 x 128 x 16 at 2.0 m needs more than 1 MB of intermediates
    ref, W = _ref_of(g, gvom, 128, 16)
    want = vd.separable(ref, W, 2.0, RES)
    allocs = g.get_tuning("voxel_atlas_allocations")
    g.set_tuning("voxel_distance_mb", 1)
    assert g.get_tuning("voxel_distance_mb") == 1
    assert field() == GVOM_ERR_CAPACITY and b"voxel_distance_mb" in err() and pid.value == -1
    with pytest.raises(gvom.GvomBackendError, match="voxel_distance_mb"):
        atlas.distance_field(2.0)
    assert g.get_tuning("voxel_atlas_allocations") == allocs                  # the handle is unchanged
    g.set_tuning("voxel_distance_mb", -1)
    assert g.get_tuning("voxel_distance_mb") == 256
    _hold_field(atlas.distance_field(2.0), want, W, 2.0, "under the default budget again")
    sharded = gvom.Gvom(*(va.DRIVE_PARAMS + (1,) + va.DRIVE_TAIL), voxel_statistics=False, _shard=(0, 1))
    assert sharded._lib.gvom_voxel_atlas_distance_field(sharded._h, None, 2.0, 0, ctypes.byref(pid), None) == GVOM_ERR_INVALID
    assert b"sharded" in sharded._lib.gvom_last_error(sharded._h)
    assert sharded._lib.gvom_voxel_distance_sample(sharded._h, 1, pp, 8, 0, ctypes.byref(pid)) == GVOM_ERR_INVALID


def _ref_of(g, gvom, xy, zs):
    """(a referee that has integrated the handle's current fused map once into a following 128 x 128 x 16 atlas, the window's origin)"""
    state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
    W = tuple(int(v) for v in origin)
    ref = va.VoxelAtlasRef(128, 16, xy, zs)
    ref.integrate(state, W)
    return ref, W


def test_the_pool_and_the_allocations(gvom, driven, hip):
    g, atlas, ref, W, first = driven
    pts = _sample_points(W, (ref.xy, ref.xy, ref.zs), RES)[:512]
    dev = hip.upload(pts)
    pc, ego = va.drive_scans()[-1]
    for cap, ub in ((26.0, True), (2.0, False)):              # warm-up: the largest working buffer first
        with atlas.distance_field(cap, unknown_blocks=ub) as f:
            f.sample(pts).release()
            f.sample_device(dev, len(pts)).release()
    allocs, sets = g.get_tuning("voxel_atlas_allocations"), g.get_tuning("device_product_sets")
    for k in range(20):                                      # steady state: scan, combine, integrate, a field and its samples
        g.process_pointcloud(pc, ego)
        g.combine_maps()
        atlas.integrate()
        with atlas.distance_field((0.4, 2.0, 26.0)[k % 3], unknown_blocks=bool(k & 1)) as f:
            f.sample(pts).release()
            f.sample_device(dev, len(pts)).release()
    assert g.get_tuning("voxel_atlas_allocations") == allocs and g.get_tuning("device_product_sets") == sets
    held = [atlas.distance_field(2.0) for _ in range(4)]     # GVOM_MAX_PRODUCT_SETS
    assert len({f.distance.ptr for f in held}) == 4
    with pytest.raises(gvom.GvomBackendError, match="exported"):
        atlas.distance_field(2.0)
    samples = [held[0].sample(pts) for _ in range(4)]
    with pytest.raises(gvom.GvomBackendError, match="exported"):
        held[0].sample(pts)
    for s in samples:
        s.release()
    held.pop().release()
    atlas.distance_field(2.0).release()                      # export, release, reuse
    for f in held:
        f.release()
    sets = g.get_tuning("device_product_sets")
    atlas.distance_field(2.0).release()
    assert g.get_tuning("device_product_sets") == sets


def test_dlpack_and_release_with_a_field_exported_through_torch():
    """one fresh child process that imports torch BEFORE the library is loaded (one HIP runtime in the process)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_voxel_distance_torch.py")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "CASE OK" in r.stdout, r.stdout[-4000:]
