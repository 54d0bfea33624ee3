"""CPU side of the voxel distance field (include/gvom_hip.h "voxel distance field"): the referee of tests/voxel_distance_ref.py in its two
forms and scipy's Euclidean distance transform held to one another on the climbing drive (the CPU oracle is the mapper, exactly as in
tests/test_voxel_atlas_cpu.py), the conditions under which tests/test_voxel_distance.py can fail, the header / binding / library
agreement, what the binding refuses before it calls the library, the halo arithmetic and hand-written cases of the definition.  No GPU.

Census of the drive (17 scans, xy 64, z 8, resolutions 0.4 / 0.2 m, following atlas 128 x 128 x 16), rings of 1 / 2 slots; it ends with
the extent at (-64, -64, -12), the window at (-32, -32, -8) and 3,294 / 3,324 occupied voxels:
  final window, cap 2.0 m: 1,859 / 1,884 voxels at 0, 20,318 / 20,293 finite and positive, 10,591 / 10,591 infinite; 398 / 383 decided by
      a source outside the box; at cap 0.4 m 1,859 / 1,884, 7,039 / 7,066 and 23,870 / 23,818
  the displaced box W + (13, -29, 2) = (-19, -61, -6), not aligned to the pair grid and across the storage seams of x, y and z: 780 / 776
      decided from outside at 2.0 m; the half-outside box of box_origins(), (32, -96, 0): 753 / 771 of all its voxels
  with the flag the final window has 28,042 / 28,067 voxels at 0, and at 0.4 m 564 / 553 are still infinite
The floors below hold for both rings.  Where these figures differ from a transform that compares rounded metres with the cap (73 voxels of
the final window at 2.0 m, ring 1), the voxels lie exactly five columns from their source: fl64(0.4 * 0.4) = 0.16000000000000003, so
fl64(a * 25) = 4.000000000000001 > fl64(2.0 * 2.0), and the definition -- squared distances against the squared cap -- reads them +inf.
For the same reason the halo of 2.0 m is 4 columns and that of 26.0 m is 64 (test_the_halo_is_computed_in_the_arithmetic_of_the_distance)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import gvom
import voxel_atlas_ref as va
import voxel_distance_ref as vd
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = (va.DRIVE_RES[0], va.DRIVE_RES[2])
SYMBOLS = ("gvom_voxel_atlas_distance_field", "gvom_voxel_distance_sample")
DISPLACED = (13, -29, 2)
OUTSIDE_FLOOR, CLASS_FLOOR = 100, 100


def _ulps(a, b):
    """the distance of two finite non-negative float32 arrays in units of the last place"""
    return np.abs(np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64) - np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64))


@pytest.fixture(scope="module")
def driven():
    """per ring length: (referee after the climbing drive, final W, first W)"""
    out = {}
    for ring in (1, 2):
        o = oracle.OracleGvom(*(va.DRIVE_PARAMS + (ring,) + va.DRIVE_TAIL))
        ref = va.VoxelAtlasRef(va.DRIVE_A, va.DRIVE_Z, va.DRIVE_XY, va.DRIVE_ZS)
        first = W = None
        for pc, ego in va.drive_scans():
            o.process_pointcloud(pc, ego)
            o.combine_maps()
            W = tuple(int(v) for v in np.asarray(o.combined_origin))
            assert W == va.window_origin(ego)
            first = first or W
            ref.integrate(np.asarray(o.combined_index_map), W)
        out[ring] = (ref, W, first)
    return out


def _boxes(ref, W, first):
    """the boxes of the GPU tests: box_origins() and the displaced one"""
    return va.box_origins(ref, first) + [tuple(W[k] + DISPLACED[k] for k in range(3))]


def _edt(ref, origin, cap, unknown_blocks):
    """scipy's transform on the class grid padded by the halo: float32 [xy, xy, z], untruncated; None where the padded grid has no source"""
    from scipy import ndimage
    hx, hz = vd.halo(cap, RES[0]), vd.halo(cap, RES[1])
    cls = vd.padded_classes(ref, origin, (hx, hx, hz))
    src = (cls == va.OCCUPIED) | ((cls == va.NEVER) if unknown_blocks else False)
    if not src.any():
        return None
    d = ndimage.distance_transform_edt(~src, sampling=(RES[1], RES[0], RES[0]))
    return np.ascontiguousarray(d[hz:hz + ref.zs, hx:hx + ref.xy, hx:hx + ref.xy].transpose(2, 1, 0)).astype(np.float32)


# ---- 1. the three references agree -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring", [1, 2])
def test_the_two_forms_of_the_referee_and_scipy_agree(driven, ring):
    ref, W, first = driven[ring]
    boxes = _boxes(ref, W, first)
    brute_force = (W, boxes[2], boxes[4])                   # the final window, the half-outside box, the displaced one
    for origin in boxes:
        for cap in (0.4, 2.0):
            fast, fast_counts = vd.separable(ref, origin, cap, RES)
            if origin in brute_force and (cap == 2.0 or origin == W):              # (the literal form takes seconds per field)
                slow, slow_counts = vd.brute(ref, origin, cap, RES)
                assert vd.same_bits(fast, slow) and np.array_equal(fast_counts, slow_counts), (origin, cap)
            assert fast.dtype == np.float32 and fast.shape == (ref.xy, ref.xy, ref.zs) and fast_counts[0] == ref.box(origin)[1][0]
            for ub in (False, True):
                mine = fast if not ub else vd.separable(ref, origin, cap, RES, unknown_blocks=True)[0]
                theirs = _edt(ref, origin, cap, ub)
                if theirs is None:
                    assert np.isinf(mine).all()
                    continue
                fin = np.isfinite(mine)
                assert (_ulps(mine[fin], theirs[fin]) <= 1).all(), (origin, cap, ub)       # two float64 evaluations rounded once to float32
                limit = np.nextafter(np.float32(cap), np.float32(0))
                assert (theirs[~fin] >= limit).all(), (origin, cap, ub)                    # beyond the cap, or within an ulp of it
    # a cap whose halo exceeds the extent in z and a 64-bit word in x, under the flag: the fast form against scipy alone
    mine = vd.separable(ref, W, 26.0, RES, unknown_blocks=True)[0]
    assert (_ulps(mine, _edt(ref, W, 26.0, True)) <= 1).all() and np.isfinite(mine).all()


# ---- 2. the conditions under which the GPU tests can fail ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring", [1, 2])
def test_census_of_the_distance_fields_of_the_drive(driven, ring):
    ref, W, first = driven[ring]
    assert ref.E == (-64, -64, -12) and W == (-32, -32, -8)
    occupied = ref.counts()["occupied"]
    boxes = _boxes(ref, W, first)
    displaced, half = boxes[4], boxes[2]
    assert displaced == (-19, -61, -6) and half == (32, -96, 0)
    fields = {cap: vd.separable(ref, W, cap, RES)[0] for cap in (0.4, 2.0)}
    census = {cap: vd.census(f) for cap, f in fields.items()}
    outside = {name: vd.decided_from_outside(ref, o, 2.0, RES) for name, o in (("window", W), ("displaced", displaced), ("half", half))}
    flagged = {cap: vd.census(vd.separable(ref, W, cap, RES, unknown_blocks=True)[0]) for cap in (0.4, 2.0)}
    print(ring, occupied, census, outside, flagged, vd.census(vd.separable(ref, displaced, 2.0, RES)[0]))
    if ring == 1:                                           # the issue's own figures are within the floors' reach: the drive is the one it measured
        assert occupied == 3294
    for cap in (0.4, 2.0):
        assert min(census[cap]) >= CLASS_FLOOR, (cap, census[cap])
    assert min(outside.values()) >= OUTSIDE_FLOOR, outside
    assert flagged[2.0][0] >= 20000 and flagged[0.4][2] >= CLASS_FLOOR, flagged
    # the displaced box is not aligned to the pair grid and crosses the storage seam on every axis
    for k, size in enumerate(ref.sizes()):
        lo = displaced[k] & (size - 1)
        assert lo + (ref.xy, ref.xy, ref.zs)[k] > size, k
    assert displaced[0] & 63
    # nearest sources that differ from the voxel in z only, and in x and y only
    _, _, near = vd.brute(ref, W, 2.0, RES, with_nearest=True)
    fin = np.isfinite(fields[2.0].transpose(2, 1, 0))
    z_only = fin & (near[..., 0] == 0) & (near[..., 1] == 0) & (near[..., 2] != 0)
    xy_only = fin & (near[..., 2] == 0) & ((near[..., 0] != 0) | (near[..., 1] != 0))
    print(ring, int(z_only.sum()), int(xy_only.sum()))
    assert z_only.sum() >= CLASS_FLOOR and xy_only.sum() >= CLASS_FLOOR
    # the wholly-outside box: nothing in reach without the flag, everything a source with it
    far = boxes[3]
    assert np.isinf(vd.separable(ref, far, 2.0, RES)[0]).all() and not vd.separable(ref, far, 2.0, RES, unknown_blocks=True)[0].any()


# ---- 3. header, binding, library ------------------------------------------------------------------------------------------------------------------
def test_the_header_the_binding_and_the_library_agree():
    header = open(os.path.join(ROOT, "include", "gvom_hip.h")).read()
    for name, value in (("GVOM_PRODUCT_VOXEL_DISTANCE", gvom.PRODUCT_VOXEL_DISTANCE), ("GVOM_PRODUCT_VOXEL_DISTANCE_SAMPLES", gvom.PRODUCT_VOXEL_DISTANCE_SAMPLES),
                        ("GVOM_DISTANCE_UNKNOWN_BLOCKS", gvom._DISTANCE_UNKNOWN_BLOCKS)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1)) == value, name
    assert (gvom.PRODUCT_VOXEL_DISTANCE, gvom.PRODUCT_VOXEL_DISTANCE_SAMPLES) == (40, 42)
    assert int(re.search(r"#define\s+GVOM_ABI_VERSION\s+(\d+)", header).group(1)) == 10 == gvom.ABI_VERSION          # additions: the version stays
    section = header[header.index("--- voxel distance field"):header.index("--- one map sharded")]
    for word in ("BOX", "SOURCES", "VALUE", "EXACTNESS", "COUNTS", "SAMPLE", "GVOM_NO_DATA", "GVOM_ERR_INVALID", "GVOM_ERR_CAPACITY", "NOT PROVIDED",
                 "signed distance", "interpolation", "incremental updates", '"voxel_distance_field"', '"voxel_distance_mb"', '"voxel_atlas_allocations"',
                 "Kinds 39 and 41 are not assigned", "fl64(a * n)", "float64 division"):
        assert word in section, word
    bound = {n: a for n, _, a in gvom.ABI}
    L = ctypes.CDLL(gvom.library_path())
    for name in SYMBOLS:
        assert name in bound and hasattr(L, name) and re.search(r"\bint %s\(gvom_t \*h" % name, section), name
    assert len(bound["gvom_voxel_atlas_distance_field"]) == 6 and len(bound["gvom_voxel_distance_sample"]) == 6
    layout = open(os.path.join(ROOT, "g-vom_amd", "csrc", "gvom_setlayout.h")).read()
    for name in ("GVOM_PRODUCT_VOXEL_DISTANCE", "GVOM_PRODUCT_VOXEL_DISTANCE_SAMPLES"):
        assert len(re.findall(r"\b%s\b" % name, layout)) >= 2, name
    assert gvom._PRODUCT_DTYPES[40] == (np.float32, np.int32) and gvom._PRODUCT_DTYPES[42] == (np.float32, np.int32)
    makefile = open(os.path.join(ROOT, "g-vom_amd", "Makefile")).read()
    assert " gvom_voxel_distance " in makefile
    host = open(os.path.join(ROOT, "g-vom_amd", "csrc", "gvom_handle.hip")).read()
    for knob in ('"voxel_distance_field"', '"voxel_distance_mb"', '"voxel_distance_halo_xy"', '"voxel_distance_halo_z"'):
        assert knob in host, knob


# ---- the binding without a GPU -------------------------------------------------------------------------------------------------------------------
class _Lib(object):
    """stands in for the loaded library: notes every call and returns 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, [tuple(a) if isinstance(a, ctypes.Array) else a for a in args]))
            if name == "gvom_voxel_atlas_distance_field":
                args[5][0], args[5][1], args[5][2] = 4, -5, 6
                args[4]._obj.value = 7
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


def test_distance_field_refuses_bad_caps_in_python_and_passes_the_rest_on():
    g = _mapper()
    a = g.create_voxel_atlas(128, 16)
    g._lib.calls = []
    for bad in (float("nan"), float("inf"), -1.0, 0.0, 0.19, None, "far"):        # 0.19: below the finer of the two resolutions (0.2 m)
        with pytest.raises(ValueError):
            a.distance_field(bad)
    with pytest.raises(ValueError):
        a.distance_field(2.0, origin_voxels=np.array([0, 0, 0]), center=(0, 0, 0))
    with pytest.raises(ValueError):
        a.distance_field(2.0, origin_voxels=np.array([0.5, 0, 0]))
    assert g._lib.calls == []
    f = a.distance_field(0.2)                                                      # one voxel of the finer resolution: the least
    call = g._lib.named("gvom_voxel_atlas_distance_field")[-1]
    assert call[1] is None and call[2] == 0.2 and call[3] == 0
    assert isinstance(f, gvom.DeviceDistanceField) and f.origin_voxels == (4, -5, 6) and f.max_distance == 0.2 and f.product_id == 7
    f = a.distance_field(2, origin_voxels=np.array([5, -6, 1 << 40]), unknown_blocks=True)
    call = g._lib.named("gvom_voxel_atlas_distance_field")[-1]
    assert call[1] == (5, -6, 1 << 40) and call[2] == 2.0 and call[3] == gvom._DISTANCE_UNKNOWN_BLOCKS
    a.distance_field(2.0, center=(0.13, -7.07, -0.6))                              # box()'s own arithmetic
    assert g._lib.named("gvom_voxel_atlas_distance_field")[-1][1] == (-32, -50, -7)
    # sample: shapes and the limits of n
    for bad in (np.zeros((0, 3)), np.zeros((4, 2)), np.zeros(3)):
        with pytest.raises(ValueError):
            f.sample(bad)
    for n in (0, -1, (1 << 26) + 1):
        with pytest.raises(ValueError):
            f.sample_device(4096, n)
    with pytest.raises(ValueError):
        f.sample_device(0, 4)
    assert g._lib.named("gvom_voxel_distance_sample") == []
    s = f.sample(np.zeros((5, 3)))
    call = g._lib.named("gvom_voxel_distance_sample")[-1]
    assert call[1] == f.product_id and call[3] == 5 and call[4] == 0 and isinstance(s, gvom.DeviceDistanceSamples)
    f.sample_device(4096, 1 << 26)
    call = g._lib.named("gvom_voxel_distance_sample")[-1]
    assert call[3] == 1 << 26 and call[4] == 1


def test_the_halo_is_computed_in_the_arithmetic_of_the_distance():
    # resolutions that are powers of two: every product is exact, the halo of cap = k * resolution is k
    for res in (0.5, 0.25, 2.0):
        for k in (1, 2, 3, 7, 64, 65, 1000):
            cap = k * res
            assert gvom.distance_halo(cap, res) == k == vd.halo(cap, res)
            assert gvom.distance_halo(math.nextafter(cap, 0.0), res) == k - 1
            assert gvom.distance_halo(math.nextafter(cap, math.inf), res) == k
    # resolutions that round: the halo is whatever fl64(a * h*h) <= fl64(cap * cap) says, found two ways (from a root, from 0)
    for res in (0.4, 0.2, 0.3, 0.1, 0.05, 1.0 / 3.0):
        a = res * res
        for k in (1, 2, 3, 5, 10, 65, 130, 333):
            for cap in (k * res, math.nextafter(k * res, 0.0), math.nextafter(k * res, math.inf)):
                h = gvom.distance_halo(cap, res)
                assert h == vd.halo(cap, res) and a * float(h * h) <= cap * cap < a * float((h + 1) * (h + 1)), (res, k, cap)
                assert abs(h - k) <= 1
    # the caps of the GPU tests on the drive's grid, and a cap the rounding decides: 0.3 * 3 < 0.9 in float64
    # fl64(0.4 * 0.4) = 0.16000000000000003 and fl64(0.2 * 0.2) = 0.04000000000000001 lie above 0.16 and 0.04: five columns are
    # fl64(a * 25) = 4.000000000000001 > 4 = 2.0^2 away, so the halo of 2.0 m is 4 columns, not 5, and that of 26.0 m is 64, not 65
    assert [gvom.distance_halo(c, 0.4) for c in (0.4, 2.0, 26.0, 26.5)] == [1, 4, 64, 66]
    assert [gvom.distance_halo(c, 0.2) for c in (0.4, 2.0, 26.0, 26.5)] == [2, 9, 129, 132]
    assert 0.3 * 3 < 0.9 and gvom.distance_halo(0.3 * 3, 0.3) == 2 and gvom.distance_halo(0.9, 0.3) == 3 and gvom.distance_halo(1.0, 0.3) == 3
    assert [gvom.distance_halo(c, 0.2) for c in (0.3, 0.9, 1.0)] == [1, 4, 4]


# ---- 4. hand-written cases of the definition ------------------------------------------------------------------------------------------------------
def _hand(sources, never=(), origin=(0, 0, 0)):
    """a 64 x 64 x 4 extent at (0, 0, 0) whose voxels are FREE but for the given OCCUPIED and NEVER world voxels; boxes of 4 x 4 x 2"""
    ref = va.VoxelAtlasRef(64, 4, 4, 2, follow=False, origin=(0, 0, 0))
    ref.cls[:] = va.FREE
    for x, y, z in sources:
        ref.cls[z, y, x] = va.OCCUPIED
    for x, y, z in never:
        ref.cls[z, y, x] = va.NEVER
    return ref


def _both(ref, origin, cap, res, **kw):
    fast = vd.separable(ref, origin, cap, res, **kw)
    if not kw.get("unknown_blocks"):
        slow = vd.brute(ref, origin, cap, res)
        assert vd.same_bits(fast[0], slow[0]) and np.array_equal(fast[1], slow[1])
    return fast


def test_hand_written_cases_of_the_definition():
    res = (0.3, 0.2)
    a, b = 0.3 * 0.3, 0.2 * 0.2
    f32 = np.float32
    # one source, in the box's corner (10, 10, 1)
    d, counts = _both(_hand([(10, 10, 1)]), (10, 10, 1), 1.0, res)
    assert d[0, 0, 0] == 0 and d[1, 0, 0] == f32(math.sqrt(a * 1.0)) and d[0, 0, 1] == f32(math.sqrt(b * 1.0))
    assert d[1, 1, 1] == f32(math.sqrt(a * 2.0 + b * 1.0)) and d[3, 0, 0] == f32(math.sqrt(a * 9.0))
    assert d[3, 2, 0] == np.inf                             # sqrt(0.09 * 13) = 1.08 m: beyond the cap of 1 m
    assert list(counts) == [1, int(np.isfinite(d).sum()), 0, 0]
    # 0.9 is the float64 below 0.3 * 3 rounded the other way: the voxel three columns away is within 0.9 m only if fl64(a * 9) <= fl64(0.9^2)
    d, _ = _both(_hand([(10, 10, 1)]), (10, 10, 1), 0.9, res)
    assert (a * 9.0 <= 0.9 * 0.9) == bool(np.isfinite(d[3, 0, 0]))
    # two equidistant sources: one value, whichever is met first
    d, _ = _both(_hand([(10, 12, 1), (14, 12, 1)]), (10, 10, 0), 1.0, res)
    assert d[2, 2, 1] == f32(math.sqrt(a * 4.0)) and d[2, 2, 0] == f32(math.sqrt(a * 4.0 + b * 1.0))
    # a source only beyond a face of the box: (9, 11, 0) is outside the box at (10, 10, 0) and decides its near side
    ref = _hand([(9, 11, 0)])
    d, counts = _both(ref, (10, 10, 0), 1.0, res)
    assert counts[0] == 0 and d[0, 1, 0] == f32(math.sqrt(a * 1.0)) and d[1, 1, 1] == f32(math.sqrt(a * 4.0 + b * 1.0))
    assert np.isinf(vd.separable(ref, (10, 10, 0), 1.0, res, box_only=True)[0]).all()
    # no source: every voxel +inf; under the flag a NEVER voxel and everything outside the extent are sources
    ref = _hand([], never=[(11, 11, 0)])
    d, counts = _both(ref, (10, 10, 0), 1.0, res)
    assert np.isinf(d).all() and list(counts) == [0, 0, 0, 0]
    d, counts = _both(ref, (10, 10, 0), 1.0, res, unknown_blocks=True)
    assert d[1, 1, 0] == 0 and d[1, 1, 1] == f32(math.sqrt(b)) and counts[0] == 1
    d, counts = _both(ref, (62, 10, 2), 1.0, res, unknown_blocks=True)          # columns 64, 65 lie outside the extent, and level 4 above the box does
    assert not d[2:, :, :].any() and counts[2] == 2 * 4 * 2
    assert d[1, 0, 0] == f32(math.sqrt(a * 1.0)) and d[0, 0, 0] == f32(math.sqrt(b * 4.0)) and d[0, 0, 1] == f32(math.sqrt(b * 1.0))
    # the sample's voxel rule: floor of a float64 division of the float32 coordinate, NaN outside the box and for non-finite coordinates
    field = np.arange(32, dtype=np.float32).reshape(4, 4, 2)
    up, down = np.nextafter(f32(3.3), f32(9)), np.nextafter(f32(3.3), f32(0))
    pts = np.array([[3.0, 3.0, 0.2], [3.3, 3.0, 0.2], [up, 3.0, 0.2], [down, 3.0, 0.2], [3.9, 3.0, 0.39], [2.9, 3.0, 0.2], [3.0, np.nan, 0.2],
                    [np.inf, 3.0, 0.2], [3.0, 3.0, 0.6], [3.0, -3.0, 0.2]], np.float32)
    got, counts = vd.gather(field, (10, 10, 1), res, pts)
    for k in range(5):
        v = [math.floor(float(pts[k, e]) / (0.3, 0.3, 0.2)[e]) - (10, 10, 1)[e] for e in range(3)]
        assert got[k] == field[v[0], v[1], v[2]], k
    assert {math.floor(float(x) / 0.3) for x in (f32(3.3), up, down)} == {10, 11}       # the face lies between neighbouring float32 values
    assert np.isnan(got[5:]).all() and list(counts) == [5, 5, int((got[:5] == 0).sum()), 10] and counts[2] >= 1
