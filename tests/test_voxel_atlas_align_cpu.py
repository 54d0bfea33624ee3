"""CPU side of scan alignment scoring against the voxel atlas (include/gvom_hip.h "voxel atlas alignment"): the referee of
tests/voxel_atlas_align_ref.py held to tests/align_ref.py's on a single integrate, the census of the climbing drive with the CPU referee
of the whole pipeline as the mapper, the voxels whose class only the halo decides, the header / binding / library / layout agreement, the
binding's marshalling through a recording stand-in library, and the layout of kind 38 under sanitizers.  No GPU.

Census (17 scans, window 64 x 64 x 8, following atlas 128 x 128 x 16, after the last integrate; 245 candidates, index 122 the true pose):
against the atlas box at each scan's own window origin index 122 is the best candidate for scans 4, 6, 8, 10 and 16, both dilations,
both ring lengths; the window referee picks a wrong candidate for scans 4 and 6 (58 / 42 and 133).  Scan 8 (6,701 returns) at the true
pose, dilate 0 / 1: score 373 / 435, occupied 238, near 0 / 31, free 103 / 72, unknown 894, outside 5,466.  In the window every pair of
scan 10 is OUTSIDE (245 x 2,486, best candidate 0); of scan 8, every return of 231 candidates, the true pose among them, while 14
turned candidates bring one or two returns in -- the best is candidate 0 under dilate 0 and candidate 203 with a score of 2 under
dilate 1 (tests/voxel_atlas_align_ref.py window_sees_nothing).  Halo-only voxels per box (halo_only there), rings of 1 / 2 slots: final
window 120 / 118, scan 8's window 562 / 562, scan 4's window 1,238 / 1,238, seam box 840 / 844, corner box 320 / 326, wholly outside 0."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import align_ref as ar
import gvom
import raycast_ref as rr
import voxel_atlas_align_ref as vaa
import voxel_atlas_ref as va
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_regs  # noqa: E402  (tools/kernel_regs.py)
SYMBOL = "gvom_voxel_atlas_score_alignments"


# ---- 1. one integrate: the atlas referee is the window referee -----------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["np2", "r37"])
def test_after_one_integrate_the_referee_equals_the_window_referee(grid):
    _, _, xy, zs = ar.GRIDS[grid]
    g = rr.build_map(oracle.OracleGvom, grid, 1)
    state, W = np.asarray(g.combined_index_map).copy(), tuple(int(v) for v in np.asarray(g.combined_origin))
    E = (W[0] - 9, W[1] - 3, W[2] - 1)
    ref = va.VoxelAtlasRef(64, 32, xy, zs, follow=False, origin=E)
    assert ref.integrate(state, W)["outside"] == 0
    cloud, M = ar.cloud_of(grid), ar.candidates(grid)
    for dilate in (0, 1):
        assert np.array_equal(vaa.box_classes(ref, W, dilate), ar.classes(state, grid, dilate))
        got, want = vaa.score(ref, W, grid, cloud, M, dilate), ar.score(state, W, grid, cloud, M, dilate)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (grid, dilate)
        if grid in ar.CENSUS_GRIDS:
            ar.census_holds(grid, dilate, want[0])
    assert vaa.halo_only(ref, W) == 0                                       # nothing outside the window is known yet


# ---- 2. the census of the drive -----------------------------------------------------------------------------------------------------------------
SCAN8 = {0: (373, 238, 0, 103, 894, 5466), 1: (435, 238, 31, 72, 894, 5466)}       # the true pose's row, per dilate


@pytest.mark.parametrize("ring", [1, 2])
def test_the_true_pose_wins_on_remembered_space_where_the_window_sees_nothing(ring):
    ref, Ws, state = vaa.cpu_drive(ring)
    scans = va.drive_scans()
    W = Ws[-1]
    for k in vaa.SCANS:
        pc, ego = scans[k]
        cloud = np.ascontiguousarray(pc, np.float32)
        M = vaa.drive_candidates(gvom, ego)
        for dilate in (0, 1):
            counts, best = vaa.score(ref, Ws[k], vaa.GRID, cloud, M, dilate)
            wcounts, wbest = ar.score(state, W, vaa.GRID, cloud, M, dilate)
            print(ring, k, dilate, "atlas", counts[vaa.BEST], best, "window", wcounts[vaa.BEST], wbest)
            assert best[0] == vaa.BEST and best[2] == len(cloud) and best[3] == ar.N_GRID, (ring, k, dilate, best)
            if k in (8, 10):                                               # the window sees nothing of it
                vaa.window_sees_nothing(k, dilate, wcounts, wbest, len(cloud))
            if k == 8:
                assert len(cloud) == 6701 and tuple(counts[vaa.BEST]) == SCAN8[dilate], (ring, dilate, counts[vaa.BEST])
            if k == 16:                                                     # the box is the final window: the true pose's row, bit for bit
                assert Ws[k] == W and np.array_equal(counts[vaa.BEST], wcounts[vaa.BEST]) and np.array_equal(best, wbest), (ring, dilate)


# ---- 3. the halo matters ------------------------------------------------------------------------------------------------------------------------
BOXES = ("final window", "scan 8's window", "scan 4's window", "seam box", "corner box", "wholly outside")
HALO_FOUND = {1: (120, 562, 1238, 840, 320, 0), 2: (118, 562, 1238, 844, 326, 0)}     # what the referee counts, per ring length


@pytest.mark.parametrize("box", range(6), ids=[b.replace(" ", "_").replace("'", "") for b in BOXES])
@pytest.mark.parametrize("ring", [1, 2])
def test_the_halo_decides_the_class_of_many_voxels_in_every_box(ring, box):
    """Halo-only: box voxels whose class differs between the extent-wide dilation and a dilation taken inside the box alone -- NEAR by an
    occupied voxel beyond the box's faces only, or UNKNOWN outside the extent where the box alone would spread NEAR.  The floor is 100
    per box (none in the box wholly outside the extent).  The referee counts 120 / 562 / 1,238 / 840 / 320 / 0 (ring 2: 118 / 562 /
    1,238 / 844 / 326 / 0)."""
    ref, Ws, _ = vaa.cpu_drive(ring)
    boxes = vaa.drive_boxes(ref, Ws)
    assert tuple(n for n, _ in boxes) == BOXES
    assert dict(boxes)["final window"] == (-32, -32, -8) and dict(boxes)["scan 8's window"] == (40, -68, 1) and dict(boxes)["scan 4's window"] == (4, -50, -3)
    assert dict(boxes)["corner box"] == (ref.E[0] + ref.A - 32, ref.E[1] - 32, ref.E[2] + ref.Z - 4)
    name, B = boxes[box]
    found = vaa.halo_only(ref, B)
    print(ring, name, B, found)
    assert found == HALO_FOUND[ring][box], (ring, name, found)
    if name == "wholly outside":
        assert found == 0 and (vaa.box_classes(ref, B, 1) == ar.UNKNOWN).all() and (vaa.box_classes(ref, B, 0) == ar.UNKNOWN).all()
    else:
        assert found >= vaa.HALO_FLOOR, (ring, name, found)


# ---- 4. header, binding, library, layout --------------------------------------------------------------------------------------------------------
def test_the_header_the_binding_the_library_and_the_layout_agree():
    header = open(os.path.join(ROOT, "include", "gvom_hip.h")).read()
    assert int(re.search(r"#define\s+GVOM_PRODUCT_VOXEL_ATLAS_ALIGNMENT\s+(\d+)", header).group(1)) == 38 == gvom.PRODUCT_VOXEL_ATLAS_ALIGNMENT
    assert not re.search(r"#define\s+GVOM_PRODUCT_\w+\s+37\b", header)
    assert int(re.search(r"#define\s+GVOM_ABI_VERSION\s+(\d+)", header).group(1)) == 10 == gvom.ABI_VERSION          # an addition: the version stays
    section = header[header.index("--- voxel atlas alignment"):header.index("--- one map sharded")]
    assert header.index("--- voxel atlas alignment") > header.index("--- voxel atlas ")
    for word in ("DEFINITION", "window := the BOX", "class of a voxel := a function of the ATLAS alone", "OF THE EXTENT", "CONSEQUENCES", "bit for bit",
                 "read-only on the atlas", "no host wait", "GVOM_NO_DATA", "GVOM_ERR_INVALID", "GVOM_ERR_CAPACITY", "NOT PROVIDED", "Kind 37 is not assigned",
                 '"voxel_atlas_alignments"'):
        assert word in section, word
    atlas = header[header.index("--- voxel atlas"):header.index("--- voxel atlas alignment")]
    assert "alignment scoring against the atlas" not in atlas              # no longer among what is not provided
    assert re.search(r"\bint %s\(gvom_t \*h, const float \*cloud" % SYMBOL, section)
    bound = {n: a for n, _, a in gvom.ABI}
    assert len(bound[SYMBOL]) == len(bound["gvom_score_alignments"]) + 2   # + origin, origin_out
    assert hasattr(ctypes.CDLL(gvom.library_path()), SYMBOL)
    layout = open(os.path.join(ROOT, "g-vom_amd", "csrc", "gvom_setlayout.h")).read()
    assert layout.count("GVOM_PRODUCT_VOXEL_ATLAS_ALIGNMENT") >= 2 and "Kind 37 is not assigned" in layout
    assert gvom._PRODUCT_DTYPES[38] == gvom._PRODUCT_DTYPES[gvom.PRODUCT_ALIGNMENT] == (np.int32, np.int32) and 37 not in gvom._PRODUCT_DTYPES
    assert issubclass(gvom.DeviceAtlasAlignments, gvom.DeviceAlignments)


# ---- 5. the binding without a GPU ---------------------------------------------------------------------------------------------------------------
class _Lib(object):
    """stands in for the loaded library: notes every call and returns `rc` from the entry point under test, 0 from the others"""

    def __init__(self):
        self.calls, self.rc = [], 0

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, [tuple(a) if isinstance(a, ctypes.Array) else a for a in args]))
            if name == "gvom_get_state":
                st = args[1]._obj
                st.has_combined = 1
                st.combined_origin[0], st.combined_origin[1], st.combined_origin[2] = -32.0, 7.0, -4.0
            if name == SYMBOL:
                if self.rc:
                    return self.rc
                args[9][0], args[9][1], args[9][2] = 4, -5, 6
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


def test_score_alignments_marshals_origin_centre_and_the_device_route():
    g = _mapper()
    a = g.create_voxel_atlas(128, 16)
    cloud, M = np.zeros((7, 3), np.float32), np.tile(np.identity(4), (3, 1, 1))
    r = a.score_alignments(cloud, M)
    call = g._lib.named(SYMBOL)[-1]
    assert call[2] == 7 and call[4] == 3 and call[5] == 0 and call[6] == 0 and call[7] == gvom.ALIGN_DEFAULT_WEIGHTS and call[8] is None
    assert isinstance(r, gvom.DeviceAtlasAlignments) and r.origin_voxels == (4, -5, 6) and list(r.origin) == [4.0, -5.0, 6.0]
    a.score_alignments(cloud, M, dilate=1, weights=(3, 2, -2, 0, -1), origin_voxels=np.array([5, -6, 1 << 40]))     # any integer origin, as box()
    call = g._lib.named(SYMBOL)[-1]
    assert call[6] == 1 and call[7] == (3, 2, -2, 0, -1) and call[8] == (5, -6, 1 << 40)
    a.score_alignments(cloud, M, center=(0.13, -7.07, -0.6))               # floor(c / resolution - size / 2), as box(center=...)
    a.box(center=(0.13, -7.07, -0.6))
    assert g._lib.named(SYMBOL)[-1][8] == (-32, -50, -7) == g._lib.named("gvom_voxel_atlas_box")[-1][1]
    n = len(g._lib.named(SYMBOL))
    for kw in (dict(origin_voxels=np.array([0, 0, 0]), center=(0, 0, 0)), dict(center=(0, 0)), dict(center=(0, np.nan, 0)), dict(origin_voxels=np.array([0, 0])),
               dict(origin_voxels=(0.5, 0, 0)), dict(dilate=2), dict(weights=(1, 2, 3)), dict(weights=(2000, 0, 0, 0, 0))):
        with pytest.raises(ValueError):
            a.score_alignments(cloud, M, **kw)
    with pytest.raises(TypeError):
        a.score_alignments(cloud.astype(np.float64), M)
    with pytest.raises(TypeError):
        a.score_alignments(cloud, M.astype(np.float32))
    with pytest.raises(ValueError):
        a.score_alignments(np.zeros((7, 2), np.float32), M)
    with pytest.raises(ValueError):
        a.score_alignments_device(0, 7, 4096, 3)
    with pytest.raises(ValueError):
        a.score_alignments_device(4096, 0, 8192, 3)
    assert len(g._lib.named(SYMBOL)) == n                                   # refused before the library was called
    r = a.score_alignments_device(4096, 7, 8192, 3, dilate=1, origin_voxels=np.array([1, 2, 3]))
    call = g._lib.named(SYMBOL)[-1]
    assert call[1].value == 4096 and call[3].value == 8192 and call[2] == 7 and call[4] == 3 and call[5] == 1 and call[6] == 1 and call[8] == (1, 2, 3)
    assert isinstance(r, gvom.DeviceAtlasAlignments)
    g._lib.rc = gvom.GVOM_NO_DATA                                          # before the first combine, or the first integrate: None
    assert a.score_alignments(cloud, M) is None and a.score_alignments_device(4096, 7, 8192, 3) is None


# ---- 6. the layout of kind 38 under sanitizers --------------------------------------------------------------------------------------------------
def test_the_atlas_alignment_layout_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "voxel_atlas_align_layout_host_test")
    src = os.path.join(ROOT, "tests", "voxel_atlas_align_layout_host_test.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src, "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "voxel atlas alignment layout host test ok" in run.stdout


def test_the_new_kernel_uses_no_scratch():
    if not os.path.exists(os.path.join(kernel_regs.LLVM, "clang-offload-bundler")):
        pytest.skip("no ROCm LLVM tools")
    found = {k: v for k, v in kernel_regs.kernels(gvom.library_path()).items() if "k_vatlas_align_field" in k}
    assert len(found) == 1
    for k, v in found.items():
        assert v["scratch"] == 0 and v["lds"] == 0 and v["vgpr"] <= 64 and v["code"] > 0, (k, v)     # (its LDS is dynamic: sized at launch)
