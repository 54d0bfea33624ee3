"""CPU side of the voxel atlas's change query (include/gvom_hip.h "voxel atlas changes"): the conditions under which the GPU tests of
tests/test_voxel_changes.py can fail, held on the C oracle alone -- the census of the hand-placed scene and of the climbing drive with the
referee of tests/voxel_changes_ref.py --, the referee on hand-written voxels, the header / binding / library agreement, what the binding
refuses before it calls the library, the set layout as a stand-alone program under sanitizers, and the kernels' resources.  No GPU.

Census of the hand-placed scene (window 64 x 64 x 8, eight boxes, ring of 2; mask 3, min_cells 2): 13 kept clusters, 7 with appeared and 7
with vanished voxels, 1 with both, 2 below min_cells, 2 across a tile border, 9 whose nearest column is not their label; 106 marked
columns, 123 appeared and 115 vanished voxels."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import gvom
import voxel_atlas_ref as va
import voxel_changes_ref as vc
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_vchange_planes", "k_vchange_codes", "k_vchange_columns", "k_vchange_clusters")


# ---- 1. the referee on hand-written voxels -----------------------------------------------------------------------------------------------
def test_codes_and_clusters_on_hand_written_voxels():
    ref = va.VoxelAtlasRef(64, 2, 4, 2, follow=False, origin=(0, 0, 0))
    FREE, OCC, NEVER = -2, 0, -1
    before = np.full((2, 4, 4), FREE, np.int32)                            # [z, y, x]
    before[0, 0, 0] = OCC; before[1, 0, 0] = OCC; before[0, 3, 3] = OCC; before[0, 1, 2] = NEVER
    ref.integrate(before.reshape(-1), (0, 0, 0))
    after = np.full((2, 4, 4), FREE, np.int32)
    after[0, 0, 0] = OCC                                                   # confirmed; the level above it vanished
    after[0, 1, 1] = OCC                                                   # appeared, next to (0, 0) by a corner
    after[0, 1, 2] = OCC                                                   # first seen: no change
    after[0, 3, 3] = NEVER                                                 # uninformative: no change
    after[1, 3, 0] = OCC                                                   # appeared, alone
    code, outside = vc.codes(ref, after.reshape(-1), (0, 0, 0))
    want = np.zeros((2, 4, 4), np.uint8)
    want[1, 0, 0] = vc.VANISHED; want[0, 1, 1] = vc.APPEARED; want[1, 3, 0] = vc.APPEARED
    assert np.array_equal(code, want) and outside == 0
    (rows, sums, cmap, counts, rows4, codes, columns), info = vc.product(ref, after.reshape(-1), (0, 0, 0), 3, 2, 4)
    assert list(counts) == [1, 3, 2, 4, 2, 1, 0, 1] and info == [1, 3, 1]
    assert list(rows[0]) == [0, 2, 0, 0, 1, 1, 5, 2] and list(sums[0]) == [1, 1] and list(rows4[0]) == [1, 1, 0, 1]   # nearest (1, 1): d2 = 2
    assert not rows[1:].any() and not rows4[1:].any() and cmap[0, 0] == 0 and cmap[1, 1] == 0 and cmap[0, 3] == vc.SMALL and (cmap == vc.NONE).sum() == 13
    assert codes.shape == (4, 4, 2) and codes[0, 0, 1] == vc.VANISHED and columns.shape == (2, 4, 4) and columns[0, 0, 3] == 1 and columns[1, 0, 0] == 1
    # mask 2: the vanished column alone, below min_cells; the levels count only masked voxels; the totals count both codes
    (rows, _, cmap, counts, rows4, _, _), info = vc.product(ref, after.reshape(-1), (0, 0, 0), 2, 1, 4)
    assert list(counts) == [1, 1, 1, 4, 2, 1, 0, 1] and list(rows4[0]) == [0, 1, 1, 1] and list(rows[0]) == [0, 1, 0, 0, 0, 0, 0, 8]
    # a window half outside the extent: outside voxels are no changes
    code, outside = vc.codes(ref, after.reshape(-1), (-2, 0, 0))
    assert outside == 16 and not code[:, :, :2].any()


# ---- 2. the census of the scene: the GPU tests can fail ------------------------------------------------------------------------------------
def test_the_hand_placed_scene_meets_its_census():
    ref, after, W = vc.oracle_scene()
    assert (ref.xy, ref.zs) == (64, 8) and len(vc.scene_scans()) == 4
    parts, info = vc.product(ref, after, W, 3, 2, 1024)
    c = vc.census(parts, info)
    print(c, list(parts[3]))
    assert c["with_appeared"] >= 3 and c["with_vanished"] >= 3 and c["with_both"] >= 1 and c["dropped"] >= 1
    assert c["across_tiles"] >= 1 and c["nearest_is_not_label"] >= 1
    assert parts[3][6] == 0 and parts[3][4] > 0 and parts[3][5] > 0
    for cap in (1, 2):                                                     # a call with max_clusters below n_kept
        small, _ = vc.product(ref, after, W, 3, 2, cap)
        assert small[3][0] == c["kept"] > cap and np.array_equal(small[0], parts[0][:cap]) and np.array_equal(small[4], parts[4][:cap])
        assert (small[2] >= cap).any()
    for mask in (1, 2):
        one, _ = vc.product(ref, after, W, mask, 2, 1024)
        assert not np.array_equal(one[2], parts[2]), mask
        assert np.array_equal(one[5], parts[5]) and np.array_equal(one[6], parts[6]) and list(one[3][4:]) == list(parts[3][4:])
    for min_cells, dropped in ((1, 0), (4, 4)):
        assert vc.product(ref, after, W, 3, min_cells, 1024)[1][2] == dropped


@pytest.mark.parametrize("follow", [True, False])
@pytest.mark.parametrize("ring", [1, 2])
def test_the_climbing_drive_has_changes_and_windows_outside_the_extent(ring, follow):
    o = oracle.OracleGvom(*(va.DRIVE_PARAMS + (ring,) + va.DRIVE_TAIL))
    ref = va.VoxelAtlasRef(va.DRIVE_A, va.DRIVE_Z, va.DRIVE_XY, va.DRIVE_ZS, follow=follow, origin=(0, 0, 0) if follow else va.fixed_origin())
    both = outside = 0
    for pc, ego in va.drive_scans():
        o.process_pointcloud(pc, ego)
        o.combine_maps()
        state, W = np.asarray(o.combined_index_map), tuple(int(v) for v in np.asarray(o.combined_origin))
        code, out = vc.codes(ref, state, W)
        E0 = ref.E
        n = ref.integrate(state, W)
        appeared, vanished = int((code == vc.APPEARED).sum()), int((code == vc.VANISHED).sum())
        if all(abs(ref.E[k] - E0[k]) < ref.sizes()[k] for k in range(3)):  # less than a whole side on every axis: the merge counts the same voxels
            assert (appeared, vanished) == (n["free_to_occupied"], n["occupied_to_free"])
        both += int(appeared > 0 and vanished > 0)
        outside += int(out > 0)
    print(ring, follow, both, outside)
    assert both >= 1 and outside >= 1


# ---- 3. header, binding, library ------------------------------------------------------------------------------------------------------------
def test_the_header_the_binding_and_the_library_agree():
    header = open(os.path.join(ROOT, "include", "gvom_hip.h")).read()
    for name, value in (("GVOM_PRODUCT_VOXEL_CHANGES", gvom.PRODUCT_VOXEL_CHANGES), ("GVOM_CHANGE_APPEARED", gvom.CHANGE_APPEARED),
                        ("GVOM_CHANGE_VANISHED", gvom.CHANGE_VANISHED)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1)) == value, name
    assert (gvom.PRODUCT_VOXEL_CHANGES, gvom.CHANGE_APPEARED, gvom.CHANGE_VANISHED) == (48, 1, 2) == (48, vc.APPEARED, vc.VANISHED)
    assert int(re.search(r"#define\s+GVOM_ABI_VERSION\s+(\d+)", header).group(1)) == 10 == gvom.ABI_VERSION          # an addition: the version stays
    section = header[header.index("--- voxel atlas changes"):header.index("--- one map sharded")]
    for word in ("CODE", "MASK", "MARKED", "CLUSTERS", "DISTANCE", "part 0", "part 6", "GVOM_NO_DATA", "GVOM_ERR_INVALID", "GVOM_ERR_CAPACITY", "NOT PROVIDED",
                 "26-connected", "level band", '"voxel_changes"', "Kind 47 is not assigned", "frontier extraction"):
        assert word in section, word
    assert re.search(r"\bint gvom_voxel_atlas_changes\(gvom_t \*h, int mask, int32_t min_cells, int32_t max_clusters, int64_t \*product_id,", section)
    bound = {n: a for n, _, a in gvom.ABI}
    I64P = ctypes.POINTER(ctypes.c_int64)
    assert bound["gvom_voxel_atlas_changes"] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_int32, I64P, I64P, I64P]
    assert hasattr(ctypes.CDLL(gvom.library_path()), "gvom_voxel_atlas_changes")
    layout = open(os.path.join(ROOT, "g-vom_amd", "csrc", "gvom_setlayout.h")).read()
    assert layout.count("GVOM_PRODUCT_VOXEL_CHANGES") >= 2
    assert gvom._PRODUCT_DTYPES[48] == vc.PART_DTYPES and gvom._PRODUCT_DTYPES[48][:3] == gvom._PRODUCT_DTYPES[gvom.PRODUCT_FRONTIERS][:3]
    makefile = open(os.path.join(ROOT, "g-vom_amd", "Makefile")).read()
    assert " gvom_voxel_changes " in makefile and "csrc/gvom_vatlas_pairs.h" in makefile
    unit = open(os.path.join(ROOT, "g-vom_amd", "csrc", "gvom_voxel_changes.hip")).read()
    for k in KERNELS:
        assert "void %s(" % k in unit, k


# ---- 4. the binding without a GPU ----------------------------------------------------------------------------------------------------------
class _Lib(object):
    """stands in for the loaded library: notes every call and returns `rc`"""

    def __init__(self):
        self.calls, self.rc = [], 0

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, [tuple(a) if isinstance(a, ctypes.Array) else a for a in args]))
            if name == "gvom_voxel_atlas_changes" and self.rc == 0:
                args[4]._obj.value = 9
                args[5][0], args[5][1], args[5][2] = -32, 7, -4
                args[6][0], args[6][1], args[6][2], args[6][3] = 3, 2, 11, 1
            if name == "gvom_device_product_export":
                args[4]._obj.value = 4096
                args[5]._obj.value = 1
            return self.rc if name == "gvom_voxel_atlas_changes" else 0
        return entry

    def named(self, name):
        return [a for n, a in self.calls if n == name]


def test_changes_refuses_bad_arguments_in_python_and_passes_the_rest_on():
    g = gvom.Gvom.__new__(gvom.Gvom)
    g._lib, g._h, g._device = _Lib(), ctypes.c_void_p(1), 0
    g.xy_size, g.xy_resolution, g.z_size, g.z_resolution = 64, 0.4, 8, 0.2
    a = g.create_voxel_atlas(128, 16)
    for kw in (dict(appeared=False, vanished=False), dict(min_cells=0), dict(min_cells=1.5), dict(min_cells="2"), dict(max_clusters=0),
               dict(max_clusters=(1 << 20) + 1), dict(max_clusters=None)):
        with pytest.raises(ValueError):
            a.changes(**kw)
    assert g._lib.named("gvom_voxel_atlas_changes") == []
    ch = a.changes()
    assert g._lib.named("gvom_voxel_atlas_changes")[-1][1:4] == [3, 2, 1024]
    assert isinstance(ch, gvom.DeviceVoxelChanges) and ch.origin_voxels == (-32, 7, -4) and ch.product_id == 9
    assert (ch.rounds, ch.n_clusters, ch.marked_columns, ch.dropped) == (3, 2, 11, 1) and gvom.DeviceVoxelChanges._dlpack_part == "codes"
    for name in ("origin_voxels", "codes", "column_counts", "cluster_map", "counts", "copy_to_host", "clusters"):
        assert hasattr(ch, name), name
    a.changes(appeared=False, min_cells=5, max_clusters=1 << 20)
    assert g._lib.named("gvom_voxel_atlas_changes")[-1][1:4] == [2, 5, 1 << 20]
    a.changes(vanished=False)
    assert g._lib.named("gvom_voxel_atlas_changes")[-1][1] == 1
    g._lib.rc = gvom.GVOM_NO_DATA
    assert a.changes() is None                                             # before the first combine
    g.__dict__.pop("_h", None)


# ---- 5. the set layout, stand-alone ----------------------------------------------------------------------------------------------------------
def test_the_voxel_changes_layout_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "voxel_changes_layout_host_test")
    src = os.path.join(ROOT, "tests", "voxel_changes_layout_host_test.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src, "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "voxel changes layout host test ok" in run.stdout


# ---- 6. the kernels' resources -----------------------------------------------------------------------------------------------------------------
def test_the_new_kernels_use_no_scratch_and_every_earlier_kernel_keeps_its_figures():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    if not os.path.exists(os.path.join(kernel_regs.LLVM, "clang-offload-bundler")):
        pytest.skip("no ROCm LLVM tools")
    every = kernel_regs.kernels(gvom.library_path())
    for k in KERNELS:
        mine = [v for name, v in every.items() if k in name]
        assert len(mine) == 1, (k, sorted(every))
        assert mine[0]["scratch"] == 0 and mine[0]["vgpr"] <= 64 and mine[0]["code"] > 0, (k, mine[0])
        assert mine[0]["lds"] == (0 if k in ("k_vchange_codes", "k_vchange_clusters") else mine[0]["lds"]) and mine[0]["lds"] <= 64, (k, mine[0])
    # profiles/voxel_changes_kernel_regs.txt: the tool's output on this library when the feature was built; every row of it still stands.
    # profiles/body_volume_kernel_regs.txt is the parent's table with the new unit's four rows behind it (tests/test_body_volume_cpu.py
    # holds it to the whole library): every row of it stands here, k_vatlas_merge and k_vatlas_box among them, whose shared lines now
    # come from csrc/gvom_vatlas_pairs.h
    names = subprocess.run(["c++filt"], input="\n".join(every).encode(), stdout=subprocess.PIPE).stdout.decode().splitlines()
    rows = sorted("%-70s vgpr %3d sgpr %3d scratch %3d lds %6d code %6d" % (nice.split("(")[0][:70], b["vgpr"], b["sgpr"], b["scratch"], b["lds"], b["code"])
                  for (raw, b), nice in zip(every.items(), names) if "vgpr" in b)
    read = lambda name: [r for r in open(os.path.join(ROOT, "profiles", name)).read().splitlines() if r and not r.startswith("#")]
    table, parent = read("voxel_changes_kernel_regs.txt"), read("body_volume_kernel_regs.txt")
    assert all(r in rows for r in table), [r for r in table if r not in rows]
    assert sorted(table) == sorted(parent), [r for r in parent if r not in table] + [r for r in table if r not in parent]
    assert sorted(r.split()[0] for r in table if r.startswith("k_vchange_")) == sorted(KERNELS)
    for k in ("k_vatlas_merge", "k_vatlas_box"):
        assert [r for r in parent if r.startswith(k + " ")] == [r for r in rows if r.startswith(k + " ")] != [], k
