"""Viewpoint scoring (gvom_score_viewpoints), the part that needs no GPU: header, library and binding agree; the referee's two forms
agree; the census of every input tests/test_viewpoints.py runs, with floors, on maps built by the CPU oracle; what the two binding
entry points hand to the library; viewpoint_poses(); the product's layout under sanitizers; the kernels' resources."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import raycast_ref as rr
import viewpoint_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbol_the_defines_and_the_binding():
    import gvom
    header = open(os.path.join(ROOT, "include", "gvom_hip.h")).read()
    assert int(re.search(r"#define\s+GVOM_ABI_VERSION\s+(\d+)", header).group(1)) == 10 == gvom.ABI_VERSION
    assert int(re.search(r"#define\s+GVOM_PRODUCT_VIEWPOINTS\s+(\d+)", header).group(1)) == gvom.PRODUCT_VIEWPOINTS == 18
    assert not re.search(r"#define\s+GVOM_PRODUCT_\w+\s+(8|9|11|13|15|17)\b", header)    # 17 stays unassigned (tests/frontier_layout_host_test.cpp)
    assert re.search(r"\bint\s+gvom_score_viewpoints\s*\(", header)
    text = header[header.index("viewpoint scoring"):]
    for word in ("per-beam results", "per-beam origin", "range weighting", "2-D cell gain", "sharded handles", "viewpoint_bitmap_mb", "DISTINCT"):
        assert word in text, word                               # the definition and NOT PROVIDED, said in the header
    codes = [int(re.search(r"#define\s+GVOM_RAY_%s\s+(\d+)" % n, header).group(1)) for n in ("CLEAR", "OCCUPIED", "UNKNOWN", "LEFT_WINDOW", "INVALID")]
    assert codes == [rr.CLEAR, rr.OCCUPIED, rr.UNKNOWN, rr.LEFT_WINDOW, rr.INVALID] == [gvom.RAY_CLEAR, gvom.RAY_OCCUPIED, gvom.RAY_UNKNOWN, gvom.RAY_LEFT_WINDOW, gvom.RAY_INVALID]
    nm = subprocess.run(["nm", "-D", "--defined-only", gvom.library_path()], capture_output=True, text=True, check=True)
    assert re.search(r" T gvom_score_viewpoints$", nm.stdout, re.M) and hasattr(ctypes.CDLL(gvom.library_path()), "gvom_score_viewpoints")
    row = [r for r in gvom.ABI if r[0] == "gvom_score_viewpoints"]
    assert len(row) == 1 and len(row[0][2]) == 10 and row[0][2][4] is ctypes.c_double
    assert gvom._PRODUCT_DTYPES[gvom.PRODUCT_VIEWPOINTS] == (np.int32, np.int32)
    assert (gvom.VIEWPOINT_MAX_POSES, gvom.VIEWPOINT_MAX_BEAMS) == (65536, 1 << 22)
    for m in ("score_viewpoints", "score_viewpoints_device"):
        assert callable(getattr(gvom.Gvom, m))
    for attr in ("copy_to_host", "best_pose", "release", "__enter__", "__exit__"):
        assert callable(getattr(gvom.DeviceViewpoints, attr))
    assert callable(gvom.viewpoint_poses)
    assert "gvom_viewpoint" in open(os.path.join(ROOT, "g-vom_amd", "Makefile")).read()


@pytest.fixture(scope="module")
def oracle_maps():
    """(dense fused state, window origin) of the CPU oracle after the four scans, per (grid, ring slots): built on first use"""
    from oracle import oracle
    built = {}

    def get(grid, bs):
        if (grid, bs) not in built:
            o = rr.build_map(oracle.OracleGvom, grid, bs)
            built[grid, bs] = (np.asarray(o.combined_index_map), np.asarray(o.combined_origin, np.float64))
        return built[grid, bs]
    return get


def test_the_two_referee_forms_agree(oracle_maps):
    for case in vr.CASES:
        grid, bs, name, strides, K, rng, ub = case
        if grid in ("w128", "v256") and K > 3:                 # the small cases only: the second form goes voxel by voxel
            continue
        state, W = oracle_maps(grid, bs)
        d, o, poses, r = vr.case_inputs(case, state, W)
        a, b = vr.product(state, W, grid, d, o, poses, r, strides, ub), vr.product_sets(state, W, grid, d, o, poses, r, strides, ub)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), vr.case_id(case)
        assert a[0].dtype == np.int32 and a[1].dtype == np.int32 and a[0].shape == (K, 8) and a[1].shape == (4,)
    # by hand: a 4 x 4 x 4 window that nobody has observed but for one occupied voxel; two beams along +x from the middle of voxel
    # (0, 1, 1), the same beam twice: each examines voxels x = 1, 2 (S = 2 of a 3.5-voxel ray; the third is the occupied one and is not
    # reached), so visits = 4 and gain = 2
    rr.GRIDS.setdefault("hand4", (1.0, 1.0, 4, 4))
    state = np.full(64, -1, np.int64)
    state[3 + 1 * 4 + 1 * 16] = 0
    d = np.array([[[1.0, 0.0, 0.0], [1.0, 0.0, 0.0]]])
    pose = vr.pose_of((0.5, 1.5, 1.5))
    rows, best = vr.product(state, np.zeros(3), "hand4", d, None, pose, 3.0)
    assert rows.tolist() == [[rr.UNKNOWN, 2, 4, 0, 2, 0, 0, 0]] and best.tolist() == [-1, 0, 1, 2]
    rows, best = vr.product(state, np.zeros(3), "hand4", d, None, pose, 4.0)       # S = 3: both beams reach the occupied voxel
    assert rows.tolist() == [[rr.UNKNOWN, 2, 4, 2, 0, 0, 0, 0]]
    rows, best = vr.product(state, np.zeros(3), "hand4", d, None, pose, 4.0, unknown_blocks=True)
    assert rows.tolist() == [[rr.UNKNOWN, 1, 2, 0, 0, 0, 2, 0]]
    state[0 + 1 * 4 + 1 * 16] = -2                              # the origin's voxel observed free: the row can be the best
    rows, best = vr.product(state, np.zeros(3), "hand4", d, None, np.stack([pose, pose]), 9.0)
    assert rows.tolist() == [[rr.CLEAR, 2, 4, 2, 0, 0, 0, 0]] * 2 and best.tolist() == [0, 2, 2, 2]


@pytest.mark.parametrize("case", vr.CASES, ids=vr.case_id)
def test_census_of_every_gpu_input(oracle_maps, case):
    """Floors: conditions on the inputs, shown by the referee alone on the oracle's maps.  Without a viewpoint with visits > gain a
    kernel that does not deduplicate would pass; without a voxel shared by beams of different model rows (different waves) one that
    deduplicates within a wave only would.  Measured when written (endings = beams OCCUPIED, CLEAR, LEFT_WINDOW, UNKNOWN, INVALID over
    the 33 viewpoints): p2 count [8487, 842, 7055, 0, 512], 31 viewpoints with visits > gain, 539 voxels shared across rows; far
    count [462, 5117, 341, 0, 185], 2 and 5 -- out there a float32 voxel coordinate has a spacing of 2 and most steps do not move."""
    grid, bs, name, strides, K, rng, ub = case
    state, W = oracle_maps(grid, bs)
    c = vr.census(case, state, W)
    print(vr.case_id(case), {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in c.items() if k != "rows"})
    rows, nb = c["rows"], c["best"][3]
    assert (rows[:, 3:].sum(axis=1) == nb).all() and (rows[:, 1] <= rows[:, 2]).all()
    occ, clear, left, unknown, invalid = c["endings"]
    if vr.has_floors(case):
        assert c["gainful"] >= 1 and c["dedup"] >= 1 and c["shared_across_rows"] >= 1
        assert occ >= 1 and clear >= 1 and left >= 1 and (unknown >= 1) == ub
        if K == 33:
            assert c["statuses"] == [rr.CLEAR, rr.OCCUPIED, rr.UNKNOWN, rr.LEFT_WINDOW, rr.INVALID]     # every origin status
            assert rows[16].tolist() == [rr.INVALID, 0, 0, 0, 0, 0, 0, nb] and np.array_equal(rows[1], rows[2])
            assert c["best"][0] >= 0
    elif rng == "short":
        assert clear == K * nb and c["gainful"] == 0 and not rows[:, 1:4].any()
    else:
        assert left >= 1 and clear == 0 and c["gainful"] >= 1
    if name == "nan8x64":
        assert invalid >= 4 * (K - (K == 33))                   # the model's four bad pixels, in every valid viewpoint


class _Recorder(object):
    """stands in for the loaded library: notes gvom_score_viewpoints' arguments, the poses read through their pointer at call time"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            if name == "gvom_score_viewpoints":
                got = list(args)
                p = got[1].value if isinstance(got[1], ctypes.c_void_p) else got[1]
                got[1] = p if got[3] else tuple((ctypes.c_double * (12 * got[2])).from_address(p))
                self.calls.append(got)
                for k, v in enumerate((5.0, -6.0, 7.0)):
                    args[8][k] = v
                args[9]._obj.value = 9
            elif name == "gvom_device_product_export":
                args[4]._obj.value = 4096
            return 0
        return entry


def test_what_the_two_entry_points_hand_to_the_library():
    import gvom
    g = gvom.Gvom.__new__(gvom.Gvom)
    g._lib, g._h = _Recorder(), None
    poses = np.arange(3 * 16, dtype=np.float64).reshape(3, 4, 4) * 0.5
    v = g.score_viewpoints(poses, 12.5, beam_stride=(2, 4), unknown_blocks=True)
    a = g._lib.calls[0]
    assert a[1] == tuple(poses[:, :3, :].reshape(-1)) and a[2:8] == [3, 0, 12.5, 2, 4, 1]       # [K, 4, 4] -> [K][12], rows 0..2
    assert v.product_id == 9 and v.origin.tolist() == [5.0, -6.0, 7.0]
    g.score_viewpoints(np.asfortranarray(poses[:, :3, :]), 3)
    g.score_viewpoints(poses[1], 3.0)
    g.score_viewpoints(poses[2, :3], np.float32(3.0))
    a, b, c = g._lib.calls[1:4]
    assert a[1] == tuple(poses[:, :3, :].reshape(-1)) and a[2:8] == [3, 0, 3.0, 1, 1, 0]
    assert b[1] == tuple(poses[1, :3].reshape(-1)) and b[2] == 1 and c[1] == tuple(poses[2, :3].reshape(-1)) and c[2] == 1
    g.score_viewpoints_device(1 << 20, 7, 2.0, beam_stride=[3, 1])
    assert g._lib.calls[4][1:8] == [1 << 20, 7, 1, 2.0, 3, 1, 0]
    n = len(g._lib.calls)
    for bad, word in ((dict(max_range=0.0), "max_range"), (dict(max_range=float("inf")), "max_range"), (dict(max_range=None), "max_range"),
                      (dict(beam_stride=(0, 1)), "beam_stride"), (dict(beam_stride=(1, 2, 3)), "beam_stride"), (dict(beam_stride=(1, 2.5)), "beam_stride")):
        with pytest.raises(ValueError, match=word):
            g.score_viewpoints(poses, **dict(dict(max_range=2.0), **bad))
    for p, err, word in ((poses.astype(np.float32), TypeError, "float64"), (poses[:, :2], ValueError, "shape"), (poses[:0], ValueError, "shape"),
                         (np.zeros((2, 2, 4, 4)), ValueError, "shape")):
        with pytest.raises(err, match=word):
            g.score_viewpoints(p, 2.0)
    for args, word in (((0, 3, 2.0), "device address"), ((1 << 20, 0, 2.0), "poses"), ((1 << 20, 65537, 2.0), "65536"), ((1 << 20, 2.5, 2.0), "poses")):
        with pytest.raises(ValueError, match=word):
            g.score_viewpoints_device(*args)
    assert len(g._lib.calls) == n                              # nothing of that reached the library
    # best_pose(): the row of the matrices handed over; None on the device route and where no pose is in free space

    class _Part(object):
        def __init__(self, a):
            self.a = a

        def copy_to_host(self):
            return self.a
    v.best = _Part(np.array([2, 41, 3, 8], np.int32))
    k, gain, pose = v.best_pose()
    assert (k, gain) == (2, 41) and np.array_equal(pose, poses[2, :3])
    v.best = _Part(np.array([-1, 0, 3, 8], np.int32))
    assert v.best_pose() is None
    for obj in (g, v._hold):
        for a in ("_h", "_held"):
            obj.__dict__.pop(a, None)                          # (nothing for __del__ to release)


def test_viewpoint_poses_builds_the_documented_grid():
    import gvom
    pts = np.array([[1.0, 2.0, 3.0], [-4.0, 5.5, 0.25]])
    yaws = [0.0, 0.7, -2.0]
    P = gvom.viewpoint_poses(pts, yaws)
    assert P.shape == (6, 4, 4) and P.dtype == np.float64
    for i in range(2):
        for j in range(3):
            assert np.array_equal(P[i * 3 + j], vr.pose_of(pts[i], yaws[j])), (i, j)    # yaw fastest
    S = vr.pose_of((0.2, -0.1, 0.9), 0.3, -0.2)
    Q = gvom.viewpoint_poses(pts, yaws, sensor_to_body=S)
    for k in range(6):
        assert np.array_equal(Q[k], P[k].dot(S))
    assert gvom.viewpoint_poses([1.0, 2.0, 3.0], 0.5).shape == (1, 4, 4)
    for args, word in ((([[1.0, 2.0]], [0.0]), "points_xyz"), ((pts, [0.0], np.identity(3)), "sensor_to_body"), ((np.zeros((300, 3)), np.zeros(300)), "65536")):
        with pytest.raises(ValueError, match=word):
            gvom.viewpoint_poses(*args)


def test_the_viewpoint_layout_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "viewpoint_layout_host_test")
    src = os.path.join(ROOT, "tests", "viewpoint_layout_host_test.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src, "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "viewpoint layout host test ok" in run.stdout


def test_the_kernels_use_no_scratch_and_the_ray_query_next_door_is_what_it_was():
    import gvom
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    if not os.path.exists(os.path.join(kernel_regs.LLVM, "clang-offload-bundler")):
        pytest.skip("no ROCm LLVM tools")
    every = kernel_regs.kernels(gvom.library_path())
    kernels = {k: v for k, v in every.items() if "k_viewpoint" in k}
    assert sorted(re.search(r"\d+(k_viewpoint[a-z_]+?)ILb", k).group(1) for k in kernels) == ["k_viewpoint_best"] * 2 + ["k_viewpoints"] * 2
    for k, v in kernels.items():
        assert v["scratch"] == 0 and v["vgpr"] <= 64 and v["code"] > 0, (k, v)
        assert v["lds"] == (32 if "best" in k else 0), (k, v)
    # k_raycast, whose lookup moved into the header both units include (csrc/gvom_raywalk.h): no scratch, no LDS and no more than the
    # 61 VGPRs it had before the move.  (Kernel for kernel, parent against new, register for register and byte for byte -- all 94
    # unchanged --: the "resources" of profiles/viewpoints_*.json, written by tools/viewpoint_bench.py --resources.  Exact figures
    # are not pinned here: a later change to k_raycast is not this test's business.)
    ray = {k: v for k, v in every.items() if "k_raycast" in k}
    assert len(ray) == 2
    for k, v in ray.items():
        assert v["scratch"] == 0 and v["lds"] == 0 and v["vgpr"] <= 61, (k, v)
