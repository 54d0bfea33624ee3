"""Body clearance scoring (gvom_body_set / gvom_score_body), the part that needs no GPU: header, library and binding agree; the
referee's two forms agree on every GPU case; what the frame means (orthonormal, the contact plane, flat ground, the mirror image); the
census of every input tests/test_body.py runs; the gate scene's statement on the CPU oracle's maps; the binding's argument checks; the
product's layout under sanitizers; the kernel's registers."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import attitude_ref as ar
import body_ref as br
import body_scenes as bs
import voxel_atlas_ref as va
import voxel_distance_ref as vd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2])


def test_the_symbols_the_defines_and_the_binding():
    import gvom
    header = open(os.path.join(ROOT, "include", "gvom_hip.h")).read()
    assert gvom.load_library().gvom_abi_version() == gvom.ABI_VERSION == int(re.search(r"#define\s+GVOM_ABI_VERSION\s+(\d+)", header).group(1))
    assert re.search(r"\bint\s+gvom_body_set\s*\(", header) and re.search(r"\bint\s+gvom_score_body\s*\(", header)
    for word, value in (("GVOM_PRODUCT_BODY", gvom.PRODUCT_BODY), ("GVOM_BODY_OK", gvom.BODY_OK), ("GVOM_BODY_COLLISION", gvom.BODY_COLLISION),
                        ("GVOM_BODY_LEFT_BOX", gvom.BODY_LEFT_BOX), ("GVOM_BODY_UNKNOWN_GROUND", gvom.BODY_UNKNOWN_GROUND),
                        ("GVOM_BODY_LEFT_WINDOW", gvom.BODY_LEFT_WINDOW), ("GVOM_BODY_INVALID", gvom.BODY_INVALID)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % word, header).group(1)) == value, word
    assert gvom.PRODUCT_BODY == 44
    assert (gvom.BODY_OK, gvom.BODY_COLLISION, gvom.BODY_LEFT_BOX, gvom.BODY_UNKNOWN_GROUND, gvom.BODY_LEFT_WINDOW, gvom.BODY_INVALID) == (
        br.OK, br.COLLISION, br.LEFT_BOX, br.UNKNOWN_GROUND, br.LEFT_WINDOW, br.INVALID) == tuple(range(6))
    assert not re.search(r"#define\s+GVOM_PRODUCT_\w+\s+43\b", header) and "43 stays unassigned" in header      # kind 43 is not defined
    assert 43 not in gvom._PRODUCT_DTYPES and not [n for n in dir(gvom) if n.startswith("PRODUCT_") and getattr(gvom, n) == 43]
    L = ctypes.CDLL(gvom.library_path())
    nm = subprocess.run(["nm", "-D", "--defined-only", gvom.library_path()], capture_output=True, text=True, check=True)
    for name, nargs in (("gvom_body_set", 3), ("gvom_score_body", 14)):
        assert hasattr(L, name)
        row = [r for r in gvom.ABI if r[0] == name]
        assert len(row) == 1 and len(row[0][2]) == nargs
        assert re.search(r" T %s$" % name, nm.stdout, re.M)
    for m in ("set_body", "score_body_of", "score_body_of_device"):
        assert callable(getattr(gvom.Gvom, m))
    assert callable(gvom.DeviceDistanceField.score_body) and callable(gvom.DeviceDistanceField.score_body_of) and callable(gvom.box_spheres)
    for attr in ("copy_to_host", "release", "__enter__", "__exit__", "__dlpack__", "__dlpack_device__"):
        assert callable(getattr(gvom.DeviceBodyClearance, attr))
    assert gvom._PRODUCT_DTYPES[gvom.PRODUCT_BODY] == (np.int32, np.float32, np.uint8)
    make = open(os.path.join(ROOT, "g-vom_amd", "Makefile")).read()
    assert "gvom_body" in make and "csrc/gvom_rollouts.h" in make
    layout = open(os.path.join(ROOT, "g-vom_amd", "csrc", "gvom_setlayout.h")).read()
    assert "case GVOM_PRODUCT_BODY" in layout and "Kind 43 is not assigned" in layout


def test_the_header_carries_the_phrases_the_definition_rests_on():
    header = " ".join(open(os.path.join(ROOT, "include", "gvom_hip.h")).read().split()).replace(" * ", " ")
    a = header.index("--- body clearance scoring")
    section = header[a:header.index("--- one map sharded")]
    for phrase in ("ONE IEEE operation in the order written", "no contraction", "calls no trigonometric function",
                   "every decision is taken on the float32 values that are stored",
                   "1 <= S <= 256", "those of rollout scoring above, word for word", "terrain attitude scoring's GROUND, word for word",
                   "Only the four wheel cells are tested against the window", "lu = sqrt(1.0 + sp*sp)", "ln = sqrt((1.0 + sp*sp) + sr*sr)",
                   "(1.0/lu, 0, sp/lu)", "(-sp/ln, -sr/ln, 1.0/ln)", "(nv*e1w, nw*e1u - nu*e1w, -(nv*e1u))", "q0 = z0 - sp*am",
                   "Cu = (bx*e1u + by*e2u) + bz*nu", "Cv = by*e2v + bz*nv", "Cw = ((bx*e1w + by*e2w) + bz*nw) + q0",
                   "X = (double)x + (Cu*c - Cv*s)", "Y = (double)y + (Cu*s + Cv*c)", "|quotient| < 2^30", "the frames agree without an offset",
                   "m_i = d_i - r_i, one float32 subtraction", "A NaN m_i is skipped".lower(), "255 with clearance = +inf",
                   "clearance < min_margin, a float32 comparison", "0 where the status is INVALID, LEFT_WINDOW, UNKNOWN_GROUND or LEFT_BOX",
                   "both -1 when first_bad == 0", "Every pose is evaluated: nothing depends on scheduling", "the voxel's half diagonal",
                   "gvom_voxel_distance_sample's rule", "Kind 43 is not assigned", "does not grow in steady state at a fixed K, T and route",
                   "NOT PROVIDED: interpolation in the field; capsules or boxes; poses with their own z; suspension; sharded handles; interpolation between poses"):
        assert phrase in section or phrase in section.lower(), phrase


def test_the_two_forms_of_the_referee_agree_on_every_gpu_case():
    n = 0
    for q in br.all_cases():
        a = br.score_case(q)
        b = br.score_loops(q["field"], q["field_origin"], q["g"], q["poses"], q["body"], q["chassis"], q["cos_sin"], q["res"], q["zres"],
                           q["origin_cells"], q["min_margin"])
        assert _same(a, b), q["name"]
        n += 1
    assert n == 3 * len(br.SHAPES) + 1 + len(br.limit_cases()) + len(br.edge_cases())


def test_the_frame_is_orthonormal_and_a_point_at_height_zero_lies_on_the_contact_plane():
    rng = np.random.default_rng(12)
    sp, sr = rng.uniform(-2, 2, 5000), rng.uniform(-2, 2, 5000)
    z0, am = rng.uniform(-3, 3, 5000), 0.35
    e1u, e1w, nu, nv, nw, e2u, e2v, e2w, q0 = br.frame(sp, sr, z0, am)
    e1, e2, n = np.stack([e1u, 0 * e1u, e1w]), np.stack([e2u, e2v, e2w]), np.stack([nu, nv, nw])
    eps = np.finfo(np.float64).eps
    for a in (e1, e2, n):
        assert (np.abs((a * a).sum(axis=0) - 1.0) <= 4 * eps).all()
    for a, b in ((e1, e2), (e1, n), (e2, n)):
        assert (np.abs((a * b).sum(axis=0)) <= 4 * eps).all()
    # e2 points to the LEFT and n UP: right-handed, e1 x e2 = n
    assert (np.abs(np.cross(e1.T, e2.T).T - n) <= 4 * eps).all() and (nw > 0).all() and (e2v > 0).all()
    # a point with bz = 0 lies on the contact plane z = z0 + sp*(u - am) + sr*v, within rounding of its terms
    body = np.array([(bx, by, 0.0, 0.1) for bx in (-1.0, 0.3, 2.5) for by in (-0.8, 0.0, 0.7)], np.float32)
    Cu, Cv, Z = br.centres(0 * sp, 0 * sp, 1 + 0 * sp, 0 * sp, (e1u, e1w, nu, nv, nw, e2u, e2v, e2w, q0), body)    # heading 0 at the origin: X = Cu, Y = Cv
    plane = (z0[:, None] + sp[:, None] * (Cu - am)) + sr[:, None] * Cv
    scale = np.abs(z0)[:, None] + np.abs(sp)[:, None] * (np.abs(Cu) + am) + np.abs(sr)[:, None] * np.abs(Cv) + 1.0
    assert (np.abs(Z - plane) <= 8 * eps * scale).all()


def test_on_flat_ground_the_centres_are_the_rotated_offsets_exactly():
    xy = 33
    res, zres, zs, oc, _ = br.GRIDS[xy]
    ch, cs = ar.case_chassis(res, None), ar.cos_sin(7)
    g = np.full((xy, xy), 0.625)
    poses = br._hover_poses(xy, 5, 9, 3)
    st = br.stance(g, poses, ch, cs, res, oc)
    assert st["wheels_known"].all() and not st["sp"].any() and not st["sr"].any() and (st["z0"] == 0.625).all()
    body = br.random_body(9, res, zres, 1)
    c, s = cs[st["h"], 0], cs[st["h"], 1]
    X, Y, Z = br.centres(st["x"], st["y"], c, s, br.frame(st["sp"], st["sr"], st["z0"], 0.5 * (ch.front_axle + ch.rear_axle)), body)
    b = body.astype(np.float64)
    assert np.array_equal(X, st["x"][..., None] + (b[:, 0] * c[..., None] - b[:, 1] * s[..., None]))
    assert np.array_equal(Y, st["y"][..., None] + (b[:, 0] * s[..., None] + b[:, 1] * c[..., None]))
    assert np.array_equal(Z, np.broadcast_to(0.625 + b[:, 2], Z.shape))


def test_the_mirror_image_across_the_x_axis_mirrors_every_result():
    """ground, field, spheres' by and poses (y, yaw) mirrored across the world's x axis: the same statuses, clearances and tightest
    spheres.  A sign error in roll, e2 or v cannot hide.  The grid is symmetric about y = 0 (origin cell -n/2) and the poses keep off
    cell borders, so that floor() sees mirror images too; H = 4: the headings' cosines and sines are exact."""
    xy, zs, res, zres = 32, 8, 0.5, 0.25
    oc, B = (-7, -16), (-7, -16, -2)
    rng = np.random.default_rng(21)
    i, j = np.meshgrid(np.arange(xy, dtype=np.float64), np.arange(xy, dtype=np.float64), indexing="ij")
    g = 0.2 * np.sin(0.4 * i) + 0.15 * np.cos(0.3 * j + 0.5) + rng.uniform(0, 0.05, (xy, xy))
    field = br.random_field(xy, zs, res, zres, 8)
    ch, cs = ar.make_chassis(1.1, -0.4, 1.0, 0.2), ar.cos_sin(4)
    body = np.array([(1.2, 0.45, 0.5, 0.1), (-0.3, -0.4, 0.6, 0.2), (0.6, 0.3, 0.8, 0.05), (0.2, -0.2, 0.3, 0.0)], np.float32)
    K, T = 6, 40
    x = (rng.integers(0, 12, (K, T)) + rng.uniform(0.1, 0.9, (K, T))) * res
    y = (rng.integers(-8, 8, (K, T)) + rng.uniform(0.1, 0.9, (K, T))) * res
    yaw = rng.integers(0, 4, (K, T)) * (np.pi / 2)
    poses = np.stack([x, y, yaw], axis=2).astype(np.float32)
    a = br.score(field, B, g, poses, body, ch, cs, res, zres, oc, np.float32(0.6))
    mposes = poses * np.array([1, -1, -1], np.float32)
    mbody = body * np.array([1, -1, 1, 1], np.float32)
    b = br.score(field[:, ::-1, :], B, g[:, ::-1], mposes, mbody, ch, cs, res, zres, oc, np.float32(0.6))
    assert _same(a, b)
    assert all((a[2][..., 0] == s).sum() >= 10 for s in (br.OK, br.COLLISION)) and np.abs(br.stance(g, poses, ch, cs, res, oc)["sr"]).max() > 0.05
    wrong = br.score(field[:, ::-1, :], B, g[:, ::-1], mposes, body, ch, cs, res, zres, oc, np.float32(0.6))      # (by not mirrored: it shows)
    assert not _same(a, wrong)


def test_the_census_of_every_gpu_input():
    inputs = [(q, e) for shape in br.SHAPES for q, e in zip(br.cases(shape), br.expected(shape))]
    others = [br.nan_case()] + list(br.limit_cases()) + list(br.edge_cases())
    inputs += list(zip(others, br.expected_other()))
    assert {q["xy"] for q, _ in inputs} == set(br.GRIDS) and {len(q["body"]) for q, _ in inputs} >= set(br.SPHERES)
    assert {len(q["cos_sin"]) for q, _ in inputs} == set(br.HEADINGS) and {q["device"] for q, _ in inputs} == {True, False}
    assert {q["pattern"] for q, _ in inputs} == set(br.GROUNDS) and {q["poses"].shape[:2] for q, _ in inputs} >= set(br.SHAPES)
    assert any(min(q["field_origin"]) < 0 for q, _ in inputs) and all(tuple(q["field_origin"][:2]) != (0, 0) for q, _ in inputs)
    n = br.census(inputs)
    print(n)
    # the status list of the definition has SIX entries (the issue's census speaks of seven: terrain attitude scoring's count)
    assert all(v >= 20 for v in n["status"]), n["status"]
    assert n["ok_finite"] >= 200 and n["ok_inf"] >= 20 and n["all_skipped"] >= 1
    assert len(n["tightest"]) >= 8
    assert n["tilt_voxel"] >= 200 and n["tilt_clearance"] >= 50 and n["tilt_status"] >= 10
    assert n["free_prefix"] >= 10 and 2 * n["tightest_pose_not_0"] >= n["free_prefix"]
    assert n["first_0"] >= 5 and n["first_T"] >= 2 and n["nan_read"] == 1
    for q, (summary, clr, pairs) in zip(br.limit_cases(), br.expected_other()[1:4]):
        k, t = q["probe"]
        assert pairs[k, t, 0] == q["expect"] == (br.COLLISION if q["name"].endswith("below") else br.OK), q["name"]
    for q, (summary, clr, pairs) in zip(br.edge_cases(), br.expected_other()[4:]):
        if q["expect"] is not None:
            assert (pairs[..., 0] == q["expect"]).all(), (q["name"], pairs[..., 0])
    names = {q["name"]: e for q, e in zip(br.edge_cases(), br.expected_other()[4:])}
    assert names["sphere on the low box face"][2][0, 0, 0] == br.OK and names["sphere on the high box face"][2][0, 0, 0] == br.LEFT_BOX
    assert names["sphere on the floor and on the ceiling"][2][0, 0, 0] == br.LEFT_BOX


@pytest.mark.parametrize("name", sorted(bs.SCENES))
def test_the_scenes_statement_on_the_cpu_oracle(name):
    """the GPU test's chain on the CPU oracle's maps alone: a VoxelAtlasRef fed from the oracle, then voxel_distance_ref, then the referee"""
    import gvom
    from oracle import oracle
    S = bs.SCENES[name]
    res, zres, xy = S["res"], S["zres"], S["xy"]
    o = oracle.OracleGvom(res, zres, xy, S["zs"], 1, *va.DRIVE_TAIL)
    o.process_pointcloud(bs.cloud(name), S["ego"])
    o.combine_maps()
    W = tuple(int(v) for v in np.asarray(o.combined_origin))
    ref = va.VoxelAtlasRef(64, 16, xy, S["zs"])
    assert ref.integrate(np.asarray(o.combined_index_map), W)["outside"] == 0
    height, inferred = np.asarray(o.height_map).reshape(xy, xy), np.asarray(o.inferred_height_map).reshape(xy, xy)
    ground = ar.ground_of(height, inferred, True)
    field = vd.separable(ref, W, bs.CAP, (res, zres))[0]
    cs = gvom.heading_cos_sin(bs.HEADINGS)
    assert np.array_equal(cs, ar.cos_sin(bs.HEADINGS))
    score = lambda body, **kw: br.score(field, W, ground, bs.poses(name), body, bs.CHASSIS, cs, res, zres, W[:2], bs.MIN_MARGIN, **kw)
    seen = {k: score(b) for k, b in bs.bodies(name).items()}
    bs.hold_statement(name, seen, score(bs.bodies(name)["low"], tilt=False))


def test_box_spheres_cover_the_box():
    import gvom
    rng = np.random.default_rng(4)
    for x0, x1, hw, z0, z1, r in ((-1.0, 3.0, 0.9, 0.4, 1.8, 0.5), (-0.3, 1.5, 0.3, 0.9, 1.2, 0.15), (0.0, 0.1, 0.05, 0.0, 0.1, 1.0)):
        b = gvom.box_spheres(x0, x1, hw, z0, z1, r)
        assert b.dtype == np.float32 and b.shape[1] == 4 and 1 <= len(b) <= 256 and (b[:, 3] == np.float32(r)).all()
        p = rng.uniform((x0, -hw, z0), (x1, hw, z1), (4000, 3))
        p = np.concatenate([p, np.array([(x, y, z) for x in (x0, x1) for y in (-hw, hw) for z in (z0, z1)])])      # and the corners
        d = np.sqrt(((p[:, None, :] - b[None, :, :3].astype(np.float64)) ** 2).sum(axis=2)).min(axis=1)
        assert (d <= r * (1 + 1e-6)).all(), (d.max(), r)
        lo, hi = np.array([x0, -hw, z0]), np.array([x1, hw, z1])
        assert ((b[:, :3] - r >= lo - r - 1e-6) & (b[:, :3] + r <= hi + r + 1e-6)).all()            # the union reaches at most r beyond a face
    for bad in ((1.0, 0.0, 0.5, 0.0, 1.0, 0.2), (0.0, 1.0, 0.0, 0.0, 1.0, 0.2), (0.0, 1.0, 0.5, 0.0, 1.0, 0.0), (0.0, 10.0, 3.0, 0.0, 3.0, 0.1),
                (0.0, float("nan"), 0.5, 0.0, 1.0, 0.2)):
        with pytest.raises(ValueError):
            gvom.box_spheres(*bad)


def test_python_arguments_are_checked_before_any_library_call():
    import gvom
    g = gvom.Gvom.__new__(gvom.Gvom)              # no handle, no library: a call that got as far as the library would not raise ValueError
    g.xy_size, g.z_size, g.xy_resolution, g.z_resolution, g._lib, g._h = 16, 8, 0.4, 0.4, None, None
    ground, field, poses, B = np.zeros((16, 16)), np.zeros((16, 16, 8), np.float32), np.zeros((2, 3, 3), np.float32), np.array([0, 0, 0])
    for bad in (np.zeros((0, 4)), np.zeros((257, 4)), np.zeros((3, 3)), np.zeros(4), [[0, 0, 0, -1.0]], [[np.nan, 0, 0, 1]], np.zeros((2, 4), dtype=object)):
        with pytest.raises(ValueError, match="spheres"):
            g.set_body(bad)
    for bad, word in ((np.zeros((16, 16, 7)), "shape"), (np.zeros((16, 16)), "shape")):
        with pytest.raises(ValueError, match=word):
            g.score_body_of(bad, B, ground, poses)
    for bad in (np.zeros(2, np.int64), np.zeros(3), None):
        with pytest.raises((ValueError, TypeError)):
            g.score_body_of(field, bad, ground, poses)
    with pytest.raises(ValueError, match="shape"):
        g.score_body_of(field, B, np.zeros((16, 15)), poses)
    with pytest.raises(ValueError, match="shape"):
        g.score_body_of(field, B, ground, np.zeros((2, 3)))
    for mm in (float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="min_margin"):
            g.score_body_of(field, B, ground, poses, min_margin=mm)
    for ptrs in ((0, 1 << 20, 1 << 21), (1 << 20, 0, 1 << 21), (1 << 20, 1 << 21, None)):
        with pytest.raises(ValueError, match="device addresses"):
            g.score_body_of_device(ptrs[0], B, ptrs[1], ptrs[2], 1, 1)
    with pytest.raises(ValueError, match="4096"):
        g.score_body_of_device(1 << 20, B, 1 << 21, 1 << 22, 1, 4097)
    g.__dict__.pop("_h", None)


def test_the_body_layout_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "body_layout_host_test")
    src = os.path.join(ROOT, "tests", "body_layout_host_test.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src, "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "body layout host test ok" in run.stdout


def test_the_kernel_uses_no_scratch_and_stays_inside_its_budget():
    import gvom
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    if not os.path.exists(os.path.join(kernel_regs.LLVM, "clang-offload-bundler")):
        pytest.skip("no ROCm LLVM tools")
    every = kernel_regs.kernels(gvom.library_path())
    kernels = [v for k, v in every.items() if "k_body" in k]
    assert len(kernels) == 1, sorted(every)
    v = kernels[0]
    assert v["scratch"] == 0 and v["vgpr"] <= 128 and v["lds"] == 0 and v["code"] > 0, v       # (6 bytes per pose of dynamic LDS: <= 24,576)
    assert 4096 * 6 <= 65536
    # profiles/body_kernel_regs.txt: every earlier kernel keeps the parent's figures, k_attitude among them with its arithmetic in the shared header
    table = open(os.path.join(ROOT, "profiles", "body_kernel_regs.txt")).read()
    at = [x for k, x in every.items() if "k_attitude" in k and "ground" not in k][0]
    row = [r for r in table.splitlines() if r.startswith("k_attitude ")][0]
    assert "vgpr %3d sgpr %3d scratch %3d lds %6d code %6d" % (at["vgpr"], at["sgpr"], at["scratch"], at["lds"], at["code"]) in row, row
