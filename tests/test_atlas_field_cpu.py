"""Atlas fields without a GPU: the constants of header and binding, the layouts under sanitizers (a stand-alone program), what the
binding refuses and hands over (a Gvom made with __new__ whose `_lib` notes the calls), the cell rule on hand-written values, the
census of every input tests/test_atlas_field.py gives the GPU -- with the toroidal twin of tests/atlas_field_ref.py as the witness
that a kernel which forgot the seam would be caught --, and the drive's outward leg with the maps of the CPU oracle."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import atlas_field_ref as afr
import atlas_ref as ar
import costfield_ref as cf
import frontier_ref as fr
import gvom
import rollouts_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = cf.UNREACHED


def test_the_header_and_the_binding_agree():
    header = open(os.path.join(ROOT, "include", "gvom_hip.h")).read()
    assert int(re.search(r"#define\s+GVOM_PRODUCT_ATLAS_FIELD\s+(\d+)", header).group(1)) == gvom.PRODUCT_ATLAS_FIELD == 26
    assert int(re.search(r"#define\s+GVOM_ABI_VERSION\s+(\d+)", header).group(1)) == 10 == gvom.ABI_VERSION      # additions: the version stays
    section = header[header.index("--- atlas fields"):header.index("--- one map sharded")]
    for word in ("DEFINITION", "MAP", "HARD", "COST", "FIELD, DIRECTION", "SNAPSHOT", "GVOM_ERR_INVALID", "GVOM_ERR_CAPACITY", "NOT PROVIDED",
                 "visibility <= 0", "max(1,", "NaN roughness", "NOT neighbours", "atlas_cost_to_go", "atlas_field_allocations", "point out of the window"):
        assert word in section, word
    for decl in ("int gvom_atlas_cost_to_go(gvom_t *h, const gvom_ctg_params *params, const int64_t *goals",
                 "int gvom_atlas_field_window(gvom_t *h, int64_t field_id, int64_t map_set_id, const int64_t origin_cells[2], int64_t *product_id);"):
        assert decl in section, decl
    bound = {n: a for n, _, a in gvom.ABI}
    assert len(bound["gvom_atlas_cost_to_go"]) == 10 and len(bound["gvom_atlas_field_window"]) == 5
    layout = open(os.path.join(ROOT, "g-vom_amd", "csrc", "gvom_setlayout.h")).read()
    assert layout.count("GVOM_PRODUCT_ATLAS_FIELD") >= 2
    assert gvom._PRODUCT_DTYPES[26] == (np.int32, np.uint8, np.uint16) == gvom._PRODUCT_DTYPES[gvom.PRODUCT_COSTFIELD]
    assert issubclass(gvom.DeviceAtlasFieldWindow, gvom.DeviceCostField)


def test_the_layouts_under_sanitizers(tmp_path):
    """kinds 26 and 7 at small, odd and the largest shapes, and the crop's addressing, in a program of its own"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "atlas_field_layout_host_test")
    src = os.path.join(ROOT, "tests", "atlas_field_layout_host_test.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", src, "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "atlas field layout host test ok" in run.stdout


# ---- the binding without a GPU -------------------------------------------------------------------------------------------------------------
XY = 6


class _Lib(object):
    """stands in for the loaded library: notes every call (pointed-to goals and origins read at call time), fills the outputs a
    binding reads, returns 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            got = list(args)
            if name == "gvom_atlas_cost_to_go":
                p = got[1]._obj
                got[1] = (p.density_threshold, p.inflation_cells2, p.base, p.soft_weight, p.unknown_cost, p.rough_weight)
                got[2] = [int(got[2][k]) for k in range(2 * got[3])]
                args[7]._obj.value = 21
                for k, v in enumerate((1, 9, 100, 1)):
                    args[8][k] = v
                args[9][0], args[9][1] = -40, 3
            if name == "gvom_atlas_field_window":
                args[4]._obj.value = 22
            for k, a in enumerate(got):
                if isinstance(a, ctypes.Array):
                    got[k] = tuple(a)
            self.calls.append((name, got))
            if name == "gvom_device_map_origin":
                args[2][0], args[2][1], args[2][2] = 5, -6, 7
            if name == "gvom_device_product_export":
                args[4]._obj.value, args[5]._obj.value = 4096, 2
                for k in range(2):
                    args[6][k], args[7][k] = 64, (1, 64)[k]
            return 0
        return entry

    def named(self, name):
        return [a for n, a in self.calls if n == name]


def _mapper():
    g = gvom.Gvom.__new__(gvom.Gvom)
    g._lib, g._h, g._device = _Lib(), ctypes.c_void_p(1), 0
    g.xy_size, g.xy_resolution = XY, 0.5
    return g


def test_cost_to_go_refuses_what_the_library_would_and_hands_the_rest_over():
    g = _mapper()
    a = g.create_atlas(64, follow=False, origin_cells=(-40, 3))
    for bad in ([(0, 0, 0)], np.zeros((0, 2)), [("a", "b")], [(np.nan, 0.0)], np.zeros((65537, 2))):
        with pytest.raises(ValueError):
            a.cost_to_go(bad)
    with pytest.raises(ValueError, match="whole numbers"):
        a.cost_to_go([(0.5, 4.0)], goals_in_cells=True)
    for out in ((-41, 3), (24, 3), (-40, 2), (-40, 67)):              # one cell beyond each edge of [-40, 24) x [3, 67)
        with pytest.raises(ValueError, match=r"outside the extent: cell \(%d, %d\), extent \[-40, 24\) x \[3, 67\)" % out):
            a.cost_to_go([(0, 10), out], goals_in_cells=True)
    with pytest.raises(ValueError, match="outside the extent"):
        a.cost_to_go([(12.0, 5.0)])                                     # metres: cell (24, 10)
    for kw in (dict(inflation_radius=-1.0), dict(inflation_radius=0.1), dict(density_threshold=float("nan")), dict(unknown="maybe"), dict(unknown=65536),
               dict(base=0), dict(soft_weight=-1), dict(rough_weight=3), dict(rough_weight=3, roughness_range=(1.0, 1.0)), dict(max_cost=0),
               dict(max_cost=2 ** 30 + 1), dict(max_rounds=-1), dict(max_rounds=1.5)):
        with pytest.raises(ValueError):
            a.cost_to_go([(0, 10)], goals_in_cells=True, **kw)
    assert g._lib.named("gvom_atlas_cost_to_go") == []
    f = a.cost_to_go([(11.99, 1.5), (-20.0, 33.49)], inflation_radius=1.0, unknown=7, soft_weight=2, include_negative=False, max_cost=500, max_rounds=3)
    (h, params, goals, n, max_cost, max_rounds, flags, _, _, _), = g._lib.named("gvom_atlas_cost_to_go")
    assert params == (50.0, 4, 1, 2, 7, 0) and goals == [23, 3, -40, 66] and (n, max_cost, max_rounds, flags) == (2, 500, 3, 1)
    assert isinstance(f, gvom.DeviceAtlasField) and f.product_id == 21 and f.origin_cells == (-40, 3) and np.array_equal(f.origin, (-20.0, 1.5))
    assert (f.converged, f.rounds, f.reached, f.goals_seeded) == (True, 9, 100, 1) and f.cost.shape == (64, 64) and f.cost.strides == (1, 64)
    assert (f.cost.dtype, f.direction.dtype, f.cell_cost.dtype) == (np.int32, np.uint8, np.uint16)
    a.cost_to_go([(0, 10)], goals_in_cells=True, unknown="blocked")
    assert g._lib.named("gvom_atlas_cost_to_go")[1][6] == 2 and g._lib.named("gvom_atlas_cost_to_go")[1][2] == [0, 10]
    # window(): one of the two, checked here
    with pytest.raises(ValueError):
        f.window()
    with pytest.raises(ValueError):
        f.window(object())
    for bad in ((1.5, 2.0), (1, 2, 3), (1 << 41, 0)):
        with pytest.raises(ValueError):
            f.window(origin_cells=bad)
    assert g._lib.named("gvom_atlas_field_window") == []
    w = f.window(origin_cells=(-3, 8))
    assert g._lib.named("gvom_atlas_field_window")[0][1:4] == [21, -1, (-3, 8)]
    assert isinstance(w, gvom.DeviceCostField) and w.product_id == 22 and w.origin_cells == (-3, 8) and np.array_equal(w.origin, (-1.5, 4.0))
    assert (w.converged, w.rounds, w.reached, w.goals_seeded) == (True, 9, 100, 1)
    m = gvom.DeviceMaps(g, 11, np.array([2.5, -3.0, 1.4]))
    with pytest.raises(ValueError):
        f.window(m, origin_cells=(0, 0))
    w = f.window(m)
    assert g._lib.named("gvom_atlas_field_window")[1][1:4] == [21, 11, None] and w.origin_cells == (5, -6) and np.array_equal(w.origin, m.origin)


def test_paths_walk_world_cells_and_stop_at_the_windows_border():
    g = _mapper()
    a = g.create_atlas(64, follow=False, origin_cells=(-40, 3))
    f = a.cost_to_go([(0, 10)], goals_in_cells=True)
    d = np.full((64, 64), gvom.CTG_NONE, np.uint8)
    d[10, 5], d[11, 5], d[12, 5], d[12, 4] = gvom.CTG_GOAL, 4, 4, 2          # (12, 4) -> up -> (12, 5) -> left twice -> the goal
    d[20, 20] = gvom.CTG_UNSETTLED
    d[63, 7] = 0                                                            # a step out of the field: not in a final field
    f._host = d
    assert f.path_from((-28, 7)) == [(-28, 7), (-28, 8), (-29, 8), (-30, 8)] and f.path_from((0, 3)) is None
    with pytest.raises(RuntimeError, match="unsettled"):
        f.path_from((-20, 23))
    with pytest.raises(RuntimeError, match="out of the field"):
        f.path_from((23, 10))
    for out in ((-41, 3), (24, 3), (0, 67)):
        with pytest.raises(ValueError, match="outside the field"):
            f.path_from(out)
    w = f.window(origin_cells=(-29, 7))                                     # field cells (11 .., 4 ..): the goal lies outside it
    w._host = d[11:11 + XY, 4:4 + XY]
    assert w.path_from((1, 0)) == [(1, 0), (1, 1), (0, 1)]                  # ends at the last cell before the step that leaves
    assert w.path_from((3, 3)) is None
    with pytest.raises(ValueError, match="outside the window"):
        w.path_from((XY, 0))
    w._host = d[10:10 + XY, 4:4 + XY]
    assert w.path_from((2, 0)) == [(2, 0), (2, 1), (1, 1), (0, 1)]          # ends at a goal


# ---- the cell rule ---------------------------------------------------------------------------------------------------------------------------
def test_the_cell_rule_on_hand_written_values():
    """cells (x, 0), x = 0 .. 7: plain free; a negative `positive` with soft_weight > 0 costs 1; NaN roughness gives q = 0; visibility
    < 0 is never observed; visibility > 0 is observed; hard by density; hard by negative; the densest cell that is not hard, clamped at 65535 under a large weight"""
    pos = np.array([[10, -2000, 10, 10, 10, 51, 10, 50]], np.int32).T
    neg = np.array([[0, 0, 0, 0, 0, 0, 1, 0]], np.int32).T
    vis = np.array([[3, 3, 3, -7, 1, 3, 3, 3]], np.int32).T
    rough = np.array([[-7.0, -7.0, np.nan, -7.0, -1.0, -7.0, -7.0, -7.0]]).T
    p = afr.params(unknown=100, soft_weight=3, rough_weight=2, base=5)
    q = 50                                                              # floor((-7 - -10) / 6 * 100)
    assert afr.cell_costs(pos, neg, vis, rough, p)[:, 0].tolist() == [5 + 30 + 2 * q, 1, 5 + 30, 5 + 30 + 100 + 2 * q, 5 + 30 + 200, 0, 0, 5 + 150 + 2 * q]
    assert afr.cell_costs(pos, neg, vis, rough, dict(p, soft_weight=65535))[:, 0].tolist() == [65535, 1, 65535, 65535, 65535, 0, 0, 65535]
    blocked = afr.cell_costs(pos, neg, vis, rough, dict(p, unknown_blocks=True, include_negative=False))[:, 0]
    assert blocked.tolist() == [5 + 30 + 2 * q, 1, 5 + 30, 0, 5 + 30 + 200, 0, 5 + 30 + 2 * q, 5 + 150 + 2 * q]
    # and on arbitrary bit patterns the rule stays inside uint16, blocked exactly where the definition says
    s = ar.synthetic_set(np.random.default_rng(26), 40)
    c = afr.cell_costs(s[0].T, s[1].T, s[2].T, s[3].T, p)
    hard = (s[0].T.astype(np.float64) > 50) | (s[1].T > 0)
    # wherever positive >= 0 and visibility >= 0 -- every map set -- the rule IS costfield_ref.travcost's
    t = afr.terrain_set(np.random.default_rng(27), 40)
    for v in afr.VARIANTS:
        pv = afr.variant_params(v)
        d2 = afr.inflation((t[0].T > 50) | (t[1].T > 0), pv["inflation_cells2"]) if pv["inflation_cells2"] else None
        assert np.array_equal(afr.cell_costs(t[0].T, t[1].T, t[2].T, t[3].T, pv), cf.travcost(t[0].T, t[1].T, t[2].T, t[3].T, d2, pv))
    assert c.min() == 0 and c.max() <= 65535 and np.array_equal(c == 0, hard) and (c[~hard & (s[0].T < -100)] == 1).all()


# ---- the census of what the GPU is given ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("follow", [True, False])
@pytest.mark.parametrize("xy,A", afr.SCENARIOS)
def test_census_of_the_synthetic_scenarios(xy, A, follow):
    ref, steps = afr.scenario(xy, A, follow)
    E = ref.E
    assert E[0] < 0 and E[1] < 0 and E[0] & (A - 1) and E[1] & (A - 1)      # a storage phase on both axes, negative coordinates
    assert any(o[0] < 0 < o[0] + xy for _, o in steps) or E[0] < 0 < E[0] + A     # the storage seam lies inside the extent
    c = afr.census(xy, A, follow)
    print(xy, A, follow, c)
    for key in ("inflation_differs_from_twin", "D_differs_from_twin", "blocked_from_outside_the_window", "blocked_goals", "pocket", "ties",
                "window_cells_outside", "windows_wholly_outside", "cut", "rank1"):
        assert c[key] >= 1, (key, c)
    assert c["ties"] >= 100 and c["D_differs_from_twin"] >= 100
    kinds = {(v[0], v[1]) for v in afr.VARIANTS}
    assert kinds == {(i, u) for i in (0, 1, 5) for u in ("free", "blocked", 250)}
    assert {v[4] for v in afr.VARIANTS} == {True, False} == {v[5] for v in afr.VARIANTS} and any(v[2] for v in afr.VARIANTS) and any(v[3] for v in afr.VARIANTS)
    assert len(afr.scenario_goals(xy, A, follow, True)) == 17 and len(afr.scenario_goals(xy, A, follow, False)) == 1


def test_census_of_the_seam():
    xy, A = 33, 128
    E = ar.fixed_origin(xy, A)
    ref = ar.AtlasRef(A, xy, False, E)
    steps, goal, start = afr.seam_case(xy, A, E)
    for s, o in steps:
        ref.integrate(s, o)
    p = afr.params(inflation_cells=3)
    flat, twin = afr.field(ref, [goal], p), afr.field(ref, [goal], p, wrap=True)
    sx, sy = start[0] - E[0], start[1] - E[1]
    assert (goal[0] - E[0], start[0] - E[0]) == (4, A - 5)
    assert flat["D"][sx, sy] == 10 * (A - 9)
    # on the torus the walls inflate across the seam: the far column and the far row are blocked there, free and reached on the flat grid
    assert (flat["D"][A - 1, 4:A - 4] != U).all() and (twin["D"][A - 1, :] == U).all() and (flat["D"][4:A - 4, 0] != U).all() and (twin["D"][:, 0] == U).all()
    assert (flat["D"] != twin["D"]).sum() >= 6 * (A - 8)
    assert (flat["c"][A - 1, :A - 4] > 0).all() and (twin["c"][A - 3:, :] == 0).all() and (flat["c"][4:, 0] > 0).all() and (twin["c"][:, :3] == 0).all()


def test_census_of_the_consumers_case():
    """what test_rollouts_and_frontiers_run_on_a_cropped_field_unchanged counts on, from the referee alone"""
    xy, A = 33, 128
    ref, steps = afr.scenario(xy, A, True)
    o = steps[-1][1]
    p = afr.params(inflation_cells=1, unknown=40, soft_weight=2)
    maps, E = afr.extent_maps(ref)
    vehicle = afr.nearest_free(afr.cell_costs(*maps, p), (o[0] - E[0] + xy // 2, o[1] - E[1] + xy // 2))
    want = afr.field(ref, [(vehicle[0] + E[0], vehicle[1] + E[1])], p)
    D, d, c = afr.window(want, o, xy)
    summary, _, _ = rr.score(c, rr.arc_poses(64, 16, xy, afr.RES, o, seed=5), rr.patch_table(16, 9), afr.RES, o, D)
    assert ((summary[:, 3] != U) & (summary[:, 3] > 0)).sum() >= 8
    vis = afr.window(dict(want, D=maps[2], dir=maps[2].astype(np.uint8), c=maps[2]), o, xy)[0]
    vis = np.where(vis == U, 0, vis)
    fwant = fr.product(c.T, vis.T, D.T, 2, 256)
    assert fwant[3][0] >= 1
    local = cf.dijkstra(c, [(vehicle[0] + E[0] - o[0], vehicle[1] + E[1] - o[1])])
    n = int((fr.frontier_mask(c.T, vis.T, D.T) & (local.T == U)).sum())
    print("frontier cells reached only by a route outside the window:", n)
    assert n >= 1


# ---- the drive, with the maps of the CPU oracle -------------------------------------------------------------------------------------------
def _drive(ring, A):
    from oracle import oracle
    o = oracle.OracleGvom(ar.DRIVE_RES, ar.DRIVE_ZRES, ar.DRIVE_XY, 8, ring, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
    ref = ar.AtlasRef(A, ar.DRIVE_XY)
    for pc, ego in afr.drive_out():
        o.process_pointcloud(pc, ego)
        maps, org = ar.mapper_set(o, o.combine_maps())
        ref.integrate([m.T for m in maps], org)
    return ref, org


def test_with_128_cells_home_has_left_the_extent():
    ref, org = _drive(1, ar.DRIVE_A)
    assert ref.E == (8, -100)
    a = _mapper().create_atlas(128)
    a.extent_origin = ref.E
    with pytest.raises(ValueError, match=r"outside the extent: cell \(0, 0\), extent \[8, 136\) x \[-100, 28\)"):
        a.cost_to_go([afr.drive_out()[0][1][:2]])


@pytest.mark.parametrize("ring", [1, 2])
def test_census_of_the_drive_with_the_cpu_oracle(ring):
    """256 cells, the outward leg: home lies outside the live window and inside the extent; without inflation and with unknown="free"
    the referee reaches the free cell nearest the vehicle along more than xy_size steps; with one cell of inflation the answer is held
    to equality whichever it is (with the oracle's maps of ring 1 the vehicle is enclosed: unreached)"""
    ref, org = _drive(ring, afr.DRIVE_A)
    xy = ar.DRIVE_XY
    scans = afr.drive_out()
    home = tuple(int(v) for v in gvom.cells_of(scans[0][1][:2], ar.DRIVE_RES))
    vehicle = tuple(int(v) for v in gvom.cells_of(scans[-1][1][:2], ar.DRIVE_RES))
    E = ref.E
    assert home == (0, 0) and not (org[0] <= home[0] < org[0] + xy and org[1] <= home[1] < org[1] + xy)
    assert E[0] <= home[0] < E[0] + afr.DRIVE_A and E[1] <= home[1] < E[1] + afr.DRIVE_A
    assert max(abs(vehicle[0] - home[0]), abs(vehicle[1] - home[1])) == 72 > xy
    want = afr.field(ref, [home], afr.params())
    start = afr.nearest_free(want["c"], (vehicle[0] - E[0], vehicle[1] - E[1]))
    Dv = int(want["D"][start])
    assert Dv != U
    x, y = start
    path = [(x, y)]
    while want["dir"][x, y] != cf.GOAL:
        k = int(want["dir"][x, y])
        x, y = x + cf.STEPS[k][0], y + cf.STEPS[k][1]
        path.append((x, y))
    assert path[-1] == (home[0] - E[0], home[1] - E[1]) and len(path) - 1 > xy and cf.path_cost(path, want["c"]) == Dv
    print("ring", ring, "vehicle cell positive", int(ref.i[0][vehicle[1] - E[1], vehicle[0] - E[0]]), "start", start, "D", Dv, "steps", len(path) - 1)
    if ring == 1:
        assert (Dv, len(path) - 1) == (872, 72) and ref.i[0][vehicle[1] - E[1], vehicle[0] - E[0]] == 100
    one = afr.field(ref, [home], afr.params(inflation_cells=1))
    s1 = afr.nearest_free(one["c"], (vehicle[0] - E[0], vehicle[1] - E[1]))
    print("ring", ring, "one cell of inflation: start", s1, "D", int(one["D"][s1]))
    if ring == 1:
        assert one["D"][s1] == U
