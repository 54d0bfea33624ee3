"""Every argument error of the product calls and the atlas calls (g-vom_amd/csrc/gvom_product_calls.hip, gvom_atlas_calls.hip) is the
recorded one: replay() makes one call per argument check that arguments alone can reach -- and, for the checks that share a helper,
calls with several bad arguments that show the order of the checks -- and notes (return code, gvom_last_error text) of each.
tests/argument_errors_recorded.json holds what the library gave before the checks were folded into shared helpers (recorded on the
MI355X with the library of the commit before); the test holds today's library to it byte for byte.

Every case is refused before any launch.  The handles are small: a 16-cell window with z_size 8, a sharded handle of 64 cells, a
128-cell window for the atlas that would be smaller than its window.  Not replayed here: the refusals of windows above 4096 cells
(test_maps_of_more_than_4096_cells_a_side_are_refused in test_costfield / test_rollouts / test_attitude / test_frontier / test_clearance,
test_windows_beyond_the_limits_are_refused in test_posefield), and four capacity limits no small window reaches: gvom_score_alignments'
class grid of 2^32 words, gvom_score_viewpoints' 2^22 beams, beams x (xy_size + z_size + 1) >= 2^31 and a window of 2^31 voxels.

The voxel atlas's three walk queries (gvom_voxel_atlas_raycast, _score_viewpoints, _score_alignments) are replayed on an atlas of 64
cells and 8 levels: the sharded handle, no atlas, every check arguments alone reach, and calls with several bad arguments for the
order; recorded with the library of the commit before their checks moved into the helpers of their window twins.  Not reached by a
small handle there: gvom_voxel_atlas_score_viewpoints' 2^22 beams, beams x (cells + levels + 1) >= 2^31 and the box of a pose of 2^31
voxels (which also needs a combined map), and gvom_voxel_atlas_score_alignments' class grid of 2^32 words."""
import ctypes
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
RECORDED = os.path.join(HERE, "argument_errors_recorded.json")
I64 = ctypes.c_int64
FAR = (1 << 40) + 1


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _i64(*v):
    return (I64 * len(v))(*v)


def replay(mod, settings):
    """[name, return code, gvom_last_error text] of every case, in order"""
    xy, zs, A = settings["xy_size"], settings["z_size"], settings["atlas_cells"]
    rest = (1, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
    g = mod.Gvom(0.5, 0.2, xy, zs, *rest, voxel_statistics=False)
    s = mod.Gvom(0.5, 0.2, settings["sharded_xy_size"], zs, *rest, voxel_statistics=False, _shard=(0, 2))
    wide = mod.Gvom(0.5, 0.2, settings["wide_xy_size"], zs, *rest, voxel_statistics=False)
    L, out, names = g._lib, [], set()
    pid, pid2, info, e2 = I64(7), I64(7), (I64 * 4)(), (I64 * 2)()
    PID = ctypes.byref(pid)

    def case(name, rc, h=g):
        assert name not in names, name
        names.add(name)
        assert rc < 0 and pid.value == -1, (name, rc, pid.value)
        out.append([name, int(rc), L.gvom_last_error(h._h).decode()])
        pid.value = 7

    def ok(rc):
        assert rc == 0, (rc, L.gvom_last_error(g._h))
        pid.value = 7

    n2 = xy * xy
    zeros32, ones32, ones16 = np.zeros(n2, np.int32), np.ones(n2, np.int32), np.ones(n2, np.uint16)
    ground, poses, one = np.zeros(n2, np.float64), np.zeros(3, np.float32), np.zeros(16, np.float64)
    goal2, goal3 = np.array([1, 1], np.int32), np.array([1, 1, -1], np.int32)
    org = _i64(0, 0)

    def table(H, cols):                                   # a table of H headings with one entry each: start, entries
        return np.arange(H + 1, dtype=np.int32), np.zeros((H, cols), np.int16)

    def footprint(h, H):
        st, of = table(H, 2)
        assert L.gvom_footprint_set(h._h, H, _p(st), _p(of)) == 0

    def primitives(h, H):
        st, pr = table(H, 4)
        pr[:, 0], pr[:, 2], pr[:, 3] = 1, np.arange(H), 1
        assert L.gvom_primitives_set(h._h, H, _p(st), _p(pr)) == 0

    def chassis(h, H, sin=0.0, **kw):
        c = mod.GvomChassis(1.0, -1.0, 1.0, 0.3, np.inf, np.inf, -np.inf)
        for k, v in kw.items():
            setattr(c, k, v)
        cs = np.zeros(2 * max(H, 1), np.float64)
        cs[0::2], cs[1::2] = 1.0, sin
        return L.gvom_chassis_set(h._h, ctypes.byref(c), H, _p(cs))

    # ---- gvom_device_product: the kinds other calls make, and the ones nobody makes
    for kind in [0, -1] + list(range(5, 34)):
        case("device_product: kind %d" % kind, L.gvom_device_product(g._h, kind, 0, PID))
    case("device_product: sharded", L.gvom_device_product(s._h, 1, 0, PID), s)
    case("device_product: sharded, kind 5", L.gvom_device_product(s._h, 5, 0, PID), s)
    case("device_product: sharded, kind 33", L.gvom_device_product(s._h, 33, 0, PID), s)

    # ---- gvom_clearance
    def cl(h=g, sid=-1, pos=zeros32, neg=None, thr=50.0, flags=0):
        return L.gvom_clearance(h._h, sid, _p(pos), _p(neg), 0, thr, 0, flags, PID)
    nan = float("nan")
    case("clearance: sharded", cl(s, flags=256, thr=nan), s)
    case("clearance: flags", cl(flags=256))
    case("clearance: flags, NaN", cl(flags=2, thr=nan))
    case("clearance: NaN", cl(thr=nan))
    case("clearance: NaN, both", cl(thr=nan, sid=12345))
    case("clearance: both", cl(sid=12345))
    case("clearance: both (negative)", cl(sid=12345, pos=None, neg=zeros32))
    case("clearance: neither", cl(pos=None))
    case("clearance: neither (negative alone)", cl(pos=None, neg=zeros32))
    case("clearance: stale set", cl(sid=12345, pos=None))
    ok(L.gvom_clearance(g._h, -1, _p(zeros32), None, 0, 50.0, 0, 0, ctypes.byref(pid2)))
    clearance_id = pid2.value                              # a product of another kind than a cost field

    # ---- gvom_raycast
    def rq(h=g, frm=poses, K=1, to=poses, n=1, flags=0):
        return L.gvom_raycast(h._h, _p(frm), K, _p(to), n, 0, flags, None, PID)
    case("raycast: sharded", rq(s, frm=None), s)
    case("raycast: from", rq(frm=None, n=0))
    case("raycast: to", rq(to=None))
    case("raycast: n, K", rq(n=0, K=2))
    case("raycast: n", rq(n=-1, K=-1))
    case("raycast: K, flags", rq(K=2, n=3, flags=4))
    case("raycast: K", rq(K=0))
    case("raycast: flags, capacity", rq(flags=4, n=(1 << 26) + 1))
    case("raycast: flags", rq(flags=8))
    case("raycast: capacity", rq(n=(1 << 26) + 1))
    case("raycast: capacity, K = n", rq(n=(1 << 26) + 1, K=(1 << 26) + 1))

    # ---- gvom_cost_to_go
    P = mod.GvomCtgParams(50.0, 0.0, 0.0, 0, 1, 0, 1, 0)

    def params(**kw):
        q = mod.GvomCtgParams(50.0, 0.0, 0.0, 0, 1, 0, 1, 0)
        for k, v in kw.items():
            setattr(q, k, v)
        return ctypes.byref(q)
    bad_params = [dict(density_threshold=nan), dict(inflation_cells2=-1), dict(base=0), dict(soft_weight=-1), dict(soft_weight=65536),
                  dict(unknown_cost=-1), dict(unknown_cost=65536), dict(rough_weight=-1), dict(rough_weight=65536),
                  dict(rough_weight=1, min_roughness=nan), dict(rough_weight=1, max_roughness=float("inf")),
                  dict(rough_weight=1, min_roughness=1.0, max_roughness=1.0)]
    high, low = np.full(n2, 1, np.int32), np.full(n2, 1, np.int32)
    high[n2 - 1], low[0] = 65536, -1

    def ctg(h=g, sid=-1, par=None, cost=ones32, goals=goal2, n=1, max_cost=0, max_rounds=0, flags=0):
        return L.gvom_cost_to_go(h._h, sid, par, _p(cost), 0, _p(goals), n, max_cost, max_rounds, flags, PID, info)
    case("cost_to_go: sharded", ctg(s, flags=4, cost=None), s)
    case("cost_to_go: flags", ctg(flags=4))
    case("cost_to_go: flags, both", ctg(flags=8, sid=12345))
    case("cost_to_go: both", ctg(sid=12345, par=ctypes.byref(P)))
    case("cost_to_go: both, goals", ctg(sid=12345, n=0))
    case("cost_to_go: neither", ctg(cost=None))
    case("cost_to_go: neither, goals", ctg(cost=None, goals=None))
    case("cost_to_go: set without parameters", ctg(sid=12345, cost=None))
    case("cost_to_go: set without parameters, goals", ctg(sid=12345, cost=None, n=0))
    case("cost_to_go: goals NULL", ctg(goals=None))
    case("cost_to_go: no goal", ctg(n=0))
    case("cost_to_go: negative goals", ctg(n=-1))
    case("cost_to_go: 65537 goals", ctg(n=65537))
    case("cost_to_go: goals, max_cost", ctg(n=0, max_cost=-1))
    case("cost_to_go: max_cost -1", ctg(max_cost=-1))
    case("cost_to_go: max_cost 2^30 + 1", ctg(max_cost=2 ** 30 + 1))
    case("cost_to_go: max_cost, max_rounds", ctg(max_cost=-1, max_rounds=-1))
    case("cost_to_go: max_rounds", ctg(max_rounds=-1))
    case("cost_to_go: max_rounds, goal outside", ctg(max_rounds=-1, goals=np.array([xy, 1], np.int32)))
    case("cost_to_go: goal outside (x = xy)", ctg(goals=np.array([xy, 1], np.int32)))
    case("cost_to_go: goal outside (y = -1)", ctg(goals=np.array([1, -1], np.int32)))
    case("cost_to_go: second goal outside, bad cost", ctg(goals=np.array([1, 1, 1, xy], np.int32), n=2, cost=high))
    case("cost_to_go: goal outside, bad parameters", ctg(sid=12345, cost=None, par=params(base=0), goals=np.array([-1, 1], np.int32)))
    for k, kw in enumerate(bad_params):
        case("cost_to_go: bad parameters %d, stale set" % k, ctg(sid=12345, cost=None, par=params(**kw)))
    case("cost_to_go: stale set", ctg(sid=12345, cost=None, par=ctypes.byref(P)))
    case("cost_to_go: host cost 65536", ctg(cost=high))
    case("cost_to_go: host cost -1", ctg(cost=low))
    ok(L.gvom_cost_to_go(g._h, -1, None, _p(ones32), 0, _p(goal2), 1, 0, 0, 0, ctypes.byref(pid2), info))
    field_id = pid2.value                                   # a live cost field

    # ---- gvom_footprint_set
    st, of = table(4, 2)

    def fp(H=4, start=st, offs=of):
        pid.value = -1                                     # (no product id in this call)
        return L.gvom_footprint_set(g._h, H, _p(start), _p(offs))
    case("footprint_set: start NULL", fp(start=None, H=0))
    case("footprint_set: offsets NULL", fp(offs=None))
    case("footprint_set: no heading", fp(H=0, start=np.array([1, 2], np.int32)))
    case("footprint_set: 1025 headings", fp(H=1025))
    case("footprint_set: start[0]", fp(start=np.array([1, 1, 2, 3, 4], np.int32)))
    case("footprint_set: an empty heading", fp(start=np.array([0, 1, 1, 2, 3], np.int32)))
    case("footprint_set: 16385 cells", fp(start=np.array([0, 1, 16386, 16387, 16388], np.int32)))
    case("footprint_set: more than 2^22 offsets", fp(H=1024, start=(np.arange(1025, dtype=np.int64) * 16384).astype(np.int32)))

    # ---- gvom_score_rollouts (no footprint table yet)
    def ro(h=g, fid=-1, c=ones16, d=None, p=poses, K=1, T=1, o=org):
        return L.gvom_score_rollouts(h._h, fid, _p(c), _p(d), _p(p), K, T, 0, o, PID)
    case("score_rollouts: sharded", ro(s, p=None), s)
    case("score_rollouts: no footprint, poses NULL", ro(p=None))
    case("score_rollouts: no footprint", ro())
    footprint(g, 4)
    case("score_rollouts: poses NULL, both", ro(p=None, fid=field_id))
    case("score_rollouts: origin NULL", ro(o=None))
    case("score_rollouts: both", ro(fid=field_id))
    case("score_rollouts: both (cost_to_go), T", ro(fid=field_id, c=None, d=zeros32, T=0))
    case("score_rollouts: neither", ro(c=None))
    case("score_rollouts: neither, T", ro(c=None, d=zeros32, T=0))
    case("score_rollouts: T 0, K 0", ro(T=0, K=0))
    case("score_rollouts: T 4097", ro(T=4097))
    case("score_rollouts: K 0, origin", ro(K=0, o=_i64(FAR, 0)))
    case("score_rollouts: K -1", ro(K=-1))
    case("score_rollouts: capacity, origin", ro(K=(1 << 26) + 1, o=_i64(FAR, 0)))
    case("score_rollouts: capacity (T = 4096)", ro(K=(1 << 14) + 1, T=4096))
    case("score_rollouts: origin x, stale field", ro(o=_i64(FAR, 0), fid=12345, c=None))
    case("score_rollouts: origin -x", ro(o=_i64(-FAR, 0)))
    case("score_rollouts: origin y", ro(o=_i64(0, FAR)))
    case("score_rollouts: origin -y", ro(o=_i64(0, -FAR)))
    case("score_rollouts: stale field", ro(fid=12345, c=None))
    case("score_rollouts: a field of another kind", ro(fid=clearance_id, c=None))

    # ---- gvom_chassis_set
    pid.value = -1
    case("chassis_set: chassis NULL", L.gvom_chassis_set(g._h, None, 0, _p(one)))
    good = mod.GvomChassis(1.0, -1.0, 1.0, 0.3, 1.0, 1.0, 0.0)
    for name, call in (("cos_sin NULL", lambda: L.gvom_chassis_set(g._h, ctypes.byref(good), 4, None)),
                       ("no heading", lambda: chassis(g, 0, front_axle=nan)), ("1025 headings", lambda: chassis(g, 1025)),
                       ("a length, axles", lambda: chassis(g, 4, belly_height=float("inf"), front_axle=-2.0)),
                       ("axles, track", lambda: chassis(g, 4, front_axle=-1.0, track=0.0)), ("track, limit", lambda: chassis(g, 4, track=-1.0, max_roll=nan)),
                       ("limit", lambda: chassis(g, 4, min_clearance=nan)),
                       ("wheel offset", lambda: chassis(g, 4, sin=-1.0, front_axle=1.7e308, track=1.7e308))):
        pid.value = -1
        case("chassis_set: " + name, call())
    cs = np.array([1.0, 0.0, 1.5, 0.0], np.float64)
    pid.value = -1
    case("chassis_set: cos_sin entry", L.gvom_chassis_set(g._h, ctypes.byref(good), 2, _p(cs)))

    # ---- gvom_score_attitude (a footprint table of 4 headings, no chassis yet)
    def at(h=g, sid=-1, gr=ground, p=poses, K=1, T=1, flags=0, o=org):
        return L.gvom_score_attitude(h._h, sid, _p(gr), _p(p), K, T, 0, flags, o, PID)
    case("score_attitude: sharded", at(s, p=None), s)
    case("score_attitude: no footprint", at(wide, p=None), wide)
    case("score_attitude: no chassis", at(p=None))
    assert chassis(g, 8) == 0
    case("score_attitude: headings", at(p=None))
    assert chassis(g, 4) == 0
    case("score_attitude: poses NULL, flags", at(p=None, flags=2))
    case("score_attitude: origin NULL", at(o=None))
    case("score_attitude: flags, both", at(flags=2, sid=12345))
    case("score_attitude: both, T", at(sid=12345, T=0))
    case("score_attitude: neither, T", at(gr=None, T=0))
    case("score_attitude: T 0, K 0", at(T=0, K=0))
    case("score_attitude: T 4097", at(T=4097))
    case("score_attitude: K 0, origin", at(K=0, o=_i64(0, FAR)))
    case("score_attitude: capacity, origin", at(K=(1 << 26) + 1, o=_i64(0, FAR)))
    case("score_attitude: capacity (T = 4096)", at(K=(1 << 14) + 1, T=4096))
    case("score_attitude: origin x, stale set", at(o=_i64(FAR, 0), sid=12345, gr=None))
    case("score_attitude: origin -x", at(o=_i64(-FAR, 0)))
    case("score_attitude: origin y", at(o=_i64(0, FAR)))
    case("score_attitude: origin -y", at(o=_i64(0, -FAR)))
    case("score_attitude: stale set", at(sid=12345, gr=None))

    # ---- gvom_score_alignments
    w5 = (ctypes.c_int32 * 5)(1, 1, 1, 1, 1)

    def al(h=g, c=poses, n=1, t=one, K=1, dilate=0, w=w5):
        return L.gvom_score_alignments(h._h, _p(c), n, _p(t), K, 0, dilate, w, PID)
    case("score_alignments: sharded", al(s, c=None), s)
    case("score_alignments: cloud NULL", al(c=None, n=0))
    case("score_alignments: transforms NULL", al(t=None))
    case("score_alignments: weights NULL", al(w=None))
    case("score_alignments: n, K", al(n=0, K=0))
    case("score_alignments: K, dilate", al(K=0, dilate=2))
    case("score_alignments: dilate, weight", al(dilate=2, w=(ctypes.c_int32 * 5)(1, 1, 1, 1, 1025)))
    case("score_alignments: weight, n", al(w=(ctypes.c_int32 * 5)(-1025, 1, 1, 1, 1), n=(1 << 20) + 1))
    case("score_alignments: n, K capacity", al(n=(1 << 20) + 1, K=65537))
    case("score_alignments: K capacity", al(K=65537))
    case("score_alignments: pairs", al(n=1 << 20, K=65536))

    # ---- gvom_frontiers
    def fr(h=g, fid=-1, sid=-1, c=ones16, d=None, v=zeros32, min_cells=1, max_clusters=1):
        return L.gvom_frontiers(h._h, fid, sid, _p(c), _p(d), _p(v), 0, min_cells, max_clusters, PID, info)
    case("frontiers: sharded", fr(s, fid=1), s)
    case("frontiers: a field id alone", fr(fid=field_id, c=None, v=None))
    case("frontiers: a set id alone, min_cells", fr(sid=12345, min_cells=0))
    case("frontiers: ids and cell_cost", fr(fid=field_id, sid=12345, v=None))
    case("frontiers: ids and cost_to_go", fr(fid=field_id, sid=12345, c=None, v=None, d=zeros32))
    case("frontiers: ids and visibility, min_cells", fr(fid=field_id, sid=12345, c=None, min_cells=0))
    case("frontiers: no cell_cost", fr(c=None))
    case("frontiers: no visibility, min_cells", fr(v=None, min_cells=0))
    case("frontiers: min_cells, max_clusters", fr(min_cells=0, max_clusters=0))
    case("frontiers: max_clusters 0, stale field", fr(max_clusters=0, fid=12345, sid=12345, c=None, v=None))
    case("frontiers: max_clusters 2^20 + 1", fr(max_clusters=(1 << 20) + 1))
    case("frontiers: stale field, stale set", fr(fid=12345, sid=12345, c=None, v=None))
    case("frontiers: a field of another kind", fr(fid=clearance_id, sid=12345, c=None, v=None))
    case("frontiers: stale set", fr(fid=field_id, sid=12345, c=None, v=None))

    # ---- gvom_score_viewpoints (no sensor model yet)
    def vp(h=g, p=one, K=1, max_range=5.0, sh=1, sw=1, flags=0):
        return L.gvom_score_viewpoints(h._h, _p(p), K, 0, max_range, sh, sw, flags, None, PID)
    case("score_viewpoints: sharded", vp(s, p=None), s)
    case("score_viewpoints: poses NULL", vp(p=None, K=0))
    case("score_viewpoints: no sensor model", vp(K=0))
    d = np.zeros((2, 4, 3), np.float64)
    d[:, :, 0] = 1.0
    g.set_sensor_model(d)
    case("score_viewpoints: K, strides", vp(K=0, sh=0))
    case("score_viewpoints: stride_h, max_range", vp(sh=0, max_range=nan))
    case("score_viewpoints: stride_w", vp(sw=0))
    case("score_viewpoints: max_range NaN, flags", vp(max_range=nan, flags=2))
    case("score_viewpoints: max_range 0", vp(max_range=0.0))
    case("score_viewpoints: max_range inf", vp(max_range=float("inf")))
    case("score_viewpoints: flags, capacity", vp(flags=2, K=65537))
    case("score_viewpoints: capacity", vp(K=65537))

    # ---- gvom_primitives_set
    st8, pr8 = table(8, 4)
    pr8[:, 0], pr8[:, 2], pr8[:, 3] = 1, np.arange(8), 1

    def ps(H=8, start=st8, prims=pr8):
        pid.value = -1
        return L.gvom_primitives_set(g._h, H, _p(start), _p(prims))
    case("primitives_set: start NULL", ps(start=None, H=0))
    case("primitives_set: prims NULL", ps(prims=None))
    case("primitives_set: no heading", ps(H=0, start=np.array([1, 2], np.int32)))
    case("primitives_set: 65 headings", ps(H=65))
    case("primitives_set: start[0]", ps(start=np.arange(1, 10, dtype=np.int32)))
    case("primitives_set: 65 primitives", ps(start=np.array([0, 65] + [66] * 7, np.int32)))
    case("primitives_set: a negative count", ps(start=np.array([0, 2, 1] + [1] * 6, np.int32)))
    for col, v in ((0, 5), (1, -5), (2, 8), (2, -1), (3, 0), (3, 256)):
        q = pr8.copy()
        q[1, col] = v
        case("primitives_set: column %d = %d" % (col, v), ps(prims=q))
    q = pr8.copy()
    q[1] = (0, 0, 1, 1)
    case("primitives_set: a self loop", ps(prims=q))

    # ---- gvom_pose_field (a footprint table of 4 headings, no primitives yet)
    def pf(h=g, fid=-1, cost=ones32, goals=goal3, n=1, max_cost=0, max_rounds=0):
        return L.gvom_pose_field(h._h, fid, _p(cost), 0, _p(goals), n, max_cost, max_rounds, PID, info)
    case("pose_field: sharded", pf(s, cost=None), s)
    case("pose_field: no footprint", pf(wide, cost=None), wide)
    case("pose_field: no primitives", pf(cost=None))
    primitives(g, 8)
    footprint(g, 65)
    case("pose_field: 65 headings", pf(cost=None))
    footprint(g, 4)
    case("pose_field: headings", pf(cost=None))
    primitives(g, 4)
    case("pose_field: both, goals", pf(fid=field_id, n=0))
    case("pose_field: neither, goals", pf(cost=None, goals=None))
    case("pose_field: goals NULL", pf(goals=None))
    case("pose_field: no goal", pf(n=0))
    case("pose_field: negative goals", pf(n=-1))
    case("pose_field: 65537 goals", pf(n=65537))
    case("pose_field: goals, max_cost", pf(n=0, max_cost=-1))
    case("pose_field: max_cost -1", pf(max_cost=-1))
    case("pose_field: max_cost 2^30 + 1", pf(max_cost=2 ** 30 + 1))
    case("pose_field: max_cost, max_rounds", pf(max_cost=-1, max_rounds=-1))
    case("pose_field: max_rounds, goal outside", pf(max_rounds=-1, goals=np.array([xy, 1, 0], np.int32)))
    case("pose_field: goal outside (x = xy), heading", pf(goals=np.array([xy, 1, 4], np.int32)))
    case("pose_field: goal outside (x = -1)", pf(goals=np.array([-1, 1, 0], np.int32)))
    case("pose_field: goal outside (y = xy)", pf(goals=np.array([1, xy, 0], np.int32)))
    case("pose_field: goal outside (y = -1)", pf(goals=np.array([1, -1, 0], np.int32)))
    case("pose_field: heading, stale field", pf(goals=np.array([1, 1, 4], np.int32), fid=12345, cost=None))
    case("pose_field: second goal's heading, bad cost", pf(goals=np.array([1, 1, 0, 1, 1, 4], np.int32), n=2, cost=high))
    case("pose_field: stale field", pf(fid=12345, cost=None))
    case("pose_field: a field of another kind", pf(fid=clearance_id, cost=None))
    case("pose_field: host cost 65536", pf(cost=high))
    case("pose_field: host cost -1", pf(cost=low))

    # ---- the atlas calls without an atlas, and on a sharded handle
    nine = (ctypes.c_void_p * 9)(*[ground.ctypes.data] * 9)
    P64 = ctypes.POINTER(I64)
    g64 = np.array([1, 1], np.int64)

    def actg(h=g, par=ctypes.byref(P), goals=g64, n=1, max_cost=0, max_rounds=0, flags=0):
        return L.gvom_atlas_cost_to_go(h._h, par, None if goals is None else goals.ctypes.data_as(P64), n, max_cost, max_rounds, flags, PID, info, e2)

    def calls(h):
        def direct(f, *a):
            pid.value = -1
            return f(h._h, *a)
        return (("clear", lambda: direct(L.gvom_atlas_clear)), ("integrate", lambda: direct(L.gvom_atlas_integrate, -1, None, 0, None)),
                ("recall", lambda: L.gvom_atlas_recall(h._h, None, ctypes.byref(pid2), PID, None)), ("extent", lambda: L.gvom_atlas_extent(h._h, PID, None)),
                ("counts", lambda: direct(L.gvom_atlas_counts, info)), ("cost_to_go", lambda: actg(h, flags=4)),
                ("frontiers", lambda: L.gvom_atlas_frontiers(h._h, 12345, 0, 0, PID, info, e2)))
    for name, call in calls(g):
        case("atlas_%s: no atlas" % name, call())
    for name, call in calls(s):
        case("atlas_%s: sharded" % name, call(), s)
    pid.value = -1
    case("atlas_field_window: sharded", L.gvom_atlas_field_window(s._h, 12345, 12345, org, PID), s)

    # ---- gvom_atlas_configure
    def cfg(h=g, cells=A, mode=1, o=org):
        pid.value = -1
        return L.gvom_atlas_configure(h._h, cells, mode, o)
    case("atlas_configure: sharded", cfg(s, cells=63), s)
    case("atlas_configure: 32 cells, mode", cfg(cells=32, mode=7))
    case("atlas_configure: 100 cells", cfg(cells=100))
    case("atlas_configure: 8192 cells", cfg(cells=8192))
    case("atlas_configure: -64 cells", cfg(cells=-64))
    case("atlas_configure: smaller than the window, mode", cfg(wide, cells=64, mode=7), wide)
    case("atlas_configure: mode, origin", cfg(mode=2, o=_i64(FAR, 0)))
    case("atlas_configure: origin x", cfg(o=_i64(-FAR, 0)))
    case("atlas_configure: origin y", cfg(o=_i64(0, FAR)))
    ok(cfg())                                              # a fixed atlas of A cells at (0, 0)

    # ---- gvom_atlas_integrate, gvom_atlas_recall
    def ai(sid=-1, maps=nine, o=org):
        pid.value = -1
        return L.gvom_atlas_integrate(g._h, sid, maps, 0, o)
    case("atlas_integrate: both (maps)", ai(sid=12345, o=None))
    case("atlas_integrate: both (origin)", ai(sid=12345, maps=None))
    case("atlas_integrate: neither", ai(maps=None, o=None))
    case("atlas_integrate: no origin", ai(o=None))
    case("atlas_integrate: no maps", ai(maps=None))
    case("atlas_integrate: stale set", ai(sid=12345, maps=None, o=None))
    eight = (ctypes.c_void_p * 9)(*([ground.ctypes.data] * 8 + [None]))
    case("atlas_integrate: a NULL map, origin", ai(maps=eight, o=_i64(FAR, 0)))
    case("atlas_integrate: origin", ai(o=_i64(0, -FAR)))
    case("atlas_recall: origin", L.gvom_atlas_recall(g._h, _i64(FAR, 0), ctypes.byref(pid2), PID, None))

    # ---- gvom_atlas_cost_to_go
    case("atlas_cost_to_go: flags, parameters NULL", actg(flags=4, par=None))
    case("atlas_cost_to_go: parameters NULL, goals", actg(par=None, goals=None))
    case("atlas_cost_to_go: goals NULL", actg(goals=None))
    case("atlas_cost_to_go: no goal", actg(n=0))
    case("atlas_cost_to_go: negative goals", actg(n=-1))
    case("atlas_cost_to_go: 65537 goals", actg(n=65537))
    case("atlas_cost_to_go: goals, max_cost", actg(n=0, max_cost=-1))
    case("atlas_cost_to_go: max_cost -1", actg(max_cost=-1))
    case("atlas_cost_to_go: max_cost 2^30 + 1", actg(max_cost=2 ** 30 + 1))
    case("atlas_cost_to_go: max_cost, max_rounds", actg(max_cost=-1, max_rounds=-1))
    case("atlas_cost_to_go: max_rounds, bad parameters", actg(max_rounds=-1, par=params(base=0)))
    for k, kw in enumerate(bad_params):
        case("atlas_cost_to_go: bad parameters %d, goal outside" % k, actg(par=params(**kw), goals=np.array([A, 1], np.int64)))
    for k, cell in enumerate(((-1, 0), (A, 0), (0, -1), (0, A))):
        case("atlas_cost_to_go: goal outside %d" % k, actg(goals=np.array(cell, np.int64)))
    case("atlas_cost_to_go: second goal outside", actg(goals=np.array([1, 1, 5, A + 7], np.int64), n=2))
    ok(L.gvom_atlas_cost_to_go(g._h, ctypes.byref(P), g64.ctypes.data_as(P64), 1, 0, 0, 0, ctypes.byref(pid2), info, e2))
    atlas_field_id = pid2.value                            # a live atlas field

    # ---- gvom_atlas_field_window, gvom_atlas_frontiers
    def fw(fid=atlas_field_id, sid=-1, o=org):
        return L.gvom_atlas_field_window(g._h, fid, sid, o, PID)
    case("atlas_field_window: stale field, both", fw(fid=12345, sid=12345))
    case("atlas_field_window: a cost field", fw(fid=field_id))
    case("atlas_field_window: both", fw(sid=12345))
    case("atlas_field_window: neither", fw(o=None))
    case("atlas_field_window: stale set", fw(sid=12345, o=None))
    case("atlas_field_window: origin x", fw(o=_i64(FAR, 0)))
    case("atlas_field_window: origin -y", fw(o=_i64(0, -FAR)))

    def afr(fid=atlas_field_id, min_cells=1, max_clusters=1):
        return L.gvom_atlas_frontiers(g._h, fid, min_cells, max_clusters, PID, info, e2)
    case("atlas_frontiers: stale field, min_cells", afr(fid=12345, min_cells=0))
    case("atlas_frontiers: a cost field", afr(fid=field_id))
    case("atlas_frontiers: min_cells, max_clusters", afr(min_cells=0, max_clusters=0))
    case("atlas_frontiers: max_clusters 0", afr(max_clusters=0))
    case("atlas_frontiers: max_clusters 2^20 + 1", afr(max_clusters=(1 << 20) + 1))

    # ---- the voxel atlas's walk queries: gvom_voxel_atlas_raycast, _score_viewpoints, _score_alignments (recorded before they were folded
    # onto the drivers of their window twins; an atlas of A cells and z_size levels, the smallest the library takes)
    e3 = (I64 * 3)()
    bare = mod.Gvom(0.5, 0.2, xy, zs, *rest, voxel_statistics=False)       # an atlas, no sensor model

    def vrq(h=g, frm=poses, K=1, to=poses, n=1, flags=0):
        return L.gvom_voxel_atlas_raycast(h._h, _p(frm), K, _p(to), n, 0, flags, e3, PID)

    def vvp(h=g, p=one, K=1, max_range=5.0, sh=1, sw=1, flags=0):
        return L.gvom_voxel_atlas_score_viewpoints(h._h, _p(p), K, 0, max_range, sh, sw, flags, e3, PID)

    def val(h=g, c=poses, n=1, t=one, K=1, dilate=0, w=w5, o=None):
        return L.gvom_voxel_atlas_score_alignments(h._h, _p(c), n, _p(t), K, 0, dilate, w, o, e3, PID)
    case("voxel_atlas_raycast: sharded", vrq(s, frm=None), s)
    case("voxel_atlas_score_viewpoints: sharded", vvp(s, p=None), s)
    case("voxel_atlas_score_alignments: sharded", val(s, c=None), s)
    case("voxel_atlas_raycast: no atlas, from", vrq(frm=None, n=0))
    case("voxel_atlas_score_viewpoints: no atlas, poses", vvp(p=None, K=0))
    case("voxel_atlas_score_alignments: no atlas, cloud", val(c=None, n=0))
    for h in (g, bare):
        assert L.gvom_voxel_atlas_configure(h._h, A, zs, 1, None) == 0, L.gvom_last_error(h._h)
    case("voxel_atlas_raycast: from", vrq(frm=None, n=0))
    case("voxel_atlas_raycast: to", vrq(to=None))
    case("voxel_atlas_raycast: n, K", vrq(n=0, K=2))
    case("voxel_atlas_raycast: n", vrq(n=-1, K=-1))
    case("voxel_atlas_raycast: K, flags", vrq(K=2, n=3, flags=4))
    case("voxel_atlas_raycast: K", vrq(K=0))
    case("voxel_atlas_raycast: flags, capacity", vrq(flags=4, n=(1 << 26) + 1))
    case("voxel_atlas_raycast: flags", vrq(flags=8))
    case("voxel_atlas_raycast: capacity", vrq(n=(1 << 26) + 1))
    case("voxel_atlas_raycast: capacity, K = n", vrq(n=(1 << 26) + 1, K=(1 << 26) + 1))
    case("voxel_atlas_score_viewpoints: poses NULL", vvp(bare, p=None, K=0), bare)
    case("voxel_atlas_score_viewpoints: no sensor model", vvp(bare, K=0), bare)
    case("voxel_atlas_score_viewpoints: K, strides", vvp(K=0, sh=0))
    case("voxel_atlas_score_viewpoints: stride_h, max_range", vvp(sh=0, max_range=nan))
    case("voxel_atlas_score_viewpoints: stride_w", vvp(sw=0))
    case("voxel_atlas_score_viewpoints: max_range NaN, flags", vvp(max_range=nan, flags=2))
    case("voxel_atlas_score_viewpoints: max_range 0", vvp(max_range=0.0))
    case("voxel_atlas_score_viewpoints: max_range inf", vvp(max_range=float("inf")))
    case("voxel_atlas_score_viewpoints: flags, capacity", vvp(flags=2, K=65537))
    case("voxel_atlas_score_viewpoints: capacity", vvp(K=65537))
    case("voxel_atlas_score_alignments: cloud NULL", val(c=None, n=0))
    case("voxel_atlas_score_alignments: transforms NULL", val(t=None))
    case("voxel_atlas_score_alignments: weights NULL", val(w=None))
    case("voxel_atlas_score_alignments: n, K", val(n=0, K=0))
    case("voxel_atlas_score_alignments: K, dilate", val(K=0, dilate=2))
    case("voxel_atlas_score_alignments: dilate, weight", val(dilate=2, w=(ctypes.c_int32 * 5)(1, 1, 1, 1, 1025)))
    case("voxel_atlas_score_alignments: weight, n", val(w=(ctypes.c_int32 * 5)(-1025, 1, 1, 1, 1), n=(1 << 20) + 1))
    case("voxel_atlas_score_alignments: n, K capacity", val(n=(1 << 20) + 1, K=65537))
    case("voxel_atlas_score_alignments: K capacity", val(K=65537, o=_i64(FAR, 0, 0)))
    case("voxel_atlas_score_alignments: pairs", val(n=1 << 20, K=65536))
    return out


def test_every_argument_error_is_the_recorded_one():
    import gvom as mod
    rc, info = mod.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    with open(RECORDED) as f:
        rec = json.load(f)
    got = replay(mod, rec["settings"])
    want = rec["results"]
    assert [r[0] for r in got] == [r[0] for r in want]      # the case list is the recorded one
    for g, w in zip(got, want):
        print("%-60s %3d %s" % tuple(g))
        assert g == w, (g, w)
