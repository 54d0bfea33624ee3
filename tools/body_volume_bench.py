#!/usr/bin/env python3
"""What a body volume (gvom_body_volume: k_volume_body) costs, and what it does to a pose field.  On m256 (256 x 256 x 256) and c4 (512 x
512 x 128) with an atlas of 1024 x 1024 x (256 | 128) voxels, after three bench scans and one integrate, against distance_field(2.0) at the
window, with the body bench's car body (S is recorded), at H = 16 and H = 64 -- every loop in a fresh child process, every child under a
`timeout` of its own, and the first child that fails ends the run:

  events       HIP events on the handle's stream around one body_volume() call (the map-set route: k_attitude_ground + k_volume_body;
               the first call also rebuilds the wheel-offset table), 20 calls: median (min .. max)
  baseline     the only way to the same numbers without the entry point, on the same library: score_body() on the H * xy rollouts of xy
               cell-centre poses -- the upload of the poses by the wall clock, the call on device poses by events; where the cell
               centres are float32 numbers and the two wheel rules agree, the statuses are compared
  kernels      k_volume_body, k_body, k_attitude_ground and k_cspace_attitude alone from ONE rocprofv3 --kernel-trace --stats run of a
               child of its own
  pose field   pose_field(body=...) against pose_field() at the same goal: milliseconds per call, rounds and reached states of both
  step         scan + combine_maps_device() per step without a query, on this library and, with --parent LIB, on the parent commit's,
               alternating, --turns runs each (default five)
  resources    tools/kernel_regs.py: the new kernel, and registers, scratch, LDS and code size of every kernel outside the new unit on
               the parent and on this library (--resources alone: no GPU needed)

    tools/body_volume_bench.py [--resources] [--parent LIB] [--configs m256,c4] [--turns N] [out.json]   (default: profiles/body_volume_<lib sha8>.json)
"""
import json
import sys
import tempfile
import time

import benchkit as bk
import body_bench as bb

CONFIGS = {"m256": 100, "c4": 40}                        # config: timed steps per repetition
SHAPES = ((16, 2.0), (64, 6.0))                           # (headings, minimum turning radius of the pose field's arcs in metres)
MIN_MARGIN, SOFT_MARGIN = 0.2, 0.6
SQUEEZE_WEIGHT = 3
CHILD_TIMEOUT = 420                                       # seconds, per child process
TURNS = 5
KERNELS = ("k_volume_body", "k_body", "k_attitude_ground", "k_cspace_attitude", "k_volume_attitude_table")
CALLS = 20


def _ready(np, gvom, g, dev):
    """three scans, one integrate, the field at the window, the body: (map set, field, body)"""
    a = g.create_voxel_atlas(bb.SIDE, bb._levels(g.z_size))
    for scan in dev:
        m = bk.scan_combine(np, g, scan)
    a.integrate()
    body = gvom.box_spheres(**bb.BODY)
    g.set_body(body)
    return m, a.distance_field(bb.CAP), body


def _tables(gvom, g, H, radius):
    g.set_footprint(gvom.rectangle_footprint(xy_resolution=g.xy_resolution, headings=H, **bb.CAR))
    g.set_chassis(gvom.chassis(**bb.CHASSIS))
    g.set_primitives(gvom.arc_primitives(H, radius, g.xy_resolution, reach=4))


def _centre_poses(np, xy, H, res, oc):
    x, y = np.meshgrid(np.arange(xy, dtype=np.float64), np.arange(xy, dtype=np.float64), indexing="ij")
    wx, wy = (oc[0] + x + 0.5) * res, (oc[1] + y + 0.5) * res
    p = np.zeros((H, xy, xy, 3), np.float32)
    p[..., 0], p[..., 1] = wx[None], wy[None]
    exact = bool(np.array_equal(p[0, ..., 0].astype(np.float64), wx) and np.array_equal(p[0, ..., 1].astype(np.float64), wy))
    p[..., 2] = (np.arange(H, dtype=np.float64) * (2.0 * np.pi) / H).astype(np.float32)[:, None, None]
    return np.ascontiguousarray(p.reshape(H * xy, xy, 3)), exact


def child_call(name, profiled):
    np, torch, gvom, g, dev = bk.setup(name)
    m, f, body = _ready(np, gvom, g, dev)
    ego = dev[2][1]
    xy, res = g.xy_size, g.xy_resolution
    stream = torch.cuda.ExternalStream(int(g._lib.gvom_stream(g._h)))
    goal = gvom.world_to_cells(np.array([[ego[0] + 2.0, ego[1]]]), res, m.origin)
    oc = [int(v) for v in np.round(np.asarray(m.origin)[:2] / res)]
    results = {}
    for H, radius in SHAPES:
        _tables(gvom, g, H, radius)
        volume = lambda: f.body_volume(m, min_margin=MIN_MARGIN, soft_margin=SOFT_MARGIN)
        poses, exact = _centre_poses(np, xy, H, res, oc)
        K, T = poses.shape[:2]
        field = m.cost_to_go(goal, goals_in_cells=True)
        if profiled:                                           # under rocprofv3: CALLS launches per call, in this order
            for _ in range(CALLS):
                volume().release()
            tp = torch.from_numpy(poses).cuda()
            torch.cuda.synchronize()
            for _ in range(CALLS):
                g._score_body(f.product_id, None, None, m.set_id, None, gvom._dev(tp.data_ptr()), K, T, 1, True, m.origin, MIN_MARGIN).release()
            with volume() as vol:
                for _ in range(3):
                    field.pose_field(goal, goals_in_cells=True, body=vol, squeeze_weight=SQUEEZE_WEIGHT).release()
            field.release()
            bk.sync(g)
            del tp
            continue
        out = {"xy": xy, "z": g.z_size, "H": H, "states": H * xy * xy, "S": int(body.shape[0])}
        out["body_volume (events on the handle's stream)"] = bk.timed_events(torch, stream, lambda: volume().release(), CALLS, warm=3)[0]
        out["body_volume_call_us (enqueue to the drained stream)"] = bk.timed(g, lambda: volume().release(), reps=5)
        vol = volume()
        status, squeeze, clr, counts = vol.copy_to_host()
        out["states_per_status"] = counts[:6].tolist()
        out["squeeze_strictly_between_0_and_100"] = int(((squeeze > 0) & (squeeze < 100)).sum())
        out["allocations"] = g.get_tuning("body_volume_allocations")
        # the baseline: the same numbers through score_body() on the cell-centre poses
        ups = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tp = torch.from_numpy(poses).cuda()
            torch.cuda.synchronize()
            ups.append(round((time.perf_counter() - t0) * 1e6, 1))
        score = lambda: g._score_body(f.product_id, None, None, m.set_id, None, gvom._dev(tp.data_ptr()), K, T, 1, True, m.origin, MIN_MARGIN)
        base = {"rollouts": K, "poses_per_rollout": T, "pose_bytes": int(poses.nbytes), "pose_upload_us": ups, "pose_upload_us_median": bk.median(ups)}
        base["score_body on device poses (events on the handle's stream)"] = bk.timed_events(torch, stream, lambda: score().release(), CALLS, warm=3)[0]
        with score() as r:
            _, pose_clr, pairs = r.copy_to_host()
        base["cell_centres_are_float32_numbers"] = exact
        base["states_whose_status_differs"] = int((pairs[..., 0].reshape(H, xy, xy) != status).sum())
        base["states_whose_clearance_bits_differ"] = int((np.ascontiguousarray(pose_clr.reshape(H, xy, xy)).view(np.uint32) != np.ascontiguousarray(clr).view(np.uint32)).sum())
        out["score_body_on_cell_centre_poses"] = base
        del tp
        # the pose field with and without the volume, the same goal
        ms = lambda call: bk.timed_waiting(call, 1, 5)
        out["pose_field_without_volume_ms"] = ms(lambda: field.pose_field(goal, goals_in_cells=True).release())
        out["pose_field_with_body_ms"] = ms(lambda: field.pose_field(goal, goals_in_cells=True, body=vol, squeeze_weight=SQUEEZE_WEIGHT).release())
        with field.pose_field(goal, goals_in_cells=True) as f0, field.pose_field(goal, goals_in_cells=True, body=vol, squeeze_weight=SQUEEZE_WEIGHT) as f1:
            out["pose_field"] = {"reached_without": f0.reached, "reached_with": f1.reached, "rounds_without": f0.rounds, "rounds_with": f1.rounds}
        vol.release()
        field.release()
        results["H%d" % H] = out
    return {"calls": CALLS, "order": ["body_volume", "score_body", "pose_field x 3"]} if profiled else results


def child_step(name, steps):
    np, torch, gvom, g, dev = bk.setup(name)

    def step(k):
        bk.scan_combine(np, g, dev[k % 3]).release()
    return bk.step_loop(g, step, steps, warm=min(10, steps))


def main():
    if bk.child(sys.argv[1:], {"call": lambda a: child_call(a[0], a[1] == "1"), "step": lambda a: child_step(a[0], int(a[1]))}):
        return
    args = bk.read_args(sys.argv[1:], configs=CONFIGS, turns=TURNS)
    parent = args["parent"]
    spawn = lambda mode, a, **kw: bk.spawn(__file__, mode, a, CHILD_TIMEOUT, **kw)
    report, configs = bk.product_report(
        "body_volume", args, {"side": bb.SIDE, "cap_m": bb.CAP, "shapes": [list(s) for s in SHAPES], "body_box_metres": bb.BODY, "chassis": bb.CHASSIS,
                              "min_margin_m": MIN_MARGIN, "soft_margin_m": SOFT_MARGIN, "squeeze_weight": SQUEEZE_WEIGHT,
                              "lane_mapping": "16 x 16 tile of cells per workgroup at one heading, x the fast lane index, direct stores"},
        lambda k: "k_volume_body" in k,
        ["the other lane mapping (lanes along a whole row of x, k_volume_attitude's shape) inside this tool: the library has only the tile; a variant built for the comparison was timed once (profiles/body_volume_mapping_*.json, DESIGN.md 9.22)",
         "the tile with its stores staged through LDS: with x the fast lane index the stores are runs along x already",
         "bodies of other sizes than the car's", "the pointer routes and the host route", "other depths than 4 gathers in flight",
         "hardware counters", "the step with a body volume per step"])
    if configs is None:
        return
    for name in args["configs"]:
        res = spawn("call", (name, 0))
        configs[name] = res
        report.save()
        with tempfile.TemporaryDirectory() as d:                             # the kernels alone: one kernel trace of a child of its own
            spawn("call", (name, 1), profile_dir=d, stats=True)
            res["kernels (rocprofv3 --kernel-trace --stats of a child of its own: both shapes together)"] = bk.kernel_stats(d, KERNELS)
        report.save()
        runs = bk.alternate(args["turns"], {"parent": parent and (lambda: spawn("step", (name, CONFIGS[name]), lib=parent)),
                                            "this": lambda: spawn("step", (name, CONFIGS[name]))})
        res["step: scan + combine_maps_device, no query"] = bk.against_parent(bk.spreads(runs), "this", "parent", "this_")
        report.save()
    print(json.dumps(report.out, indent=1))


if __name__ == "__main__":
    main()
