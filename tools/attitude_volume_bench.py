#!/usr/bin/env python3
"""What an attitude volume (gvom_attitude_volume: k_volume_attitude_table, k_attitude_ground, k_volume_attitude) and its way into the pose
field (gvom_pose_field_attitude: k_cspace_attitude) cost.  On the map sets of m256 and c4 after three bench scans
(combine_maps_device()), a 2.2 m x 4.6 m car footprint with the car's chassis, H = 16 and 64 headings -- every loop in a fresh child
process, every child under a `timeout` of its own, and the first child that fails ends the run:

  call       DeviceMaps.attitude_volume(), enqueue to the drained stream: wall time per call; the states per status
  kernel     one `rocprofv3 --kernel-trace` run per config: k_volume_attitude, k_attitude_ground, k_volume_attitude_table,
             k_cspace_attitude and -- same footprint table, same window -- k_cspace, per call
  others     the same volume through score_attitude() on the H * xy^2 cell-centre poses (upload included; the poses are float32, so
             at a resolution of 0.2 m the statuses need not all agree: the number that differ is recorded), and written in torch
             (float64, one shifted gather per footprint cell; first shown equal to the product)
  field      pose_field() without and with the volume (tilt_weight 3, the default blocks), goal 2 m ahead of the ego
  step       scan + combine_maps_device() per step on this library and, with --parent LIB (the parent commit's libgvom_hip.so), on
             that library, alternating, five runs each
  resources  tools/kernel_regs.py: the new kernels, and registers, scratch, LDS and code size of every kernel outside the new unit on
             the parent and on this library (--resources alone: no GPU needed)

    tools/attitude_volume_bench.py [--resources] [--parent LIB] [--configs m256,c4] [--turns N] [out.json]   (default: profiles/attitude_volume_<lib sha8>.json)
"""
import json
import sys
import tempfile
import time

import benchkit as bk

CONFIGS = {"m256": 60, "c4": 24}                          # config: timed steps per repetition
CAR = dict(front=3.6, rear=1.0, half_width=1.1)
CHASSIS = dict(front_axle=2.7, rear_axle=0.0, track=1.7, belly_height=0.25, max_pitch=0.35, max_roll=0.3, min_clearance=0.1)
SHAPES = ((16, 2.0), (64, 6.0))                           # (headings, minimum turning radius of the pose field's arcs in metres)
CHILD_TIMEOUT = 300                                       # seconds, per child process
KERNELS = ("k_volume_attitude_table", "k_volume_attitude", "k_attitude_ground", "k_cspace_attitude", "k_cspace", "k_attitude")
NEW_UNIT = ("k_volume_attitude", "k_cspace_attitude")
TURNS = 5


def _tables(gvom, g, H, radius):
    footprint = gvom.rectangle_footprint(xy_resolution=g.xy_resolution, headings=H, **CAR)
    g.set_footprint(footprint)
    g.set_chassis(gvom.chassis(**CHASSIS))
    g.set_primitives(gvom.arc_primitives(H, radius, g.xy_resolution, reach=4))
    return footprint


def _torch_volume(torch, np, ground, footprint, g, chassis):
    """the definition in torch on the GPU: float64, one shifted gather per wheel and footprint cell, the header's operation order"""
    xy = g.xy_size
    res = float(g.xy_resolution)
    start, offs = footprint[0].tolist(), footprint[1].astype(np.int64).tolist()
    H = len(start) - 1
    dev = ground.device
    G = torch.full((xy + 2 * 64, xy + 2 * 64), float("nan"), dtype=torch.float64, device=dev)      # [y][x] with a border that reads "outside"
    G[64:64 + xy, 64:64 + xy] = ground
    inside = torch.zeros_like(G, dtype=torch.bool)
    inside[64:64 + xy, 64:64 + xy] = True
    known = lambda v: (v > -1000.0) & (v < float("inf"))
    fa, ra, tr, bh = chassis.front_axle, chassis.rear_axle, chassis.track, chassis.belly_height
    am = 0.5 * (fa + ra)
    half = tr / 2
    ab = ((fa, half), (fa, -half), (ra, half), (ra, -half))
    status = torch.empty((H, xy, xy), dtype=torch.uint8, device=dev)
    tilt = torch.empty((H, xy, xy), dtype=torch.uint8, device=dev)
    win = lambda A, dx, dy: A[64 + dy:64 + dy + xy, 64 + dx:64 + dx + xy]
    mp, mr, mc = float(chassis.max_pitch), float(chassis.max_roll), float(chassis.min_clearance)
    for h in range(H):
        c, s = float(g.cos_sin[h, 0]), float(g.cos_sin[h, 1])
        left = torch.zeros((xy, xy), dtype=torch.bool, device=dev)
        z = []
        for a, b in ab:
            ox, oy = int(np.floor(0.5 + (a * c - b * s) / res)), int(np.floor(0.5 + (a * s + b * c) / res))
            ox, oy = max(-64, min(64, ox)), max(-64, min(64, oy))
            left |= ~win(inside, ox, oy)
            z.append(win(G, ox, oy))
        unknown = ~(known(z[0]) & known(z[1]) & known(z[2]) & known(z[3]))
        zF, zR, zL, zT = 0.5 * (z[0] + z[1]), 0.5 * (z[2] + z[3]), 0.5 * (z[0] + z[2]), 0.5 * (z[1] + z[3])
        sp, sr = (zF - zR) / (fa - ra), (zL - zT) / tr
        z0 = 0.25 * ((z[0] + z[1]) + (z[2] + z[3]))
        belly = torch.full((xy, xy), float("inf"), dtype=torch.float64, device=dev)
        for dx, dy in offs[start[h]:start[h + 1]]:
            left |= ~win(inside, dx, dy)
            gg = win(G, dx, dy)
            du, dv = ((dx + 0.5) - 0.5) * res, ((dy + 0.5) - 0.5) * res
            u, v = du * c + dv * s, dv * c - du * s
            clr = (((z0 + sp * (u - am)) + sr * v) + bh) - gg
            belly = torch.where(known(gg) & (clr < belly), clr, belly)
        p, r, bl = sp.to(torch.float32), sr.to(torch.float32), belly.to(torch.float32)
        st = torch.zeros((xy, xy), dtype=torch.uint8, device=dev)
        st[bl < mc] = 3
        st[r.abs() > mr] = 2
        st[p.abs() > mp] = 1
        st[unknown] = 4
        st[left] = 5
        t = torch.maximum(p.abs().to(torch.float64) / mp * 100.0, r.abs().to(torch.float64) / mr * 100.0)
        tl = torch.where(t > 0, torch.clamp(torch.floor(t), max=100.0), torch.zeros_like(t))
        tl = torch.where(torch.isnan(tl) | (st >= 4), torch.zeros_like(tl), tl)
        status[h], tilt[h] = st.T, tl.to(torch.uint8).T                  # planes indexed [x, y]
    return status, tilt


def child_call(name, profiled):
    np, torch, gvom, g, dev = bk.setup(name)
    for scan in dev:
        m = bk.scan_combine(np, g, scan)
    ego = dev[2][1]
    xy, res = g.xy_size, g.xy_resolution
    results, calls = {}, 13
    goal = gvom.world_to_cells(np.array([[ego[0] + 2.0, ego[1]]]), res, m.origin)
    for H, radius in SHAPES:
        footprint = _tables(gvom, g, H, radius)
        key = "H%d" % H
        volume = lambda: m.attitude_volume().release()
        field = m.cost_to_go(goal, goals_in_cells=True)
        if profiled:
            for _ in range(calls):
                volume()
            with m.attitude_volume() as vol:
                for _ in range(calls):
                    field.pose_field(goal, goals_in_cells=True, attitude=vol, tilt_weight=3).release()
            field.release()
            bk.sync(g)
            continue
        out = {"xy": xy, "H": H, "states": H * xy * xy, "footprint_cells_heading_0": int(footprint[0][1]), "footprint_cells_mean": round(float(np.diff(footprint[0]).mean()), 1)}
        out["call"] = bk.timed(g, volume)
        vol = m.attitude_volume()
        status, tilt, counts = vol.copy_to_host()
        out["states_per_status"] = counts[:7].tolist()
        out["allocations"] = g.get_tuning("attitude_volume_allocations")
        out["pose_field_without_volume"] = bk.timed(g, lambda: field.pose_field(goal, goals_in_cells=True).release(), reps=5)
        out["pose_field_with_volume"] = bk.timed(g, lambda: field.pose_field(goal, goals_in_cells=True, attitude=vol, tilt_weight=3).release(), reps=5)
        with field.pose_field(goal, goals_in_cells=True) as f0, field.pose_field(goal, goals_in_cells=True, attitude=vol, tilt_weight=3) as f1:
            out["pose_field_reached_states"] = {"without": f0.reached, "with": f1.reached, "rounds_without": f0.rounds, "rounds_with": f1.rounds}
        try:                                                              # the same volume through score_attitude() on the cell-centre poses
            oc = np.round(np.asarray(m.origin)[:2] / res)
            x, y = np.meshgrid(np.arange(xy, dtype=np.float64), np.arange(xy, dtype=np.float64), indexing="ij")
            poses = np.zeros((H, xy, xy, 3), np.float32)
            poses[..., 0], poses[..., 1] = ((oc[0] + x + 0.5) * res)[None], ((oc[1] + y + 0.5) * res)[None]
            poses[..., 2] = (np.arange(H) * (2.0 * np.pi) / H).astype(np.float32)[:, None, None]
            poses = poses.reshape(H * xy, xy, 3)
            score = lambda: m.score_attitude(poses).release()
            rec = bk.timed(g, score, reps=3, rounds=3)
            with m.score_attitude(poses) as s:
                pose_status = s.status.copy_to_host().reshape(H, xy, xy)
            rec["pose_bytes_uploaded"] = int(poses.nbytes)
            rec["states_whose_status_differs"] = int((pose_status != status).sum())
            out["score_attitude_on_cell_centre_poses"] = rec
        except Exception as e:                                            # (a comparison that cannot run is named, the run goes on)
            out["score_attitude_not_measured"] = repr(e)[:300]
        try:
            height, inferred = torch.from_dlpack(m.height_map).T.contiguous(), torch.from_dlpack(m.inferred_height_map).T.contiguous()   # [y][x]
            ground = torch.where(height > -1000.0, height, inferred)
            chassis = gvom.chassis(**CHASSIS)
            torch.cuda.synchronize()
            ts, tt = _torch_volume(torch, np, ground, footprint, g, chassis)
            torch.cuda.synchronize()
            us = []
            for _ in range(3):
                t0 = time.perf_counter()
                _torch_volume(torch, np, ground, footprint, g, chassis)
                torch.cuda.synchronize()
                us.append(round((time.perf_counter() - t0) * 1e6, 1))
            out["torch_same_volume"] = {"us": us, "us_median": bk.median(us), "status_equal_to_the_product": bool(np.array_equal(ts.cpu().numpy(), status)),
                                        "tilt_equal_to_the_product": bool(np.array_equal(tt.cpu().numpy(), tilt))}
            del height, inferred, ground, ts, tt
        except Exception as e:
            out["torch_not_measured"] = repr(e)[:300]
        vol.release()
        field.release()
        results[key] = out
    return {"calls": calls} if profiled else results


def child_step(name, steps):
    np, torch, gvom, g, dev = bk.setup(name)

    def step(k):
        bk.scan_combine(np, g, dev[k % 3]).release()
    return bk.step_loop(g, step, steps, warm=min(6, steps))


def _kernel_times(profile_dir):
    """per shape: the kernels' microseconds per launch (median) and how often each ran; the shapes follow one another in the trace, H = 16
    first -- the launches of k_volume_attitude are split evenly between them"""
    rows = bk.kernel_trace_rows(profile_dir, KERNELS, exact=True)
    out = {}
    for k in KERNELS:
        us = [u for _, kk, u in rows if kk == k]
        per = len(us) // len(SHAPES)
        if not us or per * len(SHAPES) != len(us):
            continue
        for n, (H, _) in enumerate(SHAPES):
            part = us[n * per:(n + 1) * per]
            out.setdefault("H%d" % H, {})[k] = {"launches": len(part), "median_us_per_launch": round(bk.median(part), 2), "min_us": round(min(part), 2)}
    return out or None


def main():
    if bk.child(sys.argv[1:], {"call": lambda a: child_call(a[0], a[1] == "1"), "step": lambda a: child_step(a[0], int(a[1]))}):
        return
    args = bk.read_args(sys.argv[1:], configs=CONFIGS, turns=TURNS)
    parent = args["parent"]
    spawn = lambda mode, a, **kw: bk.spawn(__file__, mode, a, CHILD_TIMEOUT, **kw)
    report, configs = bk.product_report(
        "attitude_volume", args, {"car_m": CAR, "chassis": CHASSIS, "shapes": [list(s) for s in SHAPES]}, lambda k: any(n in k for n in NEW_UNIT),
        ["c5", "windows other than 256 and 512 cells", "the host and device-pointer routes", "AV_DEPTH other than 4",
         "the (U, V) table in LDS instead of scalar loads (not built)", "hardware counters",
         "score_attitude() agreement at a resolution whose cell centres are float32 numbers (the GPU test does that at 0.5 m)"])
    if configs is None:
        return
    for name in args["configs"]:
        res = spawn("call", (name, 0))
        with tempfile.TemporaryDirectory() as d:
            spawn("call", (name, 1), profile_dir=d)
            kernel = _kernel_times(d)
        for key in res:
            res[key]["kernels"] = (kernel or {}).get(key) or "not measured (the trace did not hold the expected launches)"
        configs[name] = res
        report.save()
        runs = bk.alternate(args["turns"], {"parent": parent and (lambda: spawn("step", (name, CONFIGS[name]), lib=parent)),
                                            "this": lambda: spawn("step", (name, CONFIGS[name]))})
        res["step: scan + combine_maps_device"] = bk.against_parent(bk.spreads(runs), "this", "parent", "this_")
        report.save()
    print(json.dumps(report.out, indent=1))


if __name__ == "__main__":
    main()
