#!/usr/bin/env python3
"""What terrain attitude scoring (gvom_score_attitude: k_attitude_ground, k_attitude) costs.  On the maps of m256 (256 x 256) and c4
(512 x 512) after three bench scans, against the map set's own ground, with the car footprint of tests/rollouts_ref.py (CAR: about
325 cells per heading at 0.2 m, 64 headings) and the car chassis of tests/attitude_ref.py, for (K, T) = (4096, 64) and (16384, 128),
arcs that leave the ego a cell a pose -- every loop in a fresh child process, every child under a `timeout` of its own, and the
first child that fails ends the run:

  call       gvom_score_attitude with poses in device memory, by map set and by pointer (the same ground as one device array),
             enqueue to completion, and gvom_score_rollouts at the same shape against the cost field towards the ego, as a
             yardstick: wall time
  kernel     one `rocprofv3 --kernel-trace` run per config, the calls in a known order: k_attitude, k_attitude_ground, k_rollouts
  torch      the same scoring written in torch on the exported height maps -- index tensors of K x T x M cells in chunks of
             rollouts, gathers, float64 arithmetic, amin.  Its STATUSES are compared with the product's first; the largest
             difference of the values is reported, not judged
  step       scan + combine_maps_device() per step, without and with a score_attitude of 4096 x 64; and, with --parent LIB (the
             parent commit's libgvom_hip.so), the same step without a query on that library, alternating, five runs each
  resources  tools/kernel_regs.py: the new kernels, and registers, scratch, LDS and code size of every kernel outside the new
             unit on the parent and on this library (--resources alone: no GPU needed)

    tools/attitude_bench.py [--resources] [--parent LIB] [--configs m256,c4] [--turns N] [out.json]      (default: profiles/attitude_<lib sha8>.json)
"""
import json
import sys
import tempfile
import time

import benchkit as bk

CONFIGS = {"m256": 100, "c4": 40}                          # config: timed steps per repetition
TURNS = 5
SHAPES = ((4096, 64), (16384, 128))
CAR = dict(front=3.6, rear=1.0, half_width=1.1)            # metres: tests/rollouts_ref.py CAR
CHASSIS = dict(front_axle=2.7, rear_axle=0.0, track=1.7, belly_height=0.25, max_pitch=0.35, max_roll=0.3, min_clearance=0.1)   # angles in radians
HEADINGS = 64
CHUNK = 512                                                # rollouts per chunk of the torch form
CHILD_TIMEOUT = 420                                        # seconds, per child process


def _vehicle(gvom, g):
    table = gvom.rectangle_footprint(CAR["front"], CAR["rear"], CAR["half_width"], g.xy_resolution, headings=HEADINGS)
    g.set_footprint(table)
    g.set_chassis(gvom.chassis(**CHASSIS))
    return table


def _poses(np, K, T, ego, res, seed=1):
    """K arcs of T poses from the ego, a cell a pose, float32 [K, T, 3]"""
    rng = np.random.default_rng(seed)
    th0 = rng.uniform(-np.pi, np.pi, K)
    curv = rng.uniform(-0.04, 0.04, K)
    t = np.arange(T)
    th = th0[:, None] + curv[:, None] * t[None, :]
    x = ego[0] + np.cumsum(res * np.cos(th), axis=1)
    y = ego[1] + np.cumsum(res * np.sin(th), axis=1)
    return np.ascontiguousarray(np.stack([x, y, th], axis=2).astype(np.float32))


def _torch_score(torch, gflat, poses, offs_pad, live, wheels, cs, ch, res, oc, xy):
    """the scoring in torch on the flat [y * xy + x] float64 ground: (values float32 [K, T, 3], status uint8 [K, T]).  offs_pad
    [H, Mmax, 2] with live [H, Mmax] (False on the padding); wheels [H, 4, 2], cs [H, 2] float64.  torch may contract a product and
    a sum: the values can differ from the product's in the last bits (reported, not judged)."""
    H = offs_pad.shape[0]
    s = torch.tensor(H / (2.0 * 3.141592653589793), dtype=torch.float32, device=poses.device)
    K, T = poses.shape[:2]
    vals = torch.zeros((K, T, 3), dtype=torch.float32, device=poses.device)
    status = torch.empty((K, T), dtype=torch.uint8, device=poses.device)
    wb, am = ch.front_axle - ch.rear_axle, 0.5 * (ch.front_axle + ch.rear_axle)
    inf = float("inf")
    for k0 in range(0, K, CHUNK):
        p = poses[k0:k0 + CHUNK]
        x, y = p[..., 0].double(), p[..., 1].double()
        qx, qy = x / res, y / res
        cx, cy = torch.floor(qx).long() - oc[0], torch.floor(qy).long() - oc[1]
        fx, fy = qx - torch.floor(qx), qy - torch.floor(qy)
        h = torch.remainder(torch.round(p[..., 2] * s).long(), H)
        w = wheels[h]                                              # [k, T, 4, 2]
        wx = torch.floor((x[..., None] + w[..., 0]) / res).long() - oc[0]
        wy = torch.floor((y[..., None] + w[..., 1]) / res).long() - oc[1]
        w_in = ((wx >= 0) & (wx < xy) & (wy >= 0) & (wy < xy)).all(dim=-1)
        z = gflat[wy.clamp(0, xy - 1) * xy + wx.clamp(0, xy - 1)]
        w_known = ((z > -1000.0) & (z < inf)).all(dim=-1)
        z = torch.where((w_in & w_known)[..., None], z, torch.zeros_like(z))
        sp = (0.5 * (z[..., 0] + z[..., 1]) - 0.5 * (z[..., 2] + z[..., 3])) / wb
        sr = (0.5 * (z[..., 0] + z[..., 2]) - 0.5 * (z[..., 1] + z[..., 3])) / ch.track
        z0 = 0.25 * ((z[..., 0] + z[..., 1]) + (z[..., 2] + z[..., 3]))
        o = offs_pad[h]                                            # [k, T, Mmax, 2]: the index tensor
        lv = live[h]
        X, Y = cx[..., None] + o[..., 0], cy[..., None] + o[..., 1]
        inside = (X >= 0) & (X < xy) & (Y >= 0) & (Y < xy)
        out = (lv & ~inside).any(dim=-1)
        gg = gflat[Y.clamp(0, xy - 1) * xy + X.clamp(0, xy - 1)]       # gather
        use = lv & inside & (gg > -1000.0) & (gg < inf)
        c, sn = cs[h][..., 0:1], cs[h][..., 1:2]
        du = ((o[..., 0].double() + 0.5) - fx[..., None]) * res
        dv = ((o[..., 1].double() + 0.5) - fy[..., None]) * res
        u, v = du * c + dv * sn, dv * c - du * sn
        clr = ((z0[..., None] + sp[..., None] * (u - am)) + sr[..., None] * v + ch.belly_height) - gg
        belly = torch.where(use, clr, torch.full_like(clr, inf)).amin(dim=-1)
        a = torch.stack([sp, sr, belly], dim=-1).float()
        st = torch.zeros_like(h, dtype=torch.uint8)
        st[a[..., 2] < ch.min_clearance] = 3
        st[a[..., 1].abs() > ch.max_roll] = 2
        st[a[..., 0].abs() > ch.max_pitch] = 1
        st[~w_known] = 4
        st[~w_in | out] = 5
        a[st >= 4] = 0
        vals[k0:k0 + CHUNK], status[k0:k0 + CHUNK] = a, st
    return vals, status


def child_score(name, profiled):
    np, torch, gvom, g, dev = bk.setup(name)
    for scan in dev:
        m = bk.scan_combine(np, g, scan)
    ego = dev[2][1]
    res, xy = g.xy_resolution, g.xy_size
    table = _vehicle(gvom, g)
    ch = gvom.chassis(**CHASSIS)
    e = gvom.world_to_cells([ego[:2]], res, m.origin)[0]
    f = m.cost_to_go([e], goals_in_cells=True, inflation_radius=None, density_threshold=50, soft_weight=10)
    cells = np.diff(table[0]).astype(np.int64)
    oc = tuple(int(v) for v in np.round(np.asarray(m.origin)[:2] / res))
    # the ground of the set's maps 4 and 5 as the library builds it, [y * xy + x]
    hgt, inf_h = torch.from_dlpack(m.height_map), torch.from_dlpack(m.inferred_height_map)
    gflat = torch.where(hgt > -1000.0, hgt, inf_h).T.contiguous().view(-1)
    mmax = int(cells.max())
    pad = np.zeros((HEADINGS, mmax, 2), np.int64)
    live = np.zeros((HEADINGS, mmax), bool)
    for k in range(HEADINGS):
        pad[k, :cells[k]] = table[1][table[0][k]:table[0][k + 1]]
        live[k, :cells[k]] = True
    offs_pad, live_t = torch.from_numpy(pad).cuda(), torch.from_numpy(live).cuda()
    half = ch.track / 2
    ab = ((ch.front_axle, half), (ch.front_axle, -half), (ch.rear_axle, half), (ch.rear_axle, -half))
    wheels = np.array([[(a * c - b * s, a * s + b * c) for a, b in ab] for c, s in g.cos_sin.tolist()])
    wheels_t, cs_t = torch.from_numpy(wheels).cuda(), torch.from_numpy(g.cos_sin).cuda()
    reps, results = 20, []
    for K, T in SHAPES:
        poses = _poses(np, K, T, ego, res)
        tp = torch.from_numpy(poses).cuda()
        torch.cuda.synchronize()
        by_set = lambda: g._score_attitude(m.set_id, None, gvom._dev(tp.data_ptr()), K, T, 1, True, m.origin)
        by_ptr = lambda: g.score_attitude_of_device(gflat.data_ptr(), tp.data_ptr(), K, T, origin=m.origin)
        rollouts = lambda: g.score_rollouts_of_device(f.cell_cost.ptr, tp.data_ptr(), K, T, cost_to_go_ptr=f.cost.ptr, origin=m.origin)
        calls = (("attitude_map_set", by_set), ("attitude_pointer", by_ptr), ("rollouts", rollouts))
        if profiled:                                           # under rocprofv3: `reps` launches per call, in this order
            for _, call in calls:
                for _ in range(reps):
                    call().release()
                bk.sync(g)
            continue
        out = {"xy": xy, "K": K, "T": T, "cells_per_heading_mean": round(float(cells.mean()), 1)}
        for what, call in calls:
            t = bk.timed(g, lambda: call().release(), reps, digits=2)
            out[what + "_call_us"], out[what + "_call_us_median"] = t["us"], t["us_median"]
        r = by_set()
        summary, att, status = r.copy_to_host()
        r2 = by_ptr()
        out["map_set_equals_pointer"] = bool(all(np.array_equal(a, b, equal_nan=True) for a, b in zip((summary, att, status), r2.copy_to_host())))
        r2.release()
        out["pose_status_counts"] = np.bincount(status.ravel(), minlength=7).tolist()
        out["rollout_status_counts"] = np.bincount(summary[:, 0], minlength=7).tolist()
        # the torch form on the exported maps (zero-copy), its statuses compared first, then timed
        tv, ts = _torch_score(torch, gflat, tp, offs_pad, live_t, wheels_t, cs_t, ch, res, oc, xy)
        tv, ts = tv.cpu().numpy(), ts.cpu().numpy()
        same = ts == status
        with np.errstate(invalid="ignore"):
            diff = np.abs(tv.astype(np.float64) - att.astype(np.float64))
            diff[~np.isfinite(diff)] = 0.0
            diff[(tv == att)] = 0.0
        torch.cuda.synchronize()
        tus = []
        for rep in range(5):
            t0 = time.perf_counter()
            _torch_score(torch, gflat, tp, offs_pad, live_t, wheels_t, cs_t, ch, res, oc, xy)
            torch.cuda.synchronize()
            tus.append(round((time.perf_counter() - t0) * 1e6, 1))
        out["torch"] = {"statuses_equal": bool(same.all()), "statuses_that_differ": int((~same).sum()),
                        "largest_value_difference_where_statuses_agree": float(diff[same].max()) if same.any() else None,
                        "us": tus, "us_median": bk.median(tus), "chunk_rollouts": CHUNK, "padded_cells_per_pose": mmax}
        r.release()
        results.append(out)
    return {"calls": reps, "order": ["attitude_map_set", "attitude_pointer", "rollouts"]} if profiled else {"scoring": results}


def child_step(name, steps, score):
    np, torch, gvom, g, dev = bk.setup(name)
    K, T = SHAPES[0]
    res = g.xy_resolution
    if score:
        _vehicle(gvom, g)
    tp = [torch.from_numpy(_poses(np, K, T, ego, res)).cuda() for _, ego, _ in dev]
    torch.cuda.synchronize()

    def step(k):
        m = bk.scan_combine(np, g, dev[k % 3])
        if score:
            g._score_attitude(m.set_id, None, gvom._dev(tp[k % 3].data_ptr()), K, T, 1, True, m.origin).release()
        m.release()
    return dict(bk.step_loop(g, step, steps, warm=min(10, steps)), K=K if score else 0, T=T if score else 0)


def _kernel_times(profile_dir, calls):
    """the dispatches of a profiled run in launch order: per shape and call the kernels' times without the first three launches"""
    rows = bk.kernel_trace_rows(profile_dir, ("k_attitude_ground", "k_attitude", "k_rollouts"))

    def stats(us):
        us = us[3:]
        return {"launches": len(us), "median_us": round(bk.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}
    out = []
    att, gnd, ro = ([u for _, kk, u in rows if kk == k] for k in ("k_attitude", "k_attitude_ground", "k_rollouts"))
    if len(att) != 2 * calls * len(SHAPES) or len(gnd) != calls * len(SHAPES) or len(ro) != calls * len(SHAPES):
        return None
    for n in range(len(SHAPES)):
        out.append({"k_attitude (map set route)": stats(att[2 * n * calls:(2 * n + 1) * calls]), "k_attitude_ground": stats(gnd[n * calls:(n + 1) * calls]),
                    "k_attitude (pointer route)": stats(att[(2 * n + 1) * calls:(2 * n + 2) * calls]), "k_rollouts": stats(ro[n * calls:(n + 1) * calls])})
    return out


def _table(parent):
    """every kernel outside the new unit, its figures on the parent beside those on this library"""
    import kernel_regs
    mine, theirs = kernel_regs.kernels(bk.NEW_LIB), kernel_regs.kernels(parent)
    keys = ("vgpr", "sgpr", "scratch", "lds", "code")
    return {k: {"parent": {q: (theirs.get(k) or {}).get(q) for q in keys}, "new": {q: v.get(q) for q in keys}}
            for k, v in sorted(mine.items()) if "k_attitude" not in k}


def main():
    if bk.child(sys.argv[1:], {"score": lambda a: child_score(a[0], a[1] == "1"), "step": lambda a: child_step(a[0], int(a[1]), a[2] == "1")}):
        return
    args = bk.read_args(sys.argv[1:], configs=CONFIGS, turns=TURNS)
    parent = args["parent"]
    spawn = lambda mode, a, **kw: bk.spawn(__file__, mode, a, CHILD_TIMEOUT, **kw)
    report, configs = bk.product_report(
        "attitude", args, {"footprint_metres": CAR, "chassis": CHASSIS, "headings": HEADINGS}, lambda k: "k_attitude" in k,
        ["footprints and chassis of other sizes", "maps larger than c4's 512 x 512", "shuffled poses",
         "static instead of dynamic LDS in k_attitude", "a summary made by a second kernel"])
    if parent:
        report.out["resources"]["other_kernels"]["table"] = _table(parent)
        report.save()
    if configs is None:
        return
    for name in args["configs"]:
        steps = CONFIGS[name]
        res = spawn("score", (name, 0))
        with tempfile.TemporaryDirectory() as d:
            prof = spawn("score", (name, 1), profile_dir=d)
            kernel = _kernel_times(d, prof["calls"])
        for k, rec in enumerate(res["scoring"]):
            rec["kernels"] = kernel[k] if kernel else "not measured (the trace did not hold the expected launches)"
        configs[name] = res
        report.save()
        runs = bk.alternate(args["turns"], {"parent_without": parent and (lambda: spawn("step", (name, steps, 0), lib=parent)),
                                            "without": lambda: spawn("step", (name, steps, 0)), "with": lambda: spawn("step", (name, steps, 1))})
        step = bk.spreads(runs)
        step["query_adds_us_per_step"] = round(step["with"]["median"] - step["without"]["median"], 2)
        res["step: scan + combine_maps_device (+ score_attitude %d x %d)" % SHAPES[0]] = bk.against_parent(step, "without", "parent_without", "without_")
        report.save()
    print(json.dumps(report.out, indent=1))


if __name__ == "__main__":
    main()
