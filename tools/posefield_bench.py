#!/usr/bin/env python3
"""What a pose field (gvom_pose_field: k_cspace, k_pose_seed, k_pose_relax, k_pose_actions) costs.  On the cost fields of m256 and c4
after three bench scans (combine_maps_device() -> cost_to_go() without inflation), a 2.2 m x 4.6 m car footprint, H = 16 and 64
headings, arc primitives with reach 4, a goal near the ego and one far from it (the dearest cell of the near goal's 2-D field at
which the car can stand) -- every loop in a fresh child process, every child
under a `timeout` of its own, and the first child that fails ends the run:

  call       DeviceCostField.pose_field(), enqueue to the waited-for result: wall time, rounds, tile relaxations, what it reached; and
             the 2-D cost_to_go() on the same map
  kernel     one `rocprofv3 --kernel-trace` run per config: k_cspace, k_pose_relax (all rounds), k_pose_seed, k_pose_actions per call
  others     (m256, H = 16, near goal) scipy.sparse.csgraph.dijkstra on the same graph -- construction timed apart -- first shown
             equal to the product; and the same relaxation as whole-volume torch sweeps on the GPU, first shown equal
  step       scan + combine_maps_device() + cost_to_go() per step, without and with a pose field (H = 16, near goal); and, with
             --parent LIB (the parent commit's libgvom_hip.so), the same step without on that library, alternating, five runs each
  resources  tools/kernel_regs.py: the new kernels, and registers, scratch, LDS and code size of every kernel outside the new unit
             on the parent and on this library (--resources alone: no GPU needed)

The 6 m turning radius: an arc of 4 cells of 0.2 m turns by 0.133 rad, one bin of H = 64 (0.098 rad) but not one of H = 16 (0.393 rad),
where arc_primitives raises; H = 16 is measured with a 2 m radius, the largest whole metre that reaches the next bin.

    tools/posefield_bench.py [--resources] [--parent LIB] [--configs m256,c4] [--turns N] [out.json]   (default: profiles/posefield_<lib sha8>.json)
"""
import json
import math
import sys
import tempfile
import time

import benchkit as bk

CONFIGS = {"m256": 60, "c4": 24}                          # config: timed steps per repetition
TURNS = 5
CAR = dict(front=3.6, rear=1.0, half_width=1.1)
SHAPES = ((16, 2.0), (64, 6.0))                           # (headings, minimum turning radius in metres)
GOALS = ("near", "far")
CHILD_TIMEOUT = 300                                       # seconds, per child process
KERNELS = ("k_cspace", "k_pose_relax", "k_pose_seed", "k_pose_actions")


def _tables(gvom, g, H, radius):
    footprint = gvom.rectangle_footprint(xy_resolution=g.xy_resolution, headings=H, **CAR)
    g.set_footprint(footprint)
    table = gvom.arc_primitives(H, radius, g.xy_resolution, reach=4)
    g.set_primitives(table)
    return table, int(footprint[0][1])


def _goal(np, gvom, m, g, ego, which):
    """(1, 2) window cells, every heading a goal.  near: 2 m ahead of the ego.  far: the dearest cell of the near goal's 2-D field at
    which the car can stand on some heading (a pose cost != 0): sure to seed.  It need not be a state anything can DRIVE to: on the
    maps of profiles/posefield_c3862c46.json it is a pocket of one state, and the far entries there measure k_cspace only."""
    near = gvom.world_to_cells(np.array([[ego[0] + 2.0, ego[1]]]), g.xy_resolution, m.origin)
    if which == "near":
        return near
    with m.cost_to_go(near, goals_in_cells=True) as field:
        D = field.cost.copy_to_host().astype(np.int64)
        with field.pose_field(near, goals_in_cells=True) as f:
            stands = (f.pose_cost.copy_to_host() != 0).any(axis=0)
    D[~stands | (D == 2 ** 31 - 1)] = -1
    x, y = np.unravel_index(int(np.argmax(D)), D.shape)
    return np.array([[x, y]], np.int64)


def _graph(np, C, table):
    """the reversed graph of the definition as a scipy CSR matrix: an edge v -> u of weight w * (C[u] + C[v]) per admissible primitive"""
    import scipy.sparse as sp
    H, xy, _ = C.shape
    start, prims = table
    idx = np.arange(H * xy * xy, dtype=np.int64).reshape(H, xy, xy)
    rows, cols, vals = [], [], []
    for h in range(H):
        for dx, dy, ht, w in prims[start[h]:start[h + 1]].astype(np.int64):
            x0, x1, y0, y1 = max(0, -dx), min(xy, xy - dx), max(0, -dy), min(xy, xy - dy)
            cu, cv = C[h, x0:x1, y0:y1].astype(np.int64), C[ht, x0 + dx:x1 + dx, y0 + dy:y1 + dy].astype(np.int64)
            ok = (cu != 0) & (cv != 0)
            rows.append(idx[ht, x0 + dx:x1 + dx, y0 + dy:y1 + dy][ok])
            cols.append(idx[h, x0:x1, y0:y1][ok])
            vals.append((w * (cu + cv))[ok])
    n = H * xy * xy
    return sp.csr_matrix((np.concatenate(vals).astype(np.float64), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))


def _torch_sweeps(torch, C, D0, table, cap):
    """the same relaxation as whole-volume sweeps (one shifted add and minimum per primitive) until a sweep changes nothing"""
    H, xy, _ = C.shape
    start, prims = table
    U = 2 ** 31 - 1
    C = C.to(torch.int64)
    D = D0.clone()
    sweeps = 0
    while True:
        before = D.clone()
        for h in range(H):
            for dx, dy, ht, w in prims[start[h]:start[h + 1]].tolist():
                x0, x1, y0, y1 = max(0, -dx), min(xy, xy - dx), max(0, -dy), min(xy, xy - dy)
                cu, cv = C[h, x0:x1, y0:y1], C[ht, x0 + dx:x1 + dx, y0 + dy:y1 + dy]
                dv = D[ht, x0 + dx:x1 + dx, y0 + dy:y1 + dy]
                cand = torch.where((cu != 0) & (cv != 0) & (dv < U), dv + w * (cu + cv), torch.full_like(dv, U))
                cand = torch.where(cand <= cap, cand, torch.full_like(cand, U))
                D[h, x0:x1, y0:y1] = torch.minimum(D[h, x0:x1, y0:y1], cand)
        sweeps += 1
        if torch.equal(before, D):
            return D, sweeps


def child_call(name, profiled):
    np, torch, gvom, g, dev = bk.setup(name)
    for scan in dev:
        m = bk.scan_combine(np, g, scan)
    ego = dev[2][1]
    reps, results = 5, {}
    for H, radius in SHAPES:
        table, fp_cells = _tables(gvom, g, H, radius)
        for which in GOALS:
            goal = _goal(np, gvom, m, g, ego, which)
            key = "H%d_%s" % (H, which)
            field = m.cost_to_go(goal, goals_in_cells=True)
            call = lambda: field.pose_field(goal, goals_in_cells=True)
            if profiled:
                for _ in range(reps + 3):
                    call().release()
                field.release()
                continue
            us = bk.timed(None, lambda: call().release(), reps)["us"]      # (the call waits itself)
            f = call()
            out = {"xy": g.xy_size, "H": H, "goal_cell": [int(v) for v in goal[0]], "min_turn_radius_m": radius, "primitives_per_heading": int(table[0][1]), "halo_cells": int(np.abs(table[1][:, :2]).max()),
                   "footprint_cells_heading_0": fp_cells,
                   "call_us": us, "call_us_median": bk.median(us), "rounds": f.rounds, "tile_relaxations": g.get_tuning("pose_field_tiles"),
                   "tiles": int(math.ceil(g.xy_size / 8.0)) ** 2, "reached_states": f.reached, "seeded_states": f.goals_seeded, "converged": f.converged}
            two = bk.timed(None, lambda: m.cost_to_go(goal, goals_in_cells=True).release(), reps, warm=0)["us"]
            out["cost_to_go_2d_same_map"] = {"call_us": two, "call_us_median": bk.median(two), "rounds": field.rounds, "reached_cells": field.reached}
            if name == "m256" and H == 16 and which == "near":
                try:
                    import scipy.sparse.csgraph as csg
                    D, _, C = f.copy_to_host()
                    t0 = time.perf_counter()
                    G = _graph(np, C, table)
                    t1 = time.perf_counter()
                    seeds = np.flatnonzero(D.reshape(-1) == 0)
                    dist = csg.dijkstra(G, directed=True, indices=seeds, min_only=True)
                    t2 = time.perf_counter()
                    same = bool(np.array_equal(np.where(np.isfinite(dist) & (dist <= 2 ** 30), dist, 2 ** 31 - 1).astype(np.int64), D.reshape(-1).astype(np.int64)))
                    out["scipy_dijkstra_same_graph"] = {"equal_to_the_product": same, "graph_construction_ms": round((t1 - t0) * 1e3, 1),
                                                        "dijkstra_ms": round((t2 - t1) * 1e3, 1), "edges": int(G.nnz)}
                    tC = torch.from_dlpack(f.pose_cost)
                    tD = torch.from_dlpack(f.cost).to(torch.int64)
                    D0 = torch.where(tD == 0, torch.zeros_like(tD), torch.full_like(tD, 2 ** 31 - 1))
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    Dt, sweeps = _torch_sweeps(torch, tC, D0, (table[0], table[1]), 2 ** 30)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    out["torch_sweeps_same_relaxation"] = {"equal_to_the_product": bool(torch.equal(Dt, tD)), "sweeps": sweeps, "ms": round((t1 - t0) * 1e3, 1)}
                    del tC, tD, D0, Dt
                except Exception as e:                              # (a comparison that cannot run is named, the run goes on)
                    out["others_not_measured"] = repr(e)[:300]
            f.release()
            field.release()
            results[key] = out
    return {"calls": reps + 3} if profiled else results


def child_step(name, steps, with_field):
    np, torch, gvom, g, dev = bk.setup(name)
    if with_field:
        _tables(gvom, g, *SHAPES[0])

    def step(k):
        ego = dev[k % 3][1]
        m = bk.scan_combine(np, g, dev[k % 3])
        goal = np.array([[ego[0] + 2.0, ego[1]]])
        f = m.cost_to_go(goal)
        if with_field:
            f.pose_field(goal).release()
        f.release()
        m.release()
    return bk.step_loop(g, step, steps, warm=min(6, steps))


def _kernel_times(profile_dir, calls):
    """per shape and goal (k_pose_actions ends a call): the kernels' microseconds per call, without the first three calls"""
    rows = bk.kernel_trace_rows(profile_dir, KERNELS)
    ends = [i for i, r in enumerate(rows) if r[1] == "k_pose_actions"]
    keys = ["H%d_%s" % (H, which) for H, _ in SHAPES for which in GOALS]
    extra = [1 if key.endswith("far") else 0 for key in keys]      # choosing the far goal makes one pose field of its own, first
    if len(ends) != calls * len(keys) + sum(extra):
        return None
    out, at = {}, 0
    for n, key in enumerate(keys):
        at += extra[n]
        first = ends[at + 2] + 1                                   # behind the third call of the shape
        last = ends[at + calls - 1] + 1
        at += calls
        part, used = rows[first:last], calls - 3
        rec = {}
        for k in KERNELS:
            us = [u for _, kk, u in part if kk == k]
            rec[k] = {"launches_per_call": round(len(us) / used, 2), "us_per_call": round(sum(us) / used, 2), "median_us_per_launch": round(bk.median(us), 2) if us else None}
        rec["device_us_per_call"] = round(sum(u for _, _, u in part) / used, 2)
        out[key] = rec
    return out


def main():
    if bk.child(sys.argv[1:], {"call": lambda a: child_call(a[0], a[1] == "1"), "step": lambda a: child_step(a[0], int(a[1]), a[2] == "1")}):
        return
    args = bk.read_args(sys.argv[1:], configs=CONFIGS, turns=TURNS)
    parent = args["parent"]
    spawn = lambda mode, a, **kw: bk.spawn(__file__, mode, a, CHILD_TIMEOUT, **kw)
    report, configs = bk.product_report(
        "posefield", args, {"car_m": CAR, "shapes": [list(s) for s in SHAPES], "goals": list(GOALS), "reach_cells": 4},
        lambda k: "k_cspace" in k or "k_pose_" in k,
        ["c5", "H = 16 with a 6 m radius (arc_primitives raises: 0.8 m of arc does not reach the next of 16 headings)",
         "a row-span or sliding-maximum k_cspace in LDS (not built)", "tiles other than 8 x 8 cells x all headings (not built)",
         "scipy and the torch sweeps beyond m256, H = 16, near goal", "reverse primitives", "the host and device-pointer routes",
         "pose_field_inner / pose_field_batch other than the defaults", "hardware counters, LDS bank conflicts of k_pose_relax"])
    report.out["resources"]["k_pose_relax_dynamic_lds_bytes"] = "6 * H * (8 + 2 * halo)^2: 18,816 at H = 16, halo 3; 98,304 at H = 64, halo 4"
    report.save()
    if configs is None:
        return
    for name in args["configs"]:
        steps = CONFIGS[name]
        res = spawn("call", (name, 0))
        with tempfile.TemporaryDirectory() as d:
            prof = spawn("call", (name, 1), profile_dir=d)
            kernel = _kernel_times(d, prof["calls"])
        for key in res:
            res[key]["kernels"] = kernel[key] if kernel else "not measured (the trace did not hold the expected launches)"
        configs[name] = res
        report.save()
        runs = bk.alternate(args["turns"], {"parent_without": parent and (lambda: spawn("step", (name, steps, 0), lib=parent)),
                                            "without": lambda: spawn("step", (name, steps, 0)), "with": lambda: spawn("step", (name, steps, 1))})
        step = bk.spreads(runs)
        step["pose_field_adds_us_per_step"] = round(step["with"]["median"] - step["without"]["median"], 2)
        res["step: scan + combine_maps_device + cost_to_go (+ a pose field of H = 16, near goal)"] = bk.against_parent(step, "without", "parent_without", "without_")
        report.save()
    print(json.dumps(report.out, indent=1))


if __name__ == "__main__":
    main()
