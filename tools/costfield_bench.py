#!/usr/bin/env python3
"""What a cost-to-go field (gvom_cost_to_go) costs.  On the maps of m256, c4 and c5 after three bench scans, towards two goals -- the
unblocked cell nearest the ego, and the cell of its field furthest from it ("far") -- every loop in a fresh child process:

  call       DeviceMaps.cost_to_go() end to end (inflation = robot_radius, soft_weight 10): wall time, rounds, tile relaxations,
             reached cells; and the same call with other inner bounds and batch lengths (the alternatives tried)
  kernels    one `rocprofv3 --kernel-trace --stats` run per config and goal: k_travcost, k_ctg_seed, k_ctg_relax, k_ctg_dirs and the
             clearance kernels of the inflation
  step       scan + combine_maps_device() per step, without and with a field per step
  baselines  on the product's own cost map, each CHECKED EQUAL to the product before it is timed: the same min-relaxation as torch
             sweeps on the GPU to its fixed point (whole-map Jacobi sweeps, convergence looked at every 32 sweeps), and a CPU
             Dijkstra (scipy.sparse.csgraph.dijkstra where importable, otherwise the heap form of tests/costfield_ref.py)
  registers  tools/kernel_regs.py on the four kernels

    tools/costfield_bench.py [--configs m256,c4,c5] [out.json]      (default: profiles/costfield_<lib sha8>.json)
"""
import json
import os
import sys
import tempfile
import time

import benchkit as bk

sys.path.insert(0, os.path.join(bk.ROOT, "tests"))
CONFIGS = {"m256": 100, "c4": 40, "c5": 15}                 # config: timed steps per repetition
CHILD_TIMEOUT = 900                                         # seconds, per child process
THRESHOLD, SOFT = 50, 10
KERNELS = ("k_travcost", "k_ctg_", "k_clearance")
STEPS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))
UNREACHED = 2 ** 31 - 1


def _field_args(g):
    return dict(goals_in_cells=True, inflation_radius=float(g.robot_radius), density_threshold=THRESHOLD, soft_weight=SOFT)


def _goals(np, gvom, g, m, ego):
    """the unblocked cell nearest the ego ("ego"), and the reached cell of its field that lies furthest from it ("far")"""
    e = gvom.world_to_cells([ego[:2]], g.xy_resolution, m.origin)[0]
    with m.cost_to_go([e], **_field_args(g)) as f:
        c = f.cell_cost.copy_to_host()
    xs, ys = np.nonzero(c > 0)
    k = int(np.argmin((xs - e[0]) ** 2 + (ys - e[1]) ** 2))
    e = (int(xs[k]), int(ys[k]))
    with m.cost_to_go([e], **_field_args(g)) as f:
        D = f.cost.copy_to_host()
    xs, ys = np.nonzero(D != UNREACHED)
    k = int(np.argmax(np.abs(xs - e[0]) + np.abs(ys - e[1])))
    return {"ego": [e[0], e[1]], "far": [int(xs[k]), int(ys[k])]}


def _torch_field(torch, c, goal, check_every=32):
    """the field of an [x, y] int32 cost tensor by whole-map Jacobi sweeps in torch; returns (D int32, sweeps)"""
    xy = c.shape[0]
    big = 1 << 40
    c = c.to(torch.int64)
    pad = torch.zeros((xy + 2, xy + 2), dtype=torch.int64, device=c.device)
    pad[1:-1, 1:-1] = c
    at = lambda t, dx, dy: t[1 + dx:xy + 1 + dx, 1 + dy:xy + 1 + dy]
    w = []
    for k, (dx, dy) in enumerate(STEPS):
        ok = (c > 0) & (at(pad, dx, dy) > 0)
        if k & 1:
            ok = ok & (at(pad, dx, 0) > 0) & (at(pad, 0, dy) > 0)
        w.append(torch.where(ok, (7 if k & 1 else 5) * (c + at(pad, dx, dy)), big))
    D = torch.full((xy + 2, xy + 2), big, dtype=torch.int64, device=c.device)
    if int(c[goal[0], goal[1]]) > 0:
        D[1 + goal[0], 1 + goal[1]] = 0
    sweeps = 0
    while True:
        before = D.clone()
        for _ in range(check_every):
            best = at(D, 0, 0)
            for wk, (dx, dy) in zip(w, STEPS):
                best = torch.minimum(best, at(D, dx, dy) + wk)
            best = torch.where(best <= (1 << 30), best, at(D, 0, 0))
            D[1:-1, 1:-1] = best
        sweeps += check_every
        if bool((D == before).all()):                      # (the one host synchronisation per 32 sweeps)
            break
    inner = D[1:-1, 1:-1]
    return torch.where(inner >= big, UNREACHED, inner).to(torch.int32), sweeps


def _cpu_dijkstra(np, c, goal):
    """(D int32 [x, y], which) by scipy's Dijkstra on the explicit graph, or by the referee's heap form"""
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import dijkstra
    except ImportError:
        import costfield_ref as cf
        return cf.dijkstra(c, [goal]), "tests/costfield_ref.py heap"
    import costfield_ref as cf
    xy = c.shape[0]
    idx = np.arange(xy * xy).reshape(xy, xy)
    rows, cols, vals = [], [], []
    for wk, (dx, dy) in zip(cf.weights(c), STEPS):
        ok = wk < cf.INF
        u = idx[ok]
        xs, ys = np.nonzero(ok)
        rows.append(u); cols.append(idx[xs + dx, ys + dy]); vals.append(wk[ok])
    G = sp.csr_matrix((np.concatenate(vals).astype(np.float64), (np.concatenate(rows), np.concatenate(cols))), shape=(xy * xy, xy * xy))
    d = dijkstra(G, directed=True, indices=int(idx[goal[0], goal[1]]), limit=float(1 << 30))      # (weights < 2^53: exact in float64)
    if c[goal[0], goal[1]] <= 0:
        d[:] = np.inf
    return np.where(np.isfinite(d), d, UNREACHED).astype(np.int64).astype(np.int32).reshape(xy, xy), "scipy.sparse.csgraph.dijkstra"


def child_step(name, steps):
    np, torch, gvom, g, dev = bk.setup(name)

    def scan(k):
        return bk.scan_combine(np, g, dev[k % 3])

    for k in range(3):
        m = scan(k)
    goals = _goals(np, gvom, g, m, dev[2][1])
    out = {"xy": g.xy_size, "goals": goals, "steps": steps, "field": {}}
    kw = _field_args(g)
    for label, goal in goals.items():
        rec = {}
        for trial in range(7):                                  # the whole call, map set -> product, waited for
            t0 = time.perf_counter()
            f = m.cost_to_go([goal], **kw)
            rec.setdefault("call_us", []).append(round((time.perf_counter() - t0) * 1e6, 1))
            if trial < 6:
                f.release()
        rec["call_us_median"] = bk.median(rec["call_us"][1:])
        rec.update(rounds=f.rounds, converged=f.converged, reached=f.reached, goals_seeded=f.goals_seeded,
                   tile_relaxations=g.get_tuning("cost_to_go_tiles"), tiles=((g.xy_size + 31) // 32) ** 2)
        D, _, c = f.copy_to_host()
        c = c.astype(np.int32)
        rec["blocked_cells"] = int((c == 0).sum())
        # baseline 1: torch sweeps on the GPU, on the product's own cost map (zero-copy), checked, then timed
        tc = torch.from_dlpack(f.cell_cost).to(torch.int32)
        tD, sweeps = _torch_field(torch, tc, goal)
        same = bool(np.array_equal(tD.cpu().numpy(), D))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _torch_field(torch, tc, goal)
        torch.cuda.synchronize()
        rec["torch_sweeps"] = {"equals_product": same, "sweeps": sweeps, "us": round((time.perf_counter() - t0) * 1e6, 1)}
        del tc, tD
        # baseline 2: Dijkstra on the CPU
        cD, which = _cpu_dijkstra(np, c, goal)
        t0 = time.perf_counter()
        _cpu_dijkstra(np, c, goal)
        rec["cpu_dijkstra"] = {"form": which, "equals_product": bool(np.array_equal(cD, D)), "us": round((time.perf_counter() - t0) * 1e6, 1),
                               "includes": "building the graph from the cost map"}
        f.release()
        # the same goal on the uninflated map (more of it is free): the call only
        open_kw = dict(kw, inflation_radius=None)
        us = []
        for trial in range(6):
            t0 = time.perf_counter()
            f = m.cost_to_go([goal], **open_kw)
            us.append(round((time.perf_counter() - t0) * 1e6, 1))
            wide = {"rounds": f.rounds, "reached": f.reached, "tile_relaxations": g.get_tuning("cost_to_go_tiles")}
            f.release()
        rec["without_inflation"] = dict(wide, call_us_median=bk.median(us[1:]))
        out["field"][label] = rec
    # the alternatives tried: inner bound and batch length, whole call towards the far goal (tile size 32 and all-tiles launches
    # are the only forms built)
    far = goals.get("far", goals["ego"])
    alts = {}
    for inner, batch in ((32, 8), (64, 8), (256, 4), (256, 8), (256, 16), (1024, 8)):
        g.set_tuning("cost_to_go_inner", inner)
        g.set_tuning("cost_to_go_batch", batch)
        us = []
        for trial in range(6):
            t0 = time.perf_counter()
            f = m.cost_to_go([far], **kw)
            us.append(round((time.perf_counter() - t0) * 1e6, 1))
            rounds, tiles = f.rounds, g.get_tuning("cost_to_go_tiles")
            f.release()
        alts["inner %d, batch %d" % (inner, batch)] = {"call_us_median": bk.median(us[1:]), "rounds": rounds, "tile_relaxations": tiles}
    g.set_tuning("cost_to_go_inner", 0)
    g.set_tuning("cost_to_go_batch", 0)
    out["alternatives_far_goal"] = alts
    m.release()

    def plain(k):
        scan(k).release()

    def with_field(goal):
        def step(k):
            mm = scan(k)
            mm.cost_to_go([goal], **kw).release()
            mm.release()
        return step

    loops = [("scan+combine_maps_device", plain)] + [("+field to the %s goal" % label, with_field(goal)) for label, goal in goals.items()]
    for label, step in loops:
        out[label] = bk.step_loop(g, step, steps, warm=min(10, steps))
        del out[label]["steps"]                                # (the record's own "steps" says it)
    return out


def child_kernels(name, gx, gy):
    """Run under rocprofv3: the calls whose kernels are to be timed."""
    np, torch, gvom, g, dev = bk.setup(name)
    for scan in dev:
        m = bk.scan_combine(np, g, scan)
    for _ in range(20):
        m.cost_to_go([(gx, gy)], **_field_args(g)).release()
    bk.sync(g)
    return {"calls": 20}


def main():
    if bk.child(sys.argv[1:], {"step": lambda a: child_step(a[0], int(a[1])), "kernels": lambda a: child_kernels(a[0], int(a[1]), int(a[2]))}):
        return
    import kernel_regs
    args = bk.read_args(sys.argv[1:], has_parent=False, has_resources=False, configs=CONFIGS)
    report = bk.Report("costfield", args["path"], fresh=True)
    out = report.out
    out.update({"density_threshold": THRESHOLD, "soft_weight": SOFT, "inflation": "robot_radius",
                "registers": {k: v for k, v in kernel_regs.kernels(bk.NEW_LIB).items() if "k_ctg_" in k or "k_travcost" in k},
                "unmeasured": ["tile sizes other than 32 x 32 and a launch over a compacted tile list (neither is built)",
                               "maps larger than c5's 1024 x 1024"],
                "configs": {}})
    for name in args["configs"]:
        res = bk.spawn(__file__, "step", (name, CONFIGS[name]), CHILD_TIMEOUT)
        res["kernel_us"] = {}
        for label, goal in res["goals"].items():
            with tempfile.TemporaryDirectory() as d:
                calls = bk.spawn(__file__, "kernels", (name, goal[0], goal[1]), CHILD_TIMEOUT, profile_dir=d, stats=True)["calls"]
                stats = {k: {"launches_per_call": round(v["calls"] / calls, 2), "avg_us": v["avg_us"], "us_per_call": round(v["total_us"] / calls, 2)}
                         for k, v in bk.kernel_stats(d, KERNELS, total=True).items()}
            stats["all"] = round(sum(v["us_per_call"] for v in stats.values()), 2)
            res["kernel_us"][label] = stats
        base = res["scan+combine_maps_device"]["us_per_step_median"]
        res["added_us_per_step"] = {k[1:]: round(v["us_per_step_median"] - base, 2) for k, v in res.items()
                                    if k.startswith("+") and isinstance(v, dict)}
        out["configs"][name] = res
        report.save()                                              # (after every config: a long run leaves what it has)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
