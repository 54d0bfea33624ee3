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

    tools/costfield_bench.py [out.json]      (default: profiles/costfield_<lib sha8>.json)
"""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "g-vom_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
CONFIGS = (("m256", 100), ("c4", 40), ("c5", 15))           # (config, timed steps per repetition)
THRESHOLD, SOFT = 50, 10
KERNELS = ("k_travcost", "k_ctg_", "k_clearance")
STEPS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))
UNREACHED = 2 ** 31 - 1


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def _setup(name):
    import numpy as np
    import torch
    import gvom
    import synth
    torch.cuda.init()
    params, scans = synth.config_inputs(name, n_scans=3)
    dev = [(torch.from_numpy(np.ascontiguousarray(pc)).cuda(), ego, tf) for pc, ego, tf in scans]
    torch.cuda.synchronize()
    g = gvom.Gvom(*params, voxel_statistics=False)
    return np, torch, gvom, g, dev


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
    np, torch, gvom, g, dev = _setup(name)

    def scan(k):
        t, ego, tf = dev[k % 3]
        g.process_pointcloud_device(t.data_ptr(), t.shape[0], np.float32, ego, tf)
        return g.combine_maps_device()

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
        rec["call_us_median"] = _median(rec["call_us"][1:])
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
        rec["without_inflation"] = dict(wide, call_us_median=_median(us[1:]))
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
        alts["inner %d, batch %d" % (inner, batch)] = {"call_us_median": _median(us[1:]), "rounds": rounds, "tile_relaxations": tiles}
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
        for k in range(min(10, steps)):
            step(k)
        g._check(g._lib.gvom_sync(g._h))
        us = []
        for rep in range(3):
            t0 = time.perf_counter()
            for k in range(steps):
                step(k)
            g._check(g._lib.gvom_sync(g._h))
            us.append(round((time.perf_counter() - t0) / steps * 1e6, 2))
        out[label] = {"us_per_step": us, "us_per_step_median": _median(us)}
    return out


def child_kernels(name, gx, gy):
    """Run under rocprofv3: the calls whose kernels are to be timed."""
    np, torch, gvom, g, dev = _setup(name)
    for t, ego, tf in dev:
        g.process_pointcloud_device(t.data_ptr(), t.shape[0], np.float32, ego, tf)
        m = g.combine_maps_device()
    for _ in range(20):
        m.cost_to_go([(gx, gy)], **_field_args(g)).release()
    g._check(g._lib.gvom_sync(g._h))
    return {"calls": 20}


def _spawn(mode, args, profile_dir=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode] + [str(a) for a in args]
    if profile_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", profile_dir, "--"] + cmd
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit("%s %r failed (%d):\n%s" % (mode, args, r.returncode, r.stderr[-3000:]))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def _kernel_stats(profile_dir, calls):
    rows = {}
    for f in glob.glob(os.path.join(profile_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if any(k in r["Name"] for k in KERNELS):
                rows[r["Name"].split("(")[0]] = {"launches_per_call": round(int(r["Calls"]) / calls, 2), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                                                 "us_per_call": round(float(r["TotalDurationNs"]) / 1e3 / calls, 2)}
    return rows


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        mode = sys.argv[2]
        res = child_step(sys.argv[3], int(sys.argv[4])) if mode == "step" else child_kernels(sys.argv[3], int(sys.argv[4]), int(sys.argv[5]))
        print("RESULT " + json.dumps(res))
        return
    import kernel_regs
    import lib_identity
    new = os.path.join(ROOT, "g-vom_amd", "lib", "libgvom_hip.so")
    out = {"library": lib_identity.identity(), "density_threshold": THRESHOLD, "soft_weight": SOFT, "inflation": "robot_radius",
           "registers": {k: v for k, v in kernel_regs.kernels(new).items() if "k_ctg_" in k or "k_travcost" in k},
           "unmeasured": ["tile sizes other than 32 x 32 and a launch over a compacted tile list (neither is built)",
                          "maps larger than c5's 1024 x 1024"],
           "configs": {}}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
        ROOT, "profiles", "costfield_%s.json" % (out["library"].get("lib_sha256") or "unknown")[:8])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    for name, steps in CONFIGS:
        res = _spawn("step", (name, steps))
        res["kernel_us"] = {}
        for label, goal in res["goals"].items():
            with tempfile.TemporaryDirectory() as d:
                calls = _spawn("kernels", (name, goal[0], goal[1]), profile_dir=d)["calls"]
                stats = _kernel_stats(d, calls)
            stats["all"] = round(sum(v["us_per_call"] for v in stats.values()), 2)
            res["kernel_us"][label] = stats
        base = res["scan+combine_maps_device"]["us_per_step_median"]
        res["added_us_per_step"] = {k[1:]: round(v["us_per_step_median"] - base, 2) for k, v in res.items()
                                    if k.startswith("+") and isinstance(v, dict)}
        out["configs"][name] = res
        with open(path, "w") as f:                                  # (after every config: a long run leaves what it has)
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
