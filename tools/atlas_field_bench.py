#!/usr/bin/env python3
"""What the atlas fields (gvom_atlas_cost_to_go, gvom_atlas_field_window: k_atlas_clearance_rows, k_clearance_cols, k_atlas_travcost,
k_ctg_seed / _relax / _dirs at the atlas's side, k_atlas_field_window) cost.  On m256 (256 x 256) and c4 (512 x 512): the config's
bench scans are driven through scan + combine_maps_device() + integrate(), then the last set is integrated at every tile of a FIXED
extent of A = 1024 and 4096 cells, so that the whole extent holds terrain.  Every loop in a fresh child process, every child under a
`timeout` of its own, and the first child that fails ends the run (the per-kernel part alone is best effort: its failure is noted):

  events     HIP events on the handle's stream around one call, medians: Atlas.cost_to_go() to a goal in the extent's first tile --
             without inflation and with inflation by a robot radius (ROBOT_RADIUS metres) --, with the rounds and tile relaxations of
             each; the same stopped after one round (front ends + seed + one round + directions); window(); and, for scale, the
             window-sized cost_to_go() of a recalled set with the same parameters.  The call waits: its events bracket the host's looks
             at the counters as well
  kernels    the same calls under `rocprofv3 --kernel-trace --stats` in a run of its own: average time per kernel
  step       scan + combine_maps_device() + integrate() per step: with a field per step, and without any atlas-field call; and, with
             --parent LIB (the parent commit's libgvom_hip.so), the call-free step on that library, alternating, five runs each: the
             median has to lie inside the parent's own run-to-run spread, which is written beside it
  resources  tools/kernel_regs.py: the new kernels, and registers, scratch, LDS and code size of every kernel that existed before on
             the parent and on this library (--resources alone: no GPU needed)

    tools/atlas_field_bench.py [--resources] [--parent LIB] [--configs m256,c4] [--turns N] [--sides 1024,4096] [out.json]
                                                                     (default: profiles/atlas_field_<lib sha8>.json)
"""
import json
import shutil
import sys
import tempfile

import benchkit as bk

CONFIGS = {"m256": 60, "c4": 30}                         # config: timed steps per repetition
TURNS = 5
SIDES = (1024, 4096)
ROBOT_RADIUS = 0.6                                        # metres
CHILD_TIMEOUT = 400                                       # seconds, per child process
NEW_KERNELS = ("k_atlas_clearance_rows", "k_atlas_travcost", "k_atlas_field_window")
SHOWN = ("k_atlas_clearance_rows", "k_clearance_cols", "k_atlas_travcost", "k_ctg_seed", "k_ctg_relax", "k_ctg_dirs", "k_atlas_field_window",
         "k_clearance_rows", "k_travcost", "k_atlas_merge", "k_atlas_recall")


def _filled(np, torch, gvom, g, dev, A):
    """the drive, then the last set at every tile of a fixed extent: (atlas, last set, extent origin, a goal in the first tile)"""
    m = None
    for scan in dev:
        m = bk.scan_combine(np, g, scan)
    xy = g.xy_size
    o = m.origin_cells[:2]
    a = g.create_atlas(A, follow=False, origin_cells=o)
    a.integrate(m)
    tm = [torch.from_dlpack(getattr(m, n)) for n in gvom.DEVICE_MAP_NAMES]
    ptrs = [t.data_ptr() for t in tm]
    for j in range(0, A, xy):
        for i in range(0, A, xy):
            a.integrate_of_device(ptrs, (o[0] + i, o[1] + j))
    pos, neg, vis = (getattr(m, n).copy_to_host() for n in ("positive", "negative", "visibility"))
    free = np.argwhere((pos <= 50) & (neg <= 0) & (vis > 0))
    goal = free[len(free) // 2]
    return a, m, o, (int(o[0] + goal[0]), int(o[1] + goal[1])), tm


def child_events(name, A, reps=7):
    np, torch, gvom, g, dev = bk.setup(name)
    a, m, o, goal, tm = _filled(np, torch, gvom, g, dev, A)
    stream = torch.cuda.ExternalStream(int(g._lib.gvom_stream(g._h)))

    def timed(call, n):
        return bk.timed_events(torch, stream, call, n)

    def solve(**kw):
        f = a.cost_to_go([goal], goals_in_cells=True, **kw)
        info = {"rounds": f.rounds, "tile_relaxations": g.get_tuning("atlas_field_tiles"), "reached": f.reached, "converged": f.converged}
        f.release()
        return info

    out = {"xy": g.xy_size, "A": A, "field_MiB": round(A * A * 7 / 2 ** 20, 1), "goal": goal}
    for label, kw in (("no inflation", {}), ("inflation %.1f m" % ROBOT_RADIUS, {"inflation_radius": ROBOT_RADIUS})):
        t, info = timed(lambda: solve(**kw), reps)
        out["cost_to_go, " + label] = dict(t, **info)
        t, info = timed(lambda: solve(max_rounds=1, **kw), reps)
        out["cost_to_go stopped after one round, " + label] = dict(t, **info)
    f = a.cost_to_go([goal], goals_in_cells=True)
    t, _ = timed(lambda: f.window(m).release(), 50)
    out["window() (k_atlas_field_window, xy x xy)"] = t
    f.release()
    rec = a.recall(origin_cells=o)
    local = [goal[0] - o[0], goal[1] - o[1]]
    for label, kw in (("no inflation", {}), ("inflation %.1f m" % ROBOT_RADIUS, {"inflation_radius": ROBOT_RADIUS})):
        def window_sized():
            w = rec.cost_to_go([local], goals_in_cells=True, **kw)
            info = {"rounds": w.rounds, "tile_relaxations": g.get_tuning("cost_to_go_tiles"), "reached": w.reached}
            w.release()
            return info
        t, info = timed(window_sized, 20)
        out["for scale: cost_to_go of the recalled set (xy x xy), " + label] = dict(t, **info)
    rec.release()
    del tm
    return out


def child_profiled(name, A):
    """the calls of child_events once more, three of each: run under rocprofv3 by the parent process"""
    np, torch, gvom, g, dev = bk.setup(name)
    a, m, o, goal, tm = _filled(np, torch, gvom, g, dev, A)
    for kw in ({}, {"inflation_radius": ROBOT_RADIUS}):
        for _ in range(3):
            with a.cost_to_go([goal], goals_in_cells=True, **kw) as f:
                f.window(m).release()
    bk.sync(g)
    del tm
    return {"calls": 6}


def child_step(name, steps, mode, A):
    np, torch, gvom, g, dev = bk.setup(name)
    a = g.create_atlas(A)
    goal = None

    def step(k):
        nonlocal goal
        m = bk.scan_combine(np, g, dev[k % 3])
        a.integrate(m)
        if mode:
            if goal is None:
                goal = [m.origin_cells[0] + g.xy_size // 2, m.origin_cells[1] + g.xy_size // 2]
            a.cost_to_go([goal], goals_in_cells=True).release()
        m.release()
    return bk.step_loop(g, step, steps, warm=min(10, steps))


def kernels_one_by_one(script, args, shown, limit, total=False):
    """average microseconds per kernel of `shown` from a kernel trace of `script`'s child "profiled", in a run of its own.  Best
    effort: the events stand without it, so its failure is noted and the run goes on"""
    if not shutil.which("rocprofv3"):
        return {"not_measured": "no rocprofv3 on this machine"}
    d = tempfile.mkdtemp(prefix="atlas_prof_")
    try:
        bk.spawn(script, "profiled", args, limit, profile_dir=d, stats=True)
        stats = bk.kernel_stats(d, total=total)
        if not stats:
            return {"not_measured": "the trace left no kernel_stats.csv"}
        out = {}
        for name, v in stats.items():
            if name.replace("void ", "") in shown:
                v["average_us"] = v.pop("avg_us")
                out[name.replace("void ", "")] = v
        return out
    except SystemExit as e:
        return {"not_measured": str(e)[:500]}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    if bk.child(sys.argv[1:], {"events": lambda a: child_events(a[0], int(a[1])), "profiled": lambda a: child_profiled(a[0], int(a[1])),
                               "step": lambda a: child_step(a[0], int(a[1]), int(a[2]), int(a[3]))}):
        return
    args = bk.read_args(sys.argv[1:], configs=CONFIGS, turns=TURNS, extra={"--sides": (list(SIDES), lambda s: [int(v) for v in s.split(",")])})
    parent, sides = args["parent"], args["sides"]
    spawn = lambda mode, a, **kw: bk.spawn(__file__, mode, a, CHILD_TIMEOUT, **kw)
    report, configs = bk.product_report(
        "atlas_field", args, {"sides": sides, "robot_radius_m": ROBOT_RADIUS}, lambda k: any(n in k for n in NEW_KERNELS),
        ["follow mode and a moving extent during the solve's fill", "goals far from the first tile, more than one goal",
         "soft and roughness weights, unknown=\"blocked\"", "windows other than the config's own",
         "terrain other than the config's set repeated over the extent: the round count depends on it"])
    if configs is None:
        return
    for name in args["configs"]:
        steps = CONFIGS[name]
        res = configs.setdefault(name, {})
        res["events"] = {"A %d" % A: spawn("events", (name, A)) for A in sides}
        report.save()
        res["kernels one by one (rocprofv3 --kernel-trace --stats, a run of its own)"] = {
            "A %d" % A: kernels_one_by_one(__file__, (name, A), SHOWN, CHILD_TIMEOUT) for A in sides}
        report.save()
        runs = bk.alternate(args["turns"], {"parent_without": parent and (lambda: spawn("step", (name, steps, 0, 1024), lib=parent)),
                                            "without": lambda: spawn("step", (name, steps, 0, 1024)),
                                            "field_per_step": lambda: spawn("step", (name, max(5, steps // 6), 1, 1024))})
        step = bk.spreads(runs)
        step["a_field_per_step_adds_us_per_step"] = round(step["field_per_step"]["median"] - step["without"]["median"], 2)
        res["step: scan + combine_maps_device + integrate (+ a field per step), A 1024"] = bk.against_parent(step, "without", "parent_without", "without_")
        report.save()
    print(json.dumps(report.out, indent=1))


if __name__ == "__main__":
    main()
