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

    tools/atlas_field_bench.py [--resources] [--parent LIB] [--configs m256,c4] [--sides 1024,4096] [out.json]
                                                                     (default: profiles/atlas_field_<lib sha8>.json)
"""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "g-vom_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CONFIGS = {"m256": 60, "c4": 30}                         # config: timed steps per repetition
SIDES = (1024, 4096)
ROBOT_RADIUS = 0.6                                        # metres
CHILD_TIMEOUT = 400                                       # seconds, per child process
NEW_KERNELS = ("k_atlas_clearance_rows", "k_atlas_travcost", "k_atlas_field_window")
SHOWN = ("k_atlas_clearance_rows", "k_clearance_cols", "k_atlas_travcost", "k_ctg_seed", "k_ctg_relax", "k_ctg_dirs", "k_atlas_field_window",
         "k_clearance_rows", "k_travcost", "k_atlas_merge", "k_atlas_recall")


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def _gvom():
    """The binding, also over the parent's library: it is bound with the entry points it has."""
    import ctypes
    import gvom
    lib = ctypes.CDLL(gvom.library_path())
    gvom.ABI = [e for e in gvom.ABI if hasattr(lib, e[0])]
    return gvom


def _setup(name):
    import numpy as np
    import torch
    import synth
    torch.cuda.init()
    gvom = _gvom()
    params, scans = synth.config_inputs(name, n_scans=3)
    dev = [(torch.from_numpy(np.ascontiguousarray(pc)).cuda(), ego, tf) for pc, ego, tf in scans]
    torch.cuda.synchronize()
    g = gvom.Gvom(*params, voxel_statistics=False)
    return np, torch, gvom, g, dev


def _filled(np, torch, gvom, g, dev, A):
    """the drive, then the last set at every tile of a fixed extent: (atlas, last set, extent origin, a goal in the first tile)"""
    m = None
    for t, ego, tf in dev:
        g.process_pointcloud_device(t.data_ptr(), t.shape[0], np.float32, ego, tf)
        m = g.combine_maps_device()
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
    np, torch, gvom, g, dev = _setup(name)
    a, m, o, goal, tm = _filled(np, torch, gvom, g, dev, A)
    stream = torch.cuda.ExternalStream(int(g._lib.gvom_stream(g._h)))

    def timed(call, n):
        us, last = [], None
        for k in range(n + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            last = call()
            e1.record(stream)
            e1.synchronize()
            if k >= 2:
                us.append(e0.elapsed_time(e1) * 1e3)
        return {"median_us": round(_median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2), "calls": n}, last

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
    np, torch, gvom, g, dev = _setup(name)
    a, m, o, goal, tm = _filled(np, torch, gvom, g, dev, A)
    for kw in ({}, {"inflation_radius": ROBOT_RADIUS}):
        for _ in range(3):
            with a.cost_to_go([goal], goals_in_cells=True, **kw) as f:
                f.window(m).release()
    g._check(g._lib.gvom_sync(g._h))
    del tm
    return {"calls": 6}


def child_step(name, steps, mode, A):
    np, torch, gvom, g, dev = _setup(name)
    a = g.create_atlas(A)
    goal = None

    def step(k):
        nonlocal goal
        t, ego, tf = dev[k % 3]
        g.process_pointcloud_device(t.data_ptr(), t.shape[0], np.float32, ego, tf)
        m = g.combine_maps_device()
        a.integrate(m)
        if mode:
            if goal is None:
                goal = [m.origin_cells[0] + g.xy_size // 2, m.origin_cells[1] + g.xy_size // 2]
            a.cost_to_go([goal], goals_in_cells=True).release()
        m.release()

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
    return {"us_per_step": us, "us_per_step_median": _median(us), "steps": steps}


def _spawn(mode, args, lib=None, wrap=()):
    """one child under its own time limit; a child that fails (or runs into the limit) ends the whole run"""
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT)] + list(wrap) + [sys.executable, os.path.abspath(__file__), "--child", mode] + [str(a) for a in args]
    env = dict(os.environ, GVOM_HIP_LIBRARY=os.path.abspath(lib)) if lib else None
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    if r.returncode != 0:
        raise SystemExit("%s %r failed (%d): nothing more is started\n%s" % (mode, args, r.returncode, r.stderr[-3000:]))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def kernels_one_by_one(name, A):
    """average microseconds per kernel from a kernel trace of child_profiled, in a run of its own"""
    if not shutil.which("rocprofv3"):
        return {"not_measured": "no rocprofv3 on this machine"}
    d = tempfile.mkdtemp(prefix="atlas_field_prof_")
    try:
        _spawn("profiled", (name, A), wrap=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"))
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"not_measured": "the trace left no kernel_stats.csv"}
        out = {}
        for r in csv.DictReader(open(files[0])):
            short = r["Name"].split("(")[0].replace("void ", "")
            if short in SHOWN:
                out[short] = {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 2),
                              "min_us": round(float(r.get("MinNs", 0)) / 1e3, 2), "max_us": round(float(r.get("MaxNs", 0)) / 1e3, 2)}
        return out
    except SystemExit as e:                                         # best effort: the events above stand without it
        return {"not_measured": str(e)[:500]}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def resources(new, parent):
    """the new kernels, and every other kernel on the parent and on this library: registers, scratch, LDS, code size"""
    import kernel_regs
    mine = kernel_regs.kernels(new)
    is_new = lambda k: any(n in k for n in NEW_KERNELS)              # noqa: E731
    out = {"new_kernels": {k: v for k, v in mine.items() if is_new(k)}}
    if parent:
        theirs = kernel_regs.kernels(parent)
        rest = {k: v for k, v in mine.items() if not is_new(k)}
        keys = ("vgpr", "sgpr", "scratch", "lds", "code")
        changed = {k: {"parent": theirs.get(k), "new": v} for k, v in rest.items() if any((theirs.get(k) or {}).get(q) != v.get(q) for q in keys)}
        out["other_kernels"] = {"count": len(rest), "identical_to_parent": len(rest) - len(changed), "changed": changed,
                                "only_on_parent": sorted(k for k in theirs if k not in mine)}
    return out


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        mode, a = sys.argv[2], sys.argv[3:]
        res = {"events": lambda: child_events(a[0], int(a[1])), "profiled": lambda: child_profiled(a[0], int(a[1])),
               "step": lambda: child_step(a[0], int(a[1]), int(a[2]), int(a[3]))}[mode]()
        print("RESULT " + json.dumps(res))
        return
    import lib_identity
    args = sys.argv[1:]
    parent, only_resources, configs, sides = None, False, list(CONFIGS), list(SIDES)
    while args and args[0] in ("--parent", "--resources", "--configs", "--sides"):
        if args[0] == "--parent":
            parent, args = args[1], args[2:]
        elif args[0] == "--configs":
            configs, args = args[1].split(","), args[2:]
        elif args[0] == "--sides":
            sides, args = [int(v) for v in args[1].split(",")], args[2:]
        else:
            only_resources, args = True, args[1:]
    new = os.path.join(ROOT, "g-vom_amd", "lib", "libgvom_hip.so")
    path = args[0] if args else os.path.join(ROOT, "profiles", "atlas_field_%s.json" % (lib_identity.identity().get("lib_sha256") or "unknown")[:8])
    out = json.load(open(path)) if os.path.exists(path) else {}
    out.update({"library": lib_identity.identity(), "sides": sides, "robot_radius_m": ROBOT_RADIUS})
    out["resources"] = resources(new, parent)
    if parent:
        out["parent_library"] = {"lib_sha256": lib_identity.sha256_file(parent)}
    out.setdefault("not_measured", ["follow mode and a moving extent during the solve's fill", "goals far from the first tile, more than one goal",
                                    "soft and roughness weights, unknown=\"blocked\"", "windows other than the config's own",
                                    "terrain other than the config's set repeated over the extent: the round count depends on it"])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)

    def save():
        with open(path, "w") as f:                                  # (after every part: a run that ends early leaves what it has)
            f.write(json.dumps(out, indent=1) + "\n")
    save()
    if only_resources:
        out.setdefault("configs", "not measured")
        save()
        return
    if not isinstance(out.get("configs"), dict):
        out["configs"] = {}
    for name in configs:
        steps = CONFIGS[name]
        res = out["configs"].setdefault(name, {})
        res["events"] = {"A %d" % A: _spawn("events", (name, A)) for A in sides}
        save()
        res["kernels one by one (rocprofv3 --kernel-trace --stats, a run of its own)"] = {"A %d" % A: kernels_one_by_one(name, A) for A in sides}
        save()
        runs = {"without": [], "field_per_step": [], "parent_without": []}
        for rnd in range(5):                                        # alternating: parent, without, with, ...
            if parent:
                runs["parent_without"].append(_spawn("step", (name, steps, 0, 1024), lib=parent))
            runs["without"].append(_spawn("step", (name, steps, 0, 1024)))
            runs["field_per_step"].append(_spawn("step", (name, max(5, steps // 6), 1, 1024)))
        step = {}
        for who, rs in runs.items():
            if rs:
                meds = [r["us_per_step_median"] for r in rs]
                step[who] = {"run_medians_us": meds, "median": _median(meds), "min": min(meds), "max": max(meds)}
        step["a_field_per_step_adds_us_per_step"] = round(step["field_per_step"]["median"] - step["without"]["median"], 2)
        if parent:
            p = step["parent_without"]
            step["without_inside_parents_own_spread"] = bool(p["min"] <= step["without"]["median"] <= p["max"])
            step["without_minus_parent_median_us"] = round(step["without"]["median"] - p["median"], 2)
        res["step: scan + combine_maps_device + integrate (+ a field per step), A 1024"] = step
        save()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
