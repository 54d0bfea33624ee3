#!/usr/bin/env python3
"""What the atlas frontiers (gvom_atlas_frontiers: k_atlas_frontier_mark, then k_frontier_relax / _count / _rank / _rows / _stats at the
field's side) cost.  On the painted terrain of tools/atlas_field_bench.py -- m256's bench scans driven through scan +
combine_maps_device(), the last set integrated at every tile of a FIXED extent of A = 1024 and 4096 cells -- with a field seeded in the
extent's first tile.  Every loop in a fresh child process, every child under a `timeout` of its own, and the first child that fails
ends the run (the per-kernel part alone is best effort: its failure is noted):

  events     HIP events on the handle's stream around one DeviceAtlasField.frontiers(), medians and spread, with its rounds, tile
             relaxations, the tiles LAUNCHED ((A / 32)^2 per round: no compacted tile list is built), clusters and frontier cells.  The
             call waits: its events bracket the host's looks at the counters as well.  Against what a user has without it: the tiled
             loop of recall() + window() + frontiers() over the extent at the config's xy_size (its clusters are cut at window borders:
             NOT an equal product; their number is written beside it), and scipy.ndimage.label on the exported extent and field on the
             host (copies, mask and labelling timed apart; its frontier cells and kept components are checked against the product)
  kernels    three calls under `rocprofv3 --kernel-trace --stats` in a run of its own: average time per kernel
  step       scan + combine_maps_device() per step WITHOUT any atlas call, on this library and, with --parent LIB (the parent commit's
             libgvom_hip.so), on that one, alternating, five runs each: this library's median has to lie inside the parent's own
             run-to-run spread; both spreads are written down
  resources  tools/kernel_regs.py: the new kernel, and registers, scratch, LDS and code size of every kernel that existed before on
             the parent and on this library (--resources alone: no GPU needed)

    tools/atlas_frontier_bench.py [--resources] [--parent LIB] [--config m256] [--step-configs m256,c4] [--sides 1024,4096] [out.json]
                                                                     (default: profiles/atlas_frontiers_<lib sha8>.json)
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
import atlas_field_bench as afb                                       # noqa: E402  (the painted terrain, the set-up and the medians are its)

STEP_CONFIGS = {"m256": 60, "c4": 30}                    # config: timed steps per repetition
SIDES = (1024, 4096)
CHILD_TIMEOUT = 400                                       # seconds, per child process
NEW_KERNELS = ("k_atlas_frontier_mark",)
SHOWN = ("k_atlas_frontier_mark", "k_frontier_mark", "k_frontier_relax", "k_frontier_count", "k_frontier_rank", "k_frontier_rows", "k_frontier_stats",
         "k_atlas_recall", "k_atlas_field_window")
_median = afb._median


def _timed(torch, stream, call, n, warm=2):
    us, last = [], None
    for k in range(n + warm):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        last = call()
        e1.record(stream)
        e1.synchronize()
        if k >= warm:
            us.append(e0.elapsed_time(e1) * 1e3)
    return {"median_us": round(_median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2), "calls": n}, last


def child_events(name, A, reps=9):
    np, torch, gvom, g, dev = afb._setup(name)
    a, m, o, goal, tm = afb._filled(np, torch, gvom, g, dev, A)
    stream = torch.cuda.ExternalStream(int(g._lib.gvom_stream(g._h)))
    xy = g.xy_size
    f = a.cost_to_go([goal], goals_in_cells=True)
    out = {"xy": xy, "A": A, "seed": goal, "field": {"rounds": f.rounds, "reached": f.reached, "converged": f.converged},
           "tiles_launched_per_round": (A // 32) ** 2, "work_buffer_MiB": round(A * A * 8 / 2 ** 20, 1)}

    def whole():
        with f.frontiers() as p:
            return {"rounds": p.rounds, "tile_relaxations": g.get_tuning("atlas_frontier_tiles"), "kept_clusters": p.n_clusters,
                    "frontier_cells": p.frontier_cells, "dropped_by_min_cells": p.dropped}
    t, info = _timed(torch, stream, whole, reps)
    info["tiles_launched"] = info["rounds"] * out["tiles_launched_per_round"]
    out["frontiers() on the whole extent"] = dict(t, **info)

    def tiled():
        kept = cells = 0
        for j in range(0, A, xy):
            for i in range(0, A, xy):
                with a.recall(origin_cells=(o[0] + i, o[1] + j)) as r, f.window(r) as w, w.frontiers(r) as p:
                    kept, cells = kept + p.n_clusters, cells + p.frontier_cells
                    r.stamps.release()
        return {"windows": (A // xy) ** 2, "kept_clusters_summed_over_windows": kept, "frontier_cells_summed_over_windows": cells}
    t, info = _timed(torch, stream, tiled, 3, warm=1)
    out["for scale: recall() + window() + frontiers() per window over the extent (clusters cut at window borders: not an equal product)"] = dict(t, **info)

    from scipy import ndimage
    with f.frontiers() as p:
        want_map, want_counts = p.cluster_map.copy_to_host(), p.counts.copy_to_host()
    host = {}
    t0 = time.perf_counter()
    with a.extent_device() as e:
        vis = e.visibility.copy_to_host()
    D, _, c = f.copy_to_host()
    host["export and copies to the host, ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    t0 = time.perf_counter()
    unknown = vis <= 0
    beside = np.zeros(vis.shape, bool)
    beside[1:, :] |= unknown[:-1, :]
    beside[:-1, :] |= unknown[1:, :]
    beside[:, 1:] |= unknown[:, :-1]
    beside[:, :-1] |= unknown[:, 1:]
    mask = (c > 0) & (vis > 0) & (D < 2 ** 31 - 1) & beside
    host["mask, ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    t0 = time.perf_counter()
    comp, n = ndimage.label(mask, structure=np.ones((3, 3), int))
    sizes = np.bincount(comp.ravel())[1:]
    host["scipy.ndimage.label and sizes, ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    host["components"], host["kept_components"] = int(n), int((sizes >= 4).sum())
    host["equal to the product"] = bool(np.array_equal(mask, want_map != -1) and host["kept_components"] == int(want_counts[0]) and
                                        int(mask.sum()) == int(want_counts[1]))
    out["for scale: the same on the host (numpy mask, scipy.ndimage.label; labels and sizes only, no rows)"] = host
    if not host["equal to the product"]:
        raise SystemExit("the host labelling and the product disagree")
    f.release()
    del tm
    return out


def child_profiled(name, A):
    """three calls: run under rocprofv3 by the parent process"""
    np, torch, gvom, g, dev = afb._setup(name)
    a, m, o, goal, tm = afb._filled(np, torch, gvom, g, dev, A)
    with a.cost_to_go([goal], goals_in_cells=True) as f:
        for _ in range(3):
            f.frontiers().release()
    g._check(g._lib.gvom_sync(g._h))
    del tm
    return {"calls": 3}


def child_step(name, steps):
    """scan + combine_maps_device() per step, no atlas anywhere"""
    np, torch, gvom, g, dev = afb._setup(name)

    def step(k):
        t, ego, tf = dev[k % 3]
        g.process_pointcloud_device(t.data_ptr(), t.shape[0], np.float32, ego, tf)
        g.combine_maps_device().release()

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
        raise SystemExit("%s %r failed (%d): nothing more is started\n%s" % (mode, args, r.returncode, (r.stdout + r.stderr)[-3000:]))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def kernels_one_by_one(name, A):
    """average microseconds per kernel from a kernel trace of child_profiled, in a run of its own"""
    if not shutil.which("rocprofv3"):
        return {"not_measured": "no rocprofv3 on this machine"}
    d = tempfile.mkdtemp(prefix="atlas_frontier_prof_")
    try:
        _spawn("profiled", (name, A), wrap=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"))
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"not_measured": "the trace left no kernel_stats.csv"}
        out = {}
        for r in csv.DictReader(open(files[0])):
            short = r["Name"].split("(")[0].replace("void ", "")
            if short in SHOWN:
                out[short] = {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 2), "total_us": round(float(r["TotalDurationNs"]) / 1e3, 2)
                              if "TotalDurationNs" in r else None, "min_us": round(float(r.get("MinNs", 0)) / 1e3, 2), "max_us": round(float(r.get("MaxNs", 0)) / 1e3, 2)}
        return out
    except SystemExit as e:                                         # best effort: the events above stand without it
        return {"not_measured": str(e)[:500]}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        mode, a = sys.argv[2], sys.argv[3:]
        res = {"events": lambda: child_events(a[0], int(a[1])), "profiled": lambda: child_profiled(a[0], int(a[1])),
               "step": lambda: child_step(a[0], int(a[1]))}[mode]()
        print("RESULT " + json.dumps(res))
        return
    import lib_identity
    args = sys.argv[1:]
    parent, only_resources, config, step_configs, sides = None, False, "m256", list(STEP_CONFIGS), list(SIDES)
    while args and args[0] in ("--parent", "--resources", "--config", "--step-configs", "--sides"):
        if args[0] == "--parent":
            parent, args = args[1], args[2:]
        elif args[0] == "--config":
            config, args = args[1], args[2:]
        elif args[0] == "--step-configs":
            step_configs, args = [v for v in args[1].split(",") if v], args[2:]
        elif args[0] == "--sides":
            sides, args = [int(v) for v in args[1].split(",") if v], args[2:]
        else:
            only_resources, args = True, args[1:]
    new = os.path.join(ROOT, "g-vom_amd", "lib", "libgvom_hip.so")
    path = args[0] if args else os.path.join(ROOT, "profiles", "atlas_frontiers_%s.json" % (lib_identity.identity().get("lib_sha256") or "unknown")[:8])
    out = json.load(open(path)) if os.path.exists(path) else {}
    out.update({"library": lib_identity.identity(), "sides": sides, "config": config})
    afb.NEW_KERNELS = NEW_KERNELS
    out["resources"] = afb.resources(new, parent)
    if parent:
        out["parent_library"] = {"lib_sha256": lib_identity.sha256_file(parent)}
    out.setdefault("not_measured", ["a compacted tile list: every round launches all (A / 32)^2 tiles, most of which return at once",
                                    "follow mode, a moved extent and an atlas of another side than the field's",
                                    "terrain other than the config's set repeated over the extent: rounds and clusters depend on it",
                                    "min_cells and max_clusters other than the defaults; windows other than the config's own in the tiled loop"])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)

    def save():
        with open(path, "w") as f:                                  # (after every part: a run that ends early leaves what it has)
            f.write(json.dumps(out, indent=1) + "\n")
    save()
    if only_resources:
        out.setdefault("events", "not measured")
        save()
        return
    if sides:
        out["events"] = {"A %d" % A: _spawn("events", (config, A)) for A in sides}
        save()
        out["kernels one by one (rocprofv3 --kernel-trace --stats, a run of its own)"] = {"A %d" % A: kernels_one_by_one(config, A) for A in sides}
        save()
    for name in step_configs:
        steps = STEP_CONFIGS[name]
        runs = {"this_library": [], "parent": []}
        for rnd in range(5):                                        # alternating: parent, this, parent, ...
            if parent:
                runs["parent"].append(_spawn("step", (name, steps), lib=parent))
            runs["this_library"].append(_spawn("step", (name, steps)))
        step = {}
        for who, rs in runs.items():
            if rs:
                meds = [r["us_per_step_median"] for r in rs]
                step[who] = {"run_medians_us": meds, "median": _median(meds), "min": min(meds), "max": max(meds)}
        if parent:
            p = step["parent"]
            step["inside_parents_own_spread"] = bool(p["min"] <= step["this_library"]["median"] <= p["max"])
            step["minus_parent_median_us"] = round(step["this_library"]["median"] - p["median"], 2)
        out.setdefault("step: scan + combine_maps_device, no atlas call", {})[name] = step
        save()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
