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

    tools/atlas_frontier_bench.py [--resources] [--parent LIB] [--config m256] [--configs m256,c4] [--turns N] [--sides 1024,4096] [out.json]
                                                                     (default: profiles/atlas_frontiers_<lib sha8>.json)
"""
import json
import sys
import time

import atlas_field_bench as afb                                       # (the painted terrain and the per-kernel run are its)
import benchkit as bk

STEP_CONFIGS = {"m256": 60, "c4": 30}                    # config: timed steps per repetition
TURNS = 5
SIDES = (1024, 4096)
CHILD_TIMEOUT = 400                                       # seconds, per child process
NEW_KERNELS = ("k_atlas_frontier_mark",)
SHOWN = ("k_atlas_frontier_mark", "k_frontier_mark", "k_frontier_relax", "k_frontier_count", "k_frontier_rank", "k_frontier_rows", "k_frontier_stats",
         "k_atlas_recall", "k_atlas_field_window")


def child_events(name, A, reps=9):
    np, torch, gvom, g, dev = bk.setup(name)
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
    t, info = bk.timed_events(torch,stream, whole, reps)
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
    t, info = bk.timed_events(torch,stream, tiled, 3, warm=1)
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
    np, torch, gvom, g, dev = bk.setup(name)
    a, m, o, goal, tm = afb._filled(np, torch, gvom, g, dev, A)
    with a.cost_to_go([goal], goals_in_cells=True) as f:
        for _ in range(3):
            f.frontiers().release()
    bk.sync(g)
    del tm
    return {"calls": 3}


def child_step(name, steps):
    """scan + combine_maps_device() per step, no atlas anywhere"""
    np, torch, gvom, g, dev = bk.setup(name)

    def step(k):
        bk.scan_combine(np, g, dev[k % 3]).release()
    return bk.step_loop(g, step, steps, warm=min(10, steps))


def main():
    if bk.child(sys.argv[1:], {"events": lambda a: child_events(a[0], int(a[1])), "profiled": lambda a: child_profiled(a[0], int(a[1])),
                               "step": lambda a: child_step(a[0], int(a[1]))}):
        return
    names = lambda s: [v for v in s.split(",") if v]
    args = bk.read_args(sys.argv[1:], configs=STEP_CONFIGS, turns=TURNS,           # (--configs: the step's, as --step-configs)
                        extra={"--config": ("m256", str), "--step-configs": (None, names), "--sides": (list(SIDES), lambda s: [int(v) for v in names(s)])})
    parent, config, sides = args["parent"], args["config"], args["sides"]
    step_configs = args["configs"] if args["step_configs"] is None else args["step_configs"]
    spawn = lambda mode, a, **kw: bk.spawn(__file__, mode, a, CHILD_TIMEOUT, **kw)
    report, events = bk.product_report(
        "atlas_frontiers", args, {"sides": sides, "config": config}, lambda k: any(n in k for n in NEW_KERNELS),
        ["a compacted tile list: every round launches all (A / 32)^2 tiles, most of which return at once",
         "follow mode, a moved extent and an atlas of another side than the field's",
         "terrain other than the config's set repeated over the extent: rounds and clusters depend on it",
         "min_cells and max_clusters other than the defaults; windows other than the config's own in the tiled loop"], section="events")
    if events is None:
        return
    out = report.out
    if sides:
        events.update({"A %d" % A: spawn("events", (config, A)) for A in sides})
        report.save()
        out["kernels one by one (rocprofv3 --kernel-trace --stats, a run of its own)"] = {
            "A %d" % A: afb.kernels_one_by_one(__file__, (config, A), SHOWN, CHILD_TIMEOUT, total=True) for A in sides}
        report.save()
    for name in step_configs:
        steps = STEP_CONFIGS[name]
        runs = bk.alternate(args["turns"], {"parent": parent and (lambda: spawn("step", (name, steps), lib=parent)),
                                            "this_library": lambda: spawn("step", (name, steps))})
        out.setdefault("step: scan + combine_maps_device, no atlas call", {})[name] = bk.against_parent(bk.spreads(runs), "this_library", "parent", "")
        report.save()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
