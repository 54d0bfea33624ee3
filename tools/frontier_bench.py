#!/usr/bin/env python3
"""What frontier extraction (gvom_frontiers: k_frontier_mark, _relax, _count, _rank, _rows, _stats) costs.  On the map sets of m256
(256 x 256), c4 (512 x 512) and c5 (1024 x 1024) after three bench scans, with a cost field seeded at the ego's cell, inflated by a robot radius
of 1 m and uninflated, min_cells 4 and 1024 rows -- every loop in a fresh child process, every child under a `timeout` of its own,
and the first child that fails ends the run:

  call       DeviceCostField.frontiers(maps), enqueue to completion: wall time, rounds, tile relaxations, what it found
  kernel     one `rocprofv3 --kernel-trace` run per config: per kernel the launches and the time per call
  scipy      the three maps copied to the host, scipy.ndimage.label and numpy reductions (tests/frontier_ref.py product(), first
             shown equal to the product in all four parts), copies included
  torch      min-label propagation written in torch on the GPU: nine shifted minima per sweep until nothing changes, the labels
             first shown equal to the product's cluster map
  step       scan + combine_maps_device() + cost_to_go() per step, without and with frontiers(); and, with --parent LIB (the parent
             commit's libgvom_hip.so), the same step without on that library, alternating, five runs each
  resources  tools/kernel_regs.py: the new kernels, and registers, scratch, LDS and code size of every kernel outside the new
             unit on the parent and on this library (--resources alone: no GPU needed)

    tools/frontier_bench.py [--resources] [--parent LIB] [--configs m256,c4] [--turns N] [out.json]   (default: profiles/frontier_<lib sha8>.json)
"""
import json
import os
import sys
import tempfile
import time

import benchkit as bk

sys.path.insert(0, os.path.join(bk.ROOT, "tests"))
CONFIGS = {"m256": 100, "c4": 40, "c5": 40}               # config: timed steps per repetition
TURNS = 5
FIELDS = (("inflated", 1.0), ("uninflated", None))        # inflation radius in metres
MIN_CELLS, MAX_CLUSTERS = 4, 1024
CHILD_TIMEOUT = 300                                       # seconds, per child process
KERNELS = ("k_frontier_mark", "k_frontier_relax", "k_frontier_count", "k_frontier_rank", "k_frontier_rows", "k_frontier_stats")


def _field(gvom, g, m, ego, radius):
    e = gvom.world_to_cells([ego[:2]], g.xy_resolution, m.origin)[0]
    return m.cost_to_go([e], goals_in_cells=True, inflation_radius=radius, density_threshold=50, soft_weight=10)


def _torch_labels(torch, c, vis, D, unreached):
    """min-label propagation on [y, x] tensors: (labels int64, -1 off the frontier; sweeps)"""
    xy = c.shape[0]
    unknown = vis == 0
    beside = torch.zeros_like(unknown)
    beside[:, 1:] |= unknown[:, :-1]
    beside[:, :-1] |= unknown[:, 1:]
    beside[1:, :] |= unknown[:-1, :]
    beside[:-1, :] |= unknown[1:, :]
    mask = (c > 0) & (vis > 0) & beside & (D < unreached)
    big = xy * xy
    L = torch.where(mask, torch.arange(big, device=c.device).view(xy, xy), torch.full((xy, xy), big, device=c.device))
    sweeps = 0
    while True:
        for k in range(16):                                        # sixteen sweeps between two looks at the result
            P = torch.nn.functional.pad(L, (1, 1, 1, 1), value=big)
            best = L
            for dy in range(3):
                for dx in range(3):
                    best = torch.minimum(best, P[dy:dy + xy, dx:dx + xy])
            new = torch.where(mask, best, L)
            sweeps += 1
            same = k == 15 and torch.equal(new, L)
            L = new
        if same:
            break
    return torch.where(mask, L, torch.full_like(L, -1)), sweeps


def child_call(name, profiled):
    np, torch, gvom, g, dev = bk.setup(name)
    import frontier_ref as fr
    for scan in dev:
        m = bk.scan_combine(np, g, scan)
    ego = dev[2][1]
    reps, results = 20, {}
    for what, radius in FIELDS:
        f = _field(gvom, g, m, ego, radius)
        call = lambda: f.frontiers(m, min_cells=MIN_CELLS, max_clusters=MAX_CLUSTERS)
        if profiled:
            for _ in range(reps):
                call().release()
            bk.sync(g)
            f.release()
            continue
        t = bk.timed(None, lambda: call().release(), reps, digits=2)             # (the call waits itself)
        r = call()
        out = {"xy": g.xy_size, "field_rounds": f.rounds, "call_us": t["us"], "call_us_median": t["us_median"], "rounds": r.rounds,
               "tile_relaxations": g.get_tuning("frontier_tiles"), "kept_clusters": r.n_clusters, "frontier_cells": r.frontier_cells,
               "clusters_dropped_by_min_cells": r.dropped}
        got = r.copy_to_host()
        out["largest_cluster_cells"] = int(got[0][:, 1].max())
        # scipy on the host, copies included: equal first, then timed
        tc, tv, tD = torch.from_dlpack(f.cell_cost).view(torch.int16), torch.from_dlpack(m.visibility), torch.from_dlpack(f.cost)   # (uint16 bits)

        def on_host():
            c, vis, D = tc.cpu().numpy().view(np.uint16), tv.cpu().numpy(), tD.cpu().numpy()
            return fr.product(c.T, vis.T, D.T, MIN_CELLS, MAX_CLUSTERS)
        want = on_host()
        equal = bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2].T, want[2]) and
                     np.array_equal(got[3], want[3]))
        hs = []
        for rep in range(5):
            t0 = time.perf_counter()
            on_host()
            hs.append(round((time.perf_counter() - t0) * 1e6, 1))
        out["scipy_on_the_host"] = {"equal_to_the_product": equal, "us": hs, "us_median": bk.median(hs)}
        # min-label propagation in torch on the exported maps
        cy, vy, Dy = (tc.T != 0).to(torch.int64), tv.T.contiguous(), tD.T.contiguous().to(torch.int64)
        L, sweeps = _torch_labels(torch, cy, vy, Dy, fr.UNREACHED)
        lab = fr.labels_scipy(fr.frontier_mask(cy.cpu().numpy(), vy.cpu().numpy(), Dy.cpu().numpy()))
        ts = []
        for rep in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _torch_labels(torch, cy, vy, Dy, fr.UNREACHED)
            torch.cuda.synchronize()
            ts.append(round((time.perf_counter() - t0) * 1e6, 1))
        out["torch_min_label_propagation"] = {"labels_equal_to_the_referee": bool(np.array_equal(L.cpu().numpy(), lab)), "sweeps": sweeps,
                                              "us": ts, "us_median": bk.median(ts), "covers": "the labels only: no ranks, no statistics"}
        del tc, tv, tD
        r.release()
        f.release()
        results[what] = out
    return {"calls": reps} if profiled else results


def child_step(name, steps, with_frontiers):
    np, torch, gvom, g, dev = bk.setup(name)

    def step(k):
        ego = dev[k % 3][1]
        m = bk.scan_combine(np, g, dev[k % 3])
        f = _field(gvom, g, m, ego, FIELDS[0][1])
        if with_frontiers:
            f.frontiers(m, min_cells=MIN_CELLS, max_clusters=MAX_CLUSTERS).release()
        f.release()
        m.release()
    return bk.step_loop(g, step, steps, warm=min(10, steps))


def _kernel_times(profile_dir, calls):
    """per field variant (the launches of k_frontier_mark split the trace) and kernel: launches and microseconds per call"""
    rows = bk.kernel_trace_rows(profile_dir, KERNELS)
    marks = [i for i, r in enumerate(rows) if r[1] == "k_frontier_mark"]
    if len(marks) != calls * len(FIELDS):
        return None
    out = {}
    for n, (what, _) in enumerate(FIELDS):
        a = marks[n * calls + 3] - 1                               # (k_frontier_rows runs in front of k_frontier_mark) without the first three calls
        b = marks[(n + 1) * calls] - 1 if n + 1 < len(FIELDS) else len(rows)
        part, used = rows[a:b], calls - 3
        rec = {}
        for k in KERNELS:
            us = [u for _, kk, u in part if kk == k]
            rec[k] = {"launches_per_call": round(len(us) / used, 2), "us_per_call": round(sum(us) / used, 2), "median_us_per_launch": round(bk.median(us), 2)}
        rec["all_kernels_us_per_call"] = round(sum(u for _, _, u in part) / used, 2)
        out[what] = rec
    return out


def main():
    if bk.child(sys.argv[1:], {"call": lambda a: child_call(a[0], a[1] == "1"), "step": lambda a: child_step(a[0], int(a[1]), a[2] == "1")}):
        return
    args = bk.read_args(sys.argv[1:], configs=CONFIGS, turns=TURNS)
    parent = args["parent"]
    spawn = lambda mode, a, **kw: bk.spawn(__file__, mode, a, CHILD_TIMEOUT, **kw)
    report, configs = bk.product_report(
        "frontier", args, {"min_cells": MIN_CELLS, "max_clusters": MAX_CLUSTERS, "fields": dict(FIELDS)}, lambda k: "k_frontier" in k,
        ["pointer jumping (not built)", "the statistics without per-wave combining (not built)", "maps larger than 1024 x 1024",
         "other tile sizes", "frontier_batch and frontier_inner other than the defaults 8 and 256",
         "the pointer routes (host arrays, device addresses)"])
    if configs is None:
        return
    for name in args["configs"]:
        steps = CONFIGS[name]
        res = spawn("call", (name, 0))
        with tempfile.TemporaryDirectory() as d:
            prof = spawn("call", (name, 1), profile_dir=d)
            kernel = _kernel_times(d, prof["calls"])
        for what, _ in FIELDS:
            res[what]["kernels"] = kernel[what] if kernel else "not measured (the trace did not hold the expected launches)"
        configs[name] = res
        report.save()
        runs = bk.alternate(args["turns"], {"parent_without": parent and (lambda: spawn("step", (name, steps, 0), lib=parent)),
                                            "without": lambda: spawn("step", (name, steps, 0)), "with": lambda: spawn("step", (name, steps, 1))})
        step = bk.spreads(runs)
        step["frontiers_add_us_per_step"] = round(step["with"]["median"] - step["without"]["median"], 2)
        res["step: scan + combine_maps_device + cost_to_go (inflated) (+ frontiers)"] = bk.against_parent(step, "without", "parent_without", "without_")
        report.save()
    print(json.dumps(report.out, indent=1))


if __name__ == "__main__":
    main()
