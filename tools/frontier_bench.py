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

    tools/frontier_bench.py [--resources] [--parent LIB] [--configs m256,c4] [out.json]   (default: profiles/frontier_<lib sha8>.json)
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
CONFIGS = {"m256": 100, "c4": 40, "c5": 40}               # config: timed steps per repetition
FIELDS = (("inflated", 1.0), ("uninflated", None))        # inflation radius in metres
MIN_CELLS, MAX_CLUSTERS = 4, 1024
CHILD_TIMEOUT = 300                                       # seconds, per child process
KERNELS = ("k_frontier_mark", "k_frontier_relax", "k_frontier_count", "k_frontier_rank", "k_frontier_rows", "k_frontier_stats")


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
    np, torch, gvom, g, dev = _setup(name)
    import frontier_ref as fr
    for t, ego, tf in dev:
        g.process_pointcloud_device(t.data_ptr(), t.shape[0], np.float32, ego, tf)
        m = g.combine_maps_device()
    ego = dev[2][1]
    reps, results = 20, {}
    for what, radius in FIELDS:
        f = _field(gvom, g, m, ego, radius)
        call = lambda: f.frontiers(m, min_cells=MIN_CELLS, max_clusters=MAX_CLUSTERS)
        if profiled:
            for _ in range(reps):
                call().release()
            g._check(g._lib.gvom_sync(g._h))
            f.release()
            continue
        for _ in range(3):
            call().release()
        us = []
        for rep in range(5):
            t0 = time.perf_counter()
            for _ in range(reps):
                call().release()
            us.append(round((time.perf_counter() - t0) / reps * 1e6, 2))
        r = call()
        out = {"xy": g.xy_size, "field_rounds": f.rounds, "call_us": us, "call_us_median": _median(us), "rounds": r.rounds,
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
        out["scipy_on_the_host"] = {"equal_to_the_product": equal, "us": hs, "us_median": _median(hs)}
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
                                              "us": ts, "us_median": _median(ts), "covers": "the labels only: no ranks, no statistics"}
        del tc, tv, tD
        r.release()
        f.release()
        results[what] = out
    return {"calls": reps} if profiled else results


def child_step(name, steps, with_frontiers):
    np, torch, gvom, g, dev = _setup(name)

    def step(k):
        t, ego, tf = dev[k % 3]
        g.process_pointcloud_device(t.data_ptr(), t.shape[0], np.float32, ego, tf)
        m = g.combine_maps_device()
        f = _field(gvom, g, m, ego, FIELDS[0][1])
        if with_frontiers:
            f.frontiers(m, min_cells=MIN_CELLS, max_clusters=MAX_CLUSTERS).release()
        f.release()
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


def _spawn(mode, args, profile_dir=None, lib=None):
    """one child under its own time limit; a child that fails (or runs into the limit) ends the whole run"""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode] + [str(a) for a in args]
    if profile_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", profile_dir, "--"] + cmd
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT)] + cmd
    env = dict(os.environ, GVOM_HIP_LIBRARY=os.path.abspath(lib)) if lib else None
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    if r.returncode != 0:
        raise SystemExit("%s %r failed (%d): nothing more is started\n%s" % (mode, args, r.returncode, r.stderr[-3000:]))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def _kernel_times(profile_dir, calls):
    """per field variant (the launches of k_frontier_mark split the trace) and kernel: launches and microseconds per call"""
    rows = []
    for f in glob.glob(os.path.join(profile_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            key = [k for k in KERNELS if k in r["Kernel_Name"]]
            if key:
                rows.append((int(r["Start_Timestamp"]), key[0], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
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
            rec[k] = {"launches_per_call": round(len(us) / used, 2), "us_per_call": round(sum(us) / used, 2), "median_us_per_launch": round(_median(us), 2)}
        rec["all_kernels_us_per_call"] = round(sum(u for _, _, u in part) / used, 2)
        out[what] = rec
    return out


def resources(new, parent):
    """the new unit's kernels, and every other kernel on the parent and on this library: registers, scratch, LDS, code size"""
    import kernel_regs
    mine = kernel_regs.kernels(new)
    out = {"new_kernels": {k: v for k, v in mine.items() if "k_frontier" in k}}
    if parent:
        theirs = kernel_regs.kernels(parent)
        rest = {k: v for k, v in mine.items() if "k_frontier" not in k}
        keys = ("vgpr", "sgpr", "scratch", "lds", "code")
        changed = {k: {"parent": theirs.get(k), "new": v} for k, v in rest.items() if any((theirs.get(k) or {}).get(q) != v.get(q) for q in keys)}
        out["other_kernels"] = {"count": len(rest), "identical_to_parent": len(rest) - len(changed), "changed": changed,
                                "only_on_parent": sorted(k for k in theirs if k not in mine)}
    return out


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        mode, a = sys.argv[2], sys.argv[3:]
        res = child_call(a[0], a[1] == "1") if mode == "call" else child_step(a[0], int(a[1]), a[2] == "1")
        print("RESULT " + json.dumps(res))
        return
    import lib_identity
    args = sys.argv[1:]
    parent, only_resources, configs = None, False, list(CONFIGS)
    while args and args[0] in ("--parent", "--resources", "--configs"):
        if args[0] == "--parent":
            parent, args = args[1], args[2:]
        elif args[0] == "--configs":
            configs, args = args[1].split(","), args[2:]
        else:
            only_resources, args = True, args[1:]
    new = os.path.join(ROOT, "g-vom_amd", "lib", "libgvom_hip.so")
    path = args[0] if args else os.path.join(ROOT, "profiles", "frontier_%s.json" % (lib_identity.identity().get("lib_sha256") or "unknown")[:8])
    out = json.load(open(path)) if os.path.exists(path) else {}
    out.update({"library": lib_identity.identity(), "min_cells": MIN_CELLS, "max_clusters": MAX_CLUSTERS, "fields": dict(FIELDS)})
    out["resources"] = resources(new, parent)
    if parent:
        out["parent_library"] = {"lib_sha256": lib_identity.sha256_file(parent)}
    out.setdefault("not_measured", ["pointer jumping (not built)", "the statistics without per-wave combining (not built)", "maps larger than 1024 x 1024",
                                    "other tile sizes", "frontier_batch and frontier_inner other than the defaults 8 and 256",
                                    "the pointer routes (host arrays, device addresses)"])
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
        res = _spawn("call", (name, 0))
        with tempfile.TemporaryDirectory() as d:
            prof = _spawn("call", (name, 1), profile_dir=d)
            kernel = _kernel_times(d, prof["calls"])
        for what, _ in FIELDS:
            res[what]["kernels"] = kernel[what] if kernel else "not measured (the trace did not hold the expected launches)"
        out["configs"][name] = res
        save()
        runs = {"without": [], "with": [], "parent_without": []}
        for rnd in range(5):                                        # alternating: parent, without, with, ...
            if parent:
                runs["parent_without"].append(_spawn("step", (name, steps, 0), lib=parent))
            runs["without"].append(_spawn("step", (name, steps, 0)))
            runs["with"].append(_spawn("step", (name, steps, 1)))
        step = {}
        for who, rs in runs.items():
            if rs:
                meds = [r["us_per_step_median"] for r in rs]
                step[who] = {"run_medians_us": meds, "median": _median(meds), "min": min(meds), "max": max(meds)}
        step["frontiers_add_us_per_step"] = round(step["with"]["median"] - step["without"]["median"], 2)
        if parent:
            p = step["parent_without"]
            step["without_inside_parents_own_spread"] = bool(p["min"] <= step["without"]["median"] <= p["max"])
            step["without_minus_parent_median_us"] = round(step["without"]["median"] - p["median"], 2)
        res["step: scan + combine_maps_device + cost_to_go (inflated) (+ frontiers)"] = step
        save()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
