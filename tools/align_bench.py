#!/usr/bin/env python3
"""What scan alignment scoring (gvom_score_alignments: k_align_field, k_align_score, k_align_best) costs, and that it left the scan
and the ray query alone.  Everything goes into ONE file, profiles/align_<lib sha8>.json; a part that has not run yet is absent.

  --resources [--parent REV]   needs no GPU.  Compiles csrc/gvom_trace.hip and csrc/gvom_query.hip of REV (default HEAD) and of the
            working tree, and csrc/gvom_align.hip, for the device only, with the Makefile's flags and
            -Rpass-analysis=kernel-resource-usage: SGPRs, VGPRs, scratch, occupancy, LDS and code size per kernel.
            "trace_and_raycast_kernels_unchanged": every kernel of the two units has the same figures on both sides.
  (default) on a GPU, every loop in a fresh child process, on the maps of m256 and c4 after three scans, the last scan's cloud cut
            to n returns under K candidates of pose_candidates about its ego, K x n = 4096 x 16,384 and 9261 x 4096, dilate 0 and 1:
              kernel   one `rocprofv3 --kernel-trace --stats` run per configuration: the three kernels' us, pairs/s
              call     the whole call, device inputs, host time per call over back-to-back calls
              torch    the yardstick: the same scoring written in torch on occupancy_grid_device()'s export (transform, voxel,
                       gather, sums; candidates in chunks), which tells occupied from the rest only -- compared with the product
                       for dilate 0 under weights that do not tell free from unknown
              step     scan + combine_maps_device() per step, without and with one 9261 x 4096 query per step; and, with
                       --parent LIB (the parent commit's libgvom_hip.so), the same step without a query on that library,
                       alternating with this one

    tools/align_bench.py [--resources [--parent REV]] [--parent LIB] [--configs m256,c4] [--turns N] [out.json]
"""
import json
import os
import subprocess
import sys
import tempfile
import time

import benchkit as bk

ROOT = bk.ROOT
PKG = os.path.join(ROOT, "g-vom_amd")
CONFIGS = {"m256": 400, "c4": 100}                         # config: timed steps per repetition
TURNS = 2
CHILD_TIMEOUT = 900                                        # seconds, per child process
KERNELS = ("k_align_field", "k_align_score", "k_align_best")
SHAPES = ((4096, 16384), (9261, 4096))                     # (K, n)
STEP_SHAPE = (9261, 4096)
TORCH_WEIGHTS = (3, 0, -1, -1, 0)                          # free and unknown weigh the same: what an occupancy grid can tell
TORCH_CHUNK = 128                                          # candidates per chunk of the torch form


# ---- resources (CPU) ---------------------------------------------------------------------------------------------------------
def compiled_resources(parent):
    import raycast_bench as rb
    units = ("gvom_trace.hip", "gvom_query.hip")
    before = {}
    with tempfile.TemporaryDirectory() as d:
        tar = subprocess.run(["git", "-C", ROOT, "archive", parent, "g-vom_amd/csrc", "include"], capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", d], input=tar, check=True)
        for u in units:
            before[u] = rb._kernel_resources(os.path.join(d, "g-vom_amd", "csrc", u), os.path.join(d, "g-vom_amd", "csrc"))[0]
    csrc = os.path.join(PKG, "csrc")
    after = {u: rb._kernel_resources(os.path.join(csrc, u), csrc)[0] for u in units}
    align, listing = rb._kernel_resources(os.path.join(csrc, "gvom_align.hip"), csrc)
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", parent], capture_output=True, text=True).stdout.strip()
    return {"compiler_flags": rb._make_flags(), "parent": head, "parent_kernels": before, "branch_kernels": after,
            "trace_and_raycast_kernels": sum(len(v) for v in before.values()),
            "trace_and_raycast_kernels_unchanged": before == after and all(len(v) > 0 for v in before.values()),
            "gvom_align.hip": {"kernels": align, "listing": listing},
            "k_align_scratch_bytes": sorted({v["scratch"] for v in align.values()})}


# ---- timing (GPU) ------------------------------------------------------------------------------------------------------------
def _setup(name):
    """bk.setup() with the three scans fused, and the scans once more as host arrays"""
    np, torch, gvom, g, dev = bk.setup(name)
    for scan in dev:
        bk.scan_combine(np, g, scan).release()
    return np, torch, gvom, g, dev, [(t.cpu().numpy(), ego, tf) for t, ego, tf in dev]


def _inputs(np, torch, gvom, g, scans, K, n):
    """(cloud [n, 3] float32, candidates [K, 3, 4] float64) on the device: the last scan cut to n returns, a grid of poses about its ego"""
    pc, ego, tf = scans[-1]
    pick = (np.arange(n) * len(pc)) // n if len(pc) >= n else np.arange(n) % len(pc)
    cloud = np.ascontiguousarray(np.asarray(pc, np.float32)[pick, :3])
    base = np.identity(4) if tf is None else np.asarray(tf, np.float64).reshape(4, 4)
    xy_steps, yaw_steps = (10, 10) if K == 9261 else (7, 9)
    M = gvom.pose_candidates(base, g.xy_resolution / 2, xy_steps, 0.004, yaw_steps, pivot=ego)
    assert len(M) >= K, (len(M), K)
    M = np.ascontiguousarray(M[:K, :3, :])
    return cloud, M, torch.from_numpy(cloud).cuda(), torch.from_numpy(M).cuda()


def _torch_score(torch, g, tc, tm, weights):
    """the yardstick: counts {occupied, inside and not occupied, outside} per candidate and the score under `weights`, on the
    exported occupancy grid; candidates in chunks of TORCH_CHUNK"""
    occ = g.occupancy_grid_device()
    grid = torch.from_dlpack(occ)
    st = g._state()
    dev = tc.device
    W = torch.tensor(list(st.combined_origin), dtype=torch.float64, device=dev)
    res = torch.tensor([g.xy_resolution, g.xy_resolution, g.z_resolution], dtype=torch.float64, device=dev)
    size = torch.tensor([g.xy_size, g.xy_size, g.z_size], dtype=torch.float64, device=dev)
    x, y, z = (tc[None, :, k].double() for k in range(3))
    n = tc.shape[0]
    rows = []
    for k0 in range(0, tm.shape[0], TORCH_CHUNK):
        m = tm[k0:k0 + TORCH_CHUNK]
        w = torch.stack([(((x * m[:, r, 0:1] + y * m[:, r, 1:2]) + z * m[:, r, 2:3]) + m[:, r, 3:4]).float() for r in range(3)], dim=-1)
        v = torch.floor(w.double() / res - W)
        inside = ((v >= 0) & (v < size)).all(dim=-1)
        vi = torch.where(inside[..., None], v, torch.zeros_like(v)).long()
        hit = inside & (grid[vi[..., 0], vi[..., 1], vi[..., 2]] != 0)
        o, i = hit.sum(dim=1), inside.sum(dim=1)
        rows.append(torch.stack([o, i - o, n - i], dim=1))
    c = torch.cat(rows)
    score = weights[0] * c[:, 0] + weights[2] * c[:, 1] + weights[4] * c[:, 2]
    del grid
    occ.release()
    return c, score


def child_call(name):
    np, torch, gvom, g, dev, scans = _setup(name)
    out = {"shapes": {}}
    for K, n in SHAPES:
        cloud, M, tc, tm = _inputs(np, torch, gvom, g, scans, K, n)
        torch.cuda.synchronize()
        row = {}
        with g.score_alignments_device(tc.data_ptr(), n, tm.data_ptr(), K, dilate=0, weights=TORCH_WEIGHTS) as r:
            counts, best = r.copy_to_host()
        c, score = _torch_score(torch, g, tc, tm, TORCH_WEIGHTS)
        c, score = c.cpu().numpy(), score.cpu().numpy()
        row["torch_equals_library"] = bool(np.array_equal(c[:, 0], counts[:, 1]) and np.array_equal(c[:, 1], counts[:, 3] + counts[:, 4]) and
                                           np.array_equal(c[:, 2], counts[:, 5]) and np.array_equal(score, counts[:, 0]) and
                                           int(np.argmax(score)) == int(best[0]))
        row["class_totals_dilate0"] = [int(v) for v in counts[:, 1:].astype(np.int64).sum(axis=0)]
        row["best"] = best.tolist()
        with g.score_alignments_device(tc.data_ptr(), n, tm.data_ptr(), K, dilate=1) as r:
            row["class_totals_dilate1"] = [int(v) for v in r.counts.copy_to_host()[:, 1:].astype(np.int64).sum(axis=0)]

        def lib(dilate):
            g.score_alignments_device(tc.data_ptr(), n, tm.data_ptr(), K, dilate=dilate, weights=TORCH_WEIGHTS).release()
        for label, fn, calls in (("library_us_dilate0", lambda: lib(0), 10), ("library_us_dilate1", lambda: lib(1), 10),
                                 ("torch_us", lambda: _torch_score(torch, g, tc, tm, TORCH_WEIGHTS), 2)):
            for _ in range(2):
                fn()
            bk.sync(g); torch.cuda.synchronize()
            us = []
            for _ in range(5):
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                bk.sync(g); torch.cuda.synchronize()
                us.append(round((time.perf_counter() - t0) / calls * 1e6, 2))
            row[label] = {"per_call": us, "median": bk.median(us)}
        row["torch_over_library"] = round(row["torch_us"]["median"] / row["library_us_dilate0"]["median"], 2)
        out["shapes"]["%dx%d" % (K, n)] = row
        del tc, tm
    out["grid_bytes"] = g.get_tuning("alignment_grid_bytes")
    out["allocations"] = g.get_tuning("alignment_allocations")
    return out


def child_step(name, steps, with_query):
    np, torch, gvom, g, dev, scans = _setup(name)
    K, n = STEP_SHAPE
    if with_query:
        cloud, M, tc, tm = _inputs(np, torch, gvom, g, scans, K, n)
        torch.cuda.synchronize()

    def step(k):
        bk.scan_combine(np, g, dev[k % len(dev)]).release()
        if with_query:
            g.score_alignments_device(tc.data_ptr(), n, tm.data_ptr(), K, dilate=1).release()
    return {"us_per_step": bk.step_loop(g, step, steps, warm=20)["us_per_step"]}


def child_kernel(name, K, n, dilate):
    """Run under rocprofv3: the calls whose kernels are to be timed."""
    np, torch, gvom, g, dev, scans = _setup(name)
    cloud, M, tc, tm = _inputs(np, torch, gvom, g, scans, K, n)
    torch.cuda.synchronize()
    for _ in range(20):
        g.score_alignments_device(tc.data_ptr(), n, tm.data_ptr(), K, dilate=dilate).release()
    bk.sync(g)
    return {"calls": 20}


def main():
    if bk.child(sys.argv[1:], {"call": lambda a: child_call(a[0]), "step": lambda a: child_step(a[0], int(a[1]), a[2] == "1"),
                               "kernel": lambda a: child_kernel(a[0], int(a[1]), int(a[2]), int(a[3]))}):
        return
    args = bk.read_args(sys.argv[1:], configs=CONFIGS, turns=TURNS)        # (--parent: a revision with --resources, a library without)
    parent = args["parent"]
    spawn = lambda mode, a, **kw: bk.spawn(__file__, mode, a, CHILD_TIMEOUT, **kw)
    report = bk.Report("align", args["path"], None if args["resources"] else parent)
    out = report.out
    if args["resources"]:
        out["resources"] = compiled_resources(parent or "HEAD")
        report.save()
        print(json.dumps({k: v for k, v in out["resources"].items() if k.startswith(("trace_and", "k_align"))}))
        print(json.dumps(out["resources"]["gvom_align.hip"]["kernels"], indent=1))
        return
    out["configs"] = {}
    for name in args["configs"]:
        steps = CONFIGS[name]
        res = spawn("call", (name,))
        for key, row in res["shapes"].items():
            K, n = (int(v) for v in key.split("x"))
            for dilate in (0, 1):
                with tempfile.TemporaryDirectory() as d:
                    spawn("kernel", (name, K, n, dilate), profile_dir=d, stats=True)
                    stats = bk.kernel_stats(d, KERNELS)
                ks = {k: v for k in KERNELS for full, v in stats.items() if k in full}
                if "k_align_score" in ks:
                    ks["pairs_per_s"] = round(K * n / (ks["k_align_score"]["avg_us"] * 1e-6))
                row["kernels_dilate%d" % dilate] = ks
        runs = bk.alternate(args["turns"], {"parent_without": parent and (lambda: spawn("step", (name, steps, 0), lib=parent)["us_per_step"]),
                                            "without": lambda: spawn("step", (name, steps, 0))["us_per_step"],
                                            "with": lambda: spawn("step", (name, steps, 1))["us_per_step"]})
        step = {}                                                  # (this file's keys are older than spreads(): the repetitions run by run)
        for k, v in runs.items():
            flat = [u for r in v for u in r]
            if flat:
                step[k] = {"us_per_step": v, "median": bk.median(flat), "spread_us": round(max(flat) - min(flat), 2)}
        if parent:
            d = step["without"]["median"] - step["parent_without"]["median"]
            step["without_minus_parent_us"] = round(d, 2)
            step["within_parent_spread"] = bool(abs(d) <= step["parent_without"]["spread_us"])
        step["query"] = "%d x %d, dilate 1" % STEP_SHAPE
        res["step"] = step
        out["configs"][name] = res
        report.save()                                              # (after every config: a long run leaves what it has)
    print(json.dumps(out["configs"], indent=1))


if __name__ == "__main__":
    main()
