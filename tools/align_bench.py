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

    tools/align_bench.py [--resources [--parent REV]] [--parent LIB] [out.json]
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
PKG = os.path.join(ROOT, "g-vom_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CONFIGS = (("m256", 400), ("c4", 100))                     # (config, timed steps per repetition)
SHAPES = ((4096, 16384), (9261, 4096))                     # (K, n)
STEP_SHAPE = (9261, 4096)
TORCH_WEIGHTS = (3, 0, -1, -1, 0)                          # free and unknown weigh the same: what an occupancy grid can tell
TORCH_CHUNK = 128                                          # candidates per chunk of the torch form


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


# ---- resources (CPU) ---------------------------------------------------------------------------------------------------------
def resources(parent):
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
    for t, ego, tf in dev:
        g.process_pointcloud_device(t.data_ptr(), t.shape[0], np.float32, ego, tf)
        g.combine_maps_device().release()
    return np, torch, gvom, g, dev, scans


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
            g._check(g._lib.gvom_sync(g._h)); torch.cuda.synchronize()
            us = []
            for _ in range(5):
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                g._check(g._lib.gvom_sync(g._h)); torch.cuda.synchronize()
                us.append(round((time.perf_counter() - t0) / calls * 1e6, 2))
            row[label] = {"per_call": us, "median": _median(us)}
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
        t, e, tf = dev[k % len(dev)]
        g.process_pointcloud_device(t.data_ptr(), t.shape[0], np.float32, e, tf)
        g.combine_maps_device().release()
        if with_query:
            g.score_alignments_device(tc.data_ptr(), n, tm.data_ptr(), K, dilate=1).release()
    for k in range(20):
        step(k)
    g._check(g._lib.gvom_sync(g._h))
    us = []
    for _ in range(3):
        t0 = time.perf_counter()
        for k in range(steps):
            step(k)
        g._check(g._lib.gvom_sync(g._h))
        us.append(round((time.perf_counter() - t0) / steps * 1e6, 2))
    return {"us_per_step": us}


def child_kernel(name, K, n, dilate):
    """Run under rocprofv3: the calls whose kernels are to be timed."""
    np, torch, gvom, g, dev, scans = _setup(name)
    cloud, M, tc, tm = _inputs(np, torch, gvom, g, scans, K, n)
    torch.cuda.synchronize()
    for _ in range(20):
        g.score_alignments_device(tc.data_ptr(), n, tm.data_ptr(), K, dilate=dilate).release()
    g._check(g._lib.gvom_sync(g._h))
    return {"calls": 20}


def _spawn(mode, args, profile_dir=None, lib=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode] + [str(x) for x in args]
    if profile_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", profile_dir, "--"] + cmd
    env = dict(os.environ, GVOM_HIP_LIBRARY=os.path.abspath(lib)) if lib else None
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, env=env)
    if r.returncode != 0:
        raise SystemExit("%s %r failed (%d):\n%s" % (mode, args, r.returncode, r.stderr[-3000:]))
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def _kernel_stats(profile_dir):
    out = {}
    for f in glob.glob(os.path.join(profile_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            for k in ("k_align_field", "k_align_score", "k_align_best"):
                if k in r["Name"]:
                    out[k] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "min_us": round(float(r["MinNs"]) / 1e3, 2),
                              "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
    return out


def main():
    argv = sys.argv[1:]
    if len(argv) > 1 and argv[0] == "--child":
        mode, a = argv[1], argv[2:]
        res = (child_call(a[0]) if mode == "call" else child_step(a[0], int(a[1]), a[2] == "1") if mode == "step" else
               child_kernel(a[0], int(a[1]), int(a[2]), int(a[3])))
        print("RESULT " + json.dumps(res))
        return
    import lib_identity
    ident = lib_identity.identity()
    do_resources = "--resources" in argv
    argv = [x for x in argv if x != "--resources"]
    parent = None
    if "--parent" in argv:
        k = argv.index("--parent")
        parent, argv = argv[k + 1], argv[:k] + argv[k + 2:]
    path = argv[0] if argv else os.path.join(ROOT, "profiles", "align_%s.json" % (ident.get("lib_sha256") or "unknown")[:8])
    out = json.load(open(path)) if os.path.exists(path) else {}
    out["library"] = ident
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)

    def save():
        with open(path, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if do_resources:
        out["resources"] = resources(parent or "HEAD")
        save()
        print(json.dumps({k: v for k, v in out["resources"].items() if k.startswith(("trace_and", "k_align"))}))
        print(json.dumps(out["resources"]["gvom_align.hip"]["kernels"], indent=1))
        return
    if parent:
        out["parent_library"] = {"lib_sha256": lib_identity.sha256_file(parent)}
    out["configs"] = {}
    for name, steps in CONFIGS:
        res = _spawn("call", (name,))
        for key, row in res["shapes"].items():
            K, n = (int(v) for v in key.split("x"))
            for dilate in (0, 1):
                with tempfile.TemporaryDirectory() as d:
                    _spawn("kernel", (name, K, n, dilate), profile_dir=d)
                    ks = _kernel_stats(d)
                if "k_align_score" in ks:
                    ks["pairs_per_s"] = round(K * n / (ks["k_align_score"]["avg_us"] * 1e-6))
                row["kernels_dilate%d" % dilate] = ks
        runs = {"without": [], "with": [], "parent_without": []}
        for _ in range(2):                                         # alternating: parent, without, with, ...
            if parent:
                runs["parent_without"].append(_spawn("step", (name, steps, 0), lib=parent)["us_per_step"])
            runs["without"].append(_spawn("step", (name, steps, 0))["us_per_step"])
            runs["with"].append(_spawn("step", (name, steps, 1))["us_per_step"])
        step = {}
        for k, v in runs.items():
            flat = [u for r in v for u in r]
            if flat:
                step[k] = {"us_per_step": v, "median": _median(flat), "spread_us": round(max(flat) - min(flat), 2)}
        if parent:
            d = step["without"]["median"] - step["parent_without"]["median"]
            step["without_minus_parent_us"] = round(d, 2)
            step["within_parent_spread"] = bool(abs(d) <= step["parent_without"]["spread_us"])
        step["query"] = "%d x %d, dilate 1" % STEP_SHAPE
        res["step"] = step
        out["configs"][name] = res
        save()                                                     # (after every config: a long run leaves what it has)
    print(json.dumps(out["configs"], indent=1))


if __name__ == "__main__":
    main()
