#!/usr/bin/env python3
"""What the obstacle clearance map (gvom_clearance) costs.  On m256, c4 and c5 -- obstacle-bearing maps after three scans --
unbounded and with max_distance = robot_radius, every loop in a fresh child process:

  kernels   one `rocprofv3 --kernel-trace --stats` run per config and cap: k_clearance_rows and k_clearance_cols
  step      scan + combine_maps_device() per step, without and with DeviceMaps.clearance(); and, in the same run, the same loop
            with the same transform WRITTEN IN TORCH on the DLPack'd positive / negative maps (a dense separable min-plus, no host
            synchronisation) -- what a consumer has without this entry point.  The torch result is checked against the
            library's squared cells once before the timing.
  registers tools/kernel_regs.py on the library's k_clearance* kernels

    tools/clearance_bench.py [out.json]      (default: profiles/clearance_<lib sha8>.json)
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
CONFIGS = (("m256", 400), ("c4", 100), ("c5", 30))          # (config, timed steps per repetition)
THRESHOLD = 50


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def _torch_clearance(torch, pos, neg, thr, res, cap2):
    """(distance, squared cells) of [x, y] int32 tensors: the separable transform as dense min-plus products, in blocks of at
    most 2^26 elements"""
    xy = pos.shape[0]
    big = 1 << 29
    mask = (pos > thr) | (neg > 0)
    idx = torch.arange(xy, device=pos.device, dtype=torch.int32)
    sq = (idx[:, None] - idx[None, :]) ** 2                                    # [a, b] = (a - b)^2
    blk = max(1, (1 << 26) // (xy * xy))
    pen = torch.where(mask, 0, big).to(torch.int32)                            # [i, y]
    g2 = torch.empty((xy, xy), dtype=torch.int32, device=pos.device)
    for x0 in range(0, xy, blk):                                               # g2[x, y] = min_i (x - i)^2 + pen[i, y]
        g2[x0:x0 + blk] = (sq[x0:x0 + blk, :, None] + pen[None, :, :]).amin(dim=1)
    d2 = torch.empty((xy, xy), dtype=torch.int32, device=pos.device)
    for x0 in range(0, xy, blk):                                               # d2[x, y] = min_j g2[x, j] + (y - j)^2
        d2[x0:x0 + blk] = (g2[x0:x0 + blk, :, None] + sq[None, :, :]).amin(dim=1)
    far = d2 >= big if cap2 <= 0 else (d2 > cap2)
    d2 = torch.where(far, 2147483647, d2).to(torch.int32)
    dist = torch.where(far, float("inf"), (d2.to(torch.float64).sqrt() * res)).to(torch.float32)
    return dist, d2


def _setup(name, poses):
    import numpy as np
    import torch
    import gvom
    import synth
    torch.cuda.init()
    params, scans = synth.config_inputs(name, n_scans=poses)
    dev = [(torch.from_numpy(np.ascontiguousarray(pc)).cuda(), ego, tf) for pc, ego, tf in scans]
    torch.cuda.synchronize()
    g = gvom.Gvom(*params, voxel_statistics=False)
    return np, torch, gvom, g, dev


def child_step(name, steps):
    poses = 3
    np, torch, gvom, g, dev = _setup(name, poses)
    radius = float(g.robot_radius)
    cap2 = gvom._clearance_cap(radius, g.xy_resolution)

    def scan(k):
        t, ego, tf = dev[k % poses]
        g.process_pointcloud_device(t.data_ptr(), t.shape[0], np.float32, ego, tf)
        return g.combine_maps_device()

    def plain(k):
        scan(k).release()

    def lib(max_distance):
        def step(k):
            m = scan(k)
            m.clearance(THRESHOLD, max_distance=max_distance).release()
            m.release()
        return step

    def in_torch(c2):
        def step(k):
            m = scan(k)
            pos, neg = torch.from_dlpack(m.positive), torch.from_dlpack(m.negative)
            _torch_clearance(torch, pos, neg, THRESHOLD, g.xy_resolution, c2)
            del pos, neg
            m.release()
        return step

    # the maps hold obstacles, and the torch form computes what the library does
    for k in range(poses):
        m = scan(k)
    c = m.clearance(THRESHOLD)
    d2 = c.squared_cells.copy_to_host()
    pos = m.positive.copy_to_host()
    t_d2 = _torch_clearance(torch, torch.from_dlpack(m.positive), torch.from_dlpack(m.negative), THRESHOLD, g.xy_resolution, 0)[1]
    same = bool(np.array_equal(t_d2.cpu().numpy(), d2))
    info = {"xy": g.xy_size, "obstacle_cells": int((d2 == 0).sum()), "cells_above_threshold": int((pos > THRESHOLD).sum()),
            "robot_radius_m": radius, "max_cells2_at_robot_radius": cap2, "torch_form_equals_library": same}
    c.release()
    m.release()
    del t_d2
    out = {"maps": info, "steps": steps}
    loops = (("scan+combine_maps_device", plain, steps), ("+clearance unbounded", lib(None), steps),
             ("+clearance max_distance=robot_radius", lib(radius), steps),
             ("+torch transform unbounded", in_torch(0), max(steps // 10, 5)),
             ("+torch transform max_distance=robot_radius", in_torch(cap2), max(steps // 10, 5)))
    for label, step, n in loops:
        for k in range(min(20, n)):
            step(k)
        g._check(g._lib.gvom_sync(g._h))
        torch.cuda.synchronize()
        us = []
        for rep in range(3):
            t0 = time.perf_counter()
            for k in range(n):
                step(k)
            g._check(g._lib.gvom_sync(g._h))
            torch.cuda.synchronize()
            us.append(round((time.perf_counter() - t0) / n * 1e6, 2))
        out[label] = {"us_per_step": us, "us_per_step_median": _median(us), "steps": n}
    return out


def child_kernels(name, capped):
    """Run under rocprofv3: the calls whose kernels are to be timed."""
    np, torch, gvom, g, dev = _setup(name, 3)
    for t, ego, tf in dev:
        g.process_pointcloud_device(t.data_ptr(), t.shape[0], np.float32, ego, tf)
        m = g.combine_maps_device()
    for _ in range(50):
        m.clearance(THRESHOLD, max_distance=float(g.robot_radius) if capped else None).release()
    g._check(g._lib.gvom_sync(g._h))
    return {"calls": 50}


def _spawn(mode, args, profile_dir=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode] + [str(a) for a in args]
    if profile_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", profile_dir, "--"] + cmd
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit("%s %r failed (%d):\n%s" % (mode, args, r.returncode, r.stderr[-3000:]))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def _kernel_stats(profile_dir):
    rows = {}
    for f in glob.glob(os.path.join(profile_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "k_clearance" in r["Name"]:
                rows[r["Name"].split("(")[0]] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                                                 "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
    return rows


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        mode = sys.argv[2]
        res = child_step(sys.argv[3], int(sys.argv[4])) if mode == "step" else child_kernels(sys.argv[3], sys.argv[4] == "1")
        print("RESULT " + json.dumps(res))
        return
    import kernel_regs
    import lib_identity
    new = os.path.join(ROOT, "g-vom_amd", "lib", "libgvom_hip.so")
    out = {"library": lib_identity.identity(), "density_threshold": THRESHOLD,
           "registers": {k: v for k, v in kernel_regs.kernels(new).items() if "k_clearance" in k}, "configs": {}}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
        ROOT, "profiles", "clearance_%s.json" % (out["library"].get("lib_sha256") or "unknown")[:8])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    for name, steps in CONFIGS:
        res = _spawn("step", (name, steps))
        res["kernel_us"] = {}
        for label, capped in (("unbounded", 0), ("max_distance=robot_radius", 1)):
            with tempfile.TemporaryDirectory() as d:
                _spawn("kernels", (name, capped), profile_dir=d)
                stats = _kernel_stats(d)
            stats["both"] = round(sum(v["avg_us"] for v in stats.values()), 2)
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
