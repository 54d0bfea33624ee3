#!/usr/bin/env python3
"""What rollout scoring (gvom_score_rollouts, k_rollouts) costs.  On the maps of m256 (256 x 256) and c4 (512 x 512) after three
bench scans, against the cost field towards the ego's cell, with a car footprint of about 325 cells per heading (64 headings; the
rectangle of 18 x 11 cells in front of, 5 behind the axle, whatever the config's resolution), for (K, T) = (4096, 64) and
(16384, 128), rollouts either COHERENT (arcs that leave the ego, a cell a pose) or SHUFFLED (the same poses in random order: no two
neighbours of a rollout are neighbours on the map) -- every loop in a fresh child process:

  call       DeviceCostField.score_rollouts' device route (poses in device memory), enqueue to completion: wall time
  kernel     one `rocprofv3 --kernel-trace` run per config, the four combinations in a known order: k_rollouts; with the gathers the poses ask for
             (the cells of every valid pose's heading, counted on the host) that gives the achieved gathers / s
  torch      the same scoring written in torch on the exported cell_cost -- an index tensor of K x T x M cells (in chunks of 2048
             rollouts), gather, amax, cumsum -- CHECKED EQUAL to the product (pose costs, first blocked pose, path cost) before it
             is timed.  The acceptance bar of the kernel: it has to beat this by more than the spread of both
  step       scan + combine_maps_device() + cost_to_go() per step, without and with score_rollouts; and, with --parent LIB (the
             parent commit's libgvom_hip.so), the same step without scoring on that library, alternating with this one
  registers  tools/kernel_regs.py on the kernel

    tools/rollouts_bench.py [--parent LIB] [out.json]      (default: profiles/rollouts_<lib sha8>.json)
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
CONFIGS = (("m256", 100), ("c4", 40))                      # (config, timed steps per repetition)
SHAPES = ((4096, 64), (16384, 128))
ORDERS = ("coherent", "shuffled")
CAR_CELLS = dict(front=18.0, rear=5.0, half_width=5.5)     # in cells of the config's xy_resolution
HEADINGS = 64
THRESHOLD, SOFT = 50, 10
CHUNK = 2048                                               # rollouts per chunk of the torch form


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


def _field_args(g):
    return dict(goals_in_cells=True, inflation_radius=None, density_threshold=THRESHOLD, soft_weight=SOFT)


def _car(gvom, g):
    r = g.xy_resolution
    return gvom.rectangle_footprint(CAR_CELLS["front"] * r, CAR_CELLS["rear"] * r, CAR_CELLS["half_width"] * r, r, headings=HEADINGS)


def _poses(np, K, T, ego, res, order, seed=1):
    """K arcs of T poses from the ego, a cell a pose, float32 [K, T, 3]; shuffled: the same poses in random order"""
    rng = np.random.default_rng(seed)
    th0 = rng.uniform(-np.pi, np.pi, K)
    curv = rng.uniform(-0.04, 0.04, K)
    t = np.arange(T)
    th = th0[:, None] + curv[:, None] * t[None, :]
    x = ego[0] + np.cumsum(res * np.cos(th), axis=1)
    y = ego[1] + np.cumsum(res * np.sin(th), axis=1)
    p = np.stack([x, y, th], axis=2).astype(np.float32)
    if order == "shuffled":
        p = p.reshape(K * T, 3)[rng.permutation(K * T)].reshape(K, T, 3)
    return np.ascontiguousarray(p)


def _torch_score(torch, cflat, poses, offs_pad, res, oc, xy):
    """the scoring in torch on the flat [y * xy + x] uint16 -> int32 cost map: (pose_cost int32 [K, T], first [K], path [K]).
    offs_pad [H, Mmax, 2]: the table, every heading padded with repeats of its first cell (a maximum does not mind)."""
    H = offs_pad.shape[0]
    s = torch.tensor(H / (2.0 * 3.141592653589793), dtype=torch.float32, device=poses.device)
    K, T = poses.shape[:2]
    cost = torch.empty((K, T), dtype=torch.int32, device=poses.device)
    for k0 in range(0, K, CHUNK):
        p = poses[k0:k0 + CHUNK]
        cx = (torch.floor(p[..., 0].double() / res).long() - oc[0]).int()
        cy = (torch.floor(p[..., 1].double() / res).long() - oc[1]).int()
        h = torch.remainder(torch.round(p[..., 2] * s).long(), H)
        o = offs_pad[h]                                            # [k, T, Mmax, 2]: the index tensor
        X, Y = cx[..., None] + o[..., 0], cy[..., None] + o[..., 1]
        inside = (X >= 0) & (X < xy) & (Y >= 0) & (Y < xy)
        v = cflat[(Y.clamp(0, xy - 1) * xy + X.clamp(0, xy - 1)).long()]        # gather
        blocked = (~inside).any(dim=-1) | ((v == 0) & inside).any(dim=-1)
        cost[k0:k0 + CHUNK] = torch.where(blocked, torch.zeros_like(cx), torch.where(inside, v, torch.zeros_like(v)).amax(dim=-1))
    zero = cost == 0
    first = torch.where(zero.any(dim=1), zero.int().argmax(dim=1), torch.full((K,), T, device=cost.device))
    csum = torch.cumsum(cost.long(), dim=1)
    path = torch.where(first > 0, csum.gather(1, (first - 1).clamp(min=0)[:, None])[:, 0], torch.zeros_like(first))
    return cost, first, path


def child_score(name, profiled):
    np, torch, gvom, g, dev = _setup(name)
    for t, ego, tf in dev:
        g.process_pointcloud_device(t.data_ptr(), t.shape[0], np.float32, ego, tf)
        m = g.combine_maps_device()
    ego = dev[2][1]
    res, xy = g.xy_resolution, g.xy_size
    table = _car(gvom, g)
    g.set_footprint(table)
    e = gvom.world_to_cells([ego[:2]], res, m.origin)[0]
    f = m.cost_to_go([e], **_field_args(g))
    cells = np.diff(table[0]).astype(np.int64)
    oc = tuple(int(v) for v in np.round(np.asarray(m.origin)[:2] / res))
    cflat = torch.from_dlpack(f.cell_cost).view(torch.int16).T.contiguous().view(-1).to(torch.int32) & 0xFFFF   # cell (x, y) at [y * xy + x]
    mmax = int(cells.max())
    pad = np.stack([np.concatenate([table[1][table[0][k]:table[0][k + 1]], np.repeat(table[1][table[0][k]:table[0][k] + 1], mmax - cells[k], axis=0)])
                    for k in range(HEADINGS)]).astype(np.int32)
    offs_pad = torch.from_numpy(pad).cuda()
    reps, results = 20, []
    for K, T in SHAPES:
        for order in ORDERS:
            poses = _poses(np, K, T, ego, res, order)
            tp = torch.from_numpy(poses).cuda()
            torch.cuda.synchronize()
            call = lambda: g.score_rollouts_of_device(f.cell_cost.ptr, tp.data_ptr(), K, T, cost_to_go_ptr=f.cost.ptr, origin=m.origin)
            if profiled:                                           # under rocprofv3: `reps` launches per combination, in this order
                for _ in range(reps):
                    call().release()
                g._check(g._lib.gvom_sync(g._h))
                continue
            # the gathers the poses ask for: the cells of every pose's heading (every pose here is valid)
            hs = np.rint(poses[..., 2] * np.float32(HEADINGS / (2.0 * np.pi))).astype(np.int64) % HEADINGS
            out = {"xy": xy, "K": K, "T": T, "order": order, "cells_per_heading_mean": round(float(cells.mean()), 1), "gathers": int(cells[hs].sum())}
            for _ in range(3):
                call().release()
            g._check(g._lib.gvom_sync(g._h))
            us = []
            for rep in range(5):
                t0 = time.perf_counter()
                for _ in range(reps):
                    call().release()
                g._check(g._lib.gvom_sync(g._h))
                us.append(round((time.perf_counter() - t0) / reps * 1e6, 2))
            out["call_us"] = us
            out["call_us_median"] = _median(us)
            r = call()
            summary, cost = r.copy_to_host()
            out["status_counts"] = np.bincount(summary[:, 0], minlength=4).tolist()
            out["blocked_pose_share"] = round(float((cost == 0).mean()), 4)
            # the torch form on the exported cost map (zero-copy), checked, then timed
            tcost, tfirst, tpath = _torch_score(torch, cflat, tp, offs_pad, res, oc, xy)
            same = bool(np.array_equal(tcost.cpu().numpy(), cost.astype(np.int32)) and np.array_equal(tfirst.cpu().numpy(), summary[:, 1]) and
                        np.array_equal(tpath.cpu().numpy(), summary[:, 2]))
            del tcost, tfirst, tpath
            torch.cuda.synchronize()
            tus = []
            for rep in range(5):
                t0 = time.perf_counter()
                _torch_score(torch, cflat, tp, offs_pad, res, oc, xy)
                torch.cuda.synchronize()
                tus.append(round((time.perf_counter() - t0) * 1e6, 1))
            out["torch"] = {"equals_product": same, "us": tus, "us_median": _median(tus), "chunk_rollouts": CHUNK, "padded_cells_per_pose": mmax,
                            "index_bytes_per_call": int(K) * int(T) * mmax * 4}
            r.release()
            results.append(out)
    return {"calls": reps} if profiled else {"scoring": results}


def child_step(name, steps, score):
    np, torch, gvom, g, dev = _setup(name)
    K, T = SHAPES[0]
    res = g.xy_resolution
    if score:
        g.set_footprint(_car(gvom, g))
    tp = [torch.from_numpy(_poses(np, K, T, ego, res, "coherent")).cuda() for _, ego, _ in dev]
    torch.cuda.synchronize()

    def step(k):
        t, ego, tf = dev[k % 3]
        g.process_pointcloud_device(t.data_ptr(), t.shape[0], np.float32, ego, tf)
        m = g.combine_maps_device()
        e = gvom.world_to_cells([ego[:2]], res, m.origin)[0]
        f = m.cost_to_go([e], **_field_args(g))
        if score:
            g.score_rollouts_of_device(f.cell_cost.ptr, tp[k % 3].data_ptr(), K, T, cost_to_go_ptr=f.cost.ptr, origin=m.origin).release()
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
    return {"us_per_step": us, "us_per_step_median": _median(us), "steps": steps, "K": K if score else 0, "T": T if score else 0}


def _spawn(mode, args, profile_dir=None, lib=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode] + [str(a) for a in args]
    if profile_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", profile_dir, "--"] + cmd
    env = dict(os.environ, GVOM_HIP_LIBRARY=os.path.abspath(lib)) if lib else None
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, env=env)
    if r.returncode != 0:
        raise SystemExit("%s %r failed (%d):\n%s" % (mode, args, r.returncode, r.stderr[-3000:]))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def _kernel_times(profile_dir, calls):
    """the k_rollouts dispatches of a profiled run in launch order, `calls` per combination: per combination the kernel's times
    without its first three launches"""
    rows = []
    for f in glob.glob(os.path.join(profile_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "k_rollouts" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    out = []
    for k in range(len(rows) // calls):
        us = [u for _, u in rows[k * calls + 3:(k + 1) * calls]]
        out.append({"launches": len(us), "avg_us": round(sum(us) / len(us), 2), "median_us": round(_median(us), 2), "min_us": round(min(us), 2),
                    "max_us": round(max(us), 2)})
    return out


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        mode, a = sys.argv[2], sys.argv[3:]
        if mode == "score":
            res = child_score(a[0], a[1] == "1")
        else:
            res = child_step(a[0], int(a[1]), a[2] == "1")
        print("RESULT " + json.dumps(res))
        return
    import kernel_regs
    import lib_identity
    args = sys.argv[1:]
    parent = None
    if args and args[0] == "--parent":
        parent, args = args[1], args[2:]
    new = os.path.join(ROOT, "g-vom_amd", "lib", "libgvom_hip.so")
    out = {"library": lib_identity.identity(), "footprint_cells": CAR_CELLS, "headings": HEADINGS, "density_threshold": THRESHOLD, "soft_weight": SOFT,
           "registers": {k: v for k, v in kernel_regs.kernels(new).items() if "k_rollouts" in k},
           "unmeasured": ["a two-kernel form (poses, then summaries) and row spans instead of cell lists (neither is built)",
                          "maps larger than c4's 512 x 512", "footprints of other sizes"],
           "configs": {}}
    if parent:
        out["parent_library"] = {"lib_sha256": lib_identity.sha256_file(parent)}
    path = args[0] if args else os.path.join(ROOT, "profiles", "rollouts_%s.json" % (out["library"].get("lib_sha256") or "unknown")[:8])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    for name, steps in CONFIGS:
        res = _spawn("score", (name, 0))
        with tempfile.TemporaryDirectory() as d:
            calls = _spawn("score", (name, 1), profile_dir=d)["calls"]
            kernel = _kernel_times(d, calls)
        for k, rec in enumerate(res["scoring"]):
            rec["kernel"] = kernel[k] if len(kernel) == len(res["scoring"]) else None
            if rec["kernel"]:
                rec["gathers_per_s"] = round(rec["gathers"] / (rec["kernel"]["median_us"] * 1e-6), 0)
                rec["torch_over_kernel"] = round(rec["torch"]["us_median"] / rec["kernel"]["median_us"], 1)
            rec["torch_over_call"] = round(rec["torch"]["us_median"] / rec["call_us_median"], 1)
            # beaten by more than the spread of both: the slowest call against the fastest torch run
            rec["beats_torch_beyond_spread"] = bool(max(rec["call_us"]) < min(rec["torch"]["us"]))
        runs = {"without": [], "with": [], "parent_without": []}
        for rnd in range(2):                                        # alternating: parent, without, with, ...
            if parent:
                runs["parent_without"].append(_spawn("step", (name, steps, 0), lib=parent))
            runs["without"].append(_spawn("step", (name, steps, 0)))
            runs["with"].append(_spawn("step", (name, steps, 1)))
        step = {}
        for who, rs in runs.items():
            if rs:
                us = [u for r in rs for u in r["us_per_step"]]
                step[who] = {"us_per_step": us, "median": _median(us), "spread_us": round(max(us) - min(us), 2)}
        step["scoring_adds_us_per_step"] = round(step["with"]["median"] - step["without"]["median"], 2)
        if parent:
            d = step["without"]["median"] - step["parent_without"]["median"]
            step["without_minus_parent_us"] = round(d, 2)
            step["within_parent_spread"] = bool(abs(d) <= step["parent_without"]["spread_us"])
        res["step: scan + combine_maps_device + cost_to_go (+ score_rollouts %d x %d)" % SHAPES[0]] = step
        out["configs"][name] = res
        with open(path, "w") as f:                                  # (after every config: a long run leaves what it has)
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
