#!/usr/bin/env python3
"""What terrain attitude scoring (gvom_score_attitude: k_attitude_ground, k_attitude) costs.  On the maps of m256 (256 x 256) and c4
(512 x 512) after three bench scans, against the map set's own ground, with the car footprint of tests/rollouts_ref.py (CAR: about
325 cells per heading at 0.2 m, 64 headings) and the car chassis of tests/attitude_ref.py, for (K, T) = (4096, 64) and (16384, 128),
arcs that leave the ego a cell a pose -- every loop in a fresh child process, every child under a `timeout` of its own, and the
first child that fails ends the run:

  call       gvom_score_attitude with poses in device memory, by map set and by pointer (the same ground as one device array),
             enqueue to completion, and gvom_score_rollouts at the same shape against the cost field towards the ego, as a
             yardstick: wall time
  kernel     one `rocprofv3 --kernel-trace` run per config, the calls in a known order: k_attitude, k_attitude_ground, k_rollouts
  torch      the same scoring written in torch on the exported height maps -- index tensors of K x T x M cells in chunks of
             rollouts, gathers, float64 arithmetic, amin.  Its STATUSES are compared with the product's first; the largest
             difference of the values is reported, not judged
  step       scan + combine_maps_device() per step, without and with a score_attitude of 4096 x 64; and, with --parent LIB (the
             parent commit's libgvom_hip.so), the same step without a query on that library, alternating, five runs each
  resources  tools/kernel_regs.py: the new kernels, and registers, scratch, LDS and code size of every kernel outside the new
             unit on the parent and on this library (--resources alone: no GPU needed)

    tools/attitude_bench.py [--resources] [--parent LIB] [out.json]      (default: profiles/attitude_<lib sha8>.json)
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
CAR = dict(front=3.6, rear=1.0, half_width=1.1)            # metres: tests/rollouts_ref.py CAR
CHASSIS = dict(front_axle=2.7, rear_axle=0.0, track=1.7, belly_height=0.25, max_pitch=0.35, max_roll=0.3, min_clearance=0.1)   # angles in radians
HEADINGS = 64
CHUNK = 512                                                # rollouts per chunk of the torch form
CHILD_TIMEOUT = 420                                        # seconds, per child process


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


def _vehicle(gvom, g):
    table = gvom.rectangle_footprint(CAR["front"], CAR["rear"], CAR["half_width"], g.xy_resolution, headings=HEADINGS)
    g.set_footprint(table)
    g.set_chassis(gvom.chassis(**CHASSIS))
    return table


def _poses(np, K, T, ego, res, seed=1):
    """K arcs of T poses from the ego, a cell a pose, float32 [K, T, 3]"""
    rng = np.random.default_rng(seed)
    th0 = rng.uniform(-np.pi, np.pi, K)
    curv = rng.uniform(-0.04, 0.04, K)
    t = np.arange(T)
    th = th0[:, None] + curv[:, None] * t[None, :]
    x = ego[0] + np.cumsum(res * np.cos(th), axis=1)
    y = ego[1] + np.cumsum(res * np.sin(th), axis=1)
    return np.ascontiguousarray(np.stack([x, y, th], axis=2).astype(np.float32))


def _torch_score(torch, gflat, poses, offs_pad, live, wheels, cs, ch, res, oc, xy):
    """the scoring in torch on the flat [y * xy + x] float64 ground: (values float32 [K, T, 3], status uint8 [K, T]).  offs_pad
    [H, Mmax, 2] with live [H, Mmax] (False on the padding); wheels [H, 4, 2], cs [H, 2] float64.  torch may contract a product and
    a sum: the values can differ from the product's in the last bits (reported, not judged)."""
    H = offs_pad.shape[0]
    s = torch.tensor(H / (2.0 * 3.141592653589793), dtype=torch.float32, device=poses.device)
    K, T = poses.shape[:2]
    vals = torch.zeros((K, T, 3), dtype=torch.float32, device=poses.device)
    status = torch.empty((K, T), dtype=torch.uint8, device=poses.device)
    wb, am = ch.front_axle - ch.rear_axle, 0.5 * (ch.front_axle + ch.rear_axle)
    inf = float("inf")
    for k0 in range(0, K, CHUNK):
        p = poses[k0:k0 + CHUNK]
        x, y = p[..., 0].double(), p[..., 1].double()
        qx, qy = x / res, y / res
        cx, cy = torch.floor(qx).long() - oc[0], torch.floor(qy).long() - oc[1]
        fx, fy = qx - torch.floor(qx), qy - torch.floor(qy)
        h = torch.remainder(torch.round(p[..., 2] * s).long(), H)
        w = wheels[h]                                              # [k, T, 4, 2]
        wx = torch.floor((x[..., None] + w[..., 0]) / res).long() - oc[0]
        wy = torch.floor((y[..., None] + w[..., 1]) / res).long() - oc[1]
        w_in = ((wx >= 0) & (wx < xy) & (wy >= 0) & (wy < xy)).all(dim=-1)
        z = gflat[wy.clamp(0, xy - 1) * xy + wx.clamp(0, xy - 1)]
        w_known = ((z > -1000.0) & (z < inf)).all(dim=-1)
        z = torch.where((w_in & w_known)[..., None], z, torch.zeros_like(z))
        sp = (0.5 * (z[..., 0] + z[..., 1]) - 0.5 * (z[..., 2] + z[..., 3])) / wb
        sr = (0.5 * (z[..., 0] + z[..., 2]) - 0.5 * (z[..., 1] + z[..., 3])) / ch.track
        z0 = 0.25 * ((z[..., 0] + z[..., 1]) + (z[..., 2] + z[..., 3]))
        o = offs_pad[h]                                            # [k, T, Mmax, 2]: the index tensor
        lv = live[h]
        X, Y = cx[..., None] + o[..., 0], cy[..., None] + o[..., 1]
        inside = (X >= 0) & (X < xy) & (Y >= 0) & (Y < xy)
        out = (lv & ~inside).any(dim=-1)
        gg = gflat[Y.clamp(0, xy - 1) * xy + X.clamp(0, xy - 1)]       # gather
        use = lv & inside & (gg > -1000.0) & (gg < inf)
        c, sn = cs[h][..., 0:1], cs[h][..., 1:2]
        du = ((o[..., 0].double() + 0.5) - fx[..., None]) * res
        dv = ((o[..., 1].double() + 0.5) - fy[..., None]) * res
        u, v = du * c + dv * sn, dv * c - du * sn
        clr = ((z0[..., None] + sp[..., None] * (u - am)) + sr[..., None] * v + ch.belly_height) - gg
        belly = torch.where(use, clr, torch.full_like(clr, inf)).amin(dim=-1)
        a = torch.stack([sp, sr, belly], dim=-1).float()
        st = torch.zeros_like(h, dtype=torch.uint8)
        st[a[..., 2] < ch.min_clearance] = 3
        st[a[..., 1].abs() > ch.max_roll] = 2
        st[a[..., 0].abs() > ch.max_pitch] = 1
        st[~w_known] = 4
        st[~w_in | out] = 5
        a[st >= 4] = 0
        vals[k0:k0 + CHUNK], status[k0:k0 + CHUNK] = a, st
    return vals, status


def child_score(name, profiled):
    np, torch, gvom, g, dev = _setup(name)
    for t, ego, tf in dev:
        g.process_pointcloud_device(t.data_ptr(), t.shape[0], np.float32, ego, tf)
        m = g.combine_maps_device()
    ego = dev[2][1]
    res, xy = g.xy_resolution, g.xy_size
    table = _vehicle(gvom, g)
    ch = gvom.chassis(**CHASSIS)
    e = gvom.world_to_cells([ego[:2]], res, m.origin)[0]
    f = m.cost_to_go([e], goals_in_cells=True, inflation_radius=None, density_threshold=50, soft_weight=10)
    cells = np.diff(table[0]).astype(np.int64)
    oc = tuple(int(v) for v in np.round(np.asarray(m.origin)[:2] / res))
    # the ground of the set's maps 4 and 5 as the library builds it, [y * xy + x]
    hgt, inf_h = torch.from_dlpack(m.height_map), torch.from_dlpack(m.inferred_height_map)
    gflat = torch.where(hgt > -1000.0, hgt, inf_h).T.contiguous().view(-1)
    mmax = int(cells.max())
    pad = np.zeros((HEADINGS, mmax, 2), np.int64)
    live = np.zeros((HEADINGS, mmax), bool)
    for k in range(HEADINGS):
        pad[k, :cells[k]] = table[1][table[0][k]:table[0][k + 1]]
        live[k, :cells[k]] = True
    offs_pad, live_t = torch.from_numpy(pad).cuda(), torch.from_numpy(live).cuda()
    half = ch.track / 2
    ab = ((ch.front_axle, half), (ch.front_axle, -half), (ch.rear_axle, half), (ch.rear_axle, -half))
    wheels = np.array([[(a * c - b * s, a * s + b * c) for a, b in ab] for c, s in g.cos_sin.tolist()])
    wheels_t, cs_t = torch.from_numpy(wheels).cuda(), torch.from_numpy(g.cos_sin).cuda()
    reps, results = 20, []
    for K, T in SHAPES:
        poses = _poses(np, K, T, ego, res)
        tp = torch.from_numpy(poses).cuda()
        torch.cuda.synchronize()
        by_set = lambda: g._score_attitude(m.set_id, None, gvom._dev(tp.data_ptr()), K, T, 1, True, m.origin)
        by_ptr = lambda: g.score_attitude_of_device(gflat.data_ptr(), tp.data_ptr(), K, T, origin=m.origin)
        rollouts = lambda: g.score_rollouts_of_device(f.cell_cost.ptr, tp.data_ptr(), K, T, cost_to_go_ptr=f.cost.ptr, origin=m.origin)
        calls = (("attitude_map_set", by_set), ("attitude_pointer", by_ptr), ("rollouts", rollouts))
        if profiled:                                           # under rocprofv3: `reps` launches per call, in this order
            for _, call in calls:
                for _ in range(reps):
                    call().release()
                g._check(g._lib.gvom_sync(g._h))
            continue
        out = {"xy": xy, "K": K, "T": T, "cells_per_heading_mean": round(float(cells.mean()), 1)}
        for what, call in calls:
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
            out[what + "_call_us"] = us
            out[what + "_call_us_median"] = _median(us)
        r = by_set()
        summary, att, status = r.copy_to_host()
        r2 = by_ptr()
        out["map_set_equals_pointer"] = bool(all(np.array_equal(a, b, equal_nan=True) for a, b in zip((summary, att, status), r2.copy_to_host())))
        r2.release()
        out["pose_status_counts"] = np.bincount(status.ravel(), minlength=7).tolist()
        out["rollout_status_counts"] = np.bincount(summary[:, 0], minlength=7).tolist()
        # the torch form on the exported maps (zero-copy), its statuses compared first, then timed
        tv, ts = _torch_score(torch, gflat, tp, offs_pad, live_t, wheels_t, cs_t, ch, res, oc, xy)
        tv, ts = tv.cpu().numpy(), ts.cpu().numpy()
        same = ts == status
        with np.errstate(invalid="ignore"):
            diff = np.abs(tv.astype(np.float64) - att.astype(np.float64))
            diff[~np.isfinite(diff)] = 0.0
            diff[(tv == att)] = 0.0
        torch.cuda.synchronize()
        tus = []
        for rep in range(5):
            t0 = time.perf_counter()
            _torch_score(torch, gflat, tp, offs_pad, live_t, wheels_t, cs_t, ch, res, oc, xy)
            torch.cuda.synchronize()
            tus.append(round((time.perf_counter() - t0) * 1e6, 1))
        out["torch"] = {"statuses_equal": bool(same.all()), "statuses_that_differ": int((~same).sum()),
                        "largest_value_difference_where_statuses_agree": float(diff[same].max()) if same.any() else None,
                        "us": tus, "us_median": _median(tus), "chunk_rollouts": CHUNK, "padded_cells_per_pose": mmax}
        r.release()
        results.append(out)
    return {"calls": reps, "order": ["attitude_map_set", "attitude_pointer", "rollouts"]} if profiled else {"scoring": results}


def child_step(name, steps, score):
    np, torch, gvom, g, dev = _setup(name)
    K, T = SHAPES[0]
    res = g.xy_resolution
    if score:
        _vehicle(gvom, g)
    tp = [torch.from_numpy(_poses(np, K, T, ego, res)).cuda() for _, ego, _ in dev]
    torch.cuda.synchronize()

    def step(k):
        t, ego, tf = dev[k % 3]
        g.process_pointcloud_device(t.data_ptr(), t.shape[0], np.float32, ego, tf)
        m = g.combine_maps_device()
        if score:
            g._score_attitude(m.set_id, None, gvom._dev(tp[k % 3].data_ptr()), K, T, 1, True, m.origin).release()
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
    """the dispatches of a profiled run in launch order: per shape and call the kernels' times without the first three launches"""
    rows = {"k_attitude_ground": [], "k_attitude": [], "k_rollouts": []}
    for f in glob.glob(os.path.join(profile_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            key = "k_attitude_ground" if "k_attitude_ground" in name else ("k_attitude" if "k_attitude" in name else ("k_rollouts" if "k_rollouts" in name else None))
            if key:
                rows[key].append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))

    def stats(us):
        us = us[3:]
        return {"launches": len(us), "median_us": round(_median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}
    for v in rows.values():
        v.sort()
    out = []
    att, gnd, ro = ([u for _, u in rows[k]] for k in ("k_attitude", "k_attitude_ground", "k_rollouts"))
    if len(att) != 2 * calls * len(SHAPES) or len(gnd) != calls * len(SHAPES) or len(ro) != calls * len(SHAPES):
        return None
    for n in range(len(SHAPES)):
        out.append({"k_attitude (map set route)": stats(att[2 * n * calls:(2 * n + 1) * calls]), "k_attitude_ground": stats(gnd[n * calls:(n + 1) * calls]),
                    "k_attitude (pointer route)": stats(att[(2 * n + 1) * calls:(2 * n + 2) * calls]), "k_rollouts": stats(ro[n * calls:(n + 1) * calls])})
    return out


def resources(new, parent):
    """the new unit's kernels, and every other kernel on the parent and on this library: registers, scratch, LDS, code size"""
    import kernel_regs
    mine = kernel_regs.kernels(new)
    out = {"new_kernels": {k: v for k, v in mine.items() if "k_attitude" in k}}
    if parent:
        theirs = kernel_regs.kernels(parent)
        rest = {k: v for k, v in mine.items() if "k_attitude" not in k}
        keys = ("vgpr", "sgpr", "scratch", "lds", "code")
        changed = {k: {"parent": theirs.get(k), "new": v} for k, v in rest.items() if any((theirs.get(k) or {}).get(q) != v.get(q) for q in keys)}
        gone = sorted(k for k in theirs if k not in mine)
        out["other_kernels"] = {"count": len(rest), "identical_to_parent": len(rest) - len(changed), "changed": changed, "only_on_parent": gone,
                                "table": {k: {"parent": {q: (theirs.get(k) or {}).get(q) for q in keys}, "new": {q: v.get(q) for q in keys}} for k, v in sorted(rest.items())}}
    return out


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        mode, a = sys.argv[2], sys.argv[3:]
        res = child_score(a[0], a[1] == "1") if mode == "score" else child_step(a[0], int(a[1]), a[2] == "1")
        print("RESULT " + json.dumps(res))
        return
    import lib_identity
    args = sys.argv[1:]
    parent, only_resources = None, False
    while args and args[0] in ("--parent", "--resources"):
        if args[0] == "--parent":
            parent, args = args[1], args[2:]
        else:
            only_resources, args = True, args[1:]
    new = os.path.join(ROOT, "g-vom_amd", "lib", "libgvom_hip.so")
    path = args[0] if args else os.path.join(ROOT, "profiles", "attitude_%s.json" % (lib_identity.identity().get("lib_sha256") or "unknown")[:8])
    out = json.load(open(path)) if os.path.exists(path) else {}
    out.update({"library": lib_identity.identity(), "footprint_metres": CAR, "chassis": CHASSIS, "headings": HEADINGS})
    out["resources"] = resources(new, parent)
    if parent:
        out["parent_library"] = {"lib_sha256": lib_identity.sha256_file(parent)}
    out.setdefault("not_measured", ["footprints and chassis of other sizes", "maps larger than c4's 512 x 512", "shuffled poses",
                                    "static instead of dynamic LDS in k_attitude", "a summary made by a second kernel"])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)

    def save():
        with open(path, "w") as f:                                  # (after every part: a run that ends early leaves what it has)
            f.write(json.dumps(out, indent=1) + "\n")
    save()
    if only_resources:
        out.setdefault("configs", "not measured")
        save()
        return
    out["configs"] = {}
    for name, steps in CONFIGS:
        res = _spawn("score", (name, 0))
        with tempfile.TemporaryDirectory() as d:
            prof = _spawn("score", (name, 1), profile_dir=d)
            kernel = _kernel_times(d, prof["calls"])
        for k, rec in enumerate(res["scoring"]):
            rec["kernels"] = kernel[k] if kernel else "not measured (the trace did not hold the expected launches)"
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
        step["query_adds_us_per_step"] = round(step["with"]["median"] - step["without"]["median"], 2)
        if parent:
            p = step["parent_without"]
            step["without_inside_parents_own_spread"] = bool(p["min"] <= step["without"]["median"] <= p["max"])
            step["without_minus_parent_median_us"] = round(step["without"]["median"] - p["median"], 2)
        res["step: scan + combine_maps_device (+ score_attitude %d x %d)" % SHAPES[0]] = step
        save()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
