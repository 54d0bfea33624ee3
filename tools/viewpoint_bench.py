#!/usr/bin/env python3
"""What viewpoint scoring (gvom_score_viewpoints: k_viewpoints, k_viewpoint_best) costs.  On the fused maps of m256 and c4 after three
bench scans, a 64 x 1024 sensor model (beams between -40 and +40 degrees), K = 64 and 512 poses on a grid around the last ego, beam
strides (1, 1) and (2, 4), max_range 20 m -- every loop in a fresh child process, every child under a `timeout` of its own, and the
first child that fails ends the run:

  call       Gvom.score_viewpoints_device(), enqueue to completion: wall time, what it found, viewpoints per launch
  kernel     one `rocprofv3 --kernel-trace` run per config: k_viewpoints and k_viewpoint_best per call, and the fills that clear the
             bitmaps and the rows as a share of the device time of a call
  parts      the same answer from what the library had before (K = 64 only): the K x nb targets built on the host, uploaded, K
             raycast_device() calls, the `unknown` column summed and the statuses counted in torch -- visits and columns 3 .. 7, first
             shown equal to the product.  (The gain has no such form: k_raycast does not say which voxels it passed.)
  walk       the walk alone (K = 64): ONE raycast_device() call over the same K x nb segments, already uploaded -- k_raycast has the
             same step body and no atomics, so the difference to the call is what the bitmaps cost
  step       scan + combine_maps_device() per step, without and with a query (K = 64, strides (2, 4)); and, with --parent LIB (the
             parent commit's libgvom_hip.so), the same step without on that library, alternating, five runs each
  resources  tools/kernel_regs.py: the new kernels, and registers, scratch, LDS and code size of every kernel outside the new
             unit on the parent and on this library (--resources alone: no GPU needed)

    tools/viewpoint_bench.py [--resources] [--parent LIB] [--configs m256,c4] [out.json]   (default: profiles/viewpoints_<lib sha8>.json)
"""
import csv
import glob
import json
import math
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "g-vom_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CONFIGS = {"m256": 100, "c4": 40}                         # config: timed steps per repetition
MODEL = (64, 1024)
SHAPES = ((64, (1, 1)), (64, (2, 4)), (512, (1, 1)), (512, (2, 4)))      # (K, beam strides)
MAX_RANGE = 20.0
CHILD_TIMEOUT = 300                                       # seconds, per child process
KERNELS = ("k_viewpoints", "k_viewpoint_best", "fillBuffer")


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


def _model(np):
    H, W = MODEL
    el = np.radians(np.linspace(-40.0, 40.0, H))[:, None]
    az = (np.arange(W) * (2.0 * math.pi / W))[None, :]
    return np.ascontiguousarray(np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) * np.ones_like(az)], axis=2))


def _poses(np, gvom, ego, K):
    """K poses on a square grid of 1.25 m pitch around the ego, at its height, each under another yaw"""
    n = int(math.ceil(math.sqrt(K)))
    pts = [(ego[0] + 1.25 * (i - n / 2.0), ego[1] + 1.25 * (j - n / 2.0), ego[2] + 0.5) for j in range(n) for i in range(n)][:K]
    return np.ascontiguousarray(np.stack([gvom.viewpoint_poses([p], [0.37 * k])[0] for k, p in enumerate(pts)])[:, :3, :])


def _setup(name, with_model=True):
    import numpy as np
    import torch
    import synth
    torch.cuda.init()
    gvom = _gvom()
    params, scans = synth.config_inputs(name, n_scans=3)
    dev = [(torch.from_numpy(np.ascontiguousarray(pc)).cuda(), ego, tf) for pc, ego, tf in scans]
    torch.cuda.synchronize()
    g = gvom.Gvom(*params, voxel_statistics=False)
    if with_model:
        g.set_sensor_model(_model(np))
    return np, torch, gvom, g, dev


def _targets(np, d, pose, r, strides):
    """the definition's targets (include/gvom_hip.h "viewpoint scoring"): float32 a [3], b [nb, 3]"""
    d = d[::strides[0], ::strides[1]].reshape(-1, 3)
    C = pose.reshape(12)
    p = np.float64(r) * d
    q = np.empty_like(p)
    for c in range(3):
        q[:, c] = ((p[:, 0] * C[4 * c] + p[:, 1] * C[4 * c + 1]) + p[:, 2] * C[4 * c + 2]) + C[4 * c + 3]
    return C[[3, 7, 11]].astype(np.float32), q.astype(np.float32)


def child_call(name, profiled):
    np, torch, gvom, g, dev = _setup(name)
    for t, ego, tf in dev:
        g.process_pointcloud_device(t.data_ptr(), t.shape[0], np.float32, ego, tf)
        g.combine_maps_device().release()
    ego = dev[2][1]
    reps, results = 20, {}
    for K, strides in SHAPES:
        poses = _poses(np, gvom, ego, K)
        tp = torch.from_numpy(poses).cuda()
        torch.cuda.synchronize()
        call = lambda: g.score_viewpoints_device(tp.data_ptr(), K, MAX_RANGE, beam_stride=strides)
        key = "K%d_stride%dx%d" % (K, strides[0], strides[1])
        if profiled:
            for _ in range(reps):
                call().release()
            g._check(g._lib.gvom_sync(g._h))
            continue
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
        v = call()
        rows, best = v.copy_to_host()
        v.release()
        nb = int(best[3])
        out = {"xy": g.xy_size, "z": g.z_size, "K": K, "beams_per_viewpoint": nb, "call_us": us, "call_us_median": _median(us),
               "viewpoints_per_launch": g.get_tuning("viewpoint_batch"), "best": best.tolist(), "gain_sum": int(rows[:, 1].sum()),
               "visits_sum": int(rows[:, 2].sum()), "visits_over_gain": round(float(rows[:, 2].sum()) / max(int(rows[:, 1].sum()), 1), 2),
               "beam_endings": rows[:, 3:].sum(axis=0).tolist(), "origin_statuses": np.bincount(rows[:, 0], minlength=5).tolist()}
        out["ns_per_beam"] = round(out["call_us_median"] * 1e3 / (K * nb), 3)
        if K == 64:                                                # the same from K raycast_device() calls on uploaded targets
            d = _model(np)

            def from_parts(timed):
                t0 = time.perf_counter()
                ab = [_targets(np, d, p, MAX_RANGE, strides) for p in poses]
                t1 = time.perf_counter()
                ta = [(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()) for a, b in ab]
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                got = torch.zeros((K, 6), dtype=torch.int64, device="cuda")
                for k, (a, b) in enumerate(ta):
                    with g.raycast_device(a.data_ptr(), 1, b.data_ptr(), b.shape[0]) as rays:
                        res = torch.from_dlpack(rays.result)
                        got[k, 0] = res[:, 3].sum()
                        got[k, 1:] = torch.bincount(res[:, 0], minlength=5)[torch.tensor([1, 0, 3, 2, 4], device="cuda")]
                        del res
                got = got.cpu().numpy()
                t3 = time.perf_counter()
                return got, [round((t1 - t0) * 1e6, 1), round((t2 - t1) * 1e6, 1), round((t3 - t2) * 1e6, 1)]
            got, _ = from_parts(False)
            ts = [from_parts(True)[1] for _ in range(3)]
            # the walk alone: ONE raycast_device() call over all K x nb segments, already uploaded (k_raycast: no atomics, its targets
            # and origins read from HBM) -- what of k_viewpoints' time the walk is, and what the bitmap is
            ab = [_targets(np, d, p, MAX_RANGE, strides) for p in poses]
            A = torch.from_numpy(np.ascontiguousarray(np.concatenate([np.repeat(a[None], len(b), axis=0) for a, b in ab]))).cuda()
            B = torch.from_numpy(np.ascontiguousarray(np.concatenate([b for _, b in ab]))).cuda()
            torch.cuda.synchronize()
            one = lambda: g.raycast_device(A.data_ptr(), A.shape[0], B.data_ptr(), B.shape[0])
            for _ in range(3):
                one().release()
            g._check(g._lib.gvom_sync(g._h))
            ws = []
            for rep in range(5):
                t0 = time.perf_counter()
                for _ in range(10):
                    one().release()
                g._check(g._lib.gvom_sync(g._h))
                ws.append(round((time.perf_counter() - t0) / 10 * 1e6, 2))
            with one() as rays:
                walk_visits = int(rays.result.copy_to_host()[:, 3].astype(np.int64).sum())
            out["walk_alone_one_raycast_call"] = {"rays": int(A.shape[0]), "call_us": ws, "call_us_median": _median(ws),
                                                  "unknown_sum_equals_visits": bool(walk_visits == int(rows[:, 2].sum()))}
            del A, B
            out["from_existing_parts"] = {"covers": "visits and the beam endings; the gain has no such form",
                                          "equal_to_the_product": bool(np.array_equal(got, rows[:, 2:].astype(np.int64))),
                                          "us_build_targets_on_host": [t[0] for t in ts], "us_upload": [t[1] for t in ts],
                                          "us_K_raycast_calls_and_sums": [t[2] for t in ts],
                                          "us_median_total": _median([sum(t) for t in ts]), "uploaded_bytes": K * nb * 12}
        results[key] = out
    return {"calls": reps} if profiled else results


def child_step(name, steps, with_query):
    np, torch, gvom, g, dev = _setup(name, with_model=bool(with_query))
    K, strides = SHAPES[1]
    tp = None

    def step(k):
        t, ego, tf = dev[k % 3]
        g.process_pointcloud_device(t.data_ptr(), t.shape[0], np.float32, ego, tf)
        m = g.combine_maps_device()
        if with_query:
            g.score_viewpoints_device(tp.data_ptr(), K, MAX_RANGE, beam_stride=strides).release()
        m.release()

    if with_query:
        tp = torch.from_numpy(_poses(np, gvom, dev[2][1], K)).cuda()
        torch.cuda.synchronize()
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
    """per shape (k_viewpoint_best ends a call): the kernels' and the fills' microseconds per call, without the first three calls"""
    rows = []
    for f in glob.glob(os.path.join(profile_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            key = [k for k in KERNELS if k in r["Kernel_Name"]]
            if key:
                rows.append((int(r["Start_Timestamp"]), key[0], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    ends = [i for i, r in enumerate(rows) if r[1] == "k_viewpoint_best"]
    if len(ends) != calls * len(SHAPES):
        return None
    out = {}
    for n, (K, strides) in enumerate(SHAPES):
        first = ends[n * calls + 2] + 1                            # behind the third call of the shape
        last = ends[(n + 1) * calls - 1] + 1
        part, used = rows[first:last], calls - 3
        rec = {}
        for k in KERNELS:
            us = [u for _, kk, u in part if kk == k]
            rec[k] = {"launches_per_call": round(len(us) / used, 2), "us_per_call": round(sum(us) / used, 2), "median_us_per_launch": round(_median(us), 2) if us else None}
        total = sum(u for _, _, u in part) / used
        rec["device_us_per_call"] = round(total, 2)
        rec["clears_share_of_device_time"] = round(rec["fillBuffer"]["us_per_call"] / total, 4) if total else None
        out["K%d_stride%dx%d" % (K, strides[0], strides[1])] = rec
    return out


def resources(new, parent):
    """the new unit's kernels, and every other kernel on the parent and on this library: registers, scratch, LDS, code size"""
    import kernel_regs
    mine = kernel_regs.kernels(new)
    out = {"new_kernels": {k: v for k, v in mine.items() if "k_viewpoint" in k}}
    if parent:
        theirs = kernel_regs.kernels(parent)
        rest = {k: v for k, v in mine.items() if "k_viewpoint" not in k}
        keys = ("vgpr", "sgpr", "scratch", "lds", "code")
        changed = {k: {"parent": theirs.get(k), "new": v} for k, v in rest.items() if any((theirs.get(k) or {}).get(q) != v.get(q) for q in keys)}
        out["other_kernels"] = {"count": len(rest), "identical_to_parent": len(rest) - len(changed), "changed": changed,
                                "only_on_parent": sorted(k for k in theirs if k not in mine)}
        out["k_raycast"] = {k: v for k, v in rest.items() if "k_raycast" in k}
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
    path = args[0] if args else os.path.join(ROOT, "profiles", "viewpoints_%s.json" % (lib_identity.identity().get("lib_sha256") or "unknown")[:8])
    out = json.load(open(path)) if os.path.exists(path) else {}
    out.update({"library": lib_identity.identity(), "model": list(MODEL), "max_range_m": MAX_RANGE, "shapes": [[K, list(s)] for K, s in SHAPES]})
    out["resources"] = resources(new, parent)
    if parent:
        out["parent_library"] = {"lib_sha256": lib_identity.sha256_file(parent)}
    out.setdefault("not_measured", ["c5", "RQ_DEPTH other than 4", "per-wave combining of ORs to the same word (not built)",
                                    "non-returning ORs plus a population-count pass over the bitmaps (not built)",
                                    "viewpoint_bitmap_mb other than the default 256", "the gain from existing parts (k_raycast records no voxels)",
                                    "from_existing_parts and the walk alone at K = 512", "the host route", "hardware counters"])
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
        for key in res:
            res[key]["kernels"] = kernel[key] if kernel else "not measured (the trace did not hold the expected launches)"
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
        res["step: scan + combine_maps_device (+ a query of K = 64, strides (2, 4))"] = step
        save()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
