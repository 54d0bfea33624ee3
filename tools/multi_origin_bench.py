#!/usr/bin/env python3
"""What multi-origin scans cost, and that the single-origin scan pays nothing for them.  m256 (256^3 voxels, 131,072 returns, 8
moving poses), device-resident cloud, scan + combine_maps() (= gvom_combine_maps_into) per step, stage profiling on in every line, the bench's warm-up and step counts; every line in a
fresh child process:

  a  the PARENT commit's library (pass its libgvom_hip.so), process_pointcloud_device -- three runs: their spread is the margin
  b  this tree's library, the same call -- three runs, alternating with a's; must not be slower than a by more than a's spread
  c  process_pointcloud_origins_device, K = 1, origins = [ego]
  d  K = 4 contiguous groups, sensors 1 m apart
  e  K = 1024, index = None (i % K), origins along 1.5 m of travel
  f  process_range_image_origins_device next to the plain range-image call (64 x 2048 pixels, uint32)
  + k_trace's stage time (last_stage_ms) for each, and one `rocprofv3 --kernel-trace --stats` run of d and e (kernel times of
  the per-lane-origin instantiation next to the single-origin one's)

    tools/multi_origin_bench.py PARENT_LIB [out.json] [--regs FILE]   (default: profiles/multi_origin_<lib sha8>.json; FILE: the
                                                                       register comparison of tools/kernel_regs.py, copied in)
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
WARMUP, STEPS, POSES = 20, 200, 8                          # bench.py's defaults


def _gvom():
    """The binding, also over the parent's library: it is bound with the entry points it has."""
    import ctypes
    import gvom
    lib = ctypes.CDLL(gvom.library_path())
    gvom.ABI = [e for e in gvom.ABI if hasattr(lib, e[0])]
    return gvom


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def child(mode, steps=STEPS):
    import numpy as np
    import torch
    import synth
    torch.cuda.init()
    gvom = _gvom()
    params, scans = synth.config_inputs("m256", n_scans=POSES)
    g = gvom.Gvom(*params, voxel_statistics=False)
    n = scans[0][0].shape[0]
    dev = [(torch.from_numpy(np.ascontiguousarray(pc)).cuda(), ego, tf) for pc, ego, tf in scans]
    idx4 = torch.from_numpy((np.arange(n) * 4 // n).astype(np.int16)).cuda()
    images = None
    if mode in ("f", "f_plain"):
        scene = synth.make_scene(2)
        images = []
        for k in range(POSES):
            sensor = (0.2 * k, 0.0, 0.0)
            raw, dirs, offs = synth.range_image_scan(scene, 64, 2048, sensor, 0.0, k, np.uint32)
            if k == 0:
                g.set_sensor_model(dirs, offs, 0.001)
            cols = np.tile(np.eye(4), (2048, 1, 1))
            cols[:, 0, 3] = 1.5 * np.arange(2048) / 2048
            images.append((torch.from_numpy(raw.view(np.int32)).cuda(), sensor, synth.sensor_transform(sensor), cols))
    torch.cuda.synchronize()

    def scan(k):
        t, ego, tf = dev[k % POSES]
        e = np.asarray(ego, np.float64)
        if mode in ("a", "b"):
            g.process_pointcloud_device(t.data_ptr(), n, np.float32, ego, tf)
        elif mode == "c":
            g.process_pointcloud_origins_device(t.data_ptr(), n, np.float32, [ego], ego, tf)
        elif mode == "d":
            o = e + np.array([[0.5, 0.5, 0.0], [0.5, -0.5, 0.0], [-0.5, 0.5, 0.0], [-0.5, -0.5, 0.0]])
            g.process_pointcloud_origins_device(t.data_ptr(), n, np.float32, o, ego, tf, idx4.data_ptr())
        elif mode == "e":
            o = e + np.stack([1.5 * np.arange(1024) / 1024, np.zeros(1024), np.zeros(1024)], axis=-1)
            g.process_pointcloud_origins_device(t.data_ptr(), n, np.float32, o, ego, tf)
        else:
            im, sensor, tf2, cols = images[k % POSES]
            call = g.process_range_image_origins_device if mode == "f" else g.process_range_image_device
            call(im.data_ptr(), np.uint32, sensor, tf2, cols)

    def step(k):
        scan(k)
        g.combine_maps()

    g.set_profiling(True)
    for k in range(WARMUP):
        step(k)
    g._check(g._lib.gvom_sync(g._h))
    trace_ms = []
    t0 = time.perf_counter()
    for k in range(steps):
        step(k)
        if k % 8 == 0:
            trace_ms.append(float(g.last_stage_ms()["trace"]))
    g._check(g._lib.gvom_sync(g._h))
    us = (time.perf_counter() - t0) / steps * 1e6
    return {"us_per_step": round(us, 2), "k_trace_stage_us_median": round(_median(trace_ms) * 1e3, 2), "steps": steps,
            "knobs": {nm: g.get_tuning(nm) for nm in ("segs", "period", "interleave", "dirsort")}}


def _spawn(mode, lib, profile_dir=None, steps=STEPS):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, str(steps)]
    if profile_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", profile_dir, "--"] + cmd
    env = dict(os.environ, GVOM_HIP_LIBRARY=os.path.abspath(lib))
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("%s on %s failed (%d):\n%s" % (mode, lib, r.returncode, r.stderr[-3000:]))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def _kernel_stats(profile_dir):
    rows = {}
    for f in glob.glob(os.path.join(profile_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            rows[r["Name"].split("(")[0]] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                                             "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
    return rows


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        print("RESULT " + json.dumps(child(sys.argv[2], int(sys.argv[3]))))
        return
    import lib_identity
    args = [a for a in sys.argv[1:]]
    regs = None
    if "--regs" in args:
        i = args.index("--regs")
        regs = json.load(open(args[i + 1]))
        del args[i:i + 2]
    parent = args[0]
    new = os.path.join(ROOT, "g-vom_amd", "lib", "libgvom_hip.so")
    out = {"library": lib_identity.identity(), "parent_library": {"lib_sha256": lib_identity.sha256_file(parent)},
           "workload": "m256: 256^3 voxels, 131,072 returns, %d moving poses, device-resident cloud, scan + combine_maps, warm-up %d, %d steps"
                       % (POSES, WARMUP, STEPS)}
    runs = {"a": [], "b": []}
    for _ in range(3):                                             # a, b, a, b, a, b
        runs["a"].append(_spawn("a", parent))
        runs["b"].append(_spawn("b", new))
    a = [r["us_per_step"] for r in runs["a"]]
    b = [r["us_per_step"] for r in runs["b"]]
    out["a parent library, process_pointcloud_device"] = {"us_per_step": a, "k_trace_stage_us": [r["k_trace_stage_us_median"] for r in runs["a"]]}
    out["b this library, process_pointcloud_device"] = {"us_per_step": b, "k_trace_stage_us": [r["k_trace_stage_us_median"] for r in runs["b"]]}
    out["b against a"] = {"a_median": _median(a), "b_median": _median(b), "a_spread_us": round(max(a) - min(a), 2),
                          "b_minus_a_us": round(_median(b) - _median(a), 2),
                          "within_a_spread": _median(b) - _median(a) <= max(a) - min(a)}
    for mode, what in (("c", "c origins K=1 at the ego"), ("d", "d origins K=4 contiguous groups, sensors 1 m apart"),
                       ("e", "e origins K=1024, index=None, 1.5 m of travel"),
                       ("f_plain", "f (plain) process_range_image_device, column poses, traced from the ego"),
                       ("f", "f process_range_image_origins_device")):
        out[what] = _spawn(mode, new)
    out["kernels (rocprofv3 --kernel-trace --stats, 60 steps each)"] = {}
    for mode in ("b", "d", "e"):
        with tempfile.TemporaryDirectory() as d:
            _spawn(mode, new, profile_dir=d, steps=60)
            stats = _kernel_stats(d)
        out["kernels (rocprofv3 --kernel-trace --stats, 60 steps each)"][mode] = {
            k: v for k, v in stats.items() if "k_trace" in k or "k_encfuse" in k or "k_map2d" in k}
    if regs is not None:
        out["k_trace registers, parent against this tree (--save-temps)"] = regs
    text = json.dumps(out, indent=1)
    print(text)
    path = args[1] if len(args) > 1 else os.path.join(
        ROOT, "profiles", "multi_origin_%s.json" % (out["library"].get("lib_sha256") or "unknown")[:8])
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
