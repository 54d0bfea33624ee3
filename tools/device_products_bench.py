#!/usr/bin/env python3
"""What the device-resident 3-D products cost, and what the occupancy grid's host route gained.  Parent library (the commit
before the products; pass its libgvom_hip.so) and this tree's library, on the same machine in the same session, every loop in a
fresh child process, the two libraries alternating (parent, new, parent, new):

  occupancy_host   Gvom.get_map_as_occupancy_grid() wall time on m256 and c4 (median of the repetitions after a warm-up)
  step             m256, scan + combine_maps_device() per step, NO product call: the feature must cost nothing when unused; the
                   margin is the parent's own run-to-run spread over its repetitions of this session
  step_occupancy   the same + occupancy_grid_device() per step (new library only)
  kernels          one `rocprofv3 --kernel-trace --stats` run per config (new library only): k_occupancy in both forms of the
                   dead-column handling ("occupancy_clear" 0 / 1, the second with its fill kernel), k_read_dense on the same map;
                   bytes moved (tile tags + live state rows + V output bytes) and the bandwidth that makes

    tools/device_products_bench.py PARENT_LIB [out.json]      (default: profiles/device_products_<lib sha8>.json)
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
COPY_CEILING_TBS = 6.29                                   # the project's own device copy ceiling (profiles/)


def _gvom():
    """The binding, also over a library of an OLDER ABI (the parent): it is bound with the entry points it has."""
    import ctypes
    import gvom
    lib = ctypes.CDLL(gvom.library_path())
    lib.gvom_abi_version.restype = ctypes.c_int
    if lib.gvom_abi_version() != gvom.ABI_VERSION:
        gvom.ABI = [e for e in gvom.ABI if hasattr(lib, e[0])]
        gvom.ABI_VERSION = lib.gvom_abi_version()
    return gvom


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def child_occupancy_host():
    import synth
    gvom = _gvom()
    out = {}
    for name, reps in (("m256", 30), ("c4", 12)):
        params, scans = synth.config_inputs(name, n_scans=1)
        g = gvom.Gvom(*params, voxel_statistics=False)
        g.process_pointcloud(*scans[0])
        g.combine_maps()
        for _ in range(3):
            grid = g.get_map_as_occupancy_grid()
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            grid = g.get_map_as_occupancy_grid()
            ms.append((time.perf_counter() - t0) * 1e3)
        out[name] = {"ms_median": round(_median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "reps": reps,
                     "voxels": int(grid.size), "occupied": int(grid.sum())}
        del g
    return out


def child_step(with_occupancy):
    import numpy as np
    import torch
    import synth
    torch.cuda.init()
    gvom = _gvom()
    steps, poses = 1500, 8
    params, scans = synth.config_inputs("m256", n_scans=poses)
    dev = [(torch.from_numpy(np.ascontiguousarray(pc)).cuda(), ego, tf) for pc, ego, tf in scans]
    torch.cuda.synchronize()
    g = gvom.Gvom(*params, voxel_statistics=False)

    def step(k):
        t, ego, tf = dev[k % poses]
        g.process_pointcloud_device(t.data_ptr(), t.shape[0], np.float32, ego, tf)
        g.combine_maps_device().release()
        if with_occupancy:
            g.occupancy_grid_device().release()

    for k in range(100):
        step(k)
    g._check(g._lib.gvom_sync(g._h))
    us = []
    for rep in range(5):
        t0 = time.perf_counter()
        for k in range(steps):
            step(k)
        g._check(g._lib.gvom_sync(g._h))
        us.append(round((time.perf_counter() - t0) / steps * 1e6, 2))
    return {"us_per_step": us, "us_per_step_median": _median(us), "steps": steps}


def child_kernels(name):
    """Run under rocprofv3: the calls whose kernels are to be timed."""
    import numpy as np
    import synth
    gvom = _gvom()
    params, scans = synth.config_inputs(name, n_scans=1)
    g = gvom.Gvom(*params, voxel_statistics=False)
    g.process_pointcloud(*scans[0])
    g.combine_maps()
    for clear in (0, 1):
        g.set_tuning("occupancy_clear", clear)
        for _ in range(40):
            g.occupancy_grid_device().release()
        g._check(g._lib.gvom_sync(g._h))
    g.set_tuning("occupancy_clear", 0)
    for _ in range(3):
        state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
    # live tiles (an estimate from the dense state: a tile = 64 consecutive STORAGE x of one (y, z); dead tiles read as -1)
    xy, zs = g.xy_size, g.z_size
    seen = (state != -1).reshape(zs, xy, xy)                       # [z][y][x], window order
    seen = np.roll(seen, int(origin[0]) % xy, axis=2)              # window x -> storage x
    nseg = (xy + 63) // 64
    pad = np.zeros((zs, xy, nseg * 64), bool)
    pad[:, :, :xy] = seen
    live = int(pad.reshape(zs, xy, nseg, 64).any(axis=3).sum())
    return {"voxels": xy * xy * zs, "tiles": xy * zs * nseg, "live_tiles_estimate": live,
            "bytes_moved": xy * zs * nseg * 4 + live * 256 + xy * xy * zs}


def _spawn(mode, lib, arg=None, profile_dir=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode] + ([arg] if arg else [])
    if profile_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", profile_dir, "--"] + cmd
    env = dict(os.environ, GVOM_HIP_LIBRARY=os.path.abspath(lib))
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit("%s on %s failed (%d):\n%s" % (mode, lib, r.returncode, r.stderr[-3000:]))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def _kernel_stats(profile_dir):
    rows = {}
    for f in glob.glob(os.path.join(profile_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            rows[r["Name"]] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                               "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
    return rows


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        mode = sys.argv[2]
        res = {"occupancy_host": child_occupancy_host, "step": lambda: child_step(False), "step_occupancy": lambda: child_step(True),
               "kernels": lambda: child_kernels(sys.argv[3])}[mode]()
        print("RESULT " + json.dumps(res))
        return
    import lib_identity
    parent = sys.argv[1]
    new = os.path.join(ROOT, "g-vom_amd", "lib", "libgvom_hip.so")
    out = {"library": lib_identity.identity(), "parent_library": {"lib_sha256": lib_identity.sha256_file(parent)},
           "copy_ceiling_TBps": COPY_CEILING_TBS}
    runs = {"parent": [], "new": []}
    for rnd in range(2):                                           # parent, new, parent, new
        for who, lib in (("parent", parent), ("new", new)):
            runs[who].append(_spawn("step", lib))
    p = [u for r in runs["parent"] for u in r["us_per_step"]]
    n = [u for r in runs["new"] for u in r["us_per_step"]]
    out["step m256 scan+combine_maps_device"] = {
        "parent_us_per_step": p, "new_us_per_step": n, "parent_median": _median(p), "new_median": _median(n),
        "parent_spread_us": round(max(p) - min(p), 2), "new_minus_parent_us": round(_median(n) - _median(p), 2),
        "within_parent_spread": _median(n) - _median(p) <= max(p) - min(p)}
    out["step m256 scan+combine_maps_device+occupancy_grid_device"] = _spawn("step_occupancy", new)
    occ = {who: _spawn("occupancy_host", lib) for who, lib in (("parent", parent), ("new", new))}
    out["get_map_as_occupancy_grid wall"] = {
        cfg: {"parent_ms_median": occ["parent"][cfg]["ms_median"], "new_ms_median": occ["new"][cfg]["ms_median"],
              "speedup": round(occ["parent"][cfg]["ms_median"] / occ["new"][cfg]["ms_median"], 2),
              "parent": occ["parent"][cfg], "new": occ["new"][cfg]} for cfg in ("m256", "c4")}
    out["kernels"] = {}
    for cfg in ("m256", "c4"):
        with tempfile.TemporaryDirectory() as d:
            info = _spawn("kernels", new, cfg, profile_dir=d)
            stats = _kernel_stats(d)
        pick = {k.split("(")[0]: v for k, v in stats.items() if "k_occupancy" in k or "k_read_dense" in k or "fill" in k.lower()}
        for k, v in pick.items():
            if "k_occupancy" in k:
                v["TBps_of_bytes_moved"] = round(info["bytes_moved"] / (v["avg_us"] * 1e-6) / 1e12, 3)
        out["kernels"][cfg] = dict(info, kernel_us=pick)
    text = json.dumps(out, indent=1)
    print(text)
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(
        ROOT, "profiles", "device_products_%s.json" % (out["library"].get("lib_sha256") or "unknown")[:8])
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
