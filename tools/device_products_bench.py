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

    tools/device_products_bench.py PARENT_LIB [--turns N] [out.json]      (default: profiles/device_products_<lib sha8>.json)
"""
import json
import sys
import tempfile
import time

import benchkit as bk

COPY_CEILING_TBS = 6.29                                   # the project's own device copy ceiling (profiles/)
TURNS = 2
CHILD_TIMEOUT = 900                                       # seconds, per child process


def _older_abi(gvom, lib):
    """a library of an OLDER ABI (the parent): the binding takes its version for its own"""
    import ctypes
    lib.gvom_abi_version.restype = ctypes.c_int
    gvom.ABI_VERSION = lib.gvom_abi_version()


def _binding():
    return bk.gvom_for_library(adapt=_older_abi)


def child_occupancy_host():
    import synth
    gvom = _binding()
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
        out[name] = {"ms_median": round(bk.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "reps": reps,
                     "voxels": int(grid.size), "occupied": int(grid.sum())}
        del g
    return out


def child_step(with_occupancy):
    steps, poses = 1500, 8
    np, torch, gvom, g, dev = bk.setup("m256", poses, adapt=_older_abi)

    def step(k):
        bk.scan_combine(np, g, dev[k % poses]).release()
        if with_occupancy:
            g.occupancy_grid_device().release()
    return bk.step_loop(g, step, steps, warm=100, reps=5)


def child_kernels(name):
    """Run under rocprofv3: the calls whose kernels are to be timed."""
    import numpy as np
    import synth
    gvom = _binding()
    params, scans = synth.config_inputs(name, n_scans=1)
    g = gvom.Gvom(*params, voxel_statistics=False)
    g.process_pointcloud(*scans[0])
    g.combine_maps()
    for clear in (0, 1):
        g.set_tuning("occupancy_clear", clear)
        for _ in range(40):
            g.occupancy_grid_device().release()
        bk.sync(g)
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


def main():
    if bk.child(sys.argv[1:], {"occupancy_host": lambda a: child_occupancy_host(), "step": lambda a: child_step(False),
                               "step_occupancy": lambda a: child_step(True), "kernels": lambda a: child_kernels(a[0])}):
        return
    args = bk.read_args(sys.argv[1:], positional_parent=True, has_resources=False, turns=TURNS)
    parent, new = args["parent"], bk.NEW_LIB
    spawn = lambda mode, lib, a=(), **kw: bk.spawn(__file__, mode, a, CHILD_TIMEOUT, lib=lib, **kw)
    report = bk.Report("device_products", args["path"], parent, fresh=True)
    out = report.out
    out["copy_ceiling_TBps"] = COPY_CEILING_TBS
    runs = bk.alternate(args["turns"], {"parent": lambda: spawn("step", parent), "new": lambda: spawn("step", new)})
    p, n = bk.pooled(runs["parent"]), bk.pooled(runs["new"])
    out["step m256 scan+combine_maps_device"] = {
        "parent_us_per_step": p["us_per_step"], "new_us_per_step": n["us_per_step"], "parent_median": p["median"], "new_median": n["median"],
        "parent_spread_us": p["spread_us"], "new_minus_parent_us": round(n["median"] - p["median"], 2),
        "within_parent_spread": n["median"] - p["median"] <= p["spread_us"]}
    out["step m256 scan+combine_maps_device+occupancy_grid_device"] = spawn("step_occupancy", new)
    occ = {who: spawn("occupancy_host", lib) for who, lib in (("parent", parent), ("new", new))}
    out["get_map_as_occupancy_grid wall"] = {
        cfg: {"parent_ms_median": occ["parent"][cfg]["ms_median"], "new_ms_median": occ["new"][cfg]["ms_median"],
              "speedup": round(occ["parent"][cfg]["ms_median"] / occ["new"][cfg]["ms_median"], 2),
              "parent": occ["parent"][cfg], "new": occ["new"][cfg]} for cfg in ("m256", "c4")}
    out["kernels"] = {}
    for cfg in ("m256", "c4"):
        with tempfile.TemporaryDirectory() as d:
            info = spawn("kernels", new, (cfg,), profile_dir=d, stats=True)
            stats = bk.kernel_stats(d)
        pick = {k: v for k, v in stats.items() if "k_occupancy" in k or "k_read_dense" in k or "fill" in k.lower()}
        for k, v in pick.items():
            if "k_occupancy" in k:
                v["TBps_of_bytes_moved"] = round(info["bytes_moved"] / (v["avg_us"] * 1e-6) / 1e12, 3)
        out["kernels"][cfg] = dict(info, kernel_us=pick)
    print(json.dumps(out, indent=1))
    report.save()


if __name__ == "__main__":
    main()
