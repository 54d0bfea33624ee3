#!/usr/bin/env python3
"""The device route's share of the m256 step.  Three loops: scan + combine_maps_into (the four maps into pinned host memory,
host wait); scan + combine_maps_device + a torch consumer that reduces one map on a stream of its own (maps stay in HBM, no
host wait in the combine); scan + combine_maps_device alone (the set released at once).  Per loop: us per step and the
stage times of set_profiling (k_map2d's host and device forms under "map2d").  Clouds are device-resident (torch) in every
loop, so the differences are the combine's.

    tools/device_maps_step.py [steps] [out.json]      (default: 2000 steps, profiles/device_maps_step_<lib sha8>.json)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "g-vom_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gvom  # noqa: E402
import lib_identity  # noqa: E402
import synth  # noqa: E402


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    poses = 8
    params, scans = synth.config_inputs("m256", n_scans=poses)
    dev = [(torch.from_numpy(np.ascontiguousarray(pc)).cuda(), ego, tf) for pc, ego, tf in scans]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    acc = torch.zeros((), dtype=torch.float64, device="cuda")

    def scan(g, k):
        t, ego, tf = dev[k % poses]
        g.process_pointcloud_device(t.data_ptr(), t.shape[0], np.float32, ego, tf)

    def host_step(g, k):
        scan(g, k)
        return g.combine_maps()

    def device_step(g, k):
        scan(g, k)
        m = g.combine_maps_device()
        with torch.cuda.stream(side):
            acc.add_(torch.from_dlpack(m.roughness).sum())
        return None                                     # (the DeviceMaps is dropped here: its hold goes back at once)

    def device_only_step(g, k):
        scan(g, k)
        g.combine_maps_device().release()

    out = {"config": "m256", "steps": steps, "library": lib_identity.identity()}

    for name, step in (("combine_maps_into", host_step), ("combine_maps_device+torch", device_step),
                       ("combine_maps_device", device_only_step)):
        g = gvom.Gvom(*params, voxel_statistics=False)
        for k in range(60):                             # first-use allocations
            step(g, k)
        torch.cuda.synchronize()
        best = []
        for rep in range(3):
            t0 = time.perf_counter()
            for k in range(steps):
                step(g, k)
            torch.cuda.synchronize()
            best.append((time.perf_counter() - t0) / steps * 1e6)
        g.set_profiling(True)
        stage = []
        for k in range(40):
            step(g, k)
            stage.append(g.last_stage_ms())
        g.set_profiling(False)
        out[name] = {"us_per_step": [round(v, 2) for v in best], "us_per_step_min": round(min(best), 2),
                     "stage_us_median": {s: round(float(np.median([a[s] for a in stage])) * 1e3, 1) for s in stage[0]},
                     "device_map_sets": g.get_tuning("device_map_sets")}
        del g
    for name in ("combine_maps_device+torch", "combine_maps_device"):
        out["saving_us_per_step " + name] = round(out["combine_maps_into"]["us_per_step_min"] - out[name]["us_per_step_min"], 2)
    text = json.dumps(out, indent=1)
    print(text)
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(
        ROOT, "profiles", "device_maps_step_%s.json" % out["library"].get("lib_sha256", "unknown")[:8])
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
