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

    tools/multi_origin_bench.py PARENT_LIB [out.json] [--regs FILE] [--turns N]   (default: profiles/multi_origin_<lib sha8>.json;
                                                            FILE: the register comparison of tools/kernel_regs.py, copied in)
"""
import json
import sys
import tempfile
import time

import benchkit as bk

WARMUP, STEPS, POSES = 20, 200, 8                          # bench.py's defaults
TURNS = 3
CHILD_TIMEOUT = 600                                        # seconds, per child process


def child(mode, steps=STEPS):
    import synth
    np, torch, gvom, g, dev = bk.setup("m256", POSES)
    n = dev[0][0].shape[0]
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
    bk.sync(g)
    trace_ms = []
    t0 = time.perf_counter()
    for k in range(steps):
        step(k)
        if k % 8 == 0:
            trace_ms.append(float(g.last_stage_ms()["trace"]))
    bk.sync(g)
    us = (time.perf_counter() - t0) / steps * 1e6
    return {"us_per_step": round(us, 2), "k_trace_stage_us_median": round(bk.median(trace_ms) * 1e3, 2), "steps": steps,
            "knobs": {nm: g.get_tuning(nm) for nm in ("segs", "period", "interleave", "dirsort")}}


def main():
    if bk.child(sys.argv[1:], {mode: (lambda a, mode=mode: child(mode, int(a[0]))) for mode in ("a", "b", "c", "d", "e", "f", "f_plain")}):
        return
    args = bk.read_args(sys.argv[1:], positional_parent=True, has_resources=False, turns=TURNS,
                        extra={"--regs": (None, lambda f: json.load(open(f)))})
    parent, new = args["parent"], bk.NEW_LIB
    spawn = lambda mode, lib, steps=STEPS, **kw: bk.spawn(__file__, mode, (steps,), CHILD_TIMEOUT, lib=lib, **kw)
    report = bk.Report("multi_origin", args["path"], parent, fresh=True)
    out = report.out
    out["workload"] = ("m256: 256^3 voxels, 131,072 returns, %d moving poses, device-resident cloud, scan + combine_maps, warm-up %d, %d steps"
                       % (POSES, WARMUP, STEPS))
    runs = bk.alternate(args["turns"], {"a": lambda: spawn("a", parent), "b": lambda: spawn("b", new)})      # a, b, a, b, a, b
    a = [r["us_per_step"] for r in runs["a"]]
    b = [r["us_per_step"] for r in runs["b"]]
    out["a parent library, process_pointcloud_device"] = {"us_per_step": a, "k_trace_stage_us": [r["k_trace_stage_us_median"] for r in runs["a"]]}
    out["b this library, process_pointcloud_device"] = {"us_per_step": b, "k_trace_stage_us": [r["k_trace_stage_us_median"] for r in runs["b"]]}
    out["b against a"] = {"a_median": bk.median(a), "b_median": bk.median(b), "a_spread_us": round(max(a) - min(a), 2),
                          "b_minus_a_us": round(bk.median(b) - bk.median(a), 2),
                          "within_a_spread": bk.median(b) - bk.median(a) <= max(a) - min(a)}
    for mode, what in (("c", "c origins K=1 at the ego"), ("d", "d origins K=4 contiguous groups, sensors 1 m apart"),
                       ("e", "e origins K=1024, index=None, 1.5 m of travel"),
                       ("f_plain", "f (plain) process_range_image_device, column poses, traced from the ego"),
                       ("f", "f process_range_image_origins_device")):
        out[what] = spawn(mode, new)
    kernels = out["kernels (rocprofv3 --kernel-trace --stats, 60 steps each)"] = {}
    for mode in ("b", "d", "e"):
        with tempfile.TemporaryDirectory() as d:
            spawn(mode, new, steps=60, profile_dir=d, stats=True)
            kernels[mode] = bk.kernel_stats(d, ("k_trace", "k_encfuse", "k_map2d"))
    if args["regs"] is not None:
        out["k_trace registers, parent against this tree (--save-temps)"] = args["regs"]
    print(json.dumps(out, indent=1))
    report.save()


if __name__ == "__main__":
    main()
