#!/usr/bin/env python3
"""What range-image ingest costs and what it saves, on m256 (256^3 @0.2 m, 64 x 2048 pixels, 8 moving poses, buffer 1).  Parent
library (the commit before the feature; pass its libgvom_hip.so) and this tree's library on the same machine in the same
session, every loop in a fresh child process, the two libraries alternating (parent, new, parent, new):

  step      scan + combine per step, median of the repetitions, for the cloud routes on BOTH libraries (host float32 cloud = the
            yardstick; device cloud + combine_maps; device cloud + combine_maps_device: the feature unused must cost nothing, the
            margin being the parent's own spread) and for the range-image routes on the new one (host / device, uint16 / uint32,
            with and without column poses).  The images encode the very sweep of the cloud routes (rays without a return at the
            60 m clamp, as in the clouds), so both sides trace the same rays.
  dropout   10 / 25 / 40 % of the returns missing: the parent's host clouds of varying length (synth m256_d*) against the
            fixed-length image of the same sweep with the same pixels zeroed, and what "interleave" / "dirsort" resolve to
  kernels   one `rocprofv3 --kernel-trace --stats` run per pose mode: k_unproject per raw type and cloud type, beside its bytes
            (raw + 48 B/pixel of model + 12 or 24 B/pixel out, + 96 B/column of poses) and the bandwidth that makes

    tools/range_image_bench.py PARENT_LIB [--turns N] [out.json]      (default: profiles/range_image_<lib sha8>.json)
"""
import json
import sys
import tempfile

import benchkit as bk

COPY_CEILING_TBS = 6.29                                   # the project's own device copy ceiling (profiles/)
TURNS = 2
CHILD_TIMEOUT = 600                                       # seconds, per child process
H, W, POSES = 64, 2048, 8
CLOUD_ROUTES = ("cloud_host", "cloud_dev", "cloud_dev_maps_dev")
IMAGE_ROUTES = ("image_host_u16", "image_host_u32", "image_host_u16_poses", "image_host_u32_poses", "image_dev_u16", "image_dev_u32",
                "image_dev_u32_poses")


class _Hbm(object):
    def __init__(self):
        import ctypes
        self.c = ctypes
        self.rt = ctypes.CDLL("libamdhip64.so")
        self.rt.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.rt.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]

    def put(self, a):
        p = self.c.c_void_p()
        assert self.rt.hipMalloc(self.c.byref(p), a.nbytes) == 0
        assert self.rt.hipMemcpy(p, a.ctypes.data_as(self.c.c_void_p), a.nbytes, 1) == 0
        assert self.rt.hipDeviceSynchronize() == 0
        return p.value


def _images(np, synth, scans, rdt):
    """the m256 sweeps as range images: the analytic beam directions of synth.lidar_scan's uniform comb, millimetre ranges"""
    el = np.deg2rad(np.linspace(-22.5, 22.5, H))
    az = 2.0 * np.pi * np.arange(W) / W
    ce, se = np.cos(el)[:, None], np.sin(el)[:, None]
    dirs = np.stack([ce * np.cos(az)[None, :], ce * np.sin(az)[None, :], se * np.ones((1, W))], axis=-1)
    out = []
    for pc, ego, _ in scans:
        ps = pc.astype(np.float64) - np.asarray(ego, np.float64)
        raw = np.rint(np.sqrt((ps * ps).sum(axis=1)) / 0.001).astype(rdt).reshape(H, W)
        out.append((np.ascontiguousarray(raw), ego, synth.sensor_transform(ego)))
    return dirs, out


def _time_steps(g, step, steps):
    return dict(bk.step_loop(g, step, steps, warm=100, reps=5), interleave=g.get_tuning("interleave"), dirsort=g.get_tuning("dirsort"),
                eager_adopted_share=round(g.get_tuning("eager_adopted") / (100.0 + 5 * steps), 3))


def child_step(route):
    import numpy as np
    import synth
    gvom = bk.gvom_for_library()
    params, scans = synth.config_inputs("m256", n_scans=POSES)
    g = gvom.Gvom(*params, voxel_statistics=False)
    hbm = _Hbm()
    if route.startswith("cloud"):
        if route == "cloud_host":
            def step(k):
                g.process_pointcloud(*scans[k % POSES])
                g.combine_maps()
        else:
            dev = [(hbm.put(np.ascontiguousarray(pc)), pc.shape[0], ego, tf) for pc, ego, tf in scans]
            to_dev = route.endswith("maps_dev")

            def step(k):
                d, n, ego, tf = dev[k % POSES]
                g.process_pointcloud_device(d, n, np.float32, ego, tf)
                if to_dev:
                    g.combine_maps_device().release()
                else:
                    g.combine_maps()
    else:
        rdt = np.uint16 if "u16" in route else np.uint32
        dirs, imgs = _images(np, synth, scans, rdt)
        g.set_sensor_model(dirs, None, 0.001)
        cols = None
        if route.endswith("poses"):
            cols = np.tile(np.eye(4)[:3], (W, 1, 1))            # [W, 3, 4] C-contiguous float64: the form the binding passes on as it is
            cols[:, 0, 3] = 0.02 * np.arange(W) / W
        if "host" in route:
            def step(k):
                raw, ego, tf = imgs[k % POSES]
                g.process_range_image(raw, ego, tf, cols)
                g.combine_maps()
        else:
            dev = [(hbm.put(raw), ego, tf) for raw, ego, tf in imgs]

            def step(k):
                d, ego, tf = dev[k % POSES]
                g.process_range_image_device(d, rdt, ego, tf, cols)
                g.combine_maps()
    return _time_steps(g, step, 1000)


def child_dropout(arg):
    """arg = "<pct>_cloud" (host clouds with the returns removed: a different length every scan) or "<pct>_image" """
    import numpy as np
    import synth
    gvom = bk.gvom_for_library()
    pct, kind = arg.split("_")
    name = "m256_d" + pct
    params, scans = synth.config_inputs(name, n_scans=POSES)
    g = gvom.Gvom(*params, voxel_statistics=False)
    if kind == "cloud":
        def step(k):
            g.process_pointcloud(*scans[k % POSES])
            g.combine_maps()
        res = _time_steps(g, step, 1000)
        res["returns"] = [int(s[0].shape[0]) for s in scans]
        return res
    scene, frac, imgs = synth.make_scene(2), int(pct) / 100.0, []
    for k in range(POSES):
        sensor = (0.2 * k, 0.0, 0.0)
        raw, dirs, offs = synth.range_image_scan(scene, H, W, sensor, 0.0, k, np.uint32, clamp_misses=True,
                                                 dropout=frac * (0.9 + 0.2 * ((k * 37) % 11) / 10.0))
        imgs.append((raw, sensor, synth.sensor_transform(sensor)))
    g.set_sensor_model(dirs, offs, 0.001)

    def step(k):
        g.process_range_image(*imgs[k % POSES])
        g.combine_maps()
    res = _time_steps(g, step, 1000)
    res["returns"] = [int((im[0] != 0).sum()) for im in imgs]
    return res


def child_kernels(posed):
    """Run under rocprofv3: 40 scans per raw type and cloud type."""
    import numpy as np
    import synth
    gvom = bk.gvom_for_library()
    params, scans = synth.config_inputs("m256", n_scans=1)
    g = gvom.Gvom(*params, voxel_statistics=False)
    cols = np.tile(np.eye(4), (W, 1, 1)) if posed == "1" else None
    for rdt in (np.uint16, np.uint32, np.float32):
        dirs, imgs = _images(np, synth, scans, np.uint32)
        raw, ego, tf = imgs[0]
        raw = (raw * np.float32(0.001)).astype(np.float32) if rdt == np.float32 else raw.astype(rdt)
        g.set_sensor_model(dirs, None, 1.0 if rdt == np.float32 else 0.001)
        for cdt in (np.float32, np.float64):
            for _ in range(40):
                g.process_range_image(raw, ego, tf, cols, cdt)
                g.combine_maps()
    bk.sync(g)
    return {"pixels": H * W}


def _both(runs):
    return dict(bk.pooled(runs), interleave=runs[-1]["interleave"], dirsort=runs[-1]["dirsort"], eager_adopted_share=runs[-1]["eager_adopted_share"])


def main():
    if bk.child(sys.argv[1:], {"step": lambda a: child_step(a[0]), "dropout": lambda a: child_dropout(a[0]), "kernels": lambda a: child_kernels(a[0])}):
        return
    args = bk.read_args(sys.argv[1:], positional_parent=True, has_resources=False, turns=TURNS)
    parent, new = args["parent"], bk.NEW_LIB
    spawn = lambda mode, lib, arg, **kw: bk.spawn(__file__, mode, (arg,), CHILD_TIMEOUT, lib=lib, **kw)
    report = bk.Report("range_image", args["path"], parent, fresh=True)
    out = report.out
    out.update({"copy_ceiling_TBps": COPY_CEILING_TBS,
                "config": "m256, %d x %d pixels, %d moving poses, buffer 1, scan + combine per step" % (H, W, POSES)})
    jobs = [("parent", parent, "step", r) for r in CLOUD_ROUTES] + [("new", new, "step", r) for r in CLOUD_ROUTES + IMAGE_ROUTES]
    for pct in ("10", "25", "40"):
        jobs += [("parent", parent, "dropout", pct + "_cloud"), ("new", new, "dropout", pct + "_image")]

    def start(who, lib, mode, arg):
        print("%s %s %s" % (who, mode, arg), file=sys.stderr, flush=True)
        return spawn(mode, lib, arg)
    jobs.sort(key=lambda j: (j[2], j[3], j[0] != "parent"))         # the whole list `turns` times: parent and new alternate inside it
    runs = bk.alternate(args["turns"], {(who, mode, arg): (lambda j=(who, lib, mode, arg): start(*j)) for who, lib, mode, arg in jobs})
    res = {k: _both(v) for k, v in runs.items()}
    yard = res[("parent", "step", "cloud_host")]
    out["yardstick parent cloud_host"] = yard
    out["unchanged routes, feature unused"] = {}
    for r in CLOUD_ROUTES:
        p, n = res[("parent", "step", r)], res[("new", "step", r)]
        out["unchanged routes, feature unused"][r] = {"parent": p, "new": n, "new_minus_parent_us": round(n["median"] - p["median"], 2),
                                                      "within_parent_spread": n["median"] - p["median"] <= p["spread_us"]}
    out["range-image routes (new library)"] = {}
    for r in IMAGE_ROUTES:
        n = res[("new", "step", r)]
        out["range-image routes (new library)"][r] = dict(n, minus_yardstick_us=round(n["median"] - yard["median"], 2),
                                                          yardstick_over_this=round(yard["median"] / n["median"], 3),
                                                          not_slower_than_yardstick_by_more_than_its_spread=n["median"] - yard["median"] <= yard["spread_us"])
    out["dropout"] = {}
    for pct in ("10", "25", "40"):
        p, n = res[("parent", "dropout", pct + "_cloud")], res[("new", "dropout", pct + "_image")]
        out["dropout"][pct + " %"] = {"parent host cloud, varying length": dict(p, returns=runs[("parent", "dropout", pct + "_cloud")][-1]["returns"]),
                                      "new host uint32 image, fixed length": dict(n, returns=runs[("new", "dropout", pct + "_image")][-1]["returns"]),
                                      "image_minus_cloud_us": round(n["median"] - p["median"], 2)}
    out["k_unproject"] = {}
    for posed in ("0", "1"):
        with tempfile.TemporaryDirectory() as d:
            info = spawn("kernels", new, posed, profile_dir=d, stats=True)
            stats = bk.kernel_stats(d, ("k_unproject",), strip_args=False)
        for name, v in stats.items():
            targs = name[name.index("<") + 1:name.index(">")] if "<" in name else name
            rb = 2 if "short" in targs else 4
            cb = 24 if "double" in targs else 12
            nbytes = info["pixels"] * (rb + 48 + cb) + (W * 96 if posed == "1" else 0)
            out["k_unproject"]["<%s>%s" % (targs, " column poses" if posed == "1" else "")] = dict(
                v, bytes=nbytes, TBps=round(nbytes / (v["avg_us"] * 1e-6) / 1e12, 3),
                share_of_copy_ceiling=round(nbytes / (v["avg_us"] * 1e-6) / 1e12 / COPY_CEILING_TBS, 3))
    print(json.dumps(out, indent=1))
    report.save()


if __name__ == "__main__":
    main()
