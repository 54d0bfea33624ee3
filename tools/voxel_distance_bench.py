#!/usr/bin/env python3
"""What voxel distance fields (gvom_voxel_atlas_distance_field: k_vdist_rows, k_vdist_cols, k_vdist_levels; gvom_voxel_distance_sample:
k_vdist_sample) cost.  On m256 (256 x 256 x 256) and c4 (512 x 512 x 128) with an atlas of 1024 x 1024 x (256 | 128) voxels, after three
bench scans and one integrate -- every loop in a fresh child process, every child under a `timeout` of its own, and the first child that
fails ends the run:

  events     HIP events on the handle's stream around one call: distance_field() at caps of 2 m and 8 m, with and without
             GVOM_DISTANCE_UNKNOWN_BLOCKS, against box() in the same run -- it reads the same pairs and writes a quarter of the bytes: the
             floor any form of this product has -- and sample_device() at 2^20 points; the halos and the counts of every field
  kernels    the kernels alone from a rocprofv3 kernel trace of a second child of the same kind (every cap and flag pooled)
  scipy      scipy.ndimage.distance_transform_edt on the exported class grid on the CPU (the box alone: it cannot see beyond its faces),
             by the wall clock, and whether it equals the field within 1 ulp of float32 where both are decided by the box's own voxels
  step       scan + combine_maps_device() per step without a query, on this library and, with --parent LIB, on the parent commit's,
             alternating, --turns runs each (default three)
  resources  tools/kernel_regs.py: the new kernels, and registers, scratch, LDS and code size of every kernel outside the new unit
             on the parent and on this library (--resources alone: no GPU needed)

    tools/voxel_distance_bench.py [--resources] [--parent LIB] [--configs m256,c4] [--turns N] [out.json]
                                                                                (default: profiles/voxel_distance_<lib sha8>.json)
"""
import json
import os
import sys
import tempfile
import time

import benchkit as bk

CONFIGS = {"m256": 100, "c4": 40}                        # config: timed steps per repetition
SIDE = 1024
CAPS = (2.0, 8.0)
N_POINTS = 1 << 20
CHILD_TIMEOUT = 300                                       # seconds, per child process
TURNS = 3
KERNELS = ("k_vdist_rows", "k_vdist_cols", "k_vdist_levels", "k_vdist_sample", "k_vatlas_box")


def _levels(z_size):
    z = 1
    while z < z_size:
        z *= 2
    return z


def child_events(name):
    np, torch, gvom, g, dev = bk.setup(name)
    a = g.create_voxel_atlas(SIDE, _levels(g.z_size))
    stream = torch.cuda.ExternalStream(int(g._lib.gvom_stream(g._h)))
    for scan in dev:
        bk.scan_combine(np, g, scan).release()
    a.integrate()

    def timed(call, reps=30):
        return bk.timed_events(torch, stream, call, reps, warm=3)[0]
    out = {"xy": g.xy_size, "z": g.z_size, "A": a.cells, "Z": a.levels, "resolutions_m": [g.xy_resolution, g.z_resolution]}
    out["box (memset + k_vatlas_box, xy x xy x z bytes)"] = timed(lambda: a.box().release())
    for cap in CAPS:
        for ub in (False, True):
            key = "distance_field, cap %g m%s" % (cap, ", unknown blocks" if ub else "")
            out[key] = timed(lambda: a.distance_field(cap, unknown_blocks=ub).release())
            out[key]["halo_xy_z"] = [g.get_tuning("voxel_distance_halo_xy"), g.get_tuning("voxel_distance_halo_z")]
            with a.distance_field(cap, unknown_blocks=ub) as f:
                out[key]["counts {at 0, finite, outside, seq}"] = [int(v) for v in f.counts.copy_to_host()]
    W = np.array([int(v) for v in g._state().combined_origin], np.float64)
    res = np.array([g.xy_resolution, g.xy_resolution, g.z_resolution])
    size = np.array([g.xy_size, g.xy_size, g.z_size])
    pts = ((W + np.random.default_rng(3).uniform(-0.05, 1.05, (N_POINTS, 3)) * size) * res).astype(np.float32)
    tp = torch.from_numpy(pts).cuda()
    torch.cuda.synchronize()
    with a.distance_field(CAPS[0]) as f:
        out["sample_device, %d points" % N_POINTS] = timed(lambda: f.sample_device(tp.data_ptr(), N_POINTS).release())
        with f.sample_device(tp.data_ptr(), N_POINTS) as s:
            out["sample counts {inside, finite, at 0, n}"] = [int(v) for v in s.counts.copy_to_host()]
    return out


def child_scipy(name):
    """scipy's transform of the exported class grid on the CPU against the field; a voxel whose scipy distance reaches one of the box's
    faces first could be decided from outside the box and is left out of the comparison"""
    from scipy import ndimage
    np, torch, gvom, g, dev = bk.setup(name)
    a = g.create_voxel_atlas(SIDE, _levels(g.z_size))
    for scan in dev:
        bk.scan_combine(np, g, scan).release()
    a.integrate()
    cap = CAPS[0]
    with a.box() as box, a.distance_field(cap) as f:
        classes, dist = box.classes.copy_to_host(), f.distance.copy_to_host()
    res = (g.xy_resolution, g.xy_resolution, g.z_resolution)
    t0 = time.perf_counter()
    edt = ndimage.distance_transform_edt(classes != gvom.VOXEL_OCCUPIED, sampling=res)
    wall = time.perf_counter() - t0
    face = [np.minimum(np.arange(n) + 1, n - np.arange(n)) * r for n, r in zip(classes.shape, res)]       # metres to the nearest voxel outside, per axis
    to_face = np.minimum(np.minimum(face[0][:, None, None], face[1][None, :, None]), face[2][None, None, :])
    own = (edt < to_face) & (edt < cap * (1 - 1e-6))                            # decided by the box's own voxels, clear of the cap
    ulps = np.abs(dist[own].view(np.int32).astype(np.int64) - edt[own].astype(np.float32).view(np.int32).astype(np.int64))
    return {"cap_m": cap, "scipy_edt_wall_ms": round(wall * 1e3, 1), "voxels": int(classes.size), "compared": int(own.sum()),
            "within_1_ulp": bool((ulps <= 1).all()) if own.any() else None, "max_ulps": int(ulps.max()) if own.any() else None}


def child_step(name, steps):
    np, torch, gvom, g, dev = bk.setup(name)

    def step(k):
        bk.scan_combine(np, g, dev[k % 3]).release()
    return bk.step_loop(g, step, steps, warm=min(10, steps))


def main():
    if bk.child(sys.argv[1:], {"events": lambda a: child_events(a[0]), "scipy": lambda a: child_scipy(a[0]),
                               "step": lambda a: child_step(a[0], int(a[1]))}):
        return
    args = bk.read_args(sys.argv[1:], configs=CONFIGS, turns=TURNS)
    parent = args["parent"]
    spawn = lambda mode, a, **kw: bk.spawn(__file__, mode, a, CHILD_TIMEOUT, **kw)
    report, configs = bk.product_report(
        "voxel_distance", args, {"side": SIDE, "caps_m": list(CAPS), "points": N_POINTS}, lambda k: "k_vdist" in k,
        ["caps beyond 8 m", "atlases of 4096 cells a side", "the host route of the samples", "a y pass with its column in LDS",
         "other tile widths of k_vdist_levels than 32 columns", "the step with a field per step"])
    if configs is None:
        return
    for name in args["configs"]:
        steps = CONFIGS[name]
        res = {"events": spawn("events", (name,))}
        configs[name] = res
        report.save()
        with tempfile.TemporaryDirectory() as d:                             # the kernels alone: a kernel trace of the same child
            spawn("events", (name,), profile_dir=d, stats=True)
            res["kernels (rocprofv3 --kernel-trace --stats of the events child: every cap and flag together)"] = bk.kernel_stats(d, KERNELS)
        report.save()
        res["scipy"] = spawn("scipy", (name,))
        report.save()
        runs = bk.alternate(args["turns"], {"parent_without": parent and (lambda: spawn("step", (name, steps), lib=parent)),
                                            "without": lambda: spawn("step", (name, steps))})
        step = bk.spreads(runs)
        res["step: scan + combine_maps_device, no query"] = bk.against_parent(step, "without", "parent_without", "without_")
        report.save()
    print(json.dumps(report.out, indent=1))


if __name__ == "__main__":
    main()
