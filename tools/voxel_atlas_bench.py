#!/usr/bin/env python3
"""What the voxel atlas (gvom_voxel_atlas_*: k_vatlas_merge, k_vatlas_move, k_vatlas_box, k_vatlas_raycast, k_vatlas_viewpoints,
k_vatlas_viewpoint_best) costs.  On m256 (256 x 256 x 256) and c4 (512 x 512 x 128) with an atlas of 1024 x 1024 x (256 | 128) voxels --
every loop in a fresh child process, every child under a `timeout` of its own, and the first child that fails ends the run:

  events     HIP events on the handle's stream around one call, 50 calls each: integrate (the counters' memset, the move's slabs as the
             scans' egos give them, k_vatlas_merge), box (a memset and k_vatlas_box), clear (two memsets); counts() by the wall clock
  walk       after ONE integrate into a fixed extent around the window, where the answers are equal: gvom_raycast against
             gvom_voxel_atlas_raycast on the same 262,144 in-window segments (device route), gvom_score_viewpoints against
             gvom_voxel_atlas_score_viewpoints on the same 64 poses (a 32 x 1024 sensor) -- the whole calls by HIP events, and the
             kernels alone from a rocprofv3 kernel trace of a second child; with --parent LIB both children on that library too,
             alternating, --turns turns each: per call and per walk kernel this library's median against the parent's min .. max
  step       scan + combine_maps_device() per step: without an atlas call, with integrate(); and, with --parent LIB (the parent
             commit's libgvom_hip.so), the step without on that library, alternating, --turns runs each (default five)
  resources  tools/kernel_regs.py: the new kernels, and registers, scratch, LDS and code size of every kernel outside the new unit
             on the parent and on this library (--resources alone: no GPU needed)

    tools/voxel_atlas_bench.py [--resources] [--parent LIB] [--configs m256,c4] [--sections events,walk,step] [--turns N] [out.json]
                                                                                (default: profiles/voxel_atlas_<lib sha8>.json)
"""
import json
import os
import sys
import tempfile
import time

import benchkit as bk

CONFIGS = {"m256": 100, "c4": 40}                        # config: timed steps per repetition
SIDE = 1024
N_RAYS = 1 << 18
N_POSES = 64
CHILD_TIMEOUT = 300                                       # seconds, per child process
TURNS = 5
SECTIONS = ("events", "walk", "step")
WALK_CALLS = ("gvom_raycast (device route)", "gvom_voxel_atlas_raycast (device route)", "gvom_score_viewpoints (host poses)",
              "gvom_voxel_atlas_score_viewpoints (host poses)")
KERNELS = ("k_vatlas_merge", "k_vatlas_move", "k_vatlas_box", "k_vatlas_raycast", "k_vatlas_viewpoints", "k_vatlas_viewpoint_best",
           "k_raycast", "k_viewpoints", "k_viewpoint_best")


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

    def timed(call, reps=50):
        return bk.timed_events(torch, stream, call, reps, warm=5)[0]
    out = {"xy": g.xy_size, "z": g.z_size, "A": a.cells, "Z": a.levels, "atlas_MiB": a.cells * a.cells * a.levels // 4 >> 20}
    out["integrate, no move (memset + k_vatlas_merge)"] = timed(lambda: a.integrate())
    out["box (memset + k_vatlas_box, xy x xy x z)"] = timed(lambda: a.box().release())
    t0 = time.perf_counter()
    for _ in range(50):
        c = a.counts()
    out["counts (the call that waits), wall"] = {"us_per_call": round((time.perf_counter() - t0) / 50 * 1e6, 2)}
    out["counts after the scans"] = c
    out["clear (memsets, the whole atlas)"] = timed(lambda: a.clear(), 10)
    return out


def child_walk(name):
    """the window's walks and the atlas's on the same inputs after one integrate; equal answers first, then the calls by events"""
    np, torch, gvom, g, dev = bk.setup(name)
    for scan in dev:
        bk.scan_combine(np, g, scan).release()
    W = [int(v) for v in g._state().combined_origin]
    Z = _levels(g.z_size)
    E = [W[0] - (SIDE - g.xy_size) // 2 - 5, W[1] - (SIDE - g.xy_size) // 2 + 3, W[2] - (Z - g.z_size) // 2]
    a = g.create_voxel_atlas(SIDE, Z, follow=False, origin_voxels=np.array(E))
    a.integrate()
    stream = torch.cuda.ExternalStream(int(g._lib.gvom_stream(g._h)))
    rng = np.random.default_rng(3)
    res = np.array([g.xy_resolution, g.xy_resolution, g.z_resolution])
    size = np.array([g.xy_size, g.xy_size, g.z_size])
    ego = np.asarray(dev[-1][1], np.float64)
    # segments from around the ego to points of the window: neighbours in the array point the same way (sorted by azimuth)
    ends = (np.array(W) + rng.uniform(0.02, 0.98, (N_RAYS, 3)) * size) * res
    ends = ends[np.argsort(np.arctan2(ends[:, 1] - ego[1], ends[:, 0] - ego[0]), kind="stable")]
    starts = ego + rng.uniform(-0.5, 0.5, (N_RAYS, 3))
    ta, tb = torch.from_numpy(starts.astype(np.float32)).cuda(), torch.from_numpy(ends.astype(np.float32)).cuda()
    el = np.radians(np.linspace(-30.0, 30.0, 32))[:, None]
    az = (np.arange(1024) * (2.0 * np.pi / 1024))[None, :]
    g.set_sensor_model(np.ascontiguousarray(np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) * np.ones_like(az)], axis=2)))
    centre = (np.array(W) + 0.5 * size) * res
    pts = centre + rng.uniform(-0.2, 0.2, (N_POSES, 3)) * size * res
    poses = gvom.viewpoint_poses(pts, [0.0])
    tp = torch.from_numpy(np.ascontiguousarray(poses[:, :3, :])).cuda()
    max_range = 0.2 * g.xy_size * g.xy_resolution
    torch.cuda.synchronize()
    out = {"rays": N_RAYS, "poses": N_POSES, "beams_per_pose": 32 * 1024, "max_range_m": max_range, "A": SIDE, "Z": Z}
    with g.raycast_device(ta.data_ptr(), N_RAYS, tb.data_ptr(), N_RAYS) as w, a.raycast_device(ta.data_ptr(), N_RAYS, tb.data_ptr(), N_RAYS) as v:
        wr, wp = w.copy_to_host()
        vr_, vp, vv = v.copy_to_host()
    same = wr[:, 0] != gvom.RAY_LEFT_WINDOW
    out["rays: equal answers"] = bool(np.array_equal(vr_[same], wr[same][:, [0, 1, 3]]) and np.array_equal(vp[same].view(np.uint32), wp[same].view(np.uint32)))
    out["rays: statuses (window)"] = [int((wr[:, 0] == k).sum()) for k in range(5)]
    out["rays: mean steps"] = round(float(wr[:, 1].mean()), 1)
    with g.score_viewpoints_device(tp.data_ptr(), N_POSES, max_range) as w, a.score_viewpoints(poses, max_range) as v:
        wrows, vrows = w.rows.copy_to_host(), v.rows.copy_to_host()
    stay = wrows[:, 5] == 0
    out["viewpoints: poses without a beam that leaves the window"] = int(stay.sum())
    out["viewpoints: equal rows there"] = bool(np.array_equal(wrows[stay], vrows[stay]))
    out["viewpoints: atlas batch"] = g.get_tuning("voxel_atlas_viewpoint_batch")

    def timed(call, reps=30):
        return bk.timed_events(torch, stream, call, reps, warm=5)[0]
    out["gvom_raycast (device route)"] = timed(lambda: g.raycast_device(ta.data_ptr(), N_RAYS, tb.data_ptr(), N_RAYS).release())
    out["gvom_voxel_atlas_raycast (device route)"] = timed(lambda: a.raycast_device(ta.data_ptr(), N_RAYS, tb.data_ptr(), N_RAYS).release())
    out["gvom_score_viewpoints (host poses)"] = timed(lambda: g.score_viewpoints(poses, max_range).release(), 10)
    out["gvom_voxel_atlas_score_viewpoints (host poses)"] = timed(lambda: a.score_viewpoints(poses, max_range).release(), 10)
    a.box().release()
    a.integrate()
    return out


def child_step(name, steps, mode):
    np, torch, gvom, g, dev = bk.setup(name)
    a = g.create_voxel_atlas(SIDE, _levels(g.z_size)) if mode else None

    def step(k):
        m = bk.scan_combine(np, g, dev[k % 3])
        if mode:
            a.integrate()
        m.release()
    return bk.step_loop(g, step, steps, warm=min(10, steps))


def walk_against_parent(runs):
    """{figure: this library's median over its turns against the parent's median, min and max}: the four calls (median_us of a turn's
    HIP events) and the six walk kernels (avg_us of a turn's kernel trace)"""
    def figures(rec):
        out = {k: rec[k]["median_us"] for k in WALK_CALLS}
        out.update({k: v["avg_us"] for k, v in rec["kernels"].items() if "raycast" in k or "viewpoint" in k})
        return out
    p, t = [figures(r) for r in runs["parent"]], [figures(r) for r in runs["this"]]
    table = {}
    for key in p[0]:
        a, b = [x[key] for x in p], [x[key] for x in t]
        table[key] = {"parent_median": bk.median(a), "parent_min": min(a), "parent_max": max(a), "this_median": bk.median(b), "this_min": min(b),
                      "this_max": max(b), "this_median_inside_parents_own_spread": bool(min(a) <= bk.median(b) <= max(a))}
    return table


def main():
    if bk.child(sys.argv[1:], {"events": lambda a: child_events(a[0]), "walk": lambda a: child_walk(a[0]),
                               "step": lambda a: child_step(a[0], int(a[1]), int(a[2]))}):
        return
    args = bk.read_args(sys.argv[1:], configs=CONFIGS, turns=TURNS, extra={"--sections": (list(SECTIONS), lambda s: [v for v in s.split(",") if v])})
    sections = args["sections"]
    parent = args["parent"]
    spawn = lambda mode, a, **kw: bk.spawn(__file__, mode, a, CHILD_TIMEOUT, **kw)
    report, configs = bk.product_report(
        "voxel_atlas", args, {"side": SIDE, "rays": N_RAYS, "poses": N_POSES}, lambda k: "k_vatlas" in k,
        ["a move of a whole side (every voxel cleared)", "fixed mode in the step loop", "atlases of 4096 cells a side", "the host route of the rays",
         "k_vatlas_box with dword stores", "more than one workgroup shape of k_vatlas_merge"])
    if configs is None:
        return
    for name in args["configs"]:
        steps = CONFIGS[name]
        res = configs.setdefault(name, {})
        if "events" in sections:
            res["events"] = spawn("events", (name,))
            report.save()

        def walk_once(lib):                                                      # the calls by events, then the kernels alone: a kernel trace of the same child
            rec = spawn("walk", (name,), lib=lib)
            with tempfile.TemporaryDirectory() as d:
                spawn("walk", (name,), profile_dir=d, stats=True, lib=lib)
                rec["kernels"] = bk.kernel_stats(d, KERNELS)
            return rec
        if "walk" in sections:
            runs = bk.alternate(args["turns"] if parent else 1, {"parent": parent and (lambda: walk_once(parent)), "this": lambda: walk_once(None)})
            res["walk"] = dict(runs["this"][-1])
            res["kernels (rocprofv3 --kernel-trace --stats of the walk child)"] = res["walk"].pop("kernels")
            if parent:
                res["walk against the parent, %d alternating turns" % args["turns"]] = walk_against_parent(runs)
            report.save()
        if "step" not in sections:
            continue
        runs = bk.alternate(args["turns"], {"parent_without": parent and (lambda: spawn("step", (name, steps, 0), lib=parent)),
                                            "without": lambda: spawn("step", (name, steps, 0)),
                                            "integrate": lambda: spawn("step", (name, steps, 1))})
        step = bk.spreads(runs)
        step["integrate_adds_us_per_step"] = round(step["integrate"]["median"] - step["without"]["median"], 2)
        res["step: scan + combine_maps_device (+ integrate), A %d" % SIDE] = bk.against_parent(step, "without", "parent_without", "without_")
        report.save()
    print(json.dumps(report.out, indent=1))


if __name__ == "__main__":
    main()
