#!/usr/bin/env python3
"""What the voxel atlas's change query (gvom_voxel_atlas_changes: k_vchange_planes, k_vchange_codes, k_vchange_columns, the labelling of
gvom_frontier.hip, k_vchange_clusters) costs.  On m256 (256 x 256 x 256) and c4 (512 x 512 x 128) with an atlas of 1024 x 1024 x (256 |
128) voxels, after two bench scans and one integrate, then a third scan and its combine: the window the query sees differs from what the
atlas remembers -- every loop in a fresh child process, every child under a `timeout` of its own, and the first child that fails ends the
run:

  events     HIP events on the handle's stream around one call: changes() with every mask -- the call WAITS for the labelling, the
             events see the kernels and the waits between the batches of rounds -- against box() of the same window in the same run,
             which reads the same bits of the atlas and writes the same bytes (the floor), and against the composition a caller has
             today, written in torch on box().classes and the exported occupancy grid: two compares and column sums, no labelling
             (torch has none); part 3 and the rounds of every call; the call by the wall clock
  kernels    the kernels alone from a rocprofv3 kernel trace of a second child of the same kind (every mask pooled)
  step       scan + combine_maps_device() per step without a query, on this library and, with --parent LIB, on the parent commit's,
             alternating, --turns runs each (default three)
  resources  tools/kernel_regs.py: the new kernels, and registers, scratch, LDS and code size of every kernel outside the new unit
             on the parent and on this library (--resources alone: no GPU needed)

    tools/voxel_changes_bench.py [--resources] [--parent LIB] [--configs m256,c4] [--turns N] [out.json]
                                                                                (default: profiles/voxel_changes_<lib sha8>.json)
"""
import json
import sys
import tempfile

import benchkit as bk

CONFIGS = {"m256": 100, "c4": 40}                        # config: timed steps per repetition
SIDE = 1024
CHILD_TIMEOUT = 300                                       # seconds, per child process
TURNS = 3
KERNELS = ("k_vchange_planes", "k_vchange_codes", "k_vchange_columns", "k_vchange_clusters", "k_frontier_relax", "k_frontier_count", "k_frontier_rank",
           "k_frontier_rows", "k_frontier_stats", "k_vatlas_box")


def _levels(z_size):
    z = 1
    while z < z_size:
        z *= 2
    return z


def child_events(name):
    np, torch, gvom, g, dev = bk.setup(name)
    a = g.create_voxel_atlas(SIDE, _levels(g.z_size))
    stream = torch.cuda.ExternalStream(int(g._lib.gvom_stream(g._h)))
    for scan in dev[:2]:
        bk.scan_combine(np, g, scan).release()
    a.integrate()
    bk.scan_combine(np, g, dev[2]).release()               # the window moved on and saw more: the atlas remembers the older one

    def timed(call, reps=30):
        return bk.timed_events(torch, stream, call, reps, warm=3)[0]
    out = {"xy": g.xy_size, "z": g.z_size, "A": a.cells, "Z": a.levels}
    W = np.array([int(v) for v in g._state().combined_origin])
    out["box of the window (memset + k_vatlas_box, xy x xy x z bytes)"] = timed(lambda: a.box(W).release())
    for mask, kw in ((3, {}), (1, {"vanished": False}), (2, {"appeared": False})):
        key = "changes, mask %d" % mask
        out[key] = timed(lambda: a.changes(**kw).release())
        out[key]["call_us (wall clock: the call waits)"] = bk.timed(None, lambda: a.changes(**kw).release(), reps=5)
        with a.changes(**kw) as ch:
            out[key]["part 3 {kept, marked, in kept, cap, appeared, vanished, outside, seq}"] = [int(v) for v in ch.counts.copy_to_host()]
            out[key]["rounds"] = ch.rounds
    # what a caller has today: the class grid of the window from the atlas, the occupancy grid of the map, two compares, column sums
    with torch.cuda.stream(stream):
        def torch_form():
            box, occ = a.box(W), g.occupancy_grid_device()
            cls, o = torch.from_dlpack(box.classes), torch.from_dlpack(occ)
            appeared = (o == 1) & (cls == gvom.VOXEL_FREE)
            gone = (o == 0) & (cls == gvom.VOXEL_OCCUPIED)         # (an occupancy grid cannot tell free from never observed: an upper bound of "vanished")
            r = appeared.sum(dim=2), gone.sum(dim=2)
            del cls, o
            box.release(); occ.release()
            return r
        out["torch on box().classes and the occupancy grid: two compares, column sums, no labelling"] = timed(torch_form, reps=20)
    out["allocations"] = g.get_tuning("voxel_atlas_allocations")
    return out


def child_step(name, steps):
    np, torch, gvom, g, dev = bk.setup(name)

    def step(k):
        bk.scan_combine(np, g, dev[k % 3]).release()
    return bk.step_loop(g, step, steps, warm=min(10, steps))


def main():
    if bk.child(sys.argv[1:], {"events": lambda a: child_events(a[0]), "step": lambda a: child_step(a[0], int(a[1]))}):
        return
    args = bk.read_args(sys.argv[1:], configs=CONFIGS, turns=TURNS)
    parent = args["parent"]
    spawn = lambda mode, a, **kw: bk.spawn(__file__, mode, a, CHILD_TIMEOUT, **kw)
    report, configs = bk.product_report(
        "voxel_changes", args, {"side": SIDE}, lambda k: "k_vchange" in k,
        ["26-connected clusters in 3-D", "a level band", "a change query fused into integrate()", "atlases of 4096 cells a side",
         "other shapes of k_vchange_planes (a lane per word instead of a wave per word)", "the step with a query per step"])
    if configs is None:
        return
    for name in args["configs"]:
        steps = CONFIGS[name]
        res = {"events": spawn("events", (name,))}
        configs[name] = res
        report.save()
        with tempfile.TemporaryDirectory() as d:                             # the kernels alone: a kernel trace of the same child
            spawn("events", (name,), profile_dir=d, stats=True)
            res["kernels (rocprofv3 --kernel-trace --stats of the events child: every mask together)"] = bk.kernel_stats(d, KERNELS)
        report.save()
        runs = bk.alternate(args["turns"], {"parent_without": parent and (lambda: spawn("step", (name, steps), lib=parent)),
                                            "without": lambda: spawn("step", (name, steps))})
        step = bk.spreads(runs)
        res["step: scan + combine_maps_device, no query"] = bk.against_parent(step, "without", "parent_without", "without_")
        report.save()
    print(json.dumps(report.out, indent=1))


if __name__ == "__main__":
    main()
