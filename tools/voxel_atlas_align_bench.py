#!/usr/bin/env python3
"""What scan alignment scoring against the voxel atlas (gvom_voxel_atlas_score_alignments: k_vatlas_align_field in front of the
unchanged k_align_score / k_align_best) costs.  On m256 (256 x 256 x 256) and c4 (512 x 512 x 128) with an atlas of 1024 x 1024 x
(256 | 128) voxels -- every loop in a fresh child process, every child under a `timeout` of its own, and the first child that fails
ends the run:

  field      after ONE integrate into a fixed extent around the window, with the box at the window, where the results are equal:
             gvom_score_alignments against gvom_voxel_atlas_score_alignments on the same K x n = 4096 x 16,384 pairs (device route),
             dilate 0 and 1 -- results shown equal first, then the whole calls by HIP events, and the kernels alone (k_align_field
             against k_vatlas_align_field, and k_align_score, on the same box) from a rocprofv3 kernel trace of a second child
  step       scan + combine_maps_device() per step without a query: on this library and, with --parent LIB (the parent commit's
             libgvom_hip.so), on that library, alternating, --turns runs each (default five)
  resources  tools/kernel_regs.py: the new kernel, and registers, scratch, LDS and code size of every other kernel on the parent and
             on this library (--resources alone: no GPU needed)

    tools/voxel_atlas_align_bench.py [--resources] [--parent LIB] [--configs m256,c4] [--turns N] [out.json]
                                                                          (default: profiles/voxel_atlas_align_<lib sha8>.json)
"""
import json
import sys
import tempfile

import benchkit as bk

CONFIGS = {"m256": 100, "c4": 40}                        # config: timed steps per repetition
SIDE = 1024
N_CANDIDATES, N_RETURNS = 4096, 16384
CHILD_TIMEOUT = 300                                       # seconds, per child process
TURNS = 5
CALLS, WARM = 30, 5                                       # timed calls and warm-up calls per line of the field child
KERNELS = ("k_vatlas_align_field", "k_align_field", "k_align_score", "k_align_best")


def _levels(z_size):
    z = 1
    while z < z_size:
        z *= 2
    return z


def child_field(name):
    """the window's call and the atlas's on the same inputs after one integrate; equal results first, then the calls by events"""
    np, torch, gvom, g, dev = bk.setup(name)
    for scan in dev:
        bk.scan_combine(np, g, scan).release()
    W = [int(v) for v in g._state().combined_origin]
    Z = _levels(g.z_size)
    E = [W[0] - (SIDE - g.xy_size) // 2 - 5, W[1] - (SIDE - g.xy_size) // 2 + 3, W[2] - (Z - g.z_size) // 2]
    a = g.create_voxel_atlas(SIDE, Z, follow=False, origin_voxels=np.array(E))
    a.integrate()
    stream = torch.cuda.ExternalStream(int(g._lib.gvom_stream(g._h)))
    cloud, ego, _ = dev[-1]
    pick = torch.linspace(0, cloud.shape[0] - 1, N_RETURNS, device=cloud.device).long()
    tc = cloud[pick].float().contiguous()
    # 15 x 15 offsets x 9 yaws x 3 z offsets = 6,075 candidates, cut to size
    M = gvom.pose_candidates(np.identity(4), g.xy_resolution, 7, 0.01, 4, z_step=g.z_resolution, z_steps=1, pivot=ego)[:N_CANDIDATES]
    assert len(M) == N_CANDIDATES, len(M)
    tm = torch.from_numpy(np.ascontiguousarray(M[:, :3, :])).cuda()
    torch.cuda.synchronize()
    out = {"candidates": N_CANDIDATES, "returns": N_RETURNS, "A": SIDE, "Z": Z, "xy": g.xy_size, "z": g.z_size}
    window = lambda d: g.score_alignments_device(tc.data_ptr(), N_RETURNS, tm.data_ptr(), N_CANDIDATES, dilate=d)
    atlas = lambda d: a.score_alignments_device(tc.data_ptr(), N_RETURNS, tm.data_ptr(), N_CANDIDATES, dilate=d)
    for d in (0, 1):
        with window(d) as w, atlas(d) as v:
            wc, wb = w.copy_to_host()
            vc, vb = v.copy_to_host()
        equal = bool(np.array_equal(wc, vc) and np.array_equal(wb, vb) and tuple(v.origin_voxels) == tuple(W))
        out["dilate %d: equal results" % d] = equal
        if not equal:                                                       # nothing is timed on results that differ
            raise SystemExit("%s, dilate %d: the atlas's result differs from the window's" % (name, d))
        out["dilate %d: class totals {occupied, near, free, unknown, outside}" % d] = [int(x) for x in wc[:, 1:].astype(np.int64).sum(axis=0)]

    def timed(call):
        return bk.timed_events(torch, stream, call, CALLS, warm=WARM)[0]
    for d in (0, 1):
        out["gvom_score_alignments, dilate %d (device route)" % d] = timed(lambda: window(d).release())
        out["gvom_voxel_atlas_score_alignments, dilate %d (device route)" % d] = timed(lambda: atlas(d).release())
    return out


def child_step(name, steps):
    np, torch, gvom, g, dev = bk.setup(name)

    def step(k):
        bk.scan_combine(np, g, dev[k % 3]).release()
    return bk.step_loop(g, step, steps, warm=min(10, steps))


def _by_dilate(rows):
    """the field kernels' dispatches of the traced child, in order: one call of either per dilate for the equality check (dilate 0,
    then 1), then the timed loops dilate by dilate, CALLS + WARM dispatches each.  Any other number of dispatches ends the run."""
    out, loop = {}, CALLS + WARM
    for kernel in ("k_align_field", "k_vatlas_align_field"):
        us = [u for _, k, u in rows if k == kernel]
        if len(us) != 2 + 2 * loop:
            raise SystemExit("%s: %d dispatches in the trace, %d expected" % (kernel, len(us), 2 + 2 * loop))
        by = {"dilate 0": us[2:2 + loop], "dilate 1": us[2 + loop:]}
        out[kernel] = {d: {"median_us": round(bk.median(v), 2), "min_us": round(min(v), 2)} for d, v in by.items()}
    return out


def main():
    if bk.child(sys.argv[1:], {"field": lambda a: child_field(a[0]), "step": lambda a: child_step(a[0], int(a[1]))}):
        return
    args = bk.read_args(sys.argv[1:], configs=CONFIGS, turns=TURNS)
    parent = args["parent"]
    spawn = lambda mode, a, **kw: bk.spawn(__file__, mode, a, CHILD_TIMEOUT, **kw)
    report, configs = bk.product_report(
        "voxel_atlas_align", args, {"side": SIDE, "candidates": N_CANDIDATES, "returns": N_RETURNS}, lambda k: "k_vatlas_align_field" in k,
        ["boxes displaced from the window (other storage phases)", "boxes that leave the extent", "the host route", "a cache of the class grid keyed on the atlas's seq",
         "atlases of 4096 cells a side"])
    if configs is None:
        return
    for name in args["configs"]:
        steps = CONFIGS[name]
        res = {"field": spawn("field", (name,))}
        configs[name] = res
        report.save()
        with tempfile.TemporaryDirectory() as d:                             # the kernels alone: a kernel trace of the same child
            spawn("field", (name,), profile_dir=d, stats=True)
            res["kernels (rocprofv3 --kernel-trace --stats of the field child)"] = bk.kernel_stats(d, KERNELS)
            res["field kernels by dilate (the same trace, dispatch by dispatch)"] = _by_dilate(bk.kernel_trace_rows(d, ("k_vatlas_align_field", "k_align_field"), exact=False))
        report.save()
        runs = bk.alternate(args["turns"], {"parent_without": parent and (lambda: spawn("step", (name, steps), lib=parent)),
                                            "without": lambda: spawn("step", (name, steps))})
        res["step: scan + combine_maps_device, no query"] = bk.against_parent(bk.spreads(runs), "without", "parent_without", "without_")
        report.save()
    print(json.dumps(report.out, indent=1))


if __name__ == "__main__":
    main()
