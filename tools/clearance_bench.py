#!/usr/bin/env python3
"""What the obstacle clearance map (gvom_clearance) costs.  On m256, c4 and c5 -- obstacle-bearing maps after three scans --
unbounded and with max_distance = robot_radius, every loop in a fresh child process:

  kernels   one `rocprofv3 --kernel-trace --stats` run per config and cap: k_clearance_rows and k_clearance_cols
  step      scan + combine_maps_device() per step, without and with DeviceMaps.clearance(); and, in the same run, the same loop
            with the same transform WRITTEN IN TORCH on the DLPack'd positive / negative maps (a dense separable min-plus, no host
            synchronisation) -- what a consumer has without this entry point.  The torch result is checked against the
            library's squared cells once before the timing.
  registers tools/kernel_regs.py on the library's k_clearance* kernels

    tools/clearance_bench.py [--configs m256,c4,c5] [out.json]      (default: profiles/clearance_<lib sha8>.json)
"""
import json
import sys
import tempfile

import benchkit as bk

CONFIGS = {"m256": 400, "c4": 100, "c5": 30}                # config: timed steps per repetition
THRESHOLD = 50
CHILD_TIMEOUT = 900                                         # seconds, per child process


def _torch_clearance(torch, pos, neg, thr, res, cap2):
    """(distance, squared cells) of [x, y] int32 tensors: the separable transform as dense min-plus products, in blocks of at
    most 2^26 elements"""
    xy = pos.shape[0]
    big = 1 << 29
    mask = (pos > thr) | (neg > 0)
    idx = torch.arange(xy, device=pos.device, dtype=torch.int32)
    sq = (idx[:, None] - idx[None, :]) ** 2                                    # [a, b] = (a - b)^2
    blk = max(1, (1 << 26) // (xy * xy))
    pen = torch.where(mask, 0, big).to(torch.int32)                            # [i, y]
    g2 = torch.empty((xy, xy), dtype=torch.int32, device=pos.device)
    for x0 in range(0, xy, blk):                                               # g2[x, y] = min_i (x - i)^2 + pen[i, y]
        g2[x0:x0 + blk] = (sq[x0:x0 + blk, :, None] + pen[None, :, :]).amin(dim=1)
    d2 = torch.empty((xy, xy), dtype=torch.int32, device=pos.device)
    for x0 in range(0, xy, blk):                                               # d2[x, y] = min_j g2[x, j] + (y - j)^2
        d2[x0:x0 + blk] = (g2[x0:x0 + blk, :, None] + sq[None, :, :]).amin(dim=1)
    far = d2 >= big if cap2 <= 0 else (d2 > cap2)
    d2 = torch.where(far, 2147483647, d2).to(torch.int32)
    dist = torch.where(far, float("inf"), (d2.to(torch.float64).sqrt() * res)).to(torch.float32)
    return dist, d2


def child_step(name, steps):
    poses = 3
    np, torch, gvom, g, dev = bk.setup(name, poses)
    radius = float(g.robot_radius)
    cap2 = gvom._clearance_cap(radius, g.xy_resolution)

    def scan(k):
        return bk.scan_combine(np, g, dev[k % poses])

    def plain(k):
        scan(k).release()

    def lib(max_distance):
        def step(k):
            m = scan(k)
            m.clearance(THRESHOLD, max_distance=max_distance).release()
            m.release()
        return step

    def in_torch(c2):
        def step(k):
            m = scan(k)
            pos, neg = torch.from_dlpack(m.positive), torch.from_dlpack(m.negative)
            _torch_clearance(torch, pos, neg, THRESHOLD, g.xy_resolution, c2)
            del pos, neg
            m.release()
        return step

    # the maps hold obstacles, and the torch form computes what the library does
    for k in range(poses):
        m = scan(k)
    c = m.clearance(THRESHOLD)
    d2 = c.squared_cells.copy_to_host()
    pos = m.positive.copy_to_host()
    t_d2 = _torch_clearance(torch, torch.from_dlpack(m.positive), torch.from_dlpack(m.negative), THRESHOLD, g.xy_resolution, 0)[1]
    same = bool(np.array_equal(t_d2.cpu().numpy(), d2))
    info = {"xy": g.xy_size, "obstacle_cells": int((d2 == 0).sum()), "cells_above_threshold": int((pos > THRESHOLD).sum()),
            "robot_radius_m": radius, "max_cells2_at_robot_radius": cap2, "torch_form_equals_library": same}
    c.release()
    m.release()
    del t_d2
    out = {"maps": info, "steps": steps}
    loops = (("scan+combine_maps_device", plain, steps), ("+clearance unbounded", lib(None), steps),
             ("+clearance max_distance=robot_radius", lib(radius), steps),
             ("+torch transform unbounded", in_torch(0), max(steps // 10, 5)),
             ("+torch transform max_distance=robot_radius", in_torch(cap2), max(steps // 10, 5)))
    for label, step, n in loops:
        out[label] = bk.step_loop(g, step, n, warm=min(20, n), also=torch.cuda.synchronize)
    return out


def child_kernels(name, capped):
    """Run under rocprofv3: the calls whose kernels are to be timed."""
    np, torch, gvom, g, dev = bk.setup(name)
    for scan in dev:
        m = bk.scan_combine(np, g, scan)
    for _ in range(50):
        m.clearance(THRESHOLD, max_distance=float(g.robot_radius) if capped else None).release()
    bk.sync(g)
    return {"calls": 50}


def main():
    if bk.child(sys.argv[1:], {"step": lambda a: child_step(a[0], int(a[1])), "kernels": lambda a: child_kernels(a[0], a[1] == "1")}):
        return
    import kernel_regs
    args = bk.read_args(sys.argv[1:], has_parent=False, has_resources=False, configs=CONFIGS)
    report = bk.Report("clearance", args["path"], fresh=True)
    out = report.out
    out.update({"density_threshold": THRESHOLD, "registers": {k: v for k, v in kernel_regs.kernels(bk.NEW_LIB).items() if "k_clearance" in k}, "configs": {}})
    for name in args["configs"]:
        res = bk.spawn(__file__, "step", (name, CONFIGS[name]), CHILD_TIMEOUT)
        res["kernel_us"] = {}
        for label, capped in (("unbounded", 0), ("max_distance=robot_radius", 1)):
            with tempfile.TemporaryDirectory() as d:
                bk.spawn(__file__, "kernels", (name, capped), CHILD_TIMEOUT, profile_dir=d, stats=True)
                stats = bk.kernel_stats(d, ("k_clearance",))
            stats["both"] = round(sum(v["avg_us"] for v in stats.values()), 2)
            res["kernel_us"][label] = stats
        base = res["scan+combine_maps_device"]["us_per_step_median"]
        res["added_us_per_step"] = {k[1:]: round(v["us_per_step_median"] - base, 2) for k, v in res.items()
                                    if k.startswith("+") and isinstance(v, dict)}
        out["configs"][name] = res
        report.save()                                              # (after every config: a long run leaves what it has)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
