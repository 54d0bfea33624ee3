#!/usr/bin/env python3
"""What rollout scoring (gvom_score_rollouts, k_rollouts) costs.  On the maps of m256 (256 x 256) and c4 (512 x 512) after three
bench scans, against the cost field towards the ego's cell, with a car footprint of about 325 cells per heading (64 headings; the
rectangle of 18 x 11 cells in front of, 5 behind the axle, whatever the config's resolution), for (K, T) = (4096, 64) and
(16384, 128), rollouts either COHERENT (arcs that leave the ego, a cell a pose) or SHUFFLED (the same poses in random order: no two
neighbours of a rollout are neighbours on the map) -- every loop in a fresh child process:

  call       DeviceCostField.score_rollouts' device route (poses in device memory), enqueue to completion: wall time
  kernel     one `rocprofv3 --kernel-trace` run per config, the four combinations in a known order: k_rollouts; with the gathers the poses ask for
             (the cells of every valid pose's heading, counted on the host) that gives the achieved gathers / s
  torch      the same scoring written in torch on the exported cell_cost -- an index tensor of K x T x M cells (in chunks of 2048
             rollouts), gather, amax, cumsum -- CHECKED EQUAL to the product (pose costs, first blocked pose, path cost) before it
             is timed.  The acceptance bar of the kernel: it has to beat this by more than the spread of both
  step       scan + combine_maps_device() + cost_to_go() per step, without and with score_rollouts; and, with --parent LIB (the
             parent commit's libgvom_hip.so), the same step without scoring on that library, alternating with this one
  registers  tools/kernel_regs.py on the kernel

    tools/rollouts_bench.py [--parent LIB] [--configs m256,c4] [--turns N] [out.json]      (default: profiles/rollouts_<lib sha8>.json)
"""
import json
import sys
import tempfile
import time

import benchkit as bk

CONFIGS = {"m256": 100, "c4": 40}                          # config: timed steps per repetition
TURNS = 2
CHILD_TIMEOUT = 900                                        # seconds, per child process
SHAPES = ((4096, 64), (16384, 128))
ORDERS = ("coherent", "shuffled")
CAR_CELLS = dict(front=18.0, rear=5.0, half_width=5.5)     # in cells of the config's xy_resolution
HEADINGS = 64
THRESHOLD, SOFT = 50, 10
CHUNK = 2048                                               # rollouts per chunk of the torch form


def _field_args(g):
    return dict(goals_in_cells=True, inflation_radius=None, density_threshold=THRESHOLD, soft_weight=SOFT)


def _car(gvom, g):
    r = g.xy_resolution
    return gvom.rectangle_footprint(CAR_CELLS["front"] * r, CAR_CELLS["rear"] * r, CAR_CELLS["half_width"] * r, r, headings=HEADINGS)


def _poses(np, K, T, ego, res, order, seed=1):
    """K arcs of T poses from the ego, a cell a pose, float32 [K, T, 3]; shuffled: the same poses in random order"""
    rng = np.random.default_rng(seed)
    th0 = rng.uniform(-np.pi, np.pi, K)
    curv = rng.uniform(-0.04, 0.04, K)
    t = np.arange(T)
    th = th0[:, None] + curv[:, None] * t[None, :]
    x = ego[0] + np.cumsum(res * np.cos(th), axis=1)
    y = ego[1] + np.cumsum(res * np.sin(th), axis=1)
    p = np.stack([x, y, th], axis=2).astype(np.float32)
    if order == "shuffled":
        p = p.reshape(K * T, 3)[rng.permutation(K * T)].reshape(K, T, 3)
    return np.ascontiguousarray(p)


def _torch_score(torch, cflat, poses, offs_pad, res, oc, xy):
    """the scoring in torch on the flat [y * xy + x] uint16 -> int32 cost map: (pose_cost int32 [K, T], first [K], path [K]).
    offs_pad [H, Mmax, 2]: the table, every heading padded with repeats of its first cell (a maximum does not mind)."""
    H = offs_pad.shape[0]
    s = torch.tensor(H / (2.0 * 3.141592653589793), dtype=torch.float32, device=poses.device)
    K, T = poses.shape[:2]
    cost = torch.empty((K, T), dtype=torch.int32, device=poses.device)
    for k0 in range(0, K, CHUNK):
        p = poses[k0:k0 + CHUNK]
        cx = (torch.floor(p[..., 0].double() / res).long() - oc[0]).int()
        cy = (torch.floor(p[..., 1].double() / res).long() - oc[1]).int()
        h = torch.remainder(torch.round(p[..., 2] * s).long(), H)
        o = offs_pad[h]                                            # [k, T, Mmax, 2]: the index tensor
        X, Y = cx[..., None] + o[..., 0], cy[..., None] + o[..., 1]
        inside = (X >= 0) & (X < xy) & (Y >= 0) & (Y < xy)
        v = cflat[(Y.clamp(0, xy - 1) * xy + X.clamp(0, xy - 1)).long()]        # gather
        blocked = (~inside).any(dim=-1) | ((v == 0) & inside).any(dim=-1)
        cost[k0:k0 + CHUNK] = torch.where(blocked, torch.zeros_like(cx), torch.where(inside, v, torch.zeros_like(v)).amax(dim=-1))
    zero = cost == 0
    first = torch.where(zero.any(dim=1), zero.int().argmax(dim=1), torch.full((K,), T, device=cost.device))
    csum = torch.cumsum(cost.long(), dim=1)
    path = torch.where(first > 0, csum.gather(1, (first - 1).clamp(min=0)[:, None])[:, 0], torch.zeros_like(first))
    return cost, first, path


def child_score(name, profiled):
    np, torch, gvom, g, dev = bk.setup(name)
    for scan in dev:
        m = bk.scan_combine(np, g, scan)
    ego = dev[2][1]
    res, xy = g.xy_resolution, g.xy_size
    table = _car(gvom, g)
    g.set_footprint(table)
    e = gvom.world_to_cells([ego[:2]], res, m.origin)[0]
    f = m.cost_to_go([e], **_field_args(g))
    cells = np.diff(table[0]).astype(np.int64)
    oc = tuple(int(v) for v in np.round(np.asarray(m.origin)[:2] / res))
    cflat = torch.from_dlpack(f.cell_cost).view(torch.int16).T.contiguous().view(-1).to(torch.int32) & 0xFFFF   # cell (x, y) at [y * xy + x]
    mmax = int(cells.max())
    pad = np.stack([np.concatenate([table[1][table[0][k]:table[0][k + 1]], np.repeat(table[1][table[0][k]:table[0][k] + 1], mmax - cells[k], axis=0)])
                    for k in range(HEADINGS)]).astype(np.int32)
    offs_pad = torch.from_numpy(pad).cuda()
    reps, results = 20, []
    for K, T in SHAPES:
        for order in ORDERS:
            poses = _poses(np, K, T, ego, res, order)
            tp = torch.from_numpy(poses).cuda()
            torch.cuda.synchronize()
            call = lambda: g.score_rollouts_of_device(f.cell_cost.ptr, tp.data_ptr(), K, T, cost_to_go_ptr=f.cost.ptr, origin=m.origin)
            if profiled:                                           # under rocprofv3: `reps` launches per combination, in this order
                for _ in range(reps):
                    call().release()
                bk.sync(g)
                continue
            # the gathers the poses ask for: the cells of every pose's heading (every pose here is valid)
            hs = np.rint(poses[..., 2] * np.float32(HEADINGS / (2.0 * np.pi))).astype(np.int64) % HEADINGS
            out = {"xy": xy, "K": K, "T": T, "order": order, "cells_per_heading_mean": round(float(cells.mean()), 1), "gathers": int(cells[hs].sum())}
            t = bk.timed(g, lambda: call().release(), reps, digits=2)
            out["call_us"], out["call_us_median"] = t["us"], t["us_median"]
            r = call()
            summary, cost = r.copy_to_host()
            out["status_counts"] = np.bincount(summary[:, 0], minlength=4).tolist()
            out["blocked_pose_share"] = round(float((cost == 0).mean()), 4)
            # the torch form on the exported cost map (zero-copy), checked, then timed
            tcost, tfirst, tpath = _torch_score(torch, cflat, tp, offs_pad, res, oc, xy)
            same = bool(np.array_equal(tcost.cpu().numpy(), cost.astype(np.int32)) and np.array_equal(tfirst.cpu().numpy(), summary[:, 1]) and
                        np.array_equal(tpath.cpu().numpy(), summary[:, 2]))
            del tcost, tfirst, tpath
            torch.cuda.synchronize()
            tus = []
            for rep in range(5):
                t0 = time.perf_counter()
                _torch_score(torch, cflat, tp, offs_pad, res, oc, xy)
                torch.cuda.synchronize()
                tus.append(round((time.perf_counter() - t0) * 1e6, 1))
            out["torch"] = {"equals_product": same, "us": tus, "us_median": bk.median(tus), "chunk_rollouts": CHUNK, "padded_cells_per_pose": mmax,
                            "index_bytes_per_call": int(K) * int(T) * mmax * 4}
            r.release()
            results.append(out)
    return {"calls": reps} if profiled else {"scoring": results}


def child_step(name, steps, score):
    np, torch, gvom, g, dev = bk.setup(name)
    K, T = SHAPES[0]
    res = g.xy_resolution
    if score:
        g.set_footprint(_car(gvom, g))
    tp = [torch.from_numpy(_poses(np, K, T, ego, res, "coherent")).cuda() for _, ego, _ in dev]
    torch.cuda.synchronize()

    def step(k):
        ego = dev[k % 3][1]
        m = bk.scan_combine(np, g, dev[k % 3])
        e = gvom.world_to_cells([ego[:2]], res, m.origin)[0]
        f = m.cost_to_go([e], **_field_args(g))
        if score:
            g.score_rollouts_of_device(f.cell_cost.ptr, tp[k % 3].data_ptr(), K, T, cost_to_go_ptr=f.cost.ptr, origin=m.origin).release()
        f.release()
        m.release()
    return dict(bk.step_loop(g, step, steps, warm=min(10, steps)), K=K if score else 0, T=T if score else 0)


def _kernel_times(profile_dir, calls):
    """the k_rollouts dispatches of a profiled run in launch order, `calls` per combination: per combination the kernel's times
    without its first three launches"""
    rows = bk.kernel_trace_rows(profile_dir, ("k_rollouts",))
    out = []
    for k in range(len(rows) // calls):
        us = [u for _, _, u in rows[k * calls + 3:(k + 1) * calls]]
        out.append({"launches": len(us), "avg_us": round(sum(us) / len(us), 2), "median_us": round(bk.median(us), 2), "min_us": round(min(us), 2),
                    "max_us": round(max(us), 2)})
    return out


def main():
    if bk.child(sys.argv[1:], {"score": lambda a: child_score(a[0], a[1] == "1"), "step": lambda a: child_step(a[0], int(a[1]), a[2] == "1")}):
        return
    import kernel_regs
    args = bk.read_args(sys.argv[1:], has_resources=False, configs=CONFIGS, turns=TURNS)
    parent = args["parent"]
    spawn = lambda mode, a, **kw: bk.spawn(__file__, mode, a, CHILD_TIMEOUT, **kw)
    report = bk.Report("rollouts", args["path"], parent, fresh=True)
    out = report.out
    out.update({"footprint_cells": CAR_CELLS, "headings": HEADINGS, "density_threshold": THRESHOLD, "soft_weight": SOFT,
                "registers": {k: v for k, v in kernel_regs.kernels(bk.NEW_LIB).items() if "k_rollouts" in k},
                "unmeasured": ["a two-kernel form (poses, then summaries) and row spans instead of cell lists (neither is built)",
                               "maps larger than c4's 512 x 512", "footprints of other sizes"],
                "configs": {}})
    for name in args["configs"]:
        steps = CONFIGS[name]
        res = spawn("score", (name, 0))
        with tempfile.TemporaryDirectory() as d:
            calls = spawn("score", (name, 1), profile_dir=d)["calls"]
            kernel = _kernel_times(d, calls)
        for k, rec in enumerate(res["scoring"]):
            rec["kernel"] = kernel[k] if len(kernel) == len(res["scoring"]) else None
            if rec["kernel"]:
                rec["gathers_per_s"] = round(rec["gathers"] / (rec["kernel"]["median_us"] * 1e-6), 0)
                rec["torch_over_kernel"] = round(rec["torch"]["us_median"] / rec["kernel"]["median_us"], 1)
            rec["torch_over_call"] = round(rec["torch"]["us_median"] / rec["call_us_median"], 1)
            # beaten by more than the spread of both: the slowest call against the fastest torch run
            rec["beats_torch_beyond_spread"] = bool(max(rec["call_us"]) < min(rec["torch"]["us"]))
        runs = bk.alternate(args["turns"], {"parent_without": parent and (lambda: spawn("step", (name, steps, 0), lib=parent)),
                                            "without": lambda: spawn("step", (name, steps, 0)), "with": lambda: spawn("step", (name, steps, 1))})
        step = {who: bk.pooled(rs) for who, rs in runs.items() if rs}      # (this file's keys are older than spreads())
        step["scoring_adds_us_per_step"] = round(step["with"]["median"] - step["without"]["median"], 2)
        if parent:
            d = step["without"]["median"] - step["parent_without"]["median"]
            step["without_minus_parent_us"] = round(d, 2)
            step["within_parent_spread"] = bool(abs(d) <= step["parent_without"]["spread_us"])
        res["step: scan + combine_maps_device + cost_to_go (+ score_rollouts %d x %d)" % SHAPES[0]] = step
        out["configs"][name] = res
        report.save()                                              # (after every config: a long run leaves what it has)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
