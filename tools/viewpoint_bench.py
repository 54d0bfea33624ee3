#!/usr/bin/env python3
"""What viewpoint scoring (gvom_score_viewpoints: k_viewpoints, k_viewpoint_best) costs.  On the fused maps of m256 and c4 after three
bench scans, a 64 x 1024 sensor model (beams between -40 and +40 degrees), K = 64 and 512 poses on a grid around the last ego, beam
strides (1, 1) and (2, 4), max_range 20 m -- every loop in a fresh child process, every child under a `timeout` of its own, and the
first child that fails ends the run:

  call       Gvom.score_viewpoints_device(), enqueue to completion: wall time, what it found, viewpoints per launch
  kernel     one `rocprofv3 --kernel-trace` run per config: k_viewpoints and k_viewpoint_best per call, and the fills that clear the
             bitmaps and the rows as a share of the device time of a call
  parts      the same answer from what the library had before (K = 64 only): the K x nb targets built on the host, uploaded, K
             raycast_device() calls, the `unknown` column summed and the statuses counted in torch -- visits and columns 3 .. 7, first
             shown equal to the product.  (The gain has no such form: k_raycast does not say which voxels it passed.)
  walk       the walk alone (K = 64): ONE raycast_device() call over the same K x nb segments, already uploaded -- k_raycast has the
             same step body and no atomics, so the difference to the call is what the bitmaps cost
  step       scan + combine_maps_device() per step, without and with a query (K = 64, strides (2, 4)); and, with --parent LIB (the
             parent commit's libgvom_hip.so), the same step without on that library, alternating, five runs each
  resources  tools/kernel_regs.py: the new kernels, and registers, scratch, LDS and code size of every kernel outside the new
             unit on the parent and on this library (--resources alone: no GPU needed)

    tools/viewpoint_bench.py [--resources] [--parent LIB] [--configs m256,c4] [--turns N] [out.json]   (default: profiles/viewpoints_<lib sha8>.json)
"""
import json
import math
import sys
import tempfile
import time

import benchkit as bk

CONFIGS = {"m256": 100, "c4": 40}                         # config: timed steps per repetition
TURNS = 5
MODEL = (64, 1024)
SHAPES = ((64, (1, 1)), (64, (2, 4)), (512, (1, 1)), (512, (2, 4)))      # (K, beam strides)
MAX_RANGE = 20.0
CHILD_TIMEOUT = 300                                       # seconds, per child process
KERNELS = ("k_viewpoints", "k_viewpoint_best", "fillBuffer")


def _model(np):
    H, W = MODEL
    el = np.radians(np.linspace(-40.0, 40.0, H))[:, None]
    az = (np.arange(W) * (2.0 * math.pi / W))[None, :]
    return np.ascontiguousarray(np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) * np.ones_like(az)], axis=2))


def _poses(np, gvom, ego, K):
    """K poses on a square grid of 1.25 m pitch around the ego, at its height, each under another yaw"""
    n = int(math.ceil(math.sqrt(K)))
    pts = [(ego[0] + 1.25 * (i - n / 2.0), ego[1] + 1.25 * (j - n / 2.0), ego[2] + 0.5) for j in range(n) for i in range(n)][:K]
    return np.ascontiguousarray(np.stack([gvom.viewpoint_poses([p], [0.37 * k])[0] for k, p in enumerate(pts)])[:, :3, :])


def _setup(name, with_model=True):
    np, torch, gvom, g, dev = bk.setup(name)
    if with_model:
        g.set_sensor_model(_model(np))
    return np, torch, gvom, g, dev


def _targets(np, d, pose, r, strides):
    """the definition's targets (include/gvom_hip.h "viewpoint scoring"): float32 a [3], b [nb, 3]"""
    d = d[::strides[0], ::strides[1]].reshape(-1, 3)
    C = pose.reshape(12)
    p = np.float64(r) * d
    q = np.empty_like(p)
    for c in range(3):
        q[:, c] = ((p[:, 0] * C[4 * c] + p[:, 1] * C[4 * c + 1]) + p[:, 2] * C[4 * c + 2]) + C[4 * c + 3]
    return C[[3, 7, 11]].astype(np.float32), q.astype(np.float32)


def child_call(name, profiled):
    np, torch, gvom, g, dev = _setup(name)
    for scan in dev:
        bk.scan_combine(np, g, scan).release()
    ego = dev[2][1]
    reps, results = 20, {}
    for K, strides in SHAPES:
        poses = _poses(np, gvom, ego, K)
        tp = torch.from_numpy(poses).cuda()
        torch.cuda.synchronize()
        call = lambda: g.score_viewpoints_device(tp.data_ptr(), K, MAX_RANGE, beam_stride=strides)
        key = "K%d_stride%dx%d" % (K, strides[0], strides[1])
        if profiled:
            for _ in range(reps):
                call().release()
            bk.sync(g)
            continue
        us = bk.timed(g, lambda: call().release(), reps, digits=2)["us"]
        v = call()
        rows, best = v.copy_to_host()
        v.release()
        nb = int(best[3])
        out = {"xy": g.xy_size, "z": g.z_size, "K": K, "beams_per_viewpoint": nb, "call_us": us, "call_us_median": bk.median(us),
               "viewpoints_per_launch": g.get_tuning("viewpoint_batch"), "best": best.tolist(), "gain_sum": int(rows[:, 1].sum()),
               "visits_sum": int(rows[:, 2].sum()), "visits_over_gain": round(float(rows[:, 2].sum()) / max(int(rows[:, 1].sum()), 1), 2),
               "beam_endings": rows[:, 3:].sum(axis=0).tolist(), "origin_statuses": np.bincount(rows[:, 0], minlength=5).tolist()}
        out["ns_per_beam"] = round(out["call_us_median"] * 1e3 / (K * nb), 3)
        if K == 64:                                                # the same from K raycast_device() calls on uploaded targets
            d = _model(np)

            def from_parts(timed):
                t0 = time.perf_counter()
                ab = [_targets(np, d, p, MAX_RANGE, strides) for p in poses]
                t1 = time.perf_counter()
                ta = [(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()) for a, b in ab]
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                got = torch.zeros((K, 6), dtype=torch.int64, device="cuda")
                for k, (a, b) in enumerate(ta):
                    with g.raycast_device(a.data_ptr(), 1, b.data_ptr(), b.shape[0]) as rays:
                        res = torch.from_dlpack(rays.result)
                        got[k, 0] = res[:, 3].sum()
                        got[k, 1:] = torch.bincount(res[:, 0], minlength=5)[torch.tensor([1, 0, 3, 2, 4], device="cuda")]
                        del res
                got = got.cpu().numpy()
                t3 = time.perf_counter()
                return got, [round((t1 - t0) * 1e6, 1), round((t2 - t1) * 1e6, 1), round((t3 - t2) * 1e6, 1)]
            got, _ = from_parts(False)
            ts = [from_parts(True)[1] for _ in range(3)]
            # the walk alone: ONE raycast_device() call over all K x nb segments, already uploaded (k_raycast: no atomics, its targets
            # and origins read from HBM) -- what of k_viewpoints' time the walk is, and what the bitmap is
            ab = [_targets(np, d, p, MAX_RANGE, strides) for p in poses]
            A = torch.from_numpy(np.ascontiguousarray(np.concatenate([np.repeat(a[None], len(b), axis=0) for a, b in ab]))).cuda()
            B = torch.from_numpy(np.ascontiguousarray(np.concatenate([b for _, b in ab]))).cuda()
            torch.cuda.synchronize()
            one = lambda: g.raycast_device(A.data_ptr(), A.shape[0], B.data_ptr(), B.shape[0])
            ws = bk.timed(g, lambda: one().release(), digits=2)["us"]
            with one() as rays:
                walk_visits = int(rays.result.copy_to_host()[:, 3].astype(np.int64).sum())
            out["walk_alone_one_raycast_call"] = {"rays": int(A.shape[0]), "call_us": ws, "call_us_median": bk.median(ws),
                                                  "unknown_sum_equals_visits": bool(walk_visits == int(rows[:, 2].sum()))}
            del A, B
            out["from_existing_parts"] = {"covers": "visits and the beam endings; the gain has no such form",
                                          "equal_to_the_product": bool(np.array_equal(got, rows[:, 2:].astype(np.int64))),
                                          "us_build_targets_on_host": [t[0] for t in ts], "us_upload": [t[1] for t in ts],
                                          "us_K_raycast_calls_and_sums": [t[2] for t in ts],
                                          "us_median_total": bk.median([sum(t) for t in ts]), "uploaded_bytes": K * nb * 12}
        results[key] = out
    return {"calls": reps} if profiled else results


def child_step(name, steps, with_query):
    np, torch, gvom, g, dev = _setup(name, with_model=bool(with_query))
    K, strides = SHAPES[1]
    tp = None

    def step(k):
        m = bk.scan_combine(np, g, dev[k % 3])
        if with_query:
            g.score_viewpoints_device(tp.data_ptr(), K, MAX_RANGE, beam_stride=strides).release()
        m.release()

    if with_query:
        tp = torch.from_numpy(_poses(np, gvom, dev[2][1], K)).cuda()
        torch.cuda.synchronize()
    return bk.step_loop(g, step, steps, warm=min(10, steps))


def _kernel_times(profile_dir, calls):
    """per shape (k_viewpoint_best ends a call): the kernels' and the fills' microseconds per call, without the first three calls"""
    rows = bk.kernel_trace_rows(profile_dir, KERNELS)
    ends = [i for i, r in enumerate(rows) if r[1] == "k_viewpoint_best"]
    if len(ends) != calls * len(SHAPES):
        return None
    out = {}
    for n, (K, strides) in enumerate(SHAPES):
        first = ends[n * calls + 2] + 1                            # behind the third call of the shape
        last = ends[(n + 1) * calls - 1] + 1
        part, used = rows[first:last], calls - 3
        rec = {}
        for k in KERNELS:
            us = [u for _, kk, u in part if kk == k]
            rec[k] = {"launches_per_call": round(len(us) / used, 2), "us_per_call": round(sum(us) / used, 2), "median_us_per_launch": round(bk.median(us), 2) if us else None}
        total = sum(u for _, _, u in part) / used
        rec["device_us_per_call"] = round(total, 2)
        rec["clears_share_of_device_time"] = round(rec["fillBuffer"]["us_per_call"] / total, 4) if total else None
        out["K%d_stride%dx%d" % (K, strides[0], strides[1])] = rec
    return out


def main():
    if bk.child(sys.argv[1:], {"call": lambda a: child_call(a[0], a[1] == "1"), "step": lambda a: child_step(a[0], int(a[1]), a[2] == "1")}):
        return
    args = bk.read_args(sys.argv[1:], configs=CONFIGS, turns=TURNS)
    parent = args["parent"]
    spawn = lambda mode, a, **kw: bk.spawn(__file__, mode, a, CHILD_TIMEOUT, **kw)
    report, configs = bk.product_report(
        "viewpoints", args, {"model": list(MODEL), "max_range_m": MAX_RANGE, "shapes": [[K, list(s)] for K, s in SHAPES]}, lambda k: "k_viewpoint" in k,
        ["c5", "RQ_DEPTH other than 4", "per-wave combining of ORs to the same word (not built)",
         "non-returning ORs plus a population-count pass over the bitmaps (not built)",
         "viewpoint_bitmap_mb other than the default 256", "the gain from existing parts (k_raycast records no voxels)",
         "from_existing_parts and the walk alone at K = 512", "the host route", "hardware counters"])
    if parent:                                                      # (the kernel whose step body k_viewpoints shares, shown beside the new ones)
        import kernel_regs
        report.out["resources"]["k_raycast"] = {k: v for k, v in kernel_regs.kernels(bk.NEW_LIB).items() if "k_raycast" in k}
        report.save()
    if configs is None:
        return
    for name in args["configs"]:
        steps = CONFIGS[name]
        res = spawn("call", (name, 0))
        with tempfile.TemporaryDirectory() as d:
            prof = spawn("call", (name, 1), profile_dir=d)
            kernel = _kernel_times(d, prof["calls"])
        for key in res:
            res[key]["kernels"] = kernel[key] if kernel else "not measured (the trace did not hold the expected launches)"
        configs[name] = res
        report.save()
        runs = bk.alternate(args["turns"], {"parent_without": parent and (lambda: spawn("step", (name, steps, 0), lib=parent)),
                                            "without": lambda: spawn("step", (name, steps, 0)), "with": lambda: spawn("step", (name, steps, 1))})
        step = bk.spreads(runs)
        step["query_adds_us_per_step"] = round(step["with"]["median"] - step["without"]["median"], 2)
        res["step: scan + combine_maps_device (+ a query of K = 64, strides (2, 4))"] = bk.against_parent(step, "without", "parent_without", "without_")
        report.save()
    print(json.dumps(report.out, indent=1))


if __name__ == "__main__":
    main()
