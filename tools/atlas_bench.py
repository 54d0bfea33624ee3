#!/usr/bin/env python3
"""What the map atlas (gvom_atlas_*: k_atlas_fill, k_atlas_move, k_atlas_merge, k_atlas_recall) costs.  On the map sets of m256
(256 x 256) and c4 (512 x 512) after three bench scans, with atlases of 1024 and 4096 cells -- every loop in a fresh child process,
every child under a `timeout` of its own, and the first child that fails ends the run:

  events     HIP events on the handle's stream around one call, 50 calls each: integrate without a move (the counters' memset and
             k_atlas_merge), integrate with a move of 8 cells on both axes (+ two k_atlas_move strips), recall (a memset and
             k_atlas_recall over the window), the extent export (k_atlas_recall over A x A), clear (k_atlas_fill)
  torch      the same merge written in torch on toroidal tensors (index arithmetic, where, scatter through index_put), first shown
             equal to the product (the six parts of the extent export), then timed
  step       scan + combine_maps_device() per step: without an atlas call, with integrate(), with integrate() + recall(); and, with
             --parent LIB (the parent commit's libgvom_hip.so), the step without on that library, alternating, five runs each
  resources  tools/kernel_regs.py: the new kernels, and registers, scratch, LDS and code size of every kernel outside the new
             unit on the parent and on this library (--resources alone: no GPU needed)

    tools/atlas_bench.py [--resources] [--parent LIB] [--configs m256,c4] [--turns N] [out.json]   (default: profiles/atlas_<lib sha8>.json)
"""
import itertools
import json
import sys
import time

import benchkit as bk

CONFIGS = {"m256": 100, "c4": 40}                        # config: timed steps per repetition
SIDES = (1024, 4096)
CHILD_TIMEOUT = 300                                       # seconds, per child process
TURNS = 5


def _without_integer_origin(gvom, lib):
    """the parent's library: a DeviceMaps without its integer origin"""
    if not hasattr(lib, "gvom_device_map_origin"):
        init = gvom.DeviceMaps.__init__

        def plain(self, owner, set_id, origin):
            owner._lib.gvom_device_map_origin = lambda *a: 0
            init(self, owner, set_id, origin)
        gvom.DeviceMaps.__init__ = plain


def _torch_merge(torch, planes, stamp, maps, origin, E, A, xy, seq):
    """the definition's merge on toroidal tensors: planes = nine [A*A] tensors in set order (f64 as int64 bits), maps = nine [y][x]"""
    x = torch.arange(xy, device=stamp.device)
    X, Y = origin[0] + x[None, :].expand(xy, xy), origin[1] + x[:, None].expand(xy, xy)
    inside = (X >= E[0]) & (X < E[0] + A) & (Y >= E[1]) & (Y < E[1] + A)
    cell = ((Y & (A - 1)) * A + (X & (A - 1))).reshape(-1)

    def rank(vis, neg, inf):
        return torch.where(vis > 0, 2, torch.where((neg > 0) | (inf.view(torch.float64) > -1000.0), 1, 0))
    r_new = rank(maps[2], maps[1], maps[5]).reshape(-1)
    r_old = rank(planes[2][cell], planes[1][cell], planes[5][cell])
    write = inside.reshape(-1) & (r_new >= 1) & (r_new >= r_old)
    at = cell[write]
    for p, m in zip(planes, maps):
        p.index_put_((at,), m.reshape(-1)[write])
    stamp.index_put_((at,), torch.full_like(at, seq, dtype=torch.int32))


def child_events(name, A):
    np, torch, gvom, g, dev = bk.setup(name, adapt=_without_integer_origin)
    for scan in dev:
        m = bk.scan_combine(np, g, scan)
    xy = g.xy_size
    a = g.create_atlas(A)
    stream = torch.cuda.ExternalStream(int(g._lib.gvom_stream(g._h)))
    tm = [torch.from_dlpack(getattr(m, n)) for n in gvom.DEVICE_MAP_NAMES]            # [x, y] views with strides (1, xy)
    ptrs = [t.data_ptr() for t in tm]
    o = m.origin_cells[:2]

    def timed(call, reps=50):
        return bk.timed_events(torch, stream, call, reps, warm=5)[0]

    def move(at=itertools.count(1)):                                                    # 8 cells further with every call
        k = next(at)
        a.integrate_of_device(ptrs, (o[0] + 8 * k, o[1] + 8 * k))
    out = {"xy": xy, "A": A, "atlas_MiB": A * A * 64 >> 20}
    a.integrate(m)
    out["integrate, no move (memset + k_atlas_merge)"] = timed(lambda: a.integrate(m))
    out["integrate, move of 8 cells on both axes (+ 2 x k_atlas_move)"] = timed(move)
    a.integrate(m)
    out["recall (memset + k_atlas_recall, xy x xy)"] = timed(lambda: a.recall().release())
    out["extent export (k_atlas_recall, A x A)"] = timed(lambda: a.extent_device().release(), 10)
    t0 = time.perf_counter()
    for _ in range(50):
        a.counts()
    out["counts (the call that waits), wall"] = {"us_per_call": round((time.perf_counter() - t0) / 50 * 1e6, 2)}
    out["clear (memset + k_atlas_fill, A x A)"] = timed(lambda: a.clear(), 10)
    # the merge in torch: equal first, then timed
    a.clear()
    unknown_f = [-1.0, -1000.0, -1000.0, 0.0, 0.0, 0.0]
    planes = [torch.zeros(A * A, dtype=torch.int32, device="cuda") for _ in range(3)] + \
             [torch.full((A * A,), v, dtype=torch.float64, device="cuda").view(torch.int64) for v in unknown_f]
    stamp = torch.zeros(A * A, dtype=torch.int32, device="cuda")
    maps = [t.T.contiguous() if k < 3 else t.T.contiguous().view(torch.int64) for k, t in enumerate(tm)]
    shifted = (o[0] + 5, o[1] - 3)
    for org in (o, shifted):
        seq = a.seq + 1                                                              # (clear() leaves seq running: the stamp the product writes)
        a.integrate_of_device(ptrs, org)                                             # (the extent follows; the second move clears nothing known here)
        _torch_merge(torch, planes, stamp, maps, org, (org[0] + xy // 2 - A // 2, org[1] + xy // 2 - A // 2), A, xy, seq)
    E = (shifted[0] + xy // 2 - A // 2, shifted[1] + xy // 2 - A // 2)
    with a.extent_device() as e:
        got = [torch.from_dlpack(p).T for p in (e.positive, e.negative, e.visibility, e.roughness, e.height_map, e.stamp)]
        idx = torch.arange(A, device="cuda")
        cell = (((E[1] + idx) & (A - 1))[:, None] * A + ((E[0] + idx) & (A - 1))[None, :])
        want = [planes[0][cell], planes[1][cell], planes[2][cell], planes[3][cell], planes[4][cell], stamp[cell]]
        # (the window lies in the middle of the extent: what the second move clears was UNKNOWN, as in the torch tensors)
        equal = all(bool(torch.equal(g_ if g_.dtype != torch.float64 else g_.contiguous().view(torch.int64), w)) for g_, w in zip(got, want))
        del got
    ts = []
    for rep in range(20):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _torch_merge(torch, planes, stamp, maps, o, E, A, xy, 3 + rep)
        torch.cuda.synchronize()
        ts.append(round((time.perf_counter() - t0) * 1e6, 1))
    out["torch merge (index arithmetic, where, index_put)"] = {"equal_to_the_product": equal, "us": ts[5:], "us_median": bk.median(ts[5:]),
                                                                "covers": "the merge only: no move, no counters"}
    del tm
    return out


def child_step(name, steps, mode, A):
    np, torch, gvom, g, dev = bk.setup(name, adapt=_without_integer_origin)
    a = g.create_atlas(A) if mode else None

    def step(k):
        m = bk.scan_combine(np, g, dev[k % 3])
        if mode >= 1:
            a.integrate(m)
        if mode >= 2:
            a.recall().release()
        m.release()
    return bk.step_loop(g, step, steps, warm=min(10, steps))


def main():
    if bk.child(sys.argv[1:], {"events": lambda a: child_events(a[0], int(a[1])), "step": lambda a: child_step(a[0], int(a[1]), int(a[2]), int(a[3]))}):
        return
    args = bk.read_args(sys.argv[1:], configs=CONFIGS, turns=TURNS)
    parent = args["parent"]
    spawn = lambda mode, a, **kw: bk.spawn(__file__, mode, a, CHILD_TIMEOUT, **kw)
    report, configs = bk.product_report(
        "atlas", args, {"sides": list(SIDES)}, lambda k: "k_atlas" in k,
        ["the kernels one by one under rocprofv3 (the events bracket a call: its memset and its kernels together)",
         "integrate_of() with host arrays (a staged upload that waits)", "fixed mode", "windows larger than 512 x 512",
         "a move of A or more (every cell cleared)", "another rows-per-workgroup than 4"])
    if configs is None:
        return
    for name in args["configs"]:
        steps = CONFIGS[name]
        res = {"events": {"A %d" % A: spawn("events", (name, A)) for A in SIDES}}
        configs[name] = res
        report.save()
        runs = bk.alternate(args["turns"], {"parent_without": parent and (lambda: spawn("step", (name, steps, 0, 1024), lib=parent)),
                                            "without": lambda: spawn("step", (name, steps, 0, 1024)),
                                            "integrate": lambda: spawn("step", (name, steps, 1, 1024)),
                                            "integrate_recall": lambda: spawn("step", (name, steps, 2, 1024))})
        step = bk.spreads(runs)
        step["integrate_adds_us_per_step"] = round(step["integrate"]["median"] - step["without"]["median"], 2)
        step["integrate_and_recall_add_us_per_step"] = round(step["integrate_recall"]["median"] - step["without"]["median"], 2)
        res["step: scan + combine_maps_device (+ integrate (+ recall)), A 1024"] = bk.against_parent(step, "without", "parent_without", "without_")
        report.save()
    print(json.dumps(report.out, indent=1))


if __name__ == "__main__":
    main()
