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

    tools/atlas_bench.py [--resources] [--parent LIB] [--configs m256,c4] [out.json]   (default: profiles/atlas_<lib sha8>.json)
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "g-vom_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CONFIGS = {"m256": 100, "c4": 40}                        # config: timed steps per repetition
SIDES = (1024, 4096)
CHILD_TIMEOUT = 300                                       # seconds, per child process
KERNELS = ("k_atlas_fill", "k_atlas_move", "k_atlas_merge", "k_atlas_recall")


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def _gvom():
    """The binding, also over the parent's library: it is bound with the entry points it has."""
    import ctypes
    import gvom
    lib = ctypes.CDLL(gvom.library_path())
    gvom.ABI = [e for e in gvom.ABI if hasattr(lib, e[0])]
    if not hasattr(lib, "gvom_device_map_origin"):        # the parent: a DeviceMaps without its integer origin
        init = gvom.DeviceMaps.__init__

        def plain(self, owner, set_id, origin):
            owner._lib.gvom_device_map_origin = lambda *a: 0
            init(self, owner, set_id, origin)
        gvom.DeviceMaps.__init__ = plain
    return gvom


def _setup(name):
    import numpy as np
    import torch
    import synth
    torch.cuda.init()
    gvom = _gvom()
    params, scans = synth.config_inputs(name, n_scans=3)
    dev = [(torch.from_numpy(np.ascontiguousarray(pc)).cuda(), ego, tf) for pc, ego, tf in scans]
    torch.cuda.synchronize()
    g = gvom.Gvom(*params, voxel_statistics=False)
    return np, torch, gvom, g, dev


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
    np, torch, gvom, g, dev = _setup(name)
    for t, ego, tf in dev:
        g.process_pointcloud_device(t.data_ptr(), t.shape[0], np.float32, ego, tf)
        m = g.combine_maps_device()
    xy = g.xy_size
    a = g.create_atlas(A)
    stream = torch.cuda.ExternalStream(int(g._lib.gvom_stream(g._h)))
    tm = [torch.from_dlpack(getattr(m, n)) for n in gvom.DEVICE_MAP_NAMES]            # [x, y] views with strides (1, xy)
    ptrs = [t.data_ptr() for t in tm]
    o = m.origin_cells[:2]

    def timed(call, reps=50):
        us = []
        for k in range(reps + 5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call(k)
            e1.record(stream)
            e1.synchronize()
            if k >= 5:
                us.append(e0.elapsed_time(e1) * 1e3)
        return {"median_us": round(_median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2), "calls": reps}
    out = {"xy": xy, "A": A, "atlas_MiB": A * A * 64 >> 20}
    a.integrate(m)
    out["integrate, no move (memset + k_atlas_merge)"] = timed(lambda k: a.integrate(m))
    out["integrate, move of 8 cells on both axes (+ 2 x k_atlas_move)"] = timed(lambda k: a.integrate_of_device(ptrs, (o[0] + 8 * (k + 1), o[1] + 8 * (k + 1))))
    a.integrate(m)
    out["recall (memset + k_atlas_recall, xy x xy)"] = timed(lambda k: a.recall().release())
    out["extent export (k_atlas_recall, A x A)"] = timed(lambda k: a.extent_device().release(), 10)
    t0 = time.perf_counter()
    for _ in range(50):
        a.counts()
    out["counts (the call that waits), wall"] = {"us_per_call": round((time.perf_counter() - t0) / 50 * 1e6, 2)}
    out["clear (memset + k_atlas_fill, A x A)"] = timed(lambda k: a.clear(), 10)
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
    out["torch merge (index arithmetic, where, index_put)"] = {"equal_to_the_product": equal, "us": ts[5:], "us_median": _median(ts[5:]),
                                                                "covers": "the merge only: no move, no counters"}
    del tm
    return out


def child_step(name, steps, mode, A):
    np, torch, gvom, g, dev = _setup(name)
    a = g.create_atlas(A) if mode else None

    def step(k):
        t, ego, tf = dev[k % 3]
        g.process_pointcloud_device(t.data_ptr(), t.shape[0], np.float32, ego, tf)
        m = g.combine_maps_device()
        if mode >= 1:
            a.integrate(m)
        if mode >= 2:
            a.recall().release()
        m.release()

    for k in range(min(10, steps)):
        step(k)
    g._check(g._lib.gvom_sync(g._h))
    us = []
    for rep in range(3):
        t0 = time.perf_counter()
        for k in range(steps):
            step(k)
        g._check(g._lib.gvom_sync(g._h))
        us.append(round((time.perf_counter() - t0) / steps * 1e6, 2))
    return {"us_per_step": us, "us_per_step_median": _median(us), "steps": steps}


def _spawn(mode, args, lib=None):
    """one child under its own time limit; a child that fails (or runs into the limit) ends the whole run"""
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.abspath(__file__), "--child", mode] + [str(a) for a in args]
    env = dict(os.environ, GVOM_HIP_LIBRARY=os.path.abspath(lib)) if lib else None
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    if r.returncode != 0:
        raise SystemExit("%s %r failed (%d): nothing more is started\n%s" % (mode, args, r.returncode, r.stderr[-3000:]))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def resources(new, parent):
    """the new unit's kernels, and every other kernel on the parent and on this library: registers, scratch, LDS, code size"""
    import kernel_regs
    mine = kernel_regs.kernels(new)
    out = {"new_kernels": {k: v for k, v in mine.items() if "k_atlas" in k}}
    if parent:
        theirs = kernel_regs.kernels(parent)
        rest = {k: v for k, v in mine.items() if "k_atlas" not in k}
        keys = ("vgpr", "sgpr", "scratch", "lds", "code")
        changed = {k: {"parent": theirs.get(k), "new": v} for k, v in rest.items() if any((theirs.get(k) or {}).get(q) != v.get(q) for q in keys)}
        out["other_kernels"] = {"count": len(rest), "identical_to_parent": len(rest) - len(changed), "changed": changed,
                                "only_on_parent": sorted(k for k in theirs if k not in mine)}
    return out


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        mode, a = sys.argv[2], sys.argv[3:]
        res = child_events(a[0], int(a[1])) if mode == "events" else child_step(a[0], int(a[1]), int(a[2]), int(a[3]))
        print("RESULT " + json.dumps(res))
        return
    import lib_identity
    args = sys.argv[1:]
    parent, only_resources, configs = None, False, list(CONFIGS)
    while args and args[0] in ("--parent", "--resources", "--configs"):
        if args[0] == "--parent":
            parent, args = args[1], args[2:]
        elif args[0] == "--configs":
            configs, args = args[1].split(","), args[2:]
        else:
            only_resources, args = True, args[1:]
    new = os.path.join(ROOT, "g-vom_amd", "lib", "libgvom_hip.so")
    path = args[0] if args else os.path.join(ROOT, "profiles", "atlas_%s.json" % (lib_identity.identity().get("lib_sha256") or "unknown")[:8])
    out = json.load(open(path)) if os.path.exists(path) else {}
    out.update({"library": lib_identity.identity(), "sides": list(SIDES)})
    out["resources"] = resources(new, parent)
    if parent:
        out["parent_library"] = {"lib_sha256": lib_identity.sha256_file(parent)}
    out.setdefault("not_measured", ["the kernels one by one under rocprofv3 (the events bracket a call: its memset and its kernels together)",
                                    "integrate_of() with host arrays (a staged upload that waits)", "fixed mode", "windows larger than 512 x 512",
                                    "a move of A or more (every cell cleared)", "another rows-per-workgroup than 4"])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)

    def save():
        with open(path, "w") as f:                                  # (after every part: a run that ends early leaves what it has)
            f.write(json.dumps(out, indent=1) + "\n")
    save()
    if only_resources:
        out.setdefault("configs", "not measured")
        save()
        return
    if not isinstance(out.get("configs"), dict):
        out["configs"] = {}
    for name in configs:
        steps = CONFIGS[name]
        res = {"events": {"A %d" % A: _spawn("events", (name, A)) for A in SIDES}}
        out["configs"][name] = res
        save()
        runs = {"without": [], "integrate": [], "integrate_recall": [], "parent_without": []}
        for rnd in range(5):                                        # alternating: parent, without, with, ...
            if parent:
                runs["parent_without"].append(_spawn("step", (name, steps, 0, 1024), lib=parent))
            runs["without"].append(_spawn("step", (name, steps, 0, 1024)))
            runs["integrate"].append(_spawn("step", (name, steps, 1, 1024)))
            runs["integrate_recall"].append(_spawn("step", (name, steps, 2, 1024)))
        step = {}
        for who, rs in runs.items():
            if rs:
                meds = [r["us_per_step_median"] for r in rs]
                step[who] = {"run_medians_us": meds, "median": _median(meds), "min": min(meds), "max": max(meds)}
        step["integrate_adds_us_per_step"] = round(step["integrate"]["median"] - step["without"]["median"], 2)
        step["integrate_and_recall_add_us_per_step"] = round(step["integrate_recall"]["median"] - step["without"]["median"], 2)
        if parent:
            p = step["parent_without"]
            step["without_inside_parents_own_spread"] = bool(p["min"] <= step["without"]["median"] <= p["max"])
            step["without_minus_parent_median_us"] = round(step["without"]["median"] - p["median"], 2)
        res["step: scan + combine_maps_device (+ integrate (+ recall)), A 1024"] = step
        save()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
