#!/usr/bin/env python3
"""What a ray query (gvom_raycast, k_raycast) costs, and that moving the ray helpers into csrc/gvom_ray.h left the trace kernels
alone.  Everything goes into ONE file, profiles/raycast_<lib sha8>.json; a part that has not run yet is absent.

  --resources [--parent REV]   needs no GPU.  Compiles csrc/gvom_trace.hip of REV (default HEAD) and of the working tree, and
            csrc/gvom_query.hip, for the device only, with the Makefile's flags and -Rpass-analysis=kernel-resource-usage, and
            lists per kernel what the compiler reports (SGPRs, VGPRs, AGPRs, scratch, occupancy, LDS) plus its code size (the
            `codeLenInByte` of its assembly listing).  "trace_kernels_unchanged": every kernel of gvom_trace.hip has the same
            figures on both sides.
  (default) on a GPU, every loop in a fresh child process, m256 and c4, n = 16,384 / 131,072 / 1,048,576 rays from one viewpoint
            (the last ego) to a 2:1 grid of directions over the sphere, in sweep order and shuffled:
              kernel   one `rocprofv3 --kernel-trace --stats` run per configuration: k_raycast us, rays/s, steps/s
              step     scan + combine_maps_device() per step, without and with one 131,072-ray query (device inputs)
              torch    the yardstick: the same rays walked in lock step in torch on occupancy_grid_device()'s tensor -- one
                       gather per step, the export included; free and unknown are the same there, so it is compared with the
                       library's answer without flags on OCCUPIED / LEFT_WINDOW / CLEAR only.  ratio = torch us / library us,
                       written down whatever it is.

    tools/raycast_bench.py [--resources [--parent REV]] [--configs m256,c4] [out.json]
"""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import benchkit as bk

ROOT = bk.ROOT
PKG = os.path.join(ROOT, "g-vom_amd")
CONFIGS = {"m256": 400, "c4": 100}                         # config: timed steps per repetition
CHILD_TIMEOUT = 900                                        # seconds, per child process
RAYS = (16384, 131072, 1048576)
STEP_QUERY = 131072


# ---- resources (CPU) ---------------------------------------------------------------------------------------------------------
def _make_flags():
    text = open(os.path.join(PKG, "Makefile")).read().replace("\\\n", " ")
    flags = re.search(r"^FLAGS\s*:=(.*)$", text, re.M).group(1).split()
    return [f.replace("$(ARCH)", "gfx950") for f in flags]


def _kernel_resources(src, include_dir):
    """{kernel: {sgpr, vgpr, agpr, scratch, occupancy, lds, code_bytes}} of one unit, and the raw remark lines"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "unit.s")
        cmd = [hipcc] + _make_flags() + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-I", include_dir, src, "-o", asm]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("%s failed:\n%s" % (" ".join(cmd), r.stderr[-3000:]))
        text = open(asm).read()
    keys = {"TotalSGPRs": "sgpr", "VGPRs": "vgpr", "AGPRs": "agpr", "ScratchSize [bytes/lane]": "scratch",
            "Occupancy [waves/SIMD]": "occupancy", "LDS Size [bytes/block]": "lds"}
    out, cur, listing = {}, None, []
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (?:\S+: )?\s*(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        body = m.group(1).strip()
        listing.append(body)
        if body.startswith("Function Name:"):
            cur = body.split(":", 1)[1].strip()
            out[cur] = {}
        elif cur and ":" in body:
            k, v = body.rsplit(":", 1)
            if k.strip() in keys:
                out[cur][keys[k.strip()]] = int(v)
    for name, size in re.findall(r"^(\w+):\s*; @\w+.*?^; codeLenInByte = (\d+)", text, re.M | re.S):
        if name in out:
            out[name]["code_bytes"] = int(size)
    return out, listing


def compiled_resources(parent):
    with tempfile.TemporaryDirectory() as d:
        tar = subprocess.run(["git", "-C", ROOT, "archive", parent, "g-vom_amd/csrc", "include"], capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", d], input=tar, check=True)
        before, before_list = _kernel_resources(os.path.join(d, "g-vom_amd", "csrc", "gvom_trace.hip"), os.path.join(d, "g-vom_amd", "csrc"))
    csrc = os.path.join(PKG, "csrc")
    after, after_list = _kernel_resources(os.path.join(csrc, "gvom_trace.hip"), csrc)
    query, query_list = _kernel_resources(os.path.join(csrc, "gvom_query.hip"), csrc)
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", parent], capture_output=True, text=True).stdout.strip()
    return {"compiler_flags": _make_flags(), "parent": head,
            "gvom_trace.hip": {"parent": before, "branch": after, "parent_listing": before_list, "branch_listing": after_list},
            "trace_kernels": len(before), "trace_kernels_unchanged": before == after and len(before) > 0,
            "gvom_query.hip": {"kernels": query, "listing": query_list},
            "k_raycast_scratch_bytes": sorted({v["scratch"] for v in query.values()})}


# ---- timing (GPU) ------------------------------------------------------------------------------------------------------------
def _rays(np, g, ego, n, shuffled):
    """n targets 0.45 window widths from the ego on a 2:1 (azimuth, elevation) grid, azimuth fastest: a sweep"""
    cols = int(round((2 * n) ** 0.5))
    rows = n // cols
    assert rows * cols == n, n
    az = (np.arange(cols) + 0.5) / cols * 2 * np.pi
    el = ((np.arange(rows) + 0.5) / rows - 0.5) * np.pi * 0.5
    r = 0.45 * g.xy_size * g.xy_resolution
    t = np.stack([np.cos(el)[:, None] * np.cos(az)[None], np.cos(el)[:, None] * np.sin(az)[None],
                  np.repeat(np.sin(el)[:, None], cols, axis=1)], axis=-1).reshape(n, 3) * r + np.asarray(ego)
    if shuffled:
        t = t[np.random.default_rng(5).permutation(n)]
    return np.ascontiguousarray(t.astype(np.float32))


def _torch_walk(torch, gvom, g, a, b):
    """the yardstick: lock-step walk of the rays a -> b (float32 device tensors, metres) on the exported occupancy grid, one
    gather per step; returns (status, steps) with free and unknown alike"""
    occ = g.occupancy_grid_device()
    grid = torch.from_dlpack(occ)
    st = g._state()
    W = torch.tensor(list(st.combined_origin), dtype=torch.float64, device=a.device)
    res = torch.tensor([g.xy_resolution, g.xy_resolution, g.z_resolution], dtype=torch.float64, device=a.device)
    size = torch.tensor([g.xy_size, g.xy_size, g.z_size], dtype=torch.float64, device=a.device)
    p = (a.double() / res).float()
    e = (b.double() / res).float()
    s = e - p
    length = ((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]).double().sqrt()
    s = (s.double() / length[:, None]).float()
    smax = s.abs().max(dim=1).values
    inc = s / smax[:, None]
    step_len = (1.0 / smax.double()).abs()
    S = torch.clamp(torch.ceil((length - 1.0) / step_len), min=0).to(torch.int32)      # (the band test of ray_steps is left out)
    n = a.shape[0]
    status = torch.zeros(n, dtype=torch.int32, device=a.device)
    steps = S.clone()
    run = torch.ones(n, dtype=torch.bool, device=a.device)
    for j in range(1, int(S.max()) + 1):
        p = p + inc
        v = torch.floor(p.double() - W)
        inside = ((v >= 0) & (v < size)).all(dim=1)
        go = run & (S >= j)
        left = go & ~inside
        vi = torch.where(inside[:, None], v, torch.zeros_like(v)).long()
        hit = go & inside & (grid[vi[:, 0], vi[:, 1], vi[:, 2]] != 0)
        status = torch.where(left, 3, torch.where(hit, 1, status))
        steps = torch.where(left, j - 1, torch.where(hit, j, steps))
        run = run & ~left & ~hit
    del grid
    occ.release()
    return status, steps


def child_step(name, steps):
    np, torch, gvom, g, dev = bk.setup(name)
    for scan in dev:
        bk.scan_combine(np, g, scan).release()
    ego = dev[-1][1]
    a = torch.from_numpy(np.asarray(ego, np.float32).reshape(1, 3)).cuda()
    out = {"steps": steps, "rays": {}}
    for n in RAYS:
        for order in ("sweep", "shuffled"):
            b = torch.from_numpy(_rays(np, g, ego, n, order == "shuffled")).cuda()
            an = a.expand(n, 3).contiguous()
            torch.cuda.synchronize()
            with g.raycast_device(a.data_ptr(), 1, b.data_ptr(), n) as rays:
                res = rays.result.copy_to_host()
            t_status, t_steps = _torch_walk(torch, gvom, g, an, b)
            cmp_rows = np.isin(res[:, 0], (0, 1, 3))
            same = bool(np.array_equal(t_status.cpu().numpy()[cmp_rows], res[cmp_rows, 0]) and
                        np.array_equal(t_steps.cpu().numpy()[cmp_rows], res[cmp_rows, 1]))
            row = {"total_steps": int(res[:, 1].sum()), "status_counts": np.bincount(res[:, 0], minlength=5).tolist(),
                   "torch_walk_equals_library": same}
            reps = 5 if n <= 131072 else 3

            def lib():
                g.raycast_device(a.data_ptr(), 1, b.data_ptr(), n).release()

            def yard():
                _torch_walk(torch, gvom, g, an, b)
            for label, fn, calls in (("library_us", lib, 20), ("torch_us", yard, 3)):
                for _ in range(3):
                    fn()
                bk.sync(g); torch.cuda.synchronize()
                us = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        fn()
                    bk.sync(g); torch.cuda.synchronize()
                    us.append(round((time.perf_counter() - t0) / calls * 1e6, 2))
                row[label] = {"per_call": us, "median": bk.median(us)}
            row["torch_over_library"] = round(row["torch_us"]["median"] / row["library_us"]["median"], 2)
            out["rays"]["%d %s" % (n, order)] = row
            del b, an
    b = torch.from_numpy(_rays(np, g, ego, STEP_QUERY, False)).cuda()
    torch.cuda.synchronize()

    def plain(k):
        bk.scan_combine(np, g, dev[k % len(dev)]).release()

    def with_query(k):
        plain(k)
        g.raycast_device(a.data_ptr(), 1, b.data_ptr(), STEP_QUERY).release()
    for label, step in (("scan+combine_maps_device", plain), ("+one %d-ray query" % STEP_QUERY, with_query)):
        out[label] = bk.step_loop(g, step, steps, warm=20)
        del out[label]["steps"]                                # (the record's own "steps" says it)
    out["allocations"] = g.get_tuning("raycast_allocations")
    return out


def child_kernel(name, n, shuffled):
    """Run under rocprofv3: the calls whose kernel is to be timed."""
    np, torch, gvom, g, dev = bk.setup(name)
    for scan in dev:
        bk.scan_combine(np, g, scan).release()
    ego = dev[-1][1]
    a = torch.from_numpy(np.asarray(ego, np.float32).reshape(1, 3)).cuda()
    b = torch.from_numpy(_rays(np, g, ego, n, shuffled)).cuda()
    torch.cuda.synchronize()
    for _ in range(30):
        g.raycast_device(a.data_ptr(), 1, b.data_ptr(), n).release()
    bk.sync(g)
    return {"calls": 30}


def main():
    if bk.child(sys.argv[1:], {"step": lambda a: child_step(a[0], int(a[1])), "kernel": lambda a: child_kernel(a[0], int(a[1]), a[2] == "1")}):
        return
    args = bk.read_args(sys.argv[1:], configs=CONFIGS)                     # (--parent: a revision, for --resources)
    report = bk.Report("raycast", args["path"])
    out = report.out
    if args["resources"]:
        out["resources"] = compiled_resources(args["parent"] or "HEAD")
        report.save()
        print(json.dumps({k: v for k, v in out["resources"].items() if k.startswith(("trace_kernels", "k_raycast"))}))
        return
    out["configs"] = {}
    for name in args["configs"]:
        res = bk.spawn(__file__, "step", (name, CONFIGS[name]), CHILD_TIMEOUT)
        for key, row in res["rays"].items():
            n, order = key.split()
            with tempfile.TemporaryDirectory() as d:
                bk.spawn(__file__, "kernel", (name, n, 1 if order == "shuffled" else 0), CHILD_TIMEOUT, profile_dir=d, stats=True)
                k = next(iter(bk.kernel_stats(d, ("k_raycast",)).values()), None)
            if k:
                k["rays_per_s"] = round(int(n) / (k["avg_us"] * 1e-6))
                k["steps_per_s"] = round(row["total_steps"] / (k["avg_us"] * 1e-6))
            row["k_raycast"] = k
        base = res["scan+combine_maps_device"]["us_per_step_median"]
        res["query_added_us_per_step"] = round(res["+one %d-ray query" % STEP_QUERY]["us_per_step_median"] - base, 2)
        out["configs"][name] = res
        report.save()                                          # (after every config: a long run leaves what it has)
    print(json.dumps(out["configs"], indent=1))


if __name__ == "__main__":
    main()
