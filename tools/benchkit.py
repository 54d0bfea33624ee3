"""What the product benches (tools/*_bench.py, tools/product_calls_ab.py) do alike, and nothing else: the binding over whatever
library is loaded, the set-up of a config, the timing loops, the one launcher of a child process, the two readers of rocprofv3's
CSV files, the register comparison, the report file, the command line, and the alternating runs against the parent library.  A
tool imports this module, says what it measures, and ends in a short main().

torch, numpy and the binding are imported inside the functions that need them: `--resources` and the launching side of a tool run
without a GPU and without torch.
"""
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_LIB = os.path.join(ROOT, "g-vom_amd", "lib", "libgvom_hip.so")
for _p in ("g-vom_amd", "tools"):
    if os.path.join(ROOT, _p) not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, _p))
ENDINGS = {124: "the time limit", 137: "the time limit (killed after the grace)", 134: "abort", 139: "segmentation fault"}


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


# ---- inside a child process (GPU) ---------------------------------------------------------------------------------------------
def gvom_for_library(adapt=None):
    """The binding, also over the parent's library: it is bound with the entry points it has.  adapt(gvom, lib): what else one
    tool's parent library needs."""
    import ctypes
    import gvom
    lib = ctypes.CDLL(gvom.library_path())
    gvom.ABI = [e for e in gvom.ABI if hasattr(lib, e[0])]
    if adapt:
        adapt(gvom, lib)
    return gvom


def setup(config, n_scans=3, **gvom_kwargs):
    """(np, torch, gvom, g, dev): a mapper of `config` and its first bench scans in device memory, dev = [(cloud, ego, transform)]"""
    import numpy as np
    import torch
    import synth
    torch.cuda.init()
    gvom = gvom_for_library(**gvom_kwargs)
    params, scans = synth.config_inputs(config, n_scans=n_scans)
    dev = [(torch.from_numpy(np.ascontiguousarray(pc)).cuda(), ego, tf) for pc, ego, tf in scans]
    torch.cuda.synchronize()
    g = gvom.Gvom(*params, voxel_statistics=False)
    return np, torch, gvom, g, dev


def sync(g):
    g._check(g._lib.gvom_sync(g._h))


def scan_combine(np, g, scan):
    """one device-resident scan and the combine behind it: the map set"""
    t, ego, tf = scan
    g.process_pointcloud_device(t.data_ptr(), t.shape[0], np.float32, ego, tf)
    return g.combine_maps_device()


def timed(g, call, reps=10, rounds=5, warm=3, digits=1):
    """microseconds per call, enqueue to the drained stream, `rounds` times over `reps` calls; g = None: the call waits itself"""
    drain = (lambda: sync(g)) if g is not None else (lambda: None)
    for _ in range(warm):
        call()
    drain()
    us = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        drain()
        us.append(round((time.perf_counter() - t0) / reps * 1e6, digits))
    return {"us": us, "us_median": median(us)}


def timed_waiting(call, warm, n):
    """ms per call: the median of n single calls behind `warm` warm-up calls; `call` waits for its own work"""
    for _ in range(warm):
        call()
    ms = []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return median(ms)


def timed_events(torch, stream, call, n, warm=2):
    """HIP events on `stream` around single calls: ({median_us, min_us, max_us, calls}, what the last call returned)"""
    us, last = [], None
    for k in range(n + warm):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        last = call()
        e1.record(stream)
        e1.synchronize()
        if k >= warm:
            us.append(e0.elapsed_time(e1) * 1e3)
    return {"median_us": round(median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2), "calls": n}, last


def step_loop(g, step, steps, warm, reps=3, also=None):
    """`warm` steps, then `reps` repetitions of step(0) .. step(steps - 1), each to the drained stream (and also(), where the
    steps use a second runtime): microseconds per step"""
    def drain():
        sync(g)
        if also:
            also()
    for k in range(warm):
        step(k)
    drain()
    us = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for k in range(steps):
            step(k)
        drain()
        us.append(round((time.perf_counter() - t0) / steps * 1e6, 2))
    return {"us_per_step": us, "us_per_step_median": median(us), "steps": steps}


def child(argv, modes):
    """True if argv asks for a child (`--child MODE args...`): modes[MODE](args) runs and its record goes out as the RESULT line"""
    if len(argv) < 2 or argv[0] != "--child":
        return False
    print("RESULT " + json.dumps(modes[argv[1]](argv[2:])))
    return True


# ---- the launching side (no GPU in this process) ------------------------------------------------------------------------------
def command(program, limit, profile_dir=None, stats=False):
    """`program` (a list) under its time limit; profiled: rocprofv3's kernel trace between the limit and the program"""
    if profile_dir:
        program = ["rocprofv3", "--kernel-trace"] + (["--stats"] if stats else []) + ["--output-format", "csv", "-d", profile_dir, "--"] + list(program)
    return ["timeout", "-k", "10", str(int(limit))] + list(program)


def run(program, limit, what, profile_dir=None, stats=False, lib=None):
    """One child under its own time limit, on library `lib`: its standard output.  A child that fails, or runs into the limit,
    ends the whole run: after a fault nothing more is started on the GPU."""
    env = dict(os.environ, GVOM_HIP_LIBRARY=os.path.abspath(lib)) if lib else None
    r = subprocess.run(command(program, limit, profile_dir, stats), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    if r.returncode != 0:
        ending = ENDINGS.get(r.returncode)
        if ending and r.returncode in (124, 137):
            ending += " of %d s" % limit
        raise SystemExit("%s failed (exit status %d%s): nothing more is started\n%s"
                         % (what, r.returncode, ": " + ending if ending else "", r.stderr[-3000:]))
    return r.stdout


def spawn(script, mode, args, limit, profile_dir=None, stats=False, lib=None):
    """`script --child mode args` as one child (run()): the record of its last RESULT line"""
    args = [str(a) for a in args]
    out = run([sys.executable, os.path.abspath(script), "--child", mode] + args, limit, "%s %r" % (mode, args), profile_dir, stats, lib)
    lines = [ln for ln in out.splitlines() if ln.startswith("RESULT ")]
    if not lines:
        raise SystemExit("%s %r printed no RESULT line: nothing more is started" % (mode, args))
    return json.loads(lines[-1][7:])


def _csv_rows(profile_dir, suffix):
    for f in sorted(glob.glob(os.path.join(profile_dir, "**", "*" + suffix), recursive=True)):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                yield r


def kernel_stats(profile_dir, names=None, strip_args=True, total=False):
    """{kernel: {calls, avg_us, min_us, max_us}} of a `--kernel-trace --stats` run ({} where it left no *kernel_stats.csv).
    names: only kernels whose name holds one of them; strip_args: the name up to its "("; total: with total_us"""
    out = {}
    for r in _csv_rows(profile_dir, "kernel_stats.csv"):
        if names is None or any(k in r["Name"] for k in names):
            rec = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "min_us": round(float(r["MinNs"]) / 1e3, 2),
                   "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
            if total:
                rec["total_us"] = round(float(r["TotalDurationNs"]) / 1e3, 2) if "TotalDurationNs" in r else None
            out[r["Name"].split("(")[0] if strip_args else r["Name"]] = rec
    return out


def kernel_trace_rows(profile_dir, names, exact=False):
    """sorted [(start, kernel, us)] of a `--kernel-trace` run: every dispatch whose name holds one of `names` (the first that
    matches names it); exact: whose name, up to its "(" and behind a return type, IS one of them"""
    rows = []
    for r in _csv_rows(profile_dir, "kernel_trace.csv"):
        name = r["Kernel_Name"].split("(")[0] if exact else r["Kernel_Name"]
        key = [k for k in names if (name == k or name.endswith(" " + k) if exact else k in name)]
        if key:
            rows.append((int(r["Start_Timestamp"]), key[0], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    return rows


def resources(new_lib, parent_lib, is_new):
    """the new unit's kernels (is_new(name)), and every other kernel on the parent and on this library: registers, scratch, LDS,
    code size"""
    import kernel_regs
    mine = kernel_regs.kernels(new_lib)
    out = {"new_kernels": {k: v for k, v in mine.items() if is_new(k)}}
    if parent_lib:
        theirs = kernel_regs.kernels(parent_lib)
        rest = {k: v for k, v in mine.items() if not is_new(k)}
        keys = ("vgpr", "sgpr", "scratch", "lds", "code")
        changed = {k: {"parent": theirs.get(k), "new": v} for k, v in rest.items() if any((theirs.get(k) or {}).get(q) != v.get(q) for q in keys)}
        out["other_kernels"] = {"count": len(rest), "identical_to_parent": len(rest) - len(changed), "changed": changed,
                                "only_on_parent": sorted(k for k in theirs if k not in mine)}
    return out


class Report:
    """The file a tool writes, profiles/<stem>_<lib sha8>.json unless a path is given: `out` is its content, save() writes it --
    after every part, so that a run that ends early leaves what it has."""

    def __init__(self, stem, path=None, parent=None, fresh=False):
        import lib_identity
        ident = lib_identity.identity()
        self.path = path or os.path.join(ROOT, "profiles", "%s_%s.json" % (stem, (ident.get("lib_sha256") or "unknown")[:8]))
        self.out = {}
        if not fresh and os.path.exists(self.path):
            with open(self.path) as f:
                self.out = json.load(f)
        self.out["library"] = ident
        if parent:
            self.out["parent_library"] = {"lib_sha256": lib_identity.sha256_file(parent)}
        os.makedirs(os.path.dirname(os.path.abspath(self.path)), exist_ok=True)

    def save(self):
        with open(self.path, "w") as f:
            f.write(json.dumps(self.out, indent=1) + "\n")

    def not_measured(self, what):
        self.out.setdefault("not_measured", what)

    def section(self, key="configs", measured=True):
        """the dict under `key`, made if absent; measured=False (--resources alone): a file without it says "not measured" """
        if not measured:
            self.out.setdefault(key, "not measured")
        elif not isinstance(self.out.get(key), dict):
            self.out[key] = {}
        self.save()
        return self.out[key]


def product_report(stem, args, what, is_new, not_measured, section="configs"):
    """(report, the section its parts go into) of a product's bench, from read_args()'s record: the tool's constants (`what`), the
    resources, the parent's identity and the default of "not_measured" are in and saved.  With --resources alone the section is
    None: the file is complete."""
    report = Report(stem, args["path"], args["parent"])
    report.out.update(what)
    report.out["resources"] = resources(NEW_LIB, args["parent"], is_new)
    report.not_measured(not_measured)
    part = report.section(section, measured=not args["resources"])
    return report, None if args["resources"] else part


def read_args(argv, has_parent=True, positional_parent=False, has_resources=True, configs=None, turns=None, extra=None):
    """The command line of a bench, options in any place: [--parent LIB | LIB first] [--resources] [--configs a,b] [--turns N]
    [out.json] -> {parent, resources, configs, turns, path}.  configs: the tool's configs, all of them the default (None: no
    --configs); turns: the default number of alternating runs (None: no --turns); extra: {"--name": (default, convert)} -> key
    "name" with "-" as "_".  An unknown option or a word too many is refused."""
    valued = dict(extra or {})
    if has_parent and not positional_parent:
        valued["--parent"] = (None, str)
    if configs is not None:
        valued["--configs"] = (list(configs), lambda s: [v for v in s.split(",") if v])
    if turns is not None:
        valued["--turns"] = (turns, int)
    out = {k[2:].replace("-", "_"): d for k, (d, _) in valued.items()}
    out.update(parent=out.get("parent"), resources=False)
    words, argv = [], list(argv)
    while argv:
        a = argv.pop(0)
        if a == "--resources" and has_resources:
            out["resources"] = True
        elif a in valued:
            if not argv:
                raise SystemExit("%s needs a value" % a)
            out[a[2:].replace("-", "_")] = valued[a][1](argv.pop(0))
        elif a.startswith("--"):
            raise SystemExit("unknown option %s" % a)
        else:
            words.append(a)
    if positional_parent:
        if not words:
            raise SystemExit("the parent commit's libgvom_hip.so comes first")
        out["parent"] = words.pop(0)
    if len(words) > 1:
        raise SystemExit("one output path at the most: %r" % words)
    unknown = [c for c in (out.get("configs") or []) if c not in (configs or [])]
    if unknown:
        raise SystemExit("unknown config %s: this tool has %s" % (", ".join(unknown), ", ".join(configs)))
    if turns is not None and out["turns"] < 1:
        raise SystemExit("--turns: at least 1")
    out["path"] = words[0] if words else None
    return out


def alternate(turns, runs):
    """runs: {who: a call that starts one child, or None} with the parent first.  Every turn starts each of them once, in that
    order -- parent, this, parent, this ...  -> {who: [records]}"""
    out = {who: [] for who in runs}
    for _ in range(turns):
        for who, start in runs.items():
            if start:
                out[who].append(start())
    return out


def spread(rs):
    """the step records of one side's runs: their medians, the median of those, and the slowest and fastest run"""
    meds = [r["us_per_step_median"] for r in rs]
    return {"run_medians_us": meds, "median": median(meds), "min": min(meds), "max": max(meds)}


def pooled(rs):
    """the older summary, kept where a file's keys are older than spread(): every repetition of every run of one side in one list"""
    us = [u for r in rs for u in r["us_per_step"]]
    return {"us_per_step": us, "median": median(us), "spread_us": round(max(us) - min(us), 2)}


def spreads(runs):
    return {who: spread(rs) for who, rs in runs.items() if rs}


def against_parent(step, this, parent, prefix):
    """into `step` (spreads()): whether this library's median lies inside the parent's own run-to-run spread (its ends count as
    inside), and the difference of the medians -- under keys that begin with `prefix`.  Nothing without runs of the parent."""
    if parent in step:
        p, m = step[parent], step[this]["median"]
        step[prefix + "inside_parents_own_spread"] = bool(p["min"] <= m <= p["max"])
        step[prefix + "minus_parent_median_us"] = round(m - p["median"], 2)
    return step
