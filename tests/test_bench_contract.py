"""CPU-side checks of bench.py's contract plumbing (no GPU): the self-spawning `--gpus N` parent starts N rank
processes with the launcher environment and relays failure loudly instead of hanging; the roofline object
has the keys the contract names."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_roofline_object_has_the_contract_keys():
    import bench
    stages = {s: {"median": m, "p10": m * 0.9, "p90": m * 1.1, "samples": 20}
              for s, m in (("trace", 0.040), ("encode", 0.018), ("fuse", 0.020), ("map2d", 0.032))}
    alg = {"trace": 42.1e6, "encode": 335e6, "fuse": 200e6, "map2d": 4.4e6}
    r = bench.roofline_of(alg, stages, profiled=False)
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in r
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["kernel"] == "k_trace"
    assert abs(r["achieved"] - 42.1e6 / 40e-6 / 1e9) < 1e-6 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert r["traffic"] is None and r["valu"] is None                 # counter fields only for the profiled workload
    json.dumps(r)
    rp = bench.roofline_of(alg, stages, profiled=True)                # committed m256 passes
    assert rp["traffic"] and rp["valu"] and rp["valu"]["insts_per_launch"] > 1e6
    # the line says where `traffic` comes from: a committed PMC pass, not this run
    assert rp["traffic_source"].startswith("profiles/") and "NOT measured by this run" in rp["traffic_source"] and r["traffic_source"] is None
    # one-slot rings with the eager fusion: the scan's second kernel is k_encfuse (encode + fusion), the combine has no fusion stage
    eager = dict(stages, fuse={"median": 0.0, "p10": 0.0, "p90": 0.0, "samples": 20}, encode=dict(stages["encode"], median=0.045))
    re_ = bench.roofline_of(alg, eager, profiled="m256")
    assert re_["kernel"] == "k_encfuse" and re_["algorithmic_bytes_per_launch"] == alg["encode"] + alg["fuse"]
    assert re_["traffic_detail"]["source"].startswith(("r5_", "r6_")) or re_["traffic"] is None
    # evidence hygiene: the line names the library it measured and the one the committed counters were
    # taken on, and says when they differ; k_map2d gets its own ceiling, the host link
    for key in ("lib_sha", "traffic_lib_sha", "traffic_stale", "pcie"):
        assert key in rp, key
    assert rp["lib_sha"] is None and rp["traffic_stale"] is None and rp["pcie"] is None    # (nothing loaded, no grid given)
    rs = bench.roofline_of(alg, stages, profiled="m256", xy=256, lib_sha="0" * 64)
    assert rs["traffic_stale"] is True and rs["lib_sha"] == "0" * 64                       # no committed pass was taken on THAT library
    assert rs["pcie"]["bound"] == "pcie" and rs["pcie"]["kernel"] == "k_map2d" and rs["pcie"]["bytes_to_host"] == 20 * 256 * 256
    assert abs(rs["pcie"]["frac"] - 20 * 256 * 256 / 0.032e-3 / 1e9 / bench.PCIE_PEAK_GBS) < 1e-9
    same = rs["traffic_lib_sha"]
    if same:                                                                                # (summaries of round 6 on carry the identity)
        assert bench.roofline_of(alg, stages, profiled="m256", xy=256, lib_sha=same)["traffic_stale"] is False


def test_metric_names_the_grid_the_line_ran_on():
    """m256 IS the 256^3 grid BASELINE.json's metric is quoted on; any other config says its own grid (VERDICT r4 item 11:
    sharded c4 / c5 lines used to say "256^3 voxel grid")."""
    import bench
    assert bench.metric_for("m256", [256, 256, 256]) == bench.METRIC and "256^3" in bench.METRIC
    m = bench.metric_for("c4", [512, 512, 128])
    assert "512x512x128" in m and "256^3" not in m and "BASELINE config c4" in m


def _bench(argv, env_extra=None, timeout=300):
    env = dict(os.environ, GVOM_COMM_TIMEOUT_S="20")
    env.update(env_extra or {})
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=timeout)


def test_more_ranks_than_devices_is_refused_before_anything_is_spawned():
    """`python bench.py --gpus 2` without a launcher on a box with fewer than 2 GPUs (here: none): the parent --
    which makes no HIP call itself, the device count comes from a child process -- refuses with a clear message and
    a non-zero exit code; it neither starts ranks that would hang in the rendezvous nor prints a JSON line."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU driver is present")
    p = _bench(["--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu"])
    assert p.returncode == 2
    assert b"HIP device(s) are visible" in p.stderr
    assert not [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]


@pytest.mark.parametrize("argv", [["--gpus", "3", "--config", "c4"], ["--gpus", "8", "--config", "c4"],
                                  ["--gpus", "3", "--config", "c5"], ["--gpus", "3", "--config", "m256"],
                                  ["--gpus", "2", "--config", "c1"]])
def test_sharded_workloads_that_do_not_exist_are_refused(argv):
    """`--gpus 4 --config c4` used to bench m256 silently.  c4 splits its 4 sensors over 1 / 2 / 4 ranks,
    c5 its 16 over 1 / 2 / 4 / 8 / 16; xy_size must be a multiple of 4 x ranks; c1 has no sharded form."""
    p = _bench(argv + ["--steps", "1", "--warmup", "0", "--no-cpu"])
    assert p.returncode == 2, p.stderr.decode()[-500:]
    assert not [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]


def test_sharded_workload_table():
    import bench_sharded
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "g-vom_amd"))
    import synth
    params, beams, per_rank, desc = bench_sharded.workload("c4", 4)
    assert params[2:5] == (512, 128, 4) and beams == 128 and per_rank == 1          # 512^2 x 128, buffer 4
    params, beams, per_rank, desc = bench_sharded.workload("c5", 8)
    assert params[2:5] == (1024, 128, 8) and per_rank == 2                          # 8 ranks x 524,288 returns
    assert bench_sharded.workload("m256", 8)[2] == 1
    # the ranks' shares, concatenated in rank order, are the cloud of synth.config_inputs (what the unsharded mapper gets)
    want = synth.config_inputs("c4", n_scans=2)[1][1]
    got = [bench_sharded.make_share("c4", r, 2, 1) for r in range(2)]
    assert got[0][0].shape[0] == 2 * 262144 and got[0][1] == want[1]
    assert np.array_equal(np.concatenate([g[0] for g in got], 0), want[0])


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_the_contract_keys():
    """`python bench.py --full` (short run): ONE JSON line on stdout with the keys the driver reads, the roofline of the
    dominant kernel measured live, and the CPU baseline of the same workload."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "40", "--warmup", "10", "--no-extra",
                        "--cpu-budget", "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 40 and d["warmup"] == 10 and d["higher_is_better"] is True
    assert d["unit"] == "M points/s" and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - d["config"]["points_per_scan"] / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-6 * d["value"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and 0 < r["frac"] < 1 and r["peak"] == 8000.0
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0 and "sample" in c
    # the counters in the line say which library they belong to, and whether it is the one that ran
    import hashlib
    sys.path.insert(0, os.path.join(ROOT, "g-vom_amd"))
    import gvom
    assert r["lib_sha"] == hashlib.sha256(open(gvom.library_path(), "rb").read()).hexdigest()
    assert r["traffic_stale"] == (r["traffic_lib_sha"] != r["lib_sha"]) and 0 < r["pcie"]["frac"] < 1
    assert r["algorithmic_bytes_per_launch"] == 131072 * 12 + 4 * (2 * d["sum_hit"] + d["sum_total"]) or r["kernel"] != "k_trace"
    # the fast path is the one that ran: the combines adopted the eager fusion, the organised cloud was traced in its
    # own order; and ONE loose, box-independent guard on the rate -- a GPU step slower than five one-thread CPU steps is a
    # regression on any box (the measured ratio is ~3000)
    fp = d["fast_path"]
    assert fp["eager_adopted"] >= d["steps"] and fp["dirsort"] == 0, fp           # (the two-thread legs may drop speculations; the timed blocks adopt every one)
    assert d["value"] > 5.0 * c["value"], (d["value"], c["value"])
    # otherwise a report, not a bound (no assert on an absolute time or rate under -m gpu)
    print("bench: %.1f M points/s, %.4f ms/step, k_trace frac %.3f, cpu %.3f M points/s"
          % (d["value"], d["ms_per_step"], r["frac"], c["value"]))


@pytest.mark.gpu
def test_plain_bench_run_is_lean_and_dumps_the_last_maps(tmp_path):
    """`python bench.py --steps K --warmup W --dump-outputs DIR` (no --full): the line holds the headline only -- no roofline, CPU
    baseline or other configs -- and DIR holds the origin and four maps of the last timed step, identical from run to run."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "g-vom_amd"))
    import bench
    import gvom
    import synth
    runs = []
    for r in range(2):
        out = tmp_path / ("run%d" % r)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "13", "--warmup", "5",
                            "--dump-outputs", str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
        assert len(lines) == 1
        d = json.loads(lines[0])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in d, key
        assert d["metric"] == bench.METRIC and d["unit"] == "M points/s" and d["higher_is_better"] is True and d["dtype"] == bench.DTYPE
        assert d["steps"] == 13 and d["warmup"] == 5 and d["ms_per_step"] > 0
        assert abs(d["value"] - d["config"]["points_per_scan"] / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-6 * d["value"]
        assert not set(d) & {"roofline", "cpu_baseline", "configs", "stream", "statistics", "value_host_f32"}, sorted(d)
        runs.append({n: np.load(str(out / (n + ".npy"))) for n in bench.MAP_NAMES})
    xy = synth.CONFIGS["m256"][0][2]
    assert runs[0]["origin"].shape == (3,)
    for n in bench.MAP_NAMES:
        assert runs[0][n].dtype == np.float64 and np.array_equal(runs[0][n], runs[1][n]), n
        if n != "origin":
            assert runs[0][n].shape == (xy, xy), n
    # the dump is what a caller of the timed path receives at that step: the same 18 steps through gvom.Gvom from host memory
    params, scans = synth.config_inputs("m256", n_scans=8)
    g = gvom.Gvom(*params, device=0)
    for k in range(18):
        pc, ego, tf = scans[k % len(scans)]
        g.process_pointcloud(pc, ego, tf)
        maps = g.combine_maps()
    for n, a in zip(bench.MAP_NAMES, maps):
        assert np.array_equal(runs[0][n], np.asarray(a, np.float64)), n


def test_timed_steps_runs_exactly_the_steps_asked_for():
    import bench
    seen = []
    dt, last, k = bench.timed_steps(lambda k: seen.append(k) or ("maps", k), 7, 5)
    assert seen == [7, 8, 9, 10, 11] and last == ("maps", 11) and k == 12 and dt >= 0
    dt, last, k = bench.timed_steps(lambda k: k * 10, 0, 1)
    assert last == 0 and k == 1


def test_dump_outputs_writes_every_map_as_float64(tmp_path):
    import numpy as np
    import bench
    xy = 8
    rng = np.random.default_rng(3)
    pos, neg, vis = (np.asfortranarray(rng.integers(-5, 1000, (xy, xy)).astype(np.int32)) for _ in range(3))
    maps = (np.array([1.5, -2.0, 0.25]), pos, neg, rng.normal(size=(xy, xy)), vis)
    bench.dump_outputs(str(tmp_path / "d"), maps)
    for name, a in zip(bench.MAP_NAMES, maps):
        got = np.load(str(tmp_path / "d" / (name + ".npy")))
        assert got.dtype == np.float64 and got.shape == a.shape and np.array_equal(got, a), name
    with pytest.raises(RuntimeError):
        bench.dump_outputs(str(tmp_path / "e"), None)


def test_usable_cores_honours_the_cgroup_cpu_quota(tmp_path):
    """cpu_baseline's "all cores" = the affinity mask capped by the container's CPU quota: the GPU box shows 256 logical CPUs and
    holds 16 (cgroup v2 `cpu.max = 1600000 100000`); OpenMP threads beyond the quota are throttled, so they are not cores."""
    import bench
    mask = len(os.sched_getaffinity(0))
    v2 = tmp_path / "cpu.max"
    v2.write_text("200000 100000\n")
    n, how = bench.usable_cores((str(v2),))
    assert n == min(mask, 2) and (mask <= 2 or "quota: 2" in how)
    v2.write_text("max 100000\n")
    assert bench.usable_cores((str(v2),))[0] == mask
    d = tmp_path / "cpu"; d.mkdir()
    (d / "cpu.cfs_quota_us").write_text("-1\n"); (d / "cpu.cfs_period_us").write_text("100000\n")
    assert bench.usable_cores((str(tmp_path / "missing"), str(d / "cpu.cfs_quota_us")))[0] == mask
    (d / "cpu.cfs_quota_us").write_text("100000\n")
    assert bench.usable_cores((str(d / "cpu.cfs_quota_us"),))[0] == 1


class _VirtualClock(object):
    """time.perf_counter / time.sleep on a simulated clock: every reading advances it by 1 us (a spin loop terminates), a
    sleep by its argument plus the 80 us a real one overshoots by.  Nothing else runs on it, so a schedule can neither be
    missed nor met by luck: the accounting of bench.paced_stream is checked against numbers known in advance."""

    def __init__(self):
        self.now = 1000.0

    def perf_counter(self):
        self.now += 1e-6
        return self.now

    def sleep(self, s):
        self.now += max(0.0, s) + 8e-5


def test_paced_stream_accounting_with_a_synthetic_tick(monkeypatch):
    """bench.paced_stream (the offered-load mode behind --offered-hz): a tick that takes 2 ms against a 10 ms period meets every
    deadline with ~80 % idle time; one that takes 15 ms falls behind the schedule, and the latency -- measured from the
    SCHEDULED arrival -- grows tick by tick instead of being hidden by a late start.  On a simulated clock: a real one on a busy
    host loses the odd deadline to the scheduler, which is not what this test is about."""
    import bench
    clock = _VirtualClock()
    monkeypatch.setattr(bench, "time", clock)

    def busy(ms):
        def tick(k):
            t = clock.perf_counter() + ms * 1e-3
            while clock.perf_counter() < t:
                pass
        return tick
    ok = bench.paced_stream(busy(2.0), 100.0, 30, warm=1)
    for key in ("offered_hz", "ticks", "achieved_hz", "latency_ms", "service_ms", "deadline_misses", "late_starts", "idle_frac",
                "sustainable_hz", "what"):
        assert key in ok, key
    assert ok["deadline_misses"] == 0 and ok["late_starts"] == 0 and 1.9 < ok["latency_ms"]["p50"] < 2.1
    assert ok["latency_ms"]["max"] < 2.1 and 1.99 < ok["service_ms"]["p50"] < 2.01
    assert 0.79 < ok["idle_frac"] < 0.81 and 99.5 < ok["achieved_hz"] <= 100.5 and 495 < ok["sustainable_hz"] < 505
    over = bench.paced_stream(busy(15.0), 100.0, 20, warm=0)
    assert over["deadline_misses"] == 20 and over["late_starts"] == 19
    # tick k ends ~15 (k + 1) ms after t0 and was due at 10 k ms: latency 15 + 5 k ms, 110 ms for the last one
    assert 109.9 < over["latency_ms"]["max"] < 110.2 and 64 < over["achieved_hz"] < 67.5 and over["idle_frac"] < 0.01
    json.dumps(ok), json.dumps(over)


@pytest.mark.gpu
def test_bench_stream_mode_on_one_gpu_and_through_the_sharded_leg():
    """`bench.py --offered-hz H --ticks T`: the line gains a `stream` object (per-tick latency percentiles from hand-over of a
    HOST-resident cloud to the maps in host memory, deadline misses, idle fraction, the two-thread node pattern) -- on the
    single-GPU leg and, unchanged, on the `--gpus N` leg (here: its one-rank form)."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "c2", "--steps", "40", "--warmup", "10",
                        "--no-extra", "--no-cpu", "--offered-hz", "200", "--ticks", "60"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    d = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")][-1])
    st = d["stream"]
    assert st["offered_hz"] == 200 and st["ticks"] == 60 and st["points_per_tick"] == 131072
    # structure and identities only; the figures themselves are printed, never bounded (a busy box must not fail a run)
    lat = st["latency_ms"]
    assert 0 < lat["p50"] <= lat["p95"] <= lat["p99"] <= lat["max"]
    assert 0 <= st["deadline_misses"] <= 60 and 0.0 <= st["idle_frac"] <= 1.0 and 0 < st["achieved_hz"] <= 201
    assert st["sustainable_hz"] > 0 and set(st["two_threads"]) >= {"deadline_misses", "latency_ms"}
    assert abs(st["sustained_M_points_s"] - 131072 * st["achieved_hz"] / 1e6) < 1e-6
    print("stream c2 @200 Hz: p50 %.3f p95 %.3f max %.3f ms, %d misses, idle %.2f, sustainable %.0f Hz"
          % (lat["p50"], lat["p95"], lat["max"], st["deadline_misses"], st["idle_frac"], st["sustainable_hz"]))
    env = dict(os.environ, GVOM_BENCH_FORCE_SHARDED="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c2", "--steps", "40",
                        "--warmup", "10", "--no-cpu", "--offered-hz", "200", "--ticks", "60"], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    d = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")][-1])
    st = d["stream"]
    assert st["ticks"] == 60 and len(st["per_rank"]) == 1 and 0 <= st["deadline_misses"] <= 60
    assert st["latency_ms_slowest_rank"]["p95"] > 0 and d["sharded_equals_unsharded"] is True


@pytest.mark.gpu
def test_sharded_bench_leg_with_one_rank():
    """The N > 1 leg of bench.py (one process per GPU, RCCL bound by libgvom_hip.so, shared-memory rendezvous) run
    with ONE rank -- what a one-GPU box allows: the same code path the driver's scaling run takes, JSON contract
    included."""
    env = dict(os.environ, GVOM_BENCH_FORCE_SHARDED="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "40", "--warmup", "10",
                        "--no-cpu"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["scaling"] == "weak" and d["steps"] == 40 and d["value"] > 0
    assert abs(d["value"] - d["config"]["points_per_step"] / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-3 * d["value"]
    assert "sharded" in d["config"]["workload"] and d["config"]["points_per_gpu"] == d["config"]["points_per_step"]
    # the line carries its own correctness verdict, rank 0's k_trace roofline and the exchange figures
    assert d["sharded_equals_unsharded"] is True and d["verify"]["differing_cells"] == 0 and d["verify"]["steps"] == 3
    r = d["roofline"]
    assert r["kernel"] == "k_trace" and 0 < r["frac"] < 1 and r["algorithmic_bytes_per_launch"] > 1e7
    assert len(d["exchange"]["per_rank"]) == 1 and d["exchange"]["per_rank"][0]["sent_bytes"] == 0


@pytest.mark.gpu
def test_sharded_bench_rehearsal_with_two_rank_processes_on_one_gpu():
    """`bench.py --gpus 2 --share-device`: the N > 1 leg as the driver starts it (bench.py spawns the ranks, one process each,
    rendezvous through shared memory), with both ranks on the one GPU this box has and the library's peer-copy transport
    (RCCL refuses two ranks on one device): real multi-process exchanges of device data, and the line's own verdict that
    the sharded maps equal an unsharded mapper's."""
    p = _bench(["--gpus", "2", "--share-device", "--steps", "30", "--warmup", "10", "--no-cpu"], {"GVOM_COMM_TIMEOUT_S": "120"}, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    d = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["rehearsal_on_one_device"] is True and d["transport"].startswith("peer copies")
    assert d["sharded_equals_unsharded"] is True and d["verify"]["differing_cells"] == 0
    assert d["config"]["points_per_step"] == 2 * d["config"]["points_per_gpu"]
    assert len(d["exchange"]["per_rank"]) == 2 and all(r["sent_bytes"] > 1e6 and r["received_bytes"] > 1e6 for r in d["exchange"]["per_rank"])
    assert d["peer_transport_rank0"]["copies"] > 100
    # what the judge of a real multi-GPU run needs to see: the communicator's own view of the job
    ranks = d["ranks"]
    assert [r["rank"] for r in ranks] == [0, 1] and all(r["transport"] == "peer" and r["pci_bus_id"] for r in ranks)
    assert d["distinct_devices"] == 1 and d["communicator_ranks"] == 2          # (a rehearsal: both ranks on the one GPU)
    assert "cpu_baseline" in d and "N = 1" in d["cpu_baseline"]["see"]


@pytest.mark.gpu
def test_sharded_bench_under_the_drivers_launcher():
    """The driver starts the N > 1 bench as `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
    --master-port P bench.py --gpus N ...`: every rank process gets RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the launcher
    (bench.py spawns nothing then), the ranks find each other through the shared-memory rendezvous named after the port and the
    launcher's pid, and rank 0 prints the one JSON line.  Rehearsed with both ranks on the one GPU (--share-device, peer copies)."""
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, GVOM_COMM_TIMEOUT_S="120", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "GVOM_JOB_NONCE"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-device", "--steps", "30",
                        "--warmup", "10", "--no-cpu"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout.decode()[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 30 and d["sharded_equals_unsharded"] is True
    assert [r["rank"] for r in d["ranks"]] == [0, 1] and d["communicator_ranks"] == 2


@pytest.mark.gpu
def test_sharded_bench_falls_back_to_peer_copies_when_rccl_refuses():
    """The N > 1 leg with its default transport (AUTO) where RCCL cannot start -- two ranks on one device: both ranks agree
    on peer copies, the line says so, the maps are verified, and the rank processes leave with exit code 0."""
    p = _bench(["--gpus", "2", "--share-device", "--steps", "20", "--warmup", "6", "--no-cpu"],
                    {"GVOM_COMM_TIMEOUT_S": "120", "GVOM_BENCH_REHEARSE_AUTO": "1"}, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    d = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")][-1])
    assert d["transport"].startswith("peer copies") and "RCCL could not initialise" in d["transport"]
    assert d["sharded_equals_unsharded"] is True and d["n_gpus"] == 2


@pytest.mark.gpu
def test_sharded_bench_leg_runs_baseline_config_c4():
    """BASELINE.json config 4 (512 x 512 x 128, buffer 4, the 1,048,576-point cloud) through the sharded leg with the
    one rank a one-GPU box allows -- the workload is c4's, not a silent substitute, and the line says the sharded
    maps equal the unsharded ones."""
    p = _bench(["--gpus", "1", "--config", "c4", "--steps", "10", "--warmup", "6", "--no-cpu"],
               {"GVOM_BENCH_FORCE_SHARDED": "1"}, timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    d = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")][-1])
    assert d["config"]["name"] == "c4" and d["config"]["grid"] == [512, 512, 128] and d["config"]["buffer_size"] == 4
    assert d["config"]["points_per_step"] == 1048576
    assert d["sharded_equals_unsharded"] is True and d["verify"]["steps"] == 6
