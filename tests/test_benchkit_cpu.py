"""tools/benchkit.py, the module the product benches share: its medians and spreads, the two readers of rocprofv3's CSV files, the
child launcher (on children written here, in pure Python: nothing opens the GPU), the command line and the report file."""
import json
import os
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import benchkit as bk          # noqa: E402


def test_median_of_odd_even_and_single_inputs():
    assert bk.median([3, 1, 2]) == 2
    assert bk.median([4, 1, 3, 2]) == 2.5
    assert bk.median([7.5]) == 7.5
    assert bk.median((5, 5, 1, 9, 2)) == 5


def _runs(*medians):
    return [{"us_per_step": [m, m, m], "us_per_step_median": m, "steps": 10} for m in medians]


def test_spread_and_the_parent_margin():
    assert bk.spread(_runs(10.0, 12.0, 11.0)) == {"run_medians_us": [10.0, 12.0, 11.0], "median": 11.0, "min": 10.0, "max": 12.0}
    for mine, inside, minus in ((11.5, True, 0.5), (10.0, True, -1.0), (12.0, True, 1.0), (12.01, False, 1.01), (9.99, False, -1.01)):
        step = bk.spreads({"parent_without": _runs(10.0, 12.0, 11.0), "without": _runs(mine), "with": []})
        assert sorted(step) == ["parent_without", "without"]                       # a side without runs is left out
        bk.against_parent(step, "without", "parent_without", "without_")
        assert step["without_inside_parents_own_spread"] is inside, mine            # both ends of the parent's spread count as inside
        assert step["without_minus_parent_median_us"] == minus
    step = bk.against_parent(bk.spreads({"parent": _runs(5.0), "this_library": _runs(5.0)}), "this_library", "parent", "")
    assert step["inside_parents_own_spread"] is True and step["minus_parent_median_us"] == 0.0
    alone = bk.against_parent(bk.spreads({"parent": [], "this": _runs(5.0)}), "this", "parent", "this_")
    assert sorted(alone) == ["this"]                                                # no parent: nothing is said about one
    assert bk.pooled(_runs(10.0, 12.0)) == {"us_per_step": [10.0] * 3 + [12.0] * 3, "median": 11.0, "spread_us": 2.0}


def test_alternate_starts_the_parent_first_every_turn():
    order = []
    runs = bk.alternate(3, {"parent": lambda: order.append("p") or "P", "this": lambda: order.append("t") or "T", "absent": None})
    assert order == ["p", "t"] * 3
    assert runs == {"parent": ["P"] * 3, "this": ["T"] * 3, "absent": []}


TRACE = """"Kind","Agent_Id","Kernel_Name","Start_Timestamp","End_Timestamp"
"KERNEL_DISPATCH",1,"k_attitude_ground(float*, int)",3000,4500
"KERNEL_DISPATCH",1,"void k_x<true>(int, float*)",2000,2250
"KERNEL_DISPATCH",1,"k_attitude(Params)",1000,1100
"KERNEL_DISPATCH",1,"k_other(int)",500,600
"KERNEL_DISPATCH",1,"k_attitude(Params)",5000,5200
"""
STATS = """"Name","Calls","TotalDurationNs","AverageNs","Percentage","MinNs","MaxNs","StdDev"
"void k_x<true>(int, float*)",4,8000,2000,40.0,1500,2500,1.0
"k_attitude_ground(float*, int)",2,3000,1500,15.0,1400,1600,1.0
"k_attitude(Params)",10,9000,900,45.0,800,1000,1.0
"""


def _profile(tmp_path, name, text):
    d = tmp_path / "prof" / "host" / "1234"                                          # (rocprofv3 nests its files below -d)
    d.mkdir(parents=True, exist_ok=True)
    (d / name).write_text(text)
    return str(tmp_path / "prof")


def test_kernel_trace_rows(tmp_path):
    d = _profile(tmp_path, "1234_kernel_trace.csv", TRACE)
    names = ("k_attitude_ground", "k_attitude", "k_x")
    assert bk.kernel_trace_rows(d, names) == [(1000, "k_attitude", 0.1), (2000, "k_x", 0.25), (3000, "k_attitude_ground", 1.5), (5000, "k_attitude", 0.2)]
    # a name that is a prefix of another: the order of `names` decides without `exact`, the name itself with it
    assert [r[1] for r in bk.kernel_trace_rows(d, ("k_attitude", "k_attitude_ground"))] == ["k_attitude"] * 3
    exact = bk.kernel_trace_rows(d, ("k_attitude", "k_attitude_ground"), exact=True)
    assert [(r[0], r[1]) for r in exact] == [(1000, "k_attitude"), (3000, "k_attitude_ground"), (5000, "k_attitude")]
    assert bk.kernel_trace_rows(d, ("k_x<true>",), exact=True) == [(2000, "k_x<true>", 0.25)]      # behind its return type
    assert bk.kernel_trace_rows(str(tmp_path / "nothing here"), names) == []


def test_kernel_stats(tmp_path):
    d = _profile(tmp_path, "1234_kernel_stats.csv", STATS)
    ground = {"calls": 2, "avg_us": 1.5, "min_us": 1.4, "max_us": 1.6}
    assert bk.kernel_stats(d) == {"void k_x<true>": {"calls": 4, "avg_us": 2.0, "min_us": 1.5, "max_us": 2.5}, "k_attitude_ground": ground,
                                  "k_attitude": {"calls": 10, "avg_us": 0.9, "min_us": 0.8, "max_us": 1.0}}
    assert bk.kernel_stats(d, ("k_attitude_ground",)) == {"k_attitude_ground": ground}
    assert sorted(bk.kernel_stats(d, ("k_attitude",))) == ["k_attitude", "k_attitude_ground"]
    assert list(bk.kernel_stats(d, ("k_x",), strip_args=False)) == ["void k_x<true>(int, float*)"]
    assert bk.kernel_stats(d, ("k_x",), total=True)["void k_x<true>"]["total_us"] == 8.0
    assert bk.kernel_stats(str(tmp_path / "nothing here")) == {}


CHILD = """import json, sys, time
mode, args = sys.argv[2], sys.argv[3:]
assert sys.argv[1] == "--child"
if mode == "noisy":
    print("warming up")
    print('RESULT {"n": 1}')
    print("RESULT looks like one but comes before the last")
    print("RESULT " + json.dumps({"n": 2, "args": args}))
    print("done")
elif mode == "fails":
    sys.stderr.write("the reason it failed\\n")
    sys.exit(3)
elif mode == "sleeps":
    time.sleep(60)
elif mode == "silent":
    print("no record")
"""


@pytest.fixture
def script(tmp_path):
    p = tmp_path / "child.py"
    p.write_text(CHILD)
    return str(p)


def test_spawn_takes_the_last_result_line(script):
    assert bk.spawn(script, "noisy", ("m256", 3), 30) == {"n": 2, "args": ["m256", "3"]}
    with pytest.raises(SystemExit, match="no RESULT line"):
        bk.spawn(script, "silent", (), 30)


def test_a_failing_child_ends_the_run(script):
    started = []

    def sequence():
        for mode in ("noisy", "fails", "noisy"):
            started.append(mode)
            bk.spawn(script, mode, ("a",), 30)
    with pytest.raises(SystemExit) as e:
        sequence()
    text = str(e.value)
    assert "fails" in text and "exit status 3" in text and "the reason it failed" in text and "nothing more is started" in text
    assert started == ["noisy", "fails"]                                            # the child queued behind the failure never starts


def test_a_child_past_its_time_limit(script):
    t0 = time.monotonic()
    with pytest.raises(SystemExit) as e:
        bk.spawn(script, "sleeps", (), 1)
    assert time.monotonic() - t0 < 1 + 10                                          # the limit and the grace before the kill
    assert "exit status 124" in str(e.value) and "the time limit of 1 s" in str(e.value) and "nothing more is started" in str(e.value)


def test_what_the_other_endings_are_called():
    assert "time limit" in bk.ENDINGS[124] and "time limit" in bk.ENDINGS[137]
    assert bk.ENDINGS[134] == "abort" and bk.ENDINGS[139] == "segmentation fault"


def test_the_command_line_of_a_child():
    program = ["python3", "tool.py", "--child", "call", "m256", "1"]
    assert bk.command(program, 300) == ["timeout", "-k", "10", "300"] + program
    cmd = bk.command(program, 400, profile_dir="/tmp/p")
    assert cmd[:4] == ["timeout", "-k", "10", "400"] and cmd[4:6] == ["rocprofv3", "--kernel-trace"]
    assert cmd[cmd.index("--") + 1:] == program and cmd[cmd.index("-d") + 1] == "/tmp/p"
    assert "--stats" not in cmd and "--pmc" not in cmd and cmd[cmd.index("--output-format") + 1] == "csv"
    with_stats = bk.command(program, 900, profile_dir="/tmp/p", stats=True)
    assert with_stats[:7] == ["timeout", "-k", "10", "900", "rocprofv3", "--kernel-trace", "--stats"] and with_stats[with_stats.index("--") + 1:] == program


CONFIGS = {"m256": 60, "c4": 24}


def test_read_args_spellings_and_defaults():
    d = bk.read_args([], configs=CONFIGS, turns=5)
    assert d == {"parent": None, "resources": False, "configs": ["m256", "c4"], "turns": 5, "path": None}
    d = bk.read_args(["--resources", "--parent", "p.so", "--configs", "c4", "out.json"], configs=CONFIGS, turns=5)
    assert d == {"parent": "p.so", "resources": True, "configs": ["c4"], "turns": 5, "path": "out.json"}
    # options in any place, as align_bench, raycast_bench and product_calls_ab took them
    d = bk.read_args(["out.json", "--turns", "9", "--parent", "p.so"], has_resources=False, turns=5)
    assert (d["parent"], d["turns"], d["path"], d["resources"]) == ("p.so", 9, "out.json", False)
    # the parent as the first word: device_products_bench, multi_origin_bench, range_image_bench
    d = bk.read_args(["p.so", "out.json", "--regs", "r.json"], positional_parent=True, has_resources=False, turns=3, extra={"--regs": (None, str)})
    assert (d["parent"], d["path"], d["regs"], d["turns"]) == ("p.so", "out.json", "r.json", 3)
    assert bk.read_args(["p.so"], positional_parent=True, turns=2)["path"] is None
    # a tool's own options: atlas_field_bench, atlas_frontier_bench
    ints = lambda s: [int(v) for v in s.split(",")]
    d = bk.read_args(["--sides", "1024", "--step-configs", "m256"], configs=CONFIGS, turns=5,
                     extra={"--sides": ([1024, 4096], ints), "--step-configs": (None, lambda s: s.split(","))})
    assert d["sides"] == [1024] and d["step_configs"] == ["m256"] and d["configs"] == ["m256", "c4"]
    # clearance_bench, costfield_bench: an output path, and now the configs
    assert bk.read_args(["out.json"], has_parent=False, has_resources=False, configs=CONFIGS)["path"] == "out.json"


# tool: (its configs in order, its alternating runs, its time limit per child in seconds): what a run without options does, and the
# limits none of which may get shorter
TOOLS = {"align_bench": (["m256", "c4"], 2, 900), "atlas_bench": (["m256", "c4"], 5, 300), "atlas_field_bench": (["m256", "c4"], 5, 400),
         "atlas_frontier_bench": (["m256", "c4"], 5, 400), "attitude_bench": (["m256", "c4"], 5, 420), "attitude_volume_bench": (["m256", "c4"], 5, 300),
         "clearance_bench": (["m256", "c4", "c5"], None, 900), "costfield_bench": (["m256", "c4", "c5"], None, 900),
         "device_products_bench": (None, 2, 900), "frontier_bench": (["m256", "c4", "c5"], 5, 300), "multi_origin_bench": (None, 3, 600),
         "posefield_bench": (["m256", "c4"], 5, 300), "range_image_bench": (None, 2, 600), "raycast_bench": (["m256", "c4"], None, 900),
         "rollouts_bench": (["m256", "c4"], 2, 900), "viewpoint_bench": (["m256", "c4"], 5, 300), "product_calls_ab": (None, 5, 600)}


@pytest.mark.parametrize("tool", sorted(TOOLS))
def test_a_run_without_options_does_what_the_tool_did(tool):
    configs, turns, limit = TOOLS[tool]
    mod = __import__(tool)
    assert mod.CHILD_TIMEOUT == limit                                               # no limit got shorter
    assert getattr(mod, "TURNS", None) == turns
    has = getattr(mod, "CONFIGS", None) or getattr(mod, "STEP_CONFIGS", None)
    assert (list(has) if has else None) == configs
    d = bk.read_args([], configs=has, turns=turns)
    assert d.get("configs") == configs and d.get("turns") == turns
    for name in ("_median", "_gvom", "_spawn", "resources"):
        assert not hasattr(mod, name), name


def test_read_args_refuses_what_it_does_not_know():
    for argv, kw in ((["--config", "m256"], {}), (["--bogus"], {}), (["--turns", "2"], {"turns": None}), (["--resources"], {"has_resources": False}),
                     (["--parent", "p.so"], {"has_parent": False}), (["a.json", "b.json"], {}), (["--configs", "c9"], {}), (["--configs"], {}),
                     (["--turns", "0"], {}), ([], {"positional_parent": True})):
        with pytest.raises(SystemExit):
            bk.read_args(argv, **dict({"configs": CONFIGS, "turns": 5}, **kw))


def test_report_loads_keeps_and_saves(tmp_path):
    path = str(tmp_path / "sub" / "out.json")
    os.makedirs(os.path.dirname(path))
    with open(path, "w") as f:
        json.dump({"library": {"lib_sha256": "stale"}, "configs": {"c4": {"kept": 1}}, "not_measured": ["as recorded"]}, f)
    report = bk.Report("stem", path)
    assert report.out["configs"] == {"c4": {"kept": 1}}
    assert report.out["library"] != {"lib_sha256": "stale"} and "source_sha256" in report.out["library"]
    report.not_measured(["a default"])
    assert report.out["not_measured"] == ["as recorded"]                            # the default gives way to what the file says
    configs = report.section("configs")
    for part in ("call", "step"):                                                   # valid JSON after every part
        configs.setdefault("m256", {})[part] = {"us": 1.0}
        report.save()
        on_disk = json.load(open(path))
        assert on_disk["configs"]["c4"] == {"kept": 1} and part in on_disk["configs"]["m256"]
    assert bk.Report("stem", path, fresh=True).out.keys() == {"library"}
    other = bk.Report("stem", str(tmp_path / "new" / "o.json"))                     # its directory is made
    assert other.section("events", measured=False) == "not measured" and json.load(open(other.path))["events"] == "not measured"
    assert isinstance(other.section("configs"), dict)
    default = bk.Report("atlas", None).path
    assert os.path.dirname(default) == os.path.join(ROOT, "profiles") and os.path.basename(default).startswith("atlas_")
