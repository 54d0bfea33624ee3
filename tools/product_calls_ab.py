#!/usr/bin/env python3
"""Does a change to the host layer of the product calls cost time?  Two builds of the library -- the one before (--parent) and the
tree's own -- alternated in fresh child processes, TURNS turns each, on one machine in one sitting:

  waiting calls  cost_to_go_of, frontiers_of and pose_field_of on 256-cell maps (seeded obstacles, host maps: staged), and the atlas's
                 cost_to_go and its field's frontiers on an extent of 1024 cells: end-to-end wall time per call, median of CALLS calls
                 behind WARM warm-up calls; the calls wait for the GPU themselves
  overhead       raycast (n = 1), the voxel atlas's raycast (n = 1; an atlas of 64 cells and 8 levels) and score_rollouts_of (K = T = 1)
                 on a 16-cell window: wall time per call averaged over MANY calls, behind a gvom sync -- a change in host overhead
                 would show here
  step           bench.py --config m256 and c4: ms per step

Per measurement the median over each library's turns and the parent's own min .. max: the margin a difference is held against.

    tools/product_calls_ab.py --parent PATH/libgvom_hip.so [--turns N] [--sections waiting,overhead,m256,c4] [out.json]
                                                                      (default: 5 turns, every section, profiles/product_calls_<lib sha8>.json)
"""
import json
import os
import sys
import time

import benchkit as bk

sys.path.insert(0, os.path.join(bk.ROOT, "tests"))
TURNS, WARM, CALLS, MANY = 5, 3, 20, 2000
REST = (1, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
SECTIONS = ("waiting", "overhead", "m256", "c4")
CHILD_TIMEOUT = 600                                                        # seconds, per child process and per bench.py run


def child(sections):
    import numpy as np
    import gvom
    import posefield_ref
    out = {}
    rng = np.random.default_rng(7)
    if "waiting" in sections:
        waiting_calls(np, gvom, posefield_ref, rng, out)
    if "overhead" in sections:
        overhead_calls(np, gvom, posefield_ref, rng, out)
    return out


def waiting_calls(np, gvom, posefield_ref, rng, out):
    xy = 256
    g = gvom.Gvom(0.4, 0.2, xy, 8, *REST, voxel_statistics=False)
    cost = np.where(rng.random((xy, xy)) < 0.2, 0, rng.integers(1, 40, (xy, xy))).astype(np.uint16)
    cost[:8, :8] = 1
    vis = (rng.random((xy, xy)) < 0.6).astype(np.int32)
    field = g.cost_to_go_of(cost, [(2, 2)])
    ctg = np.asarray(field.copy_to_host()[0])
    out["cost_to_go_info"] = [int(field.rounds), int(field.reached)]
    field.release()
    out["cost_to_go_m256_ms"] = bk.timed_waiting(lambda: g.cost_to_go_of(cost, [(2, 2)]).release(), WARM, CALLS)
    fr = g.frontiers_of(cost, vis, cost_to_go=ctg)
    out["frontiers_info"] = [fr.rounds, fr.n_clusters, fr.frontier_cells]
    fr.release()
    out["frontiers_m256_ms"] = bk.timed_waiting(lambda: g.frontiers_of(cost, vis, cost_to_go=ctg).release(), WARM, CALLS)
    g.set_footprint(posefield_ref.point_footprint(16))
    g.set_primitives(gvom.arc_primitives(16, 1.0, 0.4))
    pf = g.pose_field_of(cost, [(2, 2)])
    out["pose_field_info"] = [int(pf.rounds), int(pf.reached)]
    pf.release()
    out["pose_field_m256_ms"] = bk.timed_waiting(lambda: g.pose_field_of(cost, [(2, 2)]).release(), WARM, max(5, CALLS // 4))
    del g
    # the atlas: an extent of 1024 cells, one 64-cell window of seen ground in the middle of never-seen ground
    A, w = 1024, 64
    ga = gvom.Gvom(0.4, 0.2, w, 8, *REST, voxel_statistics=False)
    a = ga.create_atlas(A, follow=False, origin_cells=(0, 0))
    maps = [np.zeros((w, w), np.int32) for _ in range(3)] + [np.zeros((w, w), np.float64) for _ in range(6)]
    maps[2][:] = 1                                                         # visibility: seen
    a.integrate_of(maps, (480, 480))
    f = a.cost_to_go([(512, 512)], goals_in_cells=True)
    out["atlas_cost_to_go_info"] = [int(f.rounds), int(f.reached)]
    out["atlas_frontiers_A1024_ms"] = bk.timed_waiting(lambda: f.frontiers(min_cells=1).release(), WARM, CALLS)
    fr = f.frontiers(min_cells=1)
    out["atlas_frontiers_info"] = [fr.rounds, fr.n_clusters, fr.frontier_cells]
    fr.release()
    f.release()
    out["atlas_cost_to_go_A1024_ms"] = bk.timed_waiting(lambda: a.cost_to_go([(512, 512)], goals_in_cells=True).release(), WARM, CALLS)
    del a, ga


def overhead_calls(np, gvom, posefield_ref, rng, out):
    """host overhead: the smallest calls, many of them"""
    s = 16
    gs = gvom.Gvom(0.4, 0.2, s, 8, *REST, voxel_statistics=False)
    pc = np.stack([rng.uniform(-2, 2, 500), rng.uniform(-2, 2, 500), rng.normal(-0.5, 0.2, 500)], axis=1).astype(np.float32)
    gs.process_pointcloud(pc, (0.0, 0.0, 0.0))
    gs.combine_maps()
    gs.set_footprint(posefield_ref.point_footprint(4))
    o, t = np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32)
    small, pose = np.ones((s, s), np.uint16), np.zeros((1, 1, 3), np.float32)

    def many(call):
        for _ in range(50):
            call()
        gs._lib.gvom_sync(gs._h)
        t0 = time.perf_counter()
        for _ in range(MANY):
            call()
        gs._lib.gvom_sync(gs._h)
        return (time.perf_counter() - t0) / MANY * 1e6
    out["raycast_n1_us"] = many(lambda: gs.raycast(o, t).release())
    va = gs.create_voxel_atlas(64, 8)
    va.integrate()
    out["voxel_atlas_raycast_n1_us"] = many(lambda: va.raycast(o, t).release())
    out["score_rollouts_K1T1_us"] = many(lambda: gs.score_rollouts_of(small, pose).release())


def _bench(lib, config, steps, warmup):
    argv = [sys.executable, os.path.join(bk.ROOT, "bench.py"), "--gpus", "1", "--config", config, "--steps", str(steps), "--warmup", str(warmup)]
    out = bk.run(argv, CHILD_TIMEOUT, "bench.py --config %s" % config, lib=lib)
    return json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])["ms_per_step"]


def main():
    if bk.child(sys.argv[1:], {"calls": lambda a: child(a[0].split(","))}):
        return
    import gvom
    args = bk.read_args(sys.argv[1:], has_resources=False, turns=TURNS, extra={"--sections": (list(SECTIONS), lambda s: [v for v in s.split(",") if v])})
    sections = args["sections"]
    if not args["parent"]:
        raise SystemExit("--parent PATH/libgvom_hip.so: the library before")
    libs = {"parent": os.path.abspath(args["parent"]), "tree": os.path.abspath(gvom.library_path())}

    def one(name):
        res = bk.spawn(__file__, "calls", (",".join(sections),), CHILD_TIMEOUT, lib=libs[name])
        if "m256" in sections:
            res["bench_m256_ms_per_step"] = _bench(libs[name], "m256", 300, 60)
        if "c4" in sections:
            res["bench_c4_ms_per_step"] = _bench(libs[name], "c4", 40, 10)
        print(name, json.dumps(res), flush=True)
        return res
    turns = bk.alternate(args["turns"], {name: (lambda name=name: one(name)) for name in libs})      # parent, tree, parent, tree ...
    table = {}
    for key in turns["parent"][0]:
        if key.endswith("_info"):
            assert all(t[key] == turns["parent"][0][key] for name in libs for t in turns[name]), key      # the same solves under both
            table[key] = turns["parent"][0][key]
            continue
        p, t = [x[key] for x in turns["parent"]], [x[key] for x in turns["tree"]]
        table[key] = {"parent_median": bk.median(p), "parent_min": min(p), "parent_max": max(p), "tree_median": bk.median(t), "tree_min": min(t),
                      "tree_max": max(t), "tree_median_inside_parent_spread": min(p) <= bk.median(t) <= max(p)}
    report = bk.Report("product_calls", args["path"], args["parent"], fresh=True)
    report.out.update({"what": __doc__.split("\n\n")[0], "turns": args["turns"], "sections": sections, "calls": CALLS, "many": MANY, "table": table, "runs": turns})
    report.save()
    for key, v in table.items():
        print(key, json.dumps(v))
    print("wrote", report.path)


if __name__ == "__main__":
    main()
