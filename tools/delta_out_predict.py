#!/usr/bin/env python3
"""tools/delta_out_predict.py CONFIG [CYCLES] -- how many of k_map2d's host-link store runs carry nothing new (CPU only).

Runs the bench's step sequence (synth.config_inputs(CONFIG, n_scans=8), the poses cycled CYCLES times, default 2) through the
CPU oracle and splits every returned map into the store runs of k_map2d's host-output [y][x] form: 32 consecutive cells in x at
fixed y (128 B of an int32 map, 256 B of roughness).  A run is DEFAULT when all its cells hold what a cell without height, without
a valid 3x3 neighbour and without a negative-obstacle verdict gets (visibility 0, positive 0, negative 0, roughness -1.0).  A run
that is default in this step and was default in the previous step AT THE SAME MEMORY POSITION (the window shift between the two
steps is part of the comparison) need not cross the link again.  Prints one JSON object: per step and per map the skippable runs,
and the byte-weighted share over all steps after the first.
"""
import json
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "g-vom_amd"))
sys.path.insert(0, _ROOT)

MAPS = (("positive", 4, 0), ("negative", 4, 0), ("roughness", 8, -1.0), ("visibility", 4, 0))    # name, bytes per cell, default
RUN = 32


def default_runs(a, default):
    """a[x, y] -> bool[xy / RUN, xy]: run (x // RUN, y) holds only `default`."""
    xy = a.shape[0]
    return (a == default).reshape(xy // RUN, RUN, xy).all(axis=1)


def main():
    import synth
    from oracle import oracle
    name = sys.argv[1] if len(sys.argv) > 1 else "m256"
    cycles = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    params, scans = synth.config_inputs(name, n_scans=8)
    xy = params[2]
    if xy % RUN:
        raise SystemExit("xy must be a multiple of %d" % RUN)
    oracle.build()
    oracle.use_all_cores(True)
    g = oracle.OracleGvom(*params)
    prev, steps = None, []
    skipped = {m[0]: 0 for m in MAPS}
    total = {m[0]: 0 for m in MAPS}
    for k in range(cycles * len(scans)):
        pc, ego, tf = scans[k % len(scans)]
        g.process_pointcloud(pc, ego, tf)
        out = g.combine_maps()
        now = {m[0]: default_runs(out[1 + i], m[2]) for i, m in enumerate(MAPS)}
        if prev is not None:
            row = {"step": k, "occupied_columns": int(out[4].sum())}
            for mname, _, _ in MAPS:
                skip = int((now[mname] & prev[mname]).sum())
                row[mname] = {"default_now": int(now[mname].sum()), "skippable": skip}
                skipped[mname] += skip
                total[mname] += now[mname].size
            steps.append(row)
        prev = now
    nsteps = len(steps)
    runs_per_map = (xy // RUN) * xy
    all_bytes = sum(b for _, b, _ in MAPS) * xy * xy
    skip_bytes = sum(skipped[m] * RUN * b for m, b, _ in MAPS) / float(nsteps)
    print(json.dumps({
        "config": name, "grid_xy": xy, "steps_compared": nsteps, "runs_per_map": runs_per_map,
        "share_skippable_per_map": {m: skipped[m] / float(total[m]) for m, _, _ in MAPS},
        "bytes_per_step": all_bytes, "bytes_skippable_per_step_mean": skip_bytes,
        "share_skippable_bytes": skip_bytes / all_bytes,
        "per_step": steps}, indent=1))


if __name__ == "__main__":
    main()
