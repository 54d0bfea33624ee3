#!/usr/bin/env python3
"""tools/delta_out_bytes.py CONFIG [STEPS] -- bytes k_map2d stores into the caller's buffer per step (needs the GPU).

Runs the bench's step sequence (synth.config_inputs(CONFIG, n_scans=8), poses cycled) and reads the buffer's content record back
after every combine (gvom_output_record: one bit per map and run of 32 cells, set = the run holds non-default values).  A step
stores the runs that are non-default now or were non-default the step before: the union of two consecutive records, 128 B per
int32 run and 256 B per roughness run.  Prints one JSON object; the CPU prediction is tools/delta_out_predict.py's."""
import json
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "g-vom_amd"))


def per_map(bits):
    """record bytes [tiles, 8 waves] -> set bits per map"""
    b = bits.reshape(-1, 8)
    a, r = b[:, :4], b[:, 4:]
    cnt = lambda x, mask: int(np.unpackbits(x & mask).sum())
    return {"visibility": cnt(a, 0x3), "roughness": cnt(a, 0xC), "positive": cnt(r, 0x3), "negative": cnt(r, 0xC)}


def main():
    import gvom
    import synth
    name = sys.argv[1] if len(sys.argv) > 1 else "m256"
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    params, scans = synth.config_inputs(name, n_scans=8)
    xy = params[2]
    g = gvom.Gvom(*params)
    width = {"visibility": 128, "roughness": 256, "positive": 128, "negative": 128}
    full = 20 * xy * xy
    prev, rows, gen0 = None, [], None
    for k in range(steps):
        pc, ego, tf = scans[k % len(scans)]
        g.process_pointcloud(pc, ego, tf)
        out = g.combine_maps()
        bits, gen = g.output_record(out[1])
        del out
        if prev is not None:
            assert gen == gen0, "the record restarted: the buffer was not recycled"
            stored = per_map(bits | prev)
            rows.append({"step": k, "stored_runs": stored, "stored_bytes": sum(stored[m] * width[m] for m in stored)})
        prev, gen0 = bits, gen
    tail = rows[len(rows) // 2:]
    mean = sum(r["stored_bytes"] for r in tail) / float(len(tail))
    print(json.dumps({"config": name, "grid_xy": xy, "full_store_bytes": full, "steps": steps,
                      "stored_bytes_mean_second_half": mean, "share_skipped": 1.0 - mean / full,
                      "first_steps": rows[:4], "last_steps": rows[-4:]}, indent=1))


if __name__ == "__main__":
    main()
