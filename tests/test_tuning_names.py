"""Every name of gvom_set_tuning and gvom_get_tuning (g-vom_amd/csrc/gvom_handle.hip) answers as recorded: replay() asks gvom_get_tuning
for every name on a fresh mapper, then sets every name to each of VALUES in turn and reads it back, and notes every return code and
value.  tests/tuning_names_recorded.json holds what the library gave before the handle's per-call state was folded into records
(tools/record_tuning_names.py, on the MI355X with the production library of the commit before); the test holds today's library to it
exactly -- the names each function accepts, what each refuses, every clamp and every default.

NAMES is every name either function compares against, and REFUSED a handful both must refuse: the empty string, the two solvers that
have "_tiles" but no readable "_rounds", a known name with a trailing blank, and the two hooks only the test library has.  The mapper
is small (32 x 32 x 8, a one-slot ring, no statistics) and never scans, so "segs", "period", "ep_row", "prio" and "interleave" read the
last scan's values -- none yet -- whatever they were set to."""
import ctypes
import gc
import json
import os

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
RECORDED = os.path.join(HERE, "tuning_names_recorded.json")
PARAMS = (0.4, 0.2, 32, 8, 1, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)       # tests/_frontier_torch.py::PARAMS at 32 cells
VALUES = (-3, 0, 1, 5, 100000)
NAMES = (
    # gvom_set_tuning, in the order of its chain
    "segs", "ep_row", "period", "prio", "interleave", "flag_kernel", "fuse1", "encfuse", "dirsort", "fastdiv", "eager", "delta_out",
    "cost_to_go_inner", "cost_to_go_batch", "frontier_inner", "frontier_batch", "pose_field_inner", "pose_field_batch",
    "viewpoint_bitmap_mb", "voxel_distance_mb", "occupancy_clear", "exported",
    # gvom_get_tuning alone, in the order of its chain
    "eager_adopted", "eager_dropped", "fuse_kernel", "encfuse_width", "encfuse_waves", "device_map_sets", "clearance_allocations",
    "clearance_lgw", "clearance_rows_per_tile", "clearance_lds_bytes", "clearance_chunks", "raycast", "raycast_allocations", "cost_to_go",
    "cost_to_go_allocations", "cost_to_go_tiles", "rollouts", "footprint", "rollout_allocations", "alignments", "attitude", "chassis",
    "attitude_allocations", "body", "body_spheres", "body_allocations", "frontiers", "frontier_allocations", "frontier_rounds",
    "frontier_tiles", "viewpoints", "viewpoint_allocations", "viewpoint_batch", "pose_field", "primitives", "pose_field_allocations",
    "pose_field_rounds", "pose_field_tiles", "atlas", "atlas_cost_to_go", "atlas_field_allocations", "atlas_field_tiles", "atlas_frontiers",
    "atlas_frontier_allocations", "atlas_frontier_rounds", "atlas_frontier_tiles", "attitude_volume", "attitude_volume_allocations",
    "body_volume", "body_volume_allocations", "atlas_allocations", "voxel_atlas", "voxel_atlas_alignments", "voxel_atlas_levels",
    "voxel_atlas_allocations", "voxel_atlas_viewpoint_batch", "voxel_changes", "voxel_distance_field", "voxel_distance_halo_xy",
    "voxel_distance_halo_z", "alignment_allocations", "alignment_grid_bytes", "alignment_points_per_block", "alignment_candidate_group",
    "device_product_sets", "output_records", "multi_origin", "multi_origin_ran", "range_image")
REFUSED = ("", "cost_to_go_rounds", "atlas_field_rounds", "segs ", "churn", "epoch_bias")


def replay(mod):
    """[case, return code, value or None] of every case, in order"""
    g = mod.Gvom(*PARAMS, voxel_statistics=False)
    L, out = g._lib, []

    def get(name):
        v = ctypes.c_int(-12345)
        rc = L.gvom_get_tuning(g._h, name.encode(), ctypes.byref(v))
        return [int(rc), int(v.value) if rc == 0 else None]

    for name in NAMES + REFUSED:
        out.append(["get %r fresh" % name] + get(name))
    settable = []
    for name in NAMES + REFUSED:
        if name == "exported":
            continue                                       # last, and back to 0: a handle that says so parks its regions when it goes
        for v in VALUES:
            rc = L.gvom_set_tuning(g._h, name.encode(), v)
            out.append(["set %r %d" % (name, v), int(rc), None])
            if rc != 0:
                break                                      # refused once, refused for every value: the name is not one of set's
            out.append(["get %r after %d" % (name, v)] + get(name))
        else:
            settable.append(name)
    for v in VALUES + (0,):
        out.append(["set 'exported' %d" % v, int(L.gvom_set_tuning(g._h, b"exported", v)), None])
        out.append(["get 'exported' after %d" % v] + get("exported"))
    assert len(settable) == 21, settable                   # (the 22 names of set's chain, "exported" apart)
    del g
    gc.collect()
    return out


def test_every_tuning_name_answers_as_recorded():
    import gvom as mod
    rc, info = mod.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    with open(RECORDED) as f:
        want = json.load(f)["results"]
    got = replay(mod)
    assert [r[0] for r in got] == [r[0] for r in want]      # the case list is the recorded one
    for g, w in zip(got, want):
        print("%-50s %4d %s" % tuple(g))
        assert g == w, (g, w)
