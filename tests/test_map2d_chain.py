"""k_map2d's chain -- staging, the ring search under the density loads, the early stores, the count published at the corner
workgroup's end -- held to the CPU oracle on every output route, after every one of six combines of a moving window.

The scenes are tests/map2d_chain_scenes.py; that they reach the ring search at every depth and at every window edge, density
windows of two load rounds, slope-only positives and runs that turn default and back is asserted on the oracle alone by
tests/test_map2d_chain_cpu.py.  The referee is computed once per grid and shared.  Integer maps are exact; roughness and the
slopes are within 1e-5, the tolerance tests/test_hip_parity.py uses for the same maps (log / atan2 may differ from glibc in the
last ulp); heights, inferred heights and the guessed delta are exact (parity.compare_records).

Routes: combine_maps() into one recurring pinned buffer (the DELTA form; its record's stored runs are the oracle's), the same
with delta_out 0, combine_maps_device() (all nine maps), combine_maps_occupancy(), two thread-ranks of a sharded map
(GATHERED_POS, row-major), and combine_maps_async()."""
import contextlib
import io

import numpy as np
import pytest

import map2d_chain_scenes as mc
import obstacle_scenes as ob
import parity
from oracle import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gvom_mod():
    import gvom
    rc, info = gvom.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    return gvom


def _steps(name):
    return enumerate(zip(mc.scans(name), mc.referee(name)))


def _hold_maps(got, rec, what, cell_count=None):
    want = rec["maps"]
    assert got is not None, what
    assert np.array_equal(np.asarray(got[0]), want[0]), what + ": origin"
    for j, name in ((1, "positive"), (2, "negative"), (4, "visibility")):
        a = np.asarray(got[j])
        assert a.dtype == np.int32 and a.shape == want[j].shape, (what, name)
        assert np.array_equal(a, want[j]), "%s: %s map differs in %d cells, first at %s" % (
            what, name, int(np.sum(a != want[j])), np.argwhere(a != want[j])[:4].tolist())
    r = np.asarray(got[3])
    assert r.dtype == np.float64 and r.shape == want[3].shape, what
    np.testing.assert_allclose(r, want[3], rtol=0, atol=1e-5, err_msg=what + ": roughness")
    if cell_count is not None:
        assert cell_count == rec["cell_count"], (what, cell_count, rec["cell_count"])


def _hold_attributes(source, rec, what):
    got = {a: getattr(source, a).copy_to_host() for a in mc.ATTRIBUTES}
    assert parity.compare_records(got, {a: rec[a] for a in got}, float_tol=1e-5) == len(mc.ATTRIBUTES), what


def _record_runs(bits):
    """record bytes [tiles, 8 waves] -> set bits per map (waves 0-3: visibility, roughness; waves 4-7: positive, negative)"""
    b = bits.reshape(-1, 8)
    a, r = b[:, :4], b[:, 4:]
    cnt = lambda x, mask: int(np.unpackbits(x & mask).sum())
    return {"visibility": cnt(a, 0x3), "roughness": cnt(a, 0xC), "positive": cnt(r, 0x3), "negative": cnt(r, 0xC)}


@pytest.mark.parametrize("name", ["g64", "g96"])
def test_recurring_buffer(gvom_mod, name):
    """DELTA: the pool hands the one buffer back at every combine; what is stored is what changed, what is read is the map"""
    g = gvom_mod.Gvom(*mc.params(name), voxel_statistics=False)
    assert g.get_tuning("delta_out") == 1
    prev, gen0, address = None, None, None
    for k, ((pc, ego), rec) in _steps(name):
        what = "%s delta combine %d" % (name, k)
        g.process_pointcloud(pc, ego)
        out = g.combine_maps()
        _hold_maps(out, rec, what, g.combined_cell_count_cpu)
        _hold_attributes(g, rec, what)
        here = out[1].__array_interface__["data"][0]
        assert address in (None, here), what + ": the buffer did not come back"
        address = here
        bits, gen = g.output_record(out[1])
        bits = bits.copy()
        now = _record_runs(bits)
        want_now = {m: int((~rec["default_runs"][i]).sum()) for i, (m, _) in enumerate(mc.MAPS)}
        print(what, "non-default runs", now)
        assert now == want_now, (what, now, want_now)
        if prev is not None:
            assert gen == gen0, what + ": the record restarted"
            stored = _record_runs(bits | prev)
            print(what, "stored runs", stored)
            assert stored == mc.stored_runs(name, k), (what, stored, mc.stored_runs(name, k))
        prev, gen0 = bits, gen
        del out
    assert g.get_tuning("output_records") == 1


def test_without_delta(gvom_mod):
    name = "g64"
    g = gvom_mod.Gvom(*mc.params(name), voxel_statistics=False)
    g.set_tuning("delta_out", 0)
    for k, ((pc, ego), rec) in _steps(name):
        what = "%s delta_out=0 combine %d" % (name, k)
        g.process_pointcloud(pc, ego)
        out = g.combine_maps()
        _hold_maps(out, rec, what, g.combined_cell_count_cpu)
        _hold_attributes(g, rec, what)
        assert g.output_record(out[1]) is None
        del out


@pytest.mark.parametrize("name", ["g64", "g96"])
def test_device_map_set(gvom_mod, name):
    g = gvom_mod.Gvom(*mc.params(name), voxel_statistics=False)
    for k, ((pc, ego), rec) in _steps(name):
        what = "%s device combine %d" % (name, k)
        g.process_pointcloud(pc, ego)
        m = g.combine_maps_device()
        assert m is not None, what
        _hold_maps((m.origin, m.positive.copy_to_host(), m.negative.copy_to_host(), m.roughness.copy_to_host(),
                    m.visibility.copy_to_host()), rec, what, g.combined_cell_count_cpu)
        _hold_attributes(m, rec, what + " (the set)")
        m.release()
        _hold_attributes(g, rec, what)


def test_occupancy_grids(gvom_mod):
    name, setting = "g64", ob.OCCUPANCY_SETTINGS[1]
    g = gvom_mod.Gvom(*mc.params(name), voxel_statistics=False)
    for k, ((pc, ego), rec) in _steps(name):
        what = "%s occupancy combine %d" % (name, k)
        g.process_pointcloud(pc, ego)
        got = g.combine_maps_occupancy(*setting)
        want = rec["occupancy"]
        assert np.array_equal(got[0], rec["maps"][0]), what
        for plane, a, w in zip(("hard", "soft", "certainty", "negative"), got[1:5], want[:4]):
            assert a.dtype == np.int8 and np.array_equal(a, w), "%s: %s plane differs in %d cells" % (what, plane, int(np.sum(a != w)))
        # the roughness plane truncates the rescaled roughness: what a roughness within 1e-5 of the referee's can give
        origin, pos, neg, rough, vis = rec["maps"]
        allowed = [oracle.ros_occupancy_grids((origin, pos, neg, rough + d, vis), *setting)[4] for d in (-1e-5, 0.0, 1e-5)]
        r = got[5]
        assert r.dtype == np.int8 and np.all((r == allowed[0]) | (r == allowed[1]) | (r == allowed[2])), what + ": roughness plane"
        assert g.combined_cell_count_cpu == rec["cell_count"], what
        _hold_attributes(g, rec, what)
        del got


def test_two_sharded_ranks(gvom_mod):
    from shard_threads import run_ranks
    name, world = "g64", 2
    recs = mc.referee(name)

    def body(r, sh):
        out = []
        for pc, ego in mc.scans(name):
            sh.process_pointcloud(np.ascontiguousarray(pc[r::world]), ego)
            maps = sh.combine_maps()
            out.append((tuple(np.array(m, order="K", copy=True) for m in maps), sh.combined_cell_count_cpu))
        return out

    with contextlib.redirect_stdout(io.StringIO()):
        results = run_ranks(world, mc.params(name), body)
    for r in range(world):
        for k, rec in enumerate(recs):
            maps, cells = results[r][k]
            _hold_maps(maps, rec, "%s, 2 ranks, rank %d, combine %d" % (name, r, k), cells)


def test_asynchronous_result(gvom_mod):
    name = "g64"
    g = gvom_mod.Gvom(*mc.params(name), voxel_statistics=False)
    for k, ((pc, ego), rec) in _steps(name):
        what = "%s async combine %d" % (name, k)
        g.process_pointcloud(pc, ego)
        out = g.combine_maps_async().result()
        _hold_maps(out, rec, what, g.combined_cell_count_cpu)
        _hold_attributes(g, rec, what)
        del out
