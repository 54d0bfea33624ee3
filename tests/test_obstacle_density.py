"""The positive-obstacle density (gvom.py:502-521: k_map2d role B, and k_posdens on sharded maps) against the CPU oracle on
scenes that HAVE densities, on every route that emits the map.

The scenes and the branch census are tests/obstacle_scenes.py; that they reach the branches -- hundreds of cells with a
density, most of them strictly between 0 and 100, windows of 15, 25 and 30 levels (a second, third and fourth round of the
kernels' eight-level loop, each ending in padding lanes), hit counts of exactly 10 and 11, a gate that rejects a thousand valid
cells, a window that has moved on all three storage axes -- is asserted on the oracle alone by tests/test_obstacle_density_cpu.py.

The referee is oracle.OracleGvom fed the same clouds (computed once per grid, shared): positive, negative and visibility maps,
origin and fused cell count exact, roughness within the project's 1e-5, the debug rows through parity.compare_records.  A
positive map that differs is reported with the cell, its window and the hit and total counts the referee summed."""
import contextlib
import io

import numpy as np
import pytest

import obstacle_scenes as ob
import parity
from oracle import oracle

pytestmark = pytest.mark.gpu

# gvom_get_tuning("fuse_kernel") (include/gvom_hip.h)
FUSE1, FUSE4_2, FUSE4_4, FUSE_SHORT, FUSE_TALL, ENCFUSE = 1, 2, 3, 4, 5, 6
ATTRIBUTES = ("height_map", "inferred_height_map", "x_slope_map", "y_slope_map", "guessed_height_delta", "roughness_map")


@pytest.fixture(scope="module")
def gvom_mod():
    import gvom
    rc, info = gvom.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    return gvom


def _route(name, k):
    """the fusion kernel whose rows the density of combine k reads"""
    if name == "tall":
        return FUSE_TALL                                   # 19-level chunks
    if name == "ragged":
        return FUSE_SHORT                                  # xy_size % 4 != 0
    if ob.GRIDS[name][4] == 1:
        return ENCFUSE                                     # one-slot ring, xy_size % 16 == 0: the adopted eager fusion
    return FUSE1 if k == 0 else FUSE4_2                    # two_rounds: one filled slot, then two


def _hold_positive(got, rec, what):
    got, want = np.asarray(got), rec["maps"][1]
    assert got.shape == want.shape and got.dtype == np.int32, (what, got.shape, got.dtype)
    if not np.array_equal(got, want):
        text = "%s: %s" % (what, ob.explain_mismatch(rec["census"], got, want))
        print(text)
        raise AssertionError(text)


def _hold_maps(got, rec, what, cell_count=None):
    """what combine_maps() returns, against the referee's"""
    want = rec["maps"]
    assert got is not None, what
    assert np.array_equal(np.asarray(got[0]), want[0]), what + ": origin"
    _hold_positive(got[1], rec, what)
    for j, name in ((2, "negative"), (4, "visibility")):
        a = np.asarray(got[j])
        assert a.dtype == np.int32 and np.array_equal(a, want[j]), "%s: %s map differs in %d cells" % (what, name, int(np.sum(a != want[j])))
    r = np.asarray(got[3])
    assert r.dtype == np.float64 and r.shape == want[3].shape
    np.testing.assert_allclose(r, want[3], rtol=0, atol=1e-5, err_msg=what + ": roughness")
    if cell_count is not None:
        assert cell_count == rec["cell_count"], (what, cell_count, rec["cell_count"])


def _hold_attributes(g, rec, what):
    """the 2-D attributes and the debug rows, through parity's comparison (heights and the guessed delta exact, slopes and
    roughness 1e-5)"""
    got = {name: getattr(g, name).copy_to_host() for name in ATTRIBUTES}
    got["debug_height_map"] = g.make_debug_height_map()
    got["debug_inferred_height_map"] = g.make_debug_inferred_height_map()
    want = {name: rec[name] for name in got}
    assert parity.compare_records(got, want, float_tol=1e-5) == len(got), what


def _hold_fused(gvom_mod, g, rec, what):
    """the fused map densely: a density that differs with THIS equal is the 2-D stage's, not the fusion's"""
    got = g.read_dense(gvom_mod.GVOM_WHICH_FUSED)
    for j, name in enumerate(("state", "hit", "total", "min-height")):
        assert np.array_equal(rec["fused_dense"][j], got[j]), "%s: fused %s differs in %d voxels" % (
            what, name, int(np.sum(rec["fused_dense"][j] != got[j])))


def _steps(name):
    return enumerate(zip(ob.scans(name), ob.referee(name)))


# ---- 1, 4. the pipeline, the density read from the rows of every fusion kernel -------------------------------------------------

@pytest.mark.parametrize("name", ["one_round", "two_rounds", "four_rounds", "gate", "ragged", "tall"])
def test_pipeline_on_every_fusion_route(gvom_mod, name):
    """three scans, a combine after each: k_map2d<., YX> into pinned host memory.  one_round / four_rounds / gate: rows written
    by the eager k_encfuse; two_rounds: k_fuse1, then k_fuse4<2>; ragged: k_fuse, short chunks; tall (32 x 32 x 300): k_fuse,
    tall chunks."""
    g = gvom_mod.Gvom(*ob.params(name), voxel_statistics=False)
    for k, ((pc, ego), rec) in _steps(name):
        what = "%s combine %d" % (name, k)
        g.process_pointcloud(pc, ego)
        _hold_maps(g.combine_maps(), rec, what, g.combined_cell_count_cpu)
        assert g.get_tuning("fuse_kernel") == _route(name, k), (what, g.get_tuning("fuse_kernel"), _route(name, k))
        assert np.array_equal(g.combined_origin.copy_to_host(), rec["combined_origin"]), what
        _hold_attributes(g, rec, what)
    _hold_fused(gvom_mod, g, rec, what)
    if _route(name, 0) == ENCFUSE:
        assert g.get_tuning("eager_adopted") == ob.N_SCANS


# ---- 2. the output forms of k_map2d ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["two_rounds", "ragged"])
def test_row_major_form(gvom_mod, name):
    """c_order=True: k_map2d<., !YX>, 8 x 32 tiles transposed through LDS into C-contiguous arrays"""
    g = gvom_mod.Gvom(*ob.params(name), voxel_statistics=False, c_order=True)
    for k, ((pc, ego), rec) in _steps(name):
        what = "%s c_order combine %d" % (name, k)
        g.process_pointcloud(pc, ego)
        got = g.combine_maps()
        assert all(np.asarray(m).flags.c_contiguous for m in got[1:]), what
        _hold_maps(got, rec, what, g.combined_cell_count_cpu)
        _hold_attributes(g, rec, what)
    _hold_fused(gvom_mod, g, rec, what)


@pytest.mark.parametrize("name", ["two_rounds", "ragged"])
def test_asynchronous_form(gvom_mod, name):
    """combine_maps_async(): fusion and k_map2d on the second stream, no completion flag"""
    g = gvom_mod.Gvom(*ob.params(name), voxel_statistics=False)
    for k, ((pc, ego), rec) in _steps(name):
        what = "%s async combine %d" % (name, k)
        g.process_pointcloud(pc, ego)
        pending = g.combine_maps_async()
        _hold_maps(pending.result(), rec, what, g.combined_cell_count_cpu)
        _hold_attributes(g, rec, what)
    _hold_fused(gvom_mod, g, rec, what)


@pytest.mark.parametrize("name", ["two_rounds", "ragged"])
def test_device_map_set(gvom_mod, name):
    """combine_maps_device(): k_map2d<., YX, DEV>, all nine maps of the set read back from device memory"""
    g = gvom_mod.Gvom(*ob.params(name), voxel_statistics=False)
    for k, ((pc, ego), rec) in _steps(name):
        what = "%s device combine %d" % (name, k)
        g.process_pointcloud(pc, ego)
        m = g.combine_maps_device()
        assert m is not None, what
        _hold_maps((m.origin, m.positive.copy_to_host(), m.negative.copy_to_host(), m.roughness.copy_to_host(),
                    m.visibility.copy_to_host()), rec, what, g.combined_cell_count_cpu)
        got = {a: getattr(m, a).copy_to_host() for a in ATTRIBUTES if a != "roughness_map"}
        assert len(got) == 5 and parity.compare_records(got, {a: rec[a] for a in got}, float_tol=1e-5) == 5, what
        m.release()
        _hold_attributes(g, rec, what)                       # the storage-order maps are written as on every other path
    _hold_fused(gvom_mod, g, rec, what)


def _hold_occupancy(got, rec, setting, what, last):
    c, xy = rec["census"], rec["census"]["xy"]
    want = rec["occupancy"][setting]
    assert np.array_equal(got[0], rec["maps"][0]), what + ": origin"
    for name, a, w in zip(("hard", "soft", "certainty", "negative"), got[1:5], want[:4]):
        assert a.dtype == np.int8 and a.shape == w.shape, (what, name)
        if not np.array_equal(a, w):
            bad = np.nonzero(a != w)[0]
            text = "%s: %s plane differs in %d cells\n%s" % (what, name, len(bad), "\n".join(
                "  got %d, referee %d, positive %d -- %s" % (a[i], w[i], rec["maps"][1][i % xy, i // xy], ob.explain(c, i % xy, i // xy))
                for i in bad[:6]))
            print(text)
            raise AssertionError(text)
    # the roughness plane is a truncation of the rescaled roughness: what a roughness within 1e-5 of the referee's can give
    origin, pos, neg, rough, vis = rec["maps"]
    allowed = [oracle.ros_occupancy_grids((origin, pos, neg, rough + d, vis), *setting)[4] for d in (-1e-5, 0.0, 1e-5)]
    assert np.array_equal(allowed[1], want[4])
    r = got[5]
    assert r.dtype == np.int8 and np.all((r == allowed[0]) | (r == allowed[1]) | (r == allowed[2])), what + ": roughness plane"
    # cells of both planes that are set from a DENSITY on either side of the threshold, not from the slope
    thr = setting[0]
    soft = int(np.sum((got[2] == 100) & np.reshape(ob.density_mask(c, 0, thr), -1, order="F")))
    hard = int(np.sum((got[1] == 100) & np.reshape(ob.density_mask(c, thr, 100), -1, order="F")))
    assert soft == int(ob.density_mask(c, 0, thr).sum()) and hard == int(ob.density_mask(c, thr, 100).sum()), (what, soft, hard)
    if last:
        assert soft >= 20 and hard >= 20, (what, soft, hard)


@pytest.mark.parametrize("setting", ob.OCCUPANCY_SETTINGS, ids=["defaults", "threshold12.5"])
@pytest.mark.parametrize("name", ["two_rounds", "ragged"])
def test_occupancy_form(gvom_mod, name, setting):
    """combine_maps_occupancy(): the P.occ branch -- five int8 planes thresholded in the kernel -- synchronous, and on a second
    handle through combine_maps_occupancy_async()"""
    g, a = (gvom_mod.Gvom(*ob.params(name), voxel_statistics=False) for _ in range(2))
    for k, ((pc, ego), rec) in _steps(name):
        what = "%s occupancy %r combine %d" % (name, setting, k)
        g.process_pointcloud(pc, ego)
        a.process_pointcloud(pc, ego)
        _hold_occupancy(g.combine_maps_occupancy(*setting), rec, setting, what, k == ob.N_SCANS - 1)
        _hold_occupancy(a.combine_maps_occupancy_async(*setting).result(), rec, setting, what + " (async)", k == ob.N_SCANS - 1)
        assert g.combined_cell_count_cpu == a.combined_cell_count_cpu == rec["cell_count"], what
        _hold_attributes(g, rec, what)


# ---- 3. sharded maps: k_posdens on the owner's rows, k_map2d<GATHERED_POS, YX> on every rank --------------------------------------

@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("name", ["two_rounds", "gate"])
def test_sharded_ranks_against_the_referee(name, world):
    """thread-ranks on one GPU (tests/shard_threads.py), every rank a strided share of each scan: the density of a cell is
    computed by the rank that owns its storage row (k_posdens) and travels with the heights; EVERY rank's returned maps --
    indexed [x, y], and flattened x-fastest as the node publishes them -- are the referee's.  Every rank's slab holds density
    cells (>= 20 at the last combine), so that no rank's k_posdens passes on zeros."""
    from shard_threads import run_ranks
    recs = ob.referee(name)
    for k, rec in enumerate(recs):
        per_rank = ob.cells_per_slab(rec["census"], rec["combined_origin"][1], world)
        assert per_rank.min() >= (20 if k == ob.N_SCANS - 1 else 1), (name, world, k, per_rank)

    def body(r, sh):
        out = []
        for pc, ego in ob.scans(name):
            sh.process_pointcloud(np.ascontiguousarray(pc[r::world]), ego)
            maps = sh.combine_maps()
            out.append((tuple(np.array(m, order="K", copy=True) for m in maps), sh.combined_cell_count_cpu))
        return out

    with contextlib.redirect_stdout(io.StringIO()):
        results = run_ranks(world, ob.params(name), body)
    for r in range(world):
        for k, rec in enumerate(recs):
            what = "%s, %d ranks, rank %d, combine %d" % (name, world, r, k)
            maps, cells = results[r][k]
            _hold_maps(maps, rec, what, cells)
            for j in (1, 2, 4):
                assert np.array_equal(np.reshape(maps[j], -1, order="F"), np.reshape(rec["maps"][j], -1, order="F")), what


# ---- 5. with the per-voxel statistics on: the density reads the rows whose layout the statistics path shares ---------------------

def test_with_voxel_statistics(gvom_mod):
    name = "one_round"
    g = gvom_mod.Gvom(*ob.params(name), voxel_statistics=True)
    w = oracle.OracleGvom(*ob.params(name), voxel_statistics=True)
    for k, ((pc, ego), rec) in _steps(name):
        what = "%s statistics combine %d" % (name, k)
        g.process_pointcloud(pc, ego)
        w.process_pointcloud(pc, ego)
        got, want = g.combine_maps(), w.combine_maps()
        assert np.array_equal(want[1], rec["maps"][1]) and w.combined_cell_count_cpu == rec["cell_count"]
        _hold_maps(got, rec, what, g.combined_cell_count_cpu)
        assert g.get_tuning("fuse_kernel") == ENCFUSE, what
        parity.compare_statistics(g, w, what=what + ": ")
    _hold_fused(gvom_mod, g, rec, what)
