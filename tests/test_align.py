"""Scan alignment scoring on the GPU (gvom_score_alignments: k_align_field, k_align_score, k_align_best; Gvom.score_alignments,
Gvom.score_alignments_device) against the referee of tests/align_ref.py: counts, scores and the best candidate with tolerance 0 --
everything is integer.  The maps of tests/raycast_ref.py on six grids (a power of two, none, taller than wide, two and three tile
segments per row, a window origin beyond 2^24 voxels) with ring lengths 1 and 2, the cloud of their last scan under 245 candidates
and four specials, dilate 0 and 1; n of 1, 63, 65, 8,192 and one more than the score kernel's returns per workgroup, K of 1, 3 and one
more than its candidate group, through host and device pointers, with weights of both signs up to +-1024; the census floors and the
unique best on the GPU's own maps; snapshots, the map left as it was, the product pool, errors, and a torch consumer in a child
process.  tests/test_align_cpu.py holds the referee's pins and the figures.

That cloud meets the class grid of k_align_field only where the last scan's returns fall.  Two further tests do not depend on where
returns happen to fall.  PLANTED MAPS UNDER LINE PROBES: sparse maps with single occupied voxels on both sides of every 16-voxel word
of a row, on the bottom, middle and top level and on both sides of the boundary between two chunks of levels, on the first and last
row and in the corners -- on six grids, two of them with rows that are no multiple of 16 voxels (72: two tile segments, the second
partial, a half-filled last word; 37: odd) -- and three probes whose counts are the class histogram of every line of the window
along each axis: every voxel of the class grid is held to the referee three times.  tests/test_align_cpu.py shows without a GPU that
these inputs tell eleven plausible defects of the kernel from the referee.  THE SCORE KERNEL AT ITS EDGES: returns on exact voxel
faces and their float32 neighbours, rotations about all three axes, resolutions that are no multiple of anything, through
k_align_score<true> (the verified reciprocals) and k_align_score<false> (the IEEE divide, "fastdiv" knob 0).

Wall time on the MI355X (pytest --durations, one run): the twelve planted cases 0.02 to 0.06 s each but for w128 (0.25 to 0.31 s) and
w192 (0.46 s; its largest probe is 36,864 candidates x 24 returns); the fourteen edge cases 0.01 to 0.07 s each."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import align_ref as ar
import raycast_ref as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = ((1024, -1024, 7, -3, 1), (-1024, 1024, 0, 5, -1024), (0, 0, 0, 0, 0), (-1, -1, -1, -1, -1))


@pytest.fixture(scope="module")
def gvom():
    import gvom as mod
    rc, info = mod.Gvom.backend_info()
    assert rc == 0 and "gfx950" in info, info
    assert mod.PRODUCT_ALIGNMENT == 12
    return mod


@pytest.fixture(scope="module")
def maps(gvom):
    """per (grid, buffer_size), built on demand and kept: (mapper, dense fused state, window origin)"""
    made = {}

    def get(grid, bs):
        if (grid, bs) not in made:
            g = rr.build_map(gvom.Gvom, grid, bs, voxel_statistics=False)
            state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
            made[grid, bs] = (g, state, np.asarray(origin, np.float64))
        return made[grid, bs]
    yield get
    made.clear()


class _Device(object):
    """arrays in device memory through the HIP runtime the library is linked against"""

    def __init__(self):
        self.rt = ctypes.CDLL("libamdhip64.so")
        self.rt.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.rt.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.rt.hipFree.argtypes = [ctypes.c_void_p]
        self.held = []

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = ctypes.c_void_p()
        assert self.rt.hipMalloc(ctypes.byref(p), a.nbytes) == 0
        assert self.rt.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0           # host to device, blocking
        self.held.append(p)
        return p.value

    def free(self):
        for p in self.held:
            self.rt.hipFree(p)
        self.held = []


def _hold(r, want, what):
    """a DeviceAlignments against the referee's (counts, best): both parts, exactly"""
    with r:
        counts, best = r.copy_to_host()
    assert counts.dtype == np.int32 and best.dtype == np.int32, what
    assert counts.shape == want[0].shape and best.shape == (4,), (what, counts.shape, best.shape)
    if not np.array_equal(counts, want[0]):
        bad = np.flatnonzero((counts != want[0]).any(axis=1))
        raise AssertionError("%s: the counts differ in %d candidates, first %d: got %r, referee %r" % (
            what, len(bad), bad[0], counts[bad[0]].tolist(), want[0][bad[0]].tolist()))
    assert best.tolist() == want[1].tolist(), (what, best.tolist(), want[1].tolist())
    return counts, best


def _long_cloud(grid, n):
    """n returns: the shared cloud, repeated with a shift of a third of a voxel where it is shorter"""
    c = ar.cloud_of(grid)
    xr, zr = ar.GRIDS[grid][:2]
    parts = [c + np.float32(k / 3.0) * np.array([xr, -xr, zr], np.float32) for k in range((n + len(c) - 1) // len(c))]
    return np.ascontiguousarray(np.concatenate(parts)[:n])


@pytest.mark.parametrize("bs", [1, 2])
@pytest.mark.parametrize("grid", ar.ALL_GRIDS)
def test_counts_scores_and_best_match_the_referee_exactly(gvom, maps, grid, bs):
    """the whole cloud under the 245 candidates and the specials, dilate 0 and 1, host and device inputs; on the census grids the
    floors of tests/align_ref.py and the unperturbed candidate as the unique best, on the GPU's own map"""
    g, state, W = maps(grid, bs)
    cloud, M = ar.cloud_of(grid), ar.candidates(grid)
    dev = _Device()
    try:
        for dilate in (0, 1):
            want = ar.score(state, W, grid, cloud, M, dilate)
            r = g.score_alignments(cloud, M, dilate=dilate)
            assert r.counts.shape == (len(M), 6) and r.counts.strides == (6, 1) and r.best.shape == (4,) and r.best.strides == (1,)
            assert r.counts.ptr % 256 == 0 and r.best.ptr % 256 == 0 and np.array_equal(r.origin, W)
            counts, best = _hold(r, want, "%s bs %d dilate %d, host" % (grid, bs, dilate))
            d = g.score_alignments_device(dev.upload(cloud), len(cloud), dev.upload(M[:, :3, :]), len(M), dilate=dilate)
            _hold(d, want, "%s bs %d dilate %d, device" % (grid, bs, dilate))
            assert (counts[:, 1:].sum(axis=1) == len(cloud)).all()
            assert np.array_equal(counts[ar.N_GRID], counts[ar.CENTRE]) and best[0] != ar.N_GRID        # the same matrix twice: the lower index wins
            assert counts[ar.N_GRID + 1, 5] == counts[ar.N_GRID + 2, 5] == counts[ar.N_GRID + 3, 5] == len(cloud)
            if grid in ar.CENSUS_GRIDS:
                t = ar.census_holds(grid, dilate, counts)
                srt = np.sort(counts[:ar.N_GRID, 0])
                print(grid, bs, "dilate", dilate, "totals", t, "best", best.tolist(), "second", int(srt[-2]))
                assert best[0] == ar.CENTRE and srt[-1] > srt[-2] and best[1] == srt[-1]
                assert len(np.unique(counts[:ar.N_GRID], axis=0)) >= ar.DISTINCT_ROWS
    finally:
        dev.free()


@pytest.fixture(scope="module")
def planted(gvom):
    """per (grid, buffer_size), built on demand and kept: (mapper, dense fused state, window origin) of a planted map"""
    made = {}

    def get(grid, bs):
        if (grid, bs) not in made:
            g = ar.planted_map(gvom.Gvom, grid, bs, voxel_statistics=False)
            state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
            made[grid, bs] = (g, state, np.asarray(origin, np.float64))
        return made[grid, bs]
    yield get
    made.clear()


@pytest.mark.parametrize("bs", [1, 2])
@pytest.mark.parametrize("grid", ar.PROBE_GRIDS)
def test_every_voxel_of_the_class_grid_is_held_to_the_referee(gvom, planted, grid, bs):
    """k_align_field, voxel by voxel: a planted map (tests/align_ref.py: single occupied voxels on both sides of every 16-voxel word
    of a row, on the bottom, the top and the middle level and on both sides of the boundary between the chunks of levels, on the
    first and the last row, in the corners; 64 returns per scan besides, so that single voxels decide their neighbours' class)
    under the three line probes, whose counts are the class histogram of every line of the window along every axis -- dilate 0
    and 1, one axis also through device inputs.  The dense state the referee reads comes from the same handle; it is held, class
    by class, to the CPU referee's planted map first.  Then the census, on the GPU's own map."""
    from oracle import oracle
    _, _, xy, zs = ar.GRIDS[grid]
    g, state, W = planted(grid, bs)
    o = ar.planted_map(oracle.OracleGvom, grid, bs)
    assert np.array_equal(W, rr.window_origin(grid, rr.ego_of(grid, ar.SCAN))) and np.array_equal(np.asarray(o.combined_origin, np.float64), W)
    assert all(int(W[k]) % (xy if k < 2 else zs) != 0 for k in range(3)), W          # non-zero storage offsets on every axis
    got, want = rr.state_class(state), rr.state_class(np.asarray(o.combined_index_map))
    assert np.array_equal(got, want), "%s, buffer %d: %d voxels differ from the oracle in their class, first %d: %d, oracle %d" % (
        grid, bs, int((got != want).sum()), np.flatnonzero(got != want)[0], got[got != want][0], want[got != want][0])
    census = ar.planted_census_holds(state, grid)
    probes = ar.line_probes(grid, W)
    dev = _Device()
    try:
        for dilate in (0, 1):
            cls = ar.classes(state, grid, dilate)
            for axis, (cloud, M) in enumerate(probes):
                what = "%s bs %d dilate %d, lines along axis %d" % (grid, bs, dilate, axis)
                want = ar.score(state, W, grid, cloud, M, dilate, cls=cls)
                counts, _ = _hold(g.score_alignments(cloud, M, dilate=dilate), want, what)
                # every window voxel once: over the candidates the counts are the histogram of the whole class grid
                assert counts[:, 1:].astype(np.int64).sum(axis=0).tolist() == np.bincount(cls.ravel(), minlength=5).tolist(), what
                if axis == 2:
                    d = g.score_alignments_device(dev.upload(cloud), len(cloud), dev.upload(M[:, :3, :]), len(M), dilate=dilate)
                    _hold(d, want, what + ", device")
    finally:
        dev.free()
    print(grid, bs, "planted, occupied, least carry:", census, "candidates", [len(M) for _, M in probes])


@pytest.mark.parametrize("bs", [1, 2])
@pytest.mark.parametrize("grid", ar.EDGE_GRIDS)
def test_the_score_kernel_at_its_edges_with_the_reciprocal_and_with_the_divide(gvom, maps, grid, bs):
    """k_align_score where a voxel index is decided by the last bit: returns on exact voxel faces of the window and their float32
    neighbours on both sides (ar.boundary_points), then returns of the shared cloud, 2,048 in all; under the identity, one voxel
    up and down every axis, rotations about the window centre around each of the three axes (small, large, a quarter and a half
    turn) and ar.rotations(); on resolutions that are no multiple of anything too (ar.OFF_GRID).  Once with the "fastdiv" knob as
    created -- k_align_score<true>, the verified reciprocals -- and once with the knob at 0 -- k_align_score<false>, the IEEE
    divide: both are held exactly to the referee, which divides.  (The mixed setting, one resolution verified and one not, cannot
    be reached through the public knob: every resolution the host's check has been given passes it.)"""
    g, state, W = maps(grid, bs)
    (cloud, m), M = ar.edge_cloud(grid, W), ar.edge_candidates(grid, W)
    runs = {}
    try:
        for knob, reads in ((None, 3), (0, 0)):
            if knob is not None:
                g.set_tuning("fastdiv", knob)
            assert g.get_tuning("fastdiv") == reads
            seen = np.zeros(5, np.int64)
            for dilate in (0, 1):
                what = "%s bs %d dilate %d fastdiv %d" % (grid, bs, dilate, reads)
                counts, best = _hold(g.score_alignments(cloud, M, dilate=dilate), ar.score(state, W, grid, cloud, M, dilate), what)
                t, up, inside, outside = ar.edge_census_holds(grid, W, dilate, cloud, m, M, counts)
                seen += t
                runs[reads, dilate] = counts
                if knob is None:
                    print(what, "totals", t, "upper 30 %", up, "boundary points inside", inside, "outside", outside, "best", best.tolist())
            assert (seen > 0).all(), (grid, bs, seen)                      # every class, OUTSIDE included, occurs
    finally:
        g.set_tuning("fastdiv", -1)                                        # as created: the maps are shared
    assert g.get_tuning("fastdiv") == 3
    for dilate in (0, 1):
        assert np.array_equal(runs[3, dilate], runs[0, dilate])


@pytest.mark.parametrize("grid", ["p2", "np2", "tall", "w192"])
def test_shapes_on_each_side_of_the_kernel_tiles(gvom, maps, grid):
    """n of 1, 63, 65 and one more than the returns per workgroup, K of 1, 3 and one more than the candidate group, alternately through
    host and device inputs, each with weights of its own"""
    g, state, W = maps(grid, 1)
    pb, cg = g.get_tuning("alignment_points_per_block"), g.get_tuning("alignment_candidate_group")
    assert pb >= 64 and cg >= 1
    M = ar.candidates(grid)
    M = np.concatenate([M[ar.CENTRE - 1:ar.CENTRE + 2], M[ar.N_GRID:], M[:ar.CENTRE - 1]])      # the centre among the first three, the specials early
    cls = {d: ar.classes(state, grid, d) for d in (0, 1)}
    dev = _Device()
    case = 0
    try:
        for n in (1, 63, 65, pb + 1, 2 * pb):
            cloud = _long_cloud(grid, n)
            for K in (1, 3, cg + 1, 2 * cg):
                dilate, w = (case // 4 + case) % 2, WEIGHTS[case % len(WEIGHTS)]
                want = ar.score(state, W, grid, cloud, M[:K], dilate, weights=w, cls=cls[dilate])
                if case % 3 == 0:
                    r = g.score_alignments_device(dev.upload(cloud), n, dev.upload(M[:K, :3, :]), K, dilate=dilate, weights=w)
                else:
                    r = g.score_alignments(cloud, M[:K] if case % 3 == 1 else M[:K, :3, :], dilate=dilate, weights=w)
                _hold(r, want, "%s n %d K %d dilate %d weights %r" % (grid, n, K, dilate, w))
                case += 1
    finally:
        dev.free()
    assert case == 20


def test_weights_only_change_the_scores(gvom, maps):
    g, state, W = maps("np2", 2)
    cloud, M = ar.cloud_of("np2"), ar.candidates("np2")
    base = ar.score(state, W, "np2", cloud, M, 1)
    for w in WEIGHTS + ((0, 0, 0, 0, 1024),):
        want = ar.score(state, W, "np2", cloud, M, 1, weights=w)
        assert np.array_equal(want[0][:, 1:], base[0][:, 1:])
        counts, best = _hold(g.score_alignments(cloud, M, dilate=1, weights=np.array(w, np.int64)), want, "weights %r" % (w,))
        assert np.array_equal(counts[:, 0], (counts[:, 1:].astype(np.int64) * np.array(w)).sum(axis=1))
    # all scores equal: the best is candidate 0; the largest score there is: 2^20 returns' worth does not fit this cloud, 1024 * n does
    assert _hold(g.score_alignments(cloud, M, weights=(0, 0, 0, 0, 0)), ar.score(state, W, "np2", cloud, M, 0, weights=(0,) * 5), "zero")[1][0] == 0
    top = _hold(g.score_alignments(cloud, M, weights=(1024,) * 5), ar.score(state, W, "np2", cloud, M, 0, weights=(1024,) * 5), "1024")[1]
    assert top.tolist() == [0, 1024 * len(cloud), len(cloud), len(M)]


def test_a_query_sees_the_current_map_and_leaves_it_unchanged(gvom):
    grid = "np2"
    g = rr.build_map(gvom.Gvom, grid, 2, voxel_statistics=False)
    cloud, M = ar.cloud_of(grid), ar.candidates(grid)
    before = g.read_dense(gvom.GVOM_WHICH_FUSED)
    held = g.score_alignments(cloud, M, dilate=1)
    first = held.copy_to_host()
    after = g.read_dense(gvom.GVOM_WHICH_FUSED)
    for a, b in zip(before[:4], after[:4]):                     # state, hit, total, min height: the query is read-only
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(before[4], after[4]) and before[5] == after[5]
    # a further scan and combine: the window moves on, the next query answers for the new map, the held product stays
    ego = rr.ego_of(grid, rr.N_SCANS)
    g.process_pointcloud(rr.cloud_of(grid, 1), ego)
    g.combine_maps()
    state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
    W = np.asarray(origin, np.float64)
    assert not np.array_equal(W, before[4])
    want = ar.score(state, W, grid, cloud, M, 1)
    later = g.score_alignments(cloud, M, dilate=1)
    assert later.counts.ptr != held.counts.ptr and np.array_equal(later.origin, W) and np.array_equal(held.origin, before[4])
    now = _hold(later, want, "after a further scan and combine")
    assert not np.array_equal(now[0], first[0])
    again = held.copy_to_host()
    assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])
    _hold(held, ar.score(before[0], before[4], grid, cloud, M, 1), "the held snapshot")
    # dilate changing between calls: the class grid is rebuilt every time
    for dilate in (0, 1, 0):
        _hold(g.score_alignments(cloud, M, dilate=dilate), ar.score(state, W, grid, cloud, M, dilate), "dilate %d" % dilate)


def test_pool_reuse_and_no_allocation_in_steady_state(gvom, maps):
    grid = "p2"
    _, _, xy, zs = ar.GRIDS[grid]
    g = rr.build_map(gvom.Gvom, grid, 1, voxel_statistics=False)
    state, _, _, _, origin, _ = g.read_dense(gvom.GVOM_WHICH_FUSED)
    W = np.asarray(origin, np.float64)
    cloud, M = ar.cloud_of(grid), ar.candidates(grid)
    want = ar.score(state, W, grid, cloud, M, 1)
    assert g.get_tuning("alignments") == 1 and g.get_tuning("alignment_allocations") == 0 and g.get_tuning("alignment_grid_bytes") == 0
    call = lambda m=M: g.score_alignments(cloud, m, dilate=1)
    first = call()
    assert g.get_tuning("alignment_allocations") == 3             # the product set, the class grid and the host staging buffer
    grid_bytes = g.get_tuning("alignment_grid_bytes")             # (what is allocated: a grow-only buffer comes with headroom)
    assert xy * ((xy + 15) // 16) * zs * 4 == xy * xy * zs // 4 <= grid_bytes <= xy * xy * zs // 2
    assert g.get_tuning("device_product_sets") == 1
    ptr = first.counts.ptr
    first.release()
    for _ in range(3):                                           # released: everything is reused
        with call() as r:
            assert r.counts.ptr == ptr
            _hold(r, want, "reused set")
    assert g.get_tuning("alignment_allocations") == 3 and g.get_tuning("device_product_sets") == 1
    assert g.get_tuning("alignment_grid_bytes") == grid_bytes
    # a held export keeps the product alive across the next calls
    held = call()
    other = call(M[:7])
    assert other.counts.ptr != held.counts.ptr and g.get_tuning("device_product_sets") == 2
    _hold(other, ar.score(state, W, grid, cloud, M[:7], 1), "a second set")
    _hold(held, want, "held across a call")
    with call() as r:                                            # (both are free again: the smaller set is given up for one that holds K)
        _hold(r, want, "after both came back")
    allocs, sets = g.get_tuning("alignment_allocations"), g.get_tuning("device_product_sets")
    for _ in range(3):
        with call() as r:
            _hold(r, want, "steady state")
    assert g.get_tuning("alignment_allocations") == allocs and g.get_tuning("device_product_sets") == sets
    assert g.get_tuning("alignment_grid_bytes") == grid_bytes
    hold4 = [call() for _ in range(4)]
    assert len({r.counts.ptr for r in hold4}) == 4 and g.get_tuning("device_product_sets") == 4
    with pytest.raises(gvom.GvomBackendError, match="all 4 device product sets of this kind"):
        call()
    hold4[1].release()
    with call() as r:
        _hold(r, want, "after a release")
    assert g.get_tuning("device_product_sets") == 4
    with pytest.raises(gvom.GvomBackendError, match="unknown or stale device product id"):
        hold4[1].copy_to_host()


def test_errors(gvom):
    grid = "tall"
    fresh = gvom.Gvom(*rr.params(grid, 1), voxel_statistics=False)
    cloud, M = ar.cloud_of(grid), np.ascontiguousarray(ar.candidates(grid)[:, :3, :])
    assert fresh.score_alignments(cloud, M) is None               # before the first combine: no data
    fresh.process_pointcloud(cloud, rr.ego_of(grid, 0))
    assert fresh.score_alignments(cloud, M) is None
    assert fresh.get_tuning("alignment_allocations") == 0
    g = rr.build_map(gvom.Gvom, grid, 1, voxel_statistics=False)
    pid = ctypes.c_int64(-1)
    w5 = (ctypes.c_int32 * 5)(2, 1, -1, 0, 0)
    cp, tp = cloud.ctypes.data_as(ctypes.c_void_p), M.ctypes.data_as(ctypes.c_void_p)

    def raw(c=cp, n=len(cloud), t=tp, K=len(M), dilate=0, w=w5, out=pid):
        return g._lib.gvom_score_alignments(g._h, c, n, t, K, 0, dilate, w, ctypes.byref(out) if out is not None else None)
    assert raw() == 0 and pid.value >= 0
    INVALID, CAPACITY = gvom.GVOM_ERR_INVALID, -4
    for kw, rc, word in ((dict(dilate=2), INVALID, "dilate"), (dict(dilate=-1), INVALID, "dilate"),
                         (dict(w=(ctypes.c_int32 * 5)(0, 1025, 0, 0, 0)), INVALID, "weight"), (dict(w=(ctypes.c_int32 * 5)(0, 0, 0, 0, -1025)), INVALID, "weight"),
                         (dict(n=0), INVALID, "n must be"), (dict(K=0), INVALID, "K must be"), (dict(c=None), INVALID, "NULL"), (dict(t=None), INVALID, "NULL"),
                         (dict(w=None), INVALID, "NULL"), (dict(n=(1 << 20) + 1, K=1), CAPACITY, "2\\^20"), (dict(K=65537, n=1), CAPACITY, "65536"),
                         (dict(n=1 << 20, K=4097), CAPACITY, "2\\^32")):
        assert raw(**kw) == rc, kw
        assert pid.value == -1, kw
        assert re.search(word, g._lib.gvom_last_error(g._h).decode()), (kw, g._lib.gvom_last_error(g._h))
    assert raw(out=None) == INVALID                               # NULL product_id
    with pytest.raises(ValueError, match="dilate"):
        g._check_args(raw(dilate=3))
    with pytest.raises(gvom.GvomBackendError, match="gvom_score_alignments"):
        g._device_product(gvom.PRODUCT_ALIGNMENT)
    with pytest.raises(gvom.GvomBackendError, match="unknown product kind"):
        g._device_product(11)
    with pytest.raises(TypeError, match="float32"):
        g.score_alignments(cloud.astype(np.float64), M)
    sharded = gvom.Gvom(*rr.params("p2", 1), voxel_statistics=False, _shard=(0, 2))
    with pytest.raises(ValueError, match="sharded handles are not supported"):
        sharded.score_alignments(cloud, M)


def _torch_case(name):
    """One case per fresh child process that imports torch BEFORE the library is loaded (one HIP runtime in the process)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_align_torch.py"), name],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "CASE OK " + name in r.stdout, r.stdout[-4000:]


def test_a_torch_consumer_finds_the_best_candidate_itself():
    _torch_case("argmax")
