"""Shared by tests/test_query_cycle.py (GPU) and tests/test_query_cycle_cpu.py (no GPU): the scripts that take a mapper through every
point of its scan cycle, the mirror that says what the fused map is at each point, and the bundle of map queries held there.

THE RULE the scripts hold (include/gvom_hip.h "the current fused map"): a query -- gvom_raycast, gvom_score_viewpoints,
gvom_score_alignments, gvom_device_product (occupancy grid), the dense read hook -- answers for the map of the most recently BEGUN
combine, synchronous or asynchronous.  A scan, accepted or rejected, changes nothing a query sees until the next combine; a combine
changes nothing a product made before it holds.

THE MIRROR is oracle.OracleGvom driven with the same scans and combines.  After each of its combines the dense fused arrays are taken
with scenarios.dense_from_compact and W = combined_origin.  The oracle has no asynchronous form: the mirror combines at the moment
combine_maps_async() is BEGUN, which is the rule above.  Where a scan has been accepted and not combined yet the mirror can also say
what a combine at that moment WOULD give (Cycle.speculated: a deep copy of the oracle, combined): on a one-slot ring that is what the
speculative fusion has written into the spare buffer, the map a query must NOT answer for.

THE QUERY BUNDLE Q(g, map): one call of each kind on the GPU handle, each held to its referee on the mirror's (state, W) with the
comparison the product's own test uses -- integers with tolerance 0, positions by bit pattern, the product's `.origin` == W:
  raycast              512 rays: rr.rays_of(grid, state, W) thinned [::8], with unknown_blocks=True and with the default flags; rr.walk
                       (at K the families start from K's own ego and use K's own scan, rays_of(..., last=(ego, cloud)): from the
                       ego of scan 3, ten windows away, 477 of the 512 rays would leave the window with their first step)
  score_viewpoints     model m5x37 of tests/viewpoint_ref.py at the ego of the map's last scan and 1.5 m to either side, and one pose
                       with a NaN entry; a third of the window; vr.product
  score_alignments     ar.cloud_of(grid) under the first 16 of ar.candidates(grid) and its four specials, dilate=1; ar.score
  occupancy_grid_device() and get_map_as_occupancy_grid()     state >= 0 in [x, y, z] order
  read_dense(GVOM_WHICH_FUSED)     state and window origin
The referee's answers are computed once per map and shared by the points that ask about it.

THE SCRIPT (run_script) names every point in every assertion message.  After every combine the four 2-D maps and the dense fused
arrays are held to the oracle as tests/test_hip_parity.py test_tile_epoch_renumbering_before_the_counter_wraps does: the queries in
between changed nothing.
  P0  nothing combined yet -- before the first scan, and again after it (on a one-slot ring the spare buffer then holds a speculation
      while no map exists): every query reports no data and the allocation counters stay 0
  A   scan 0, combine_maps(), Q
  B   scan 1, Q on the map of A (one-slot ring: the speculation sits in the spare buffer)
  C   scan 2, Q on the map of A (a second speculation; one-slot ring: the slot was rewritten)
  D   combine_maps(), Q on the new map (one-slot ring: "fuse_kernel" 6, adopted)
  E   combine_maps() with no scan in between, Q: the previous map enters and decays; no voxel changes its class
  F   scan 6 and combine_maps_device(), Q; the DeviceMaps are kept.  (The scan is this file's: without it F would ask about a map
      whose voxel classes equal E's and D's, and no query could tell the three apart -- tests/test_query_cycle_cpu.py shows it.  E alone
      stays the point without a scan.  Scan 6 lies beyond scans 3 .. 5 on the egos' line, so the window then moves back.)
  G   scan 3 and combine_maps_async(), Q BEFORE .result(): the answer is for the map of THIS combine
  H   scan 4 while the combine is pending, Q (still G's map); .result(), held to the oracle's maps; Q again
  I   two rejected scans (an empty cloud; one of only NaN returns, from another ego), Q unchanged
  J   scan 5 and combine_maps_occupancy(), Q
  K   a scan whose ego lies ten windows away (far_scan: scan 0 moved there; a uniform cloud out there leaves 10 of 512 rays CLEAR),
      combine_maps(), Q: nothing of the previous map is inside
  L   the products kept at A, D and G (a raycast product and an occupancy grid each) still hold their first bytes; the DeviceMaps of
      F still give a cost_to_go() from the ego's cell (and the free cell nearest to it: the ego's own is blocked) equal to
      cost_to_go_of() of the cost map of F's own maps, copied out at F"""
import copy

import numpy as np
import pytest

import align_ref as ar
import costfield_ref as cf
import raycast_ref as rr
import scenarios
import viewpoint_ref as vr
from oracle import oracle

F32 = np.float32
MODEL = "m5x37"
FAR_SCAN = "far"                                              # Cycle.scan(FAR_SCAN): far_scan() below
SCRIPT_POINTS = ("A", "B", "C", "D", "E", "F", "G", "H pending", "H", "I", "J", "K")
CHANGED_FLOOR = 256                                           # of 512 rays, between a point's map and the map a wrong answer would come from
STATUS_FLOOR = 12                                             # rays per status at every point (the invalid family: 96 / 8)


def far_scan(grid):
    """(cloud, ego) of the scan at K: scan 0 of tests/raycast_ref.py -- a lidar sweep of the scene of boxes -- moved ten windows along
    x, ten against y and three window heights up, a whole number of voxels on every axis; float32 returns, a float32-representable ego"""
    xr, zr, xy, zs = rr.GRIDS[grid]
    off = np.array([10.0 * xy * xr, -10.0 * xy * xr, 3.0 * zs * zr])
    pc = (rr.cloud_of(grid, 0).astype(np.float64) + off).astype(F32)
    return np.ascontiguousarray(pc), tuple(float(F32(v + o)) for v, o in zip(rr.ego_of(grid, 0), off))


# ---- the mirror's maps, the inputs of the bundle and the referee's answers -----------------------------------------------------------
class Map(object):
    """one combine of the mirror: the dense fused arrays (state first), W, the oracle's 2-D maps and cell count, the ego of the last
    scan accepted before it; `want` = the referee's answers to the bundle on this map, computed once"""

    def __init__(self, grid, label, o, maps2d, ego, rays_from=None):
        self.grid, self.label, self.ego, self.rays_from = grid, label, tuple(ego), rays_from
        self.dense = scenarios.dense_from_compact(o.combined_index_map, o.combined_hit_count, o.combined_total_count, o.combined_min_height)
        self.state = self.dense[0]
        self.W = np.asarray(o.combined_origin, np.float64).copy()
        self.maps2d = maps2d
        self.cells = o.combined_cell_count_cpu
        self._inputs = self._want = None

    @property
    def inputs(self):
        if self._inputs is None:
            self._inputs = inputs_of(self)
        return self._inputs

    @property
    def want(self):
        if self._want is None:
            self._want = answers(self.inputs, self)
        return self._want


def inputs_of(m):
    """what the bundle asks at a point whose current map is m"""
    A, B, fam = rr.rays_of(m.grid, m.state, m.W, last=m.rays_from)
    A, B, fam = np.ascontiguousarray(A[::8]), np.ascontiguousarray(B[::8]), fam[::8]
    assert len(B) == 512
    ego = np.array(m.ego, np.float64)
    nan = vr.pose_of(ego, 0.3)
    nan[1, 2] = np.nan
    poses = np.stack([vr.pose_of(ego), vr.pose_of(ego + (1.5, 0.0, 0.0), 0.6), nan, vr.pose_of(ego - (1.5, 0.0, 0.0), -0.9)])
    M = ar.candidates(m.grid)
    return dict(A=A, B=B, fam=fam, poses=poses, range=vr.max_range_of(m.grid, "third"), cloud=ar.cloud_of(m.grid),
                M=np.ascontiguousarray(np.concatenate([M[:16], M[ar.N_GRID:]])))


def answers(inp, m):
    """the referee's answers to the inputs `inp` on the map m (m.want = answers(m.inputs, m))"""
    d, o = vr.model(MODEL)
    xy, zs = rr.GRIDS[m.grid][2:]
    return {("rays", True): rr.walk(m.state, m.W, m.grid, inp["A"], inp["B"], unknown_blocks=True),
            ("rays", False): rr.walk(m.state, m.W, m.grid, inp["A"], inp["B"]),
            "viewpoints": vr.product(m.state, m.W, m.grid, d, o, inp["poses"], inp["range"]),
            "alignments": ar.score(m.state, m.W, m.grid, inp["cloud"], inp["M"], 1),
            "occupancy": np.reshape(m.state, (xy, xy, zs), order="F") >= 0}


def rays_changed(a, b):
    """rays whose answer (result row or stop position, NaN == NaN) differs between two walks"""
    (ra, pa), (rb, pb) = a, b
    same_pos = (_bits(pa) == _bits(pb)) | (np.isnan(pa) & np.isnan(pb))
    return int(((ra != rb).any(axis=1) | ~same_pos.all(axis=1)).sum())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- holding the GPU's products to the referee ---------------------------------------------------------------------------------------
def hold_rays(rays, want, W, what):
    assert rays is not None, what + ": no data"
    with rays:
        assert np.array_equal(rays.origin, W), "%s: origin %r, mirror %r" % (what, rays.origin, W)
        result, position = rays.copy_to_host()
    wr, wp = want
    assert result.dtype == np.int32 and position.dtype == F32 and result.shape == wr.shape and position.shape == wp.shape, what
    if not np.array_equal(result, wr):
        bad = np.flatnonzero((result != wr).any(axis=1))
        raise AssertionError("%s: %d rays differ, first %d: got %r, referee %r" % (what, len(bad), bad[0], result[bad[0]], wr[bad[0]]))
    same = (_bits(position) == _bits(wp)) | (np.isnan(position) & np.isnan(wp))
    assert same.all(), "%s: %d positions differ" % (what, int((~same).any(axis=1).sum()))
    assert np.array_equal(np.isnan(position), np.isnan(wp)), what


def hold_viewpoints(v, want, W, what):
    assert v is not None, what + ": no data"
    with v:
        assert np.array_equal(v.origin, W), "%s: origin %r, mirror %r" % (what, v.origin, W)
        rows, best = v.copy_to_host()
    assert rows.dtype == np.int32 and best.dtype == np.int32 and rows.shape == want[0].shape and best.shape == (4,), what
    if not np.array_equal(rows, want[0]):
        bad = np.flatnonzero((rows != want[0]).any(axis=1))
        raise AssertionError("%s: %d viewpoints differ, first %d: got %r, referee %r" % (what, len(bad), bad[0], rows[bad[0]], want[0][bad[0]]))
    assert np.array_equal(best, want[1]), (what, best, want[1])


def hold_alignments(r, want, W, what):
    assert r is not None, what + ": no data"
    with r:
        assert np.array_equal(r.origin, W), "%s: origin %r, mirror %r" % (what, r.origin, W)
        counts, best = r.copy_to_host()
    assert counts.dtype == np.int32 and best.dtype == np.int32 and counts.shape == want[0].shape and best.shape == (4,), what
    if not np.array_equal(counts, want[0]):
        bad = np.flatnonzero((counts != want[0]).any(axis=1))
        raise AssertionError("%s: the counts differ in %d candidates, first %d: got %r, referee %r" % (
            what, len(bad), bad[0], counts[bad[0]].tolist(), want[0][bad[0]].tolist()))
    assert best.tolist() == want[1].tolist(), (what, best.tolist(), want[1].tolist())


def Q(g, mod, m, what):
    """the query bundle on the handle g, held to the mirror's map m"""
    inp, want = m.inputs, m.want
    for ub in (True, False):
        hold_rays(g.raycast(inp["A"], inp["B"], unknown_blocks=ub), want["rays", ub], m.W, "%s: raycast, unknown_blocks %d" % (what, ub))
    hold_viewpoints(g.score_viewpoints(inp["poses"], inp["range"]), want["viewpoints"], m.W, what + ": score_viewpoints")
    hold_alignments(g.score_alignments(inp["cloud"], inp["M"], dilate=1), want["alignments"], m.W, what + ": score_alignments")
    occ = g.occupancy_grid_device()
    assert occ is not None, what + ": occupancy_grid_device: no data"
    with occ:
        grid = occ.copy_to_host()
    assert grid.dtype == np.uint8 and grid.shape == want["occupancy"].shape and grid.max() <= 1, what
    assert np.array_equal(grid != 0, want["occupancy"]), "%s: occupancy_grid_device differs in %d voxels" % (what, int(((grid != 0) != want["occupancy"]).sum()))
    host = g.get_map_as_occupancy_grid()
    assert np.array_equal(host, want["occupancy"]), "%s: get_map_as_occupancy_grid differs in %d voxels" % (what, int((host != want["occupancy"]).sum()))
    d = g.read_dense(mod.GVOM_WHICH_FUSED)
    assert d is not None and np.array_equal(d[0], m.state), "%s: read_dense state differs in %d voxels" % (what, int((d[0] != m.state).sum()))
    assert np.array_equal(np.asarray(d[4], np.float64), m.W), "%s: read_dense origin %r, mirror %r" % (what, d[4], m.W)


def no_data(g, mod, grid, what):
    """before the first combine: every query of the bundle says so and allocates nothing"""
    a = np.array([[0.1, 0.2, 0.1], [1.0, -1.0, 0.0]], F32)
    M = ar.candidates(grid)[:4]
    assert g.raycast(a, a + F32(2.0)) is None, what
    assert g.score_viewpoints(np.stack([vr.pose_of((0.0, 0.0, 0.0))]), vr.max_range_of(grid, "third")) is None, what
    assert g.score_alignments(ar.cloud_of(grid)[:64], M, dilate=1) is None, what
    assert g.occupancy_grid_device() is None, what
    with pytest.raises(AttributeError):
        g.get_map_as_occupancy_grid()
    assert g.read_dense(mod.GVOM_WHICH_FUSED) is None, what
    for name in ("raycast_allocations", "viewpoint_allocations", "alignment_allocations", "device_product_sets"):
        assert g.get_tuning(name) == 0, (what, name, g.get_tuning(name))


def hold_maps(got, m, what):
    """the origin and the four 2-D maps of a combine against the oracle's: integers exactly, the roughness within 1e-5"""
    want = m.maps2d
    for i in (0, 1, 2, 4):
        assert np.array_equal(np.asarray(got[i]), want[i]), "%s: map %d differs from the oracle" % (what, i)
    assert np.allclose(np.asarray(got[3]), want[3], rtol=0, atol=1e-5), "%s: the roughness map differs from the oracle" % what


def hold_dense(g, mod, m, what):
    assert g.combined_cell_count_cpu == m.cells, "%s: %r fused cells, oracle %r" % (what, g.combined_cell_count_cpu, m.cells)
    d = g.read_dense(mod.GVOM_WHICH_FUSED)
    for j in range(4):
        assert np.array_equal(np.asarray(m.dense[j]), d[j]), "%s: dense fused array %d differs from the oracle" % (what, j)
    assert np.array_equal(np.asarray(d[4], np.float64), m.W), what


def hold_occupancy_grids(got, m, what):
    """combine_maps_occupancy() against the node's post-processing of the ORACLE's maps.  hard, soft, certainty and negative come
    from integer maps: exact.  The roughness grid truncates ((clip(r, -10, 0) - 10) / 10) * 100 = 10 r + const: the GPU's float
    roughness may differ from the oracle's by 1e-5 (the parity bar), the scaled value by 1e-4, so the grid is held exactly wherever
    the oracle's scaled value is further than 1e-3 from a whole number (the dense arrays behind it are held exactly by hold_dense)."""
    want = oracle.ros_occupancy_grids(m.maps2d)
    assert np.array_equal(got[0], m.maps2d[0]), what
    for name, a, b in zip(("hard", "soft", "certainty", "negative"), got[1:5], want[:4]):
        assert a.dtype == np.int8 and np.array_equal(a, b), "%s: the %s grid differs in %d cells" % (what, name, int((a != b).sum()))
    with np.errstate(invalid="ignore"):
        r = np.reshape(((np.maximum(np.minimum(m.maps2d[3], 0), -10) + -10) / 10.0) * 100, -1, order="F")
    sure = np.abs(r - np.round(r)) > 1e-3
    assert sure.sum() >= sure.size // 2
    assert np.array_equal(got[5][sure], want[4][sure]), "%s: the roughness grid differs in %d cells" % (what, int((got[5][sure] != want[4][sure]).sum()))


# ---- the cycle: the GPU handle (or none: the census) and its mirror, step by step ------------------------------------------------------
class Cycle(object):
    """A mapper `g` of module `mod` (None: the mirror alone, for the census) and the oracle fed the same calls.  `points` collects
    (label, current map, [the maps a wrong answer could come from]) at every Q."""

    def __init__(self, grid, bs, mod=None, stats=False, **kw):
        self.grid, self.bs, self.mod = grid, bs, mod
        self.o = oracle.OracleGvom(*rr.params(grid, bs))
        self.g = None
        if mod is not None:
            self.g = mod.Gvom(*rr.params(grid, bs), voxel_statistics=stats, **kw)
            self.g.set_sensor_model(*vr.model(MODEL))
        self.cur = self.prev = None
        self.ego = None                                       # of the last accepted scan
        self.fresh = False                                    # an accepted scan has not been combined yet
        self.pending = None
        self.points, self.kept = [], []

    def scan(self, k):
        pc, ego = (rr.cloud_of(self.grid, k), rr.ego_of(self.grid, k)) if k != FAR_SCAN else far_scan(self.grid)
        self.o.process_pointcloud(pc.copy(), ego)
        if self.g is not None:
            self.g.process_pointcloud(pc, ego)
        self.ego, self.fresh = ego, True
        self.rays_from = (ego, pc) if k == FAR_SCAN else None

    def reject(self, pc, ego):
        filled = self.o.buffer_index
        self.o.process_pointcloud(pc.copy(), ego)
        assert self.o.buffer_index == filled                  # the oracle refused it
        if self.g is not None:
            self.g.process_pointcloud(pc, ego)

    def speculated(self):
        """what a combine at this moment would give: on a one-slot ring, what the spare buffer holds"""
        o = copy.deepcopy(self.o)
        return Map(self.grid, "speculated", o, o.combine_maps(), self.ego, self.rays_from)

    def combine(self, kind, label):
        """kind: sync, device, occupancy, async (begun here, ended by finish()).  Returns what the GPU call returned."""
        maps2d = self.o.combine_maps()
        self.prev, self.cur = self.cur, Map(self.grid, label, self.o, maps2d, self.ego, self.rays_from)
        self.fresh = False
        g, m, out = self.g, self.cur, None
        if g is None:
            return None
        what = "%s: %s" % (label, kind)
        if kind == "sync":
            out = g.combine_maps()
            hold_maps(out, m, what)
        elif kind == "device":
            out = g.combine_maps_device()
            hold_maps((out.origin, out.positive.copy_to_host(), out.negative.copy_to_host(), out.roughness.copy_to_host(),
                       out.visibility.copy_to_host()), m, what)
        elif kind == "occupancy":
            out = g.combine_maps_occupancy()
            hold_occupancy_grids(out, m, what)
        else:
            assert kind == "async"
            self.pending = (g.combine_maps_async(), m)
            return self.pending[0]
        hold_dense(g, self.mod, m, what)
        return out

    def finish(self, label):
        if self.g is not None:
            pending, m = self.pending
            self.pending = None
            got = pending.result()
            hold_maps(got, m, label + ": result()")
            hold_dense(self.g, self.mod, m, label + ": result()")

    def P0(self, what):
        """run_script's two points before the first combine, behind no_data(): for what a subclass attaches to the handle
        (tests/voxel_atlas_cycle.py: a voxel atlas)"""

    def Q(self, label):
        others = [m for m in (self.prev,) if m is not None]
        if self.g is None and self.fresh:
            others.append(self.speculated())
        self.points.append((label, self.cur, others))
        if self.g is not None:
            Q(self.g, self.mod, self.cur, "%s, ring of %d, point %s (map of %s)" % (self.grid, self.bs, label, self.cur.label))

    def keep(self, label):
        """a raycast product and an occupancy grid of the current map, held until the end, and their bytes now"""
        if self.g is None:
            return
        inp = self.cur.inputs
        rays, occ = self.g.raycast(inp["A"], inp["B"], unknown_blocks=True), self.g.occupancy_grid_device()
        self.kept.append((label, rays, occ, [a.tobytes() for a in rays.copy_to_host()] + [occ.copy_to_host().tobytes()]))

    def check_kept(self, label):
        for name, rays, occ, before in self.kept:
            now = [a.tobytes() for a in rays.copy_to_host()] + [occ.copy_to_host().tobytes()]
            assert now == before, "%s: a product kept at %s has changed" % (label, name)
            rays.release()
            occ.release()
        self.kept = []


def cost_map_of(dm):
    """the cost map of a DeviceMaps' own maps (default cost parameters), from their host copies"""
    return cf.travcost(dm.positive.copy_to_host(), dm.negative.copy_to_host(), dm.visibility.copy_to_host(), dm.roughness.copy_to_host(), None, {})


def goal_cells(cost, ego, xy_resolution, origin_world):
    """the goals of the field at L: the cell under the ego and the free cell nearest to it (under the ego the map is usually blocked:
    a goal there seeds nothing)"""
    x, y = cf.world_to_cells([ego[:2]], xy_resolution, origin_world)[0]
    return np.array([(x, y), cf._free_near(cost, int(x), int(y))], np.int64)


def run_script(c):
    """the points P0 .. L of the module docstring on the cycle c; returns c"""
    g, grid = c.g, c.grid
    if g is not None:
        no_data(g, c.mod, grid, "P0")
    c.P0("P0")
    c.scan(0)
    if g is not None:
        no_data(g, c.mod, grid, "P0, after scan 0")
    c.P0("P0, after scan 0")
    c.combine("sync", "A"); c.Q("A"); c.keep("A")
    c.scan(1); c.Q("B")
    c.scan(2); c.Q("C")
    c.combine("sync", "D")
    if g is not None and c.bs == 1:
        assert g.get_tuning("fuse_kernel") == 6, "D: the speculation of scan 2 was not adopted"
    c.Q("D"); c.keep("D")
    c.combine("sync", "E"); c.Q("E")
    c.scan(6)
    dm = c.combine("device", "F"); c.Q("F")
    if g is not None:
        ego_f, cost_f = c.ego, cost_map_of(dm)
    c.scan(3)
    c.combine("async", "G"); c.Q("G"); c.keep("G")
    c.scan(4); c.Q("H pending")
    c.finish("H"); c.Q("H")
    c.reject(np.zeros((0, 3), F32), rr.ego_of(grid, 7))
    c.reject(np.full((40, 3), np.nan, F32), rr.ego_of(grid, 7))
    c.Q("I")
    c.scan(5)
    c.combine("occupancy", "J"); c.Q("J")
    c.scan(FAR_SCAN)
    c.combine("sync", "K"); c.Q("K")
    if g is not None:
        c.check_kept("L")
        cells = goal_cells(cost_f, ego_f, g.xy_resolution, dm.origin)
        with dm.cost_to_go(cells, goals_in_cells=True) as held, g.cost_to_go_of(cost_f, cells) as again:
            a, b = held.copy_to_host(), again.copy_to_host()
            assert held.reached == again.reached > 0 and held.goals_seeded == again.goals_seeded >= 1, "L: the field of F's maps reaches nothing"
        assert np.array_equal(a[2], cost_f), "L: the cost map of the DeviceMaps kept at F has changed"
        for k in range(3):
            assert np.array_equal(a[k], b[k]), "L: part %d of cost_to_go() on the DeviceMaps kept at F differs from cost_to_go_of() of their copy" % k
        dm.release()
    return c


# ---- the script across the tile-epoch renumbering --------------------------------------------------------------------------------------
EPOCH_LIMIT = 0xFFFFFF00
# epochs left before the limit when step 4 begins.  A scan takes one epoch and a fusion one; a renumbering happens at the start of
# the first scan or fusion that finds the counter at or beyond the limit.  Ring of 3: as tests/test_hip_parity.py -- 3 left: scan 4,
# combine 4, scan 5 take them and combine 5 renumbers; 2 left: scan 5 renumbers.  One-slot ring: an eager scan takes both epochs of a
# step (its own and its speculative fusion's) and the adopting combine none, so with 3 left the counter passes the limit inside
# scan 5 and combine 5 renumbers -- with a speculation waiting, which the renumbering drops --, and only a counter AT the limit
# (0 left) makes a scan renumber: scan 4.
EPOCHS_LEFT = {(3, "combine"): 3, (3, "scan"): 2, (1, "combine"): 3, (1, "scan"): 0}
EPOCH_STEPS = 7


def run_epoch_script(c, site):
    """seven steps of scan k and combine_maps(); the bias is set before step 4; Q after every scan (on the previous map) and after
    every combine of steps 3 .. 5; a raycast product and an occupancy grid kept from step 3 hold their bytes to the end"""
    for k in range(EPOCH_STEPS):
        if k == 4 and c.g is not None:
            c.g.set_tuning("epoch_bias", EPOCH_LIMIT - 2 * 4 - EPOCHS_LEFT[c.bs, site])
        c.scan(k)
        if 4 <= k <= 5:
            c.Q("after scan %d" % k)
        c.combine("sync", "combine %d" % k)
        if 3 <= k <= 5:
            c.Q("after combine %d" % k)
        if k == 3:
            c.keep("combine 3")
    c.Q("the end")
    c.check_kept("the end")
    return c


# ---- the query thread ------------------------------------------------------------------------------------------------------------------
THREAD_STEPS, THREAD_CALLS = 10, 200


def thread_mirror(grid, bs):
    """(maps of the ten steps, A, B): the oracle after scan k and a combine, k = 0 .. 9, and the 512 rays every call of the query
    thread casts (those of the map of step 3, whose ego rr.rays_of starts its families from)"""
    c = Cycle(grid, bs)
    maps = []
    for k in range(THREAD_STEPS):
        c.scan(k)
        c.combine("sync", "step %d" % k)
        maps.append(c.cur)
    inp = maps[rr.N_SCANS - 1].inputs
    return maps, inp["A"], inp["B"]
