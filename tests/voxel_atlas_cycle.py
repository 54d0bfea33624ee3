"""Shared by tests/test_voxel_atlas_cycle.py (GPU) and tests/test_voxel_atlas_cycle_cpu.py (no GPU): the voxel atlas at every point of
the scan cycle.  tests/query_cycle.py has the rule, the mirror and the scripts; this file attaches a voxel atlas to the cycle.

WHY: gvom_voxel_atlas_integrate merges the LIVE fused buffers -- h->fused[h->cur], its state and tile tags under the epoch of
occ_params(), on the handle's stream behind join_second_stream() -- where the 2-D map atlas merges a DeviceMaps snapshot.  That is the
state that moves underneath a query during a scan cycle: the spare buffer of a one-slot ring holds a speculation after every scan,
combine_maps_async() fuses on the second stream from three filled slots on, an adopting combine flips `cur`, the tile-epoch renumbering
rewrites the fused map's tags, a jump of the window moves a following extent by more than its side.  A wrong buffer, a stale epoch or
a missing join would poison a memory that lasts for the rest of a run.

THE REFEREE is tests/voxel_atlas_ref.py VoxelAtlasRef, fed ONLY from the oracle mirror: Map.state and Map.W of Cycle.cur -- never from
the handle's read_dense().  So the atlas on the GPU is held to (CPU oracle of the pipeline) -> (numpy referee of the atlas), and the two
cannot be wrong together.

AtlasCycle.Q(label) first runs the parent's bundle -- the window queries must hold with an atlas attached and integrates in between --
and then, at EVERY point (B, C, "H pending", H and I included, where the current map has not changed and the referee demands
first_seen = free_to_occupied = occupied_to_free = 0):
  integrate            atlas.integrate() and ref.integrate(cur.state, cur.W); extent_origin, seq and all eleven counts equal
  box                  at the current window (the default) and at the window of the first point (A: remembered space, which a small
                       extent partly loses): classes at every voxel and the four counts
  raycast              the bundle's 512 rays, unknown_blocks True and False, against va.atlas_walk: result rows, world voxel, positions
                       by bit pattern with NaN equal to NaN
  score_viewpoints     the bundle's poses and range against va.viewpoints on ref.dense_state()
  score_alignments     the bundle's cloud and candidates, dilate=1, at the default box and at the first window, against
                       voxel_atlas_align_ref.score
Before the first combine (the P0 hook of run_script) integrate() reports no data and seq stays 0.
run_async_first_script is this file's own: there integrate() is the first call behind an asynchronous combine on the second stream.
Q is made of hooks (before_bundle, before_merge, merges_at, after_merge) that do nothing here: tests/voxel_changes_cycle.py puts the
atlas's change query in front of the bundle and of the merge, and merges only where its schedule says.

Without a handle (g=None: the census) Q records in `trail`, per point, the referee's counts, and -- for every map a wrong answer would
come from (Cycle.Q's `others`: the map before, and what a combine at that moment would give) -- the counts that merging THAT map would
have given and how many world voxels it would have left in another class; and how many of the 512 rays that the window answers
LEFT_WINDOW the atlas answers otherwise."""
import copy
import functools

import numpy as np

import query_cycle as qc
import raycast_ref as rr
import viewpoint_ref as vr
import voxel_atlas_align_ref as vaa
import voxel_atlas_ref as va

F32 = np.float32
FOLLOWING = dict(cells=64, levels=32, follow=True)            # the smallest legal atlas; on p2 exactly the window's size
CHANGED_VOXELS_FLOOR = 1000                                   # world voxels in another class after merging a wrong map
THREAD_INTEGRATES = 40


def fixed(offset):
    """a fixed 128 x 128 x 64 atlas whose corner lies `offset` voxels below the window origin of point A"""
    return dict(cells=128, levels=64, follow=False, offset=tuple(offset))


@functools.lru_cache(maxsize=None)
def first_window(grid):
    """the window origin of point A (scan 0, combined), from the mirror: a fixed atlas is placed before the first scan"""
    c = qc.Cycle(grid, 1)
    c.scan(0)
    c.combine("sync", "A")
    return tuple(int(v) for v in c.cur.W)


def world_difference(a, b):
    """world voxels that two VoxelAtlasRef hold in different classes; outside its extent an atlas knows nothing (NEVER)"""
    ov = a._overlap(b.E, b.sizes())
    known_a, known_b = int((a.cls != va.NEVER).sum()), int((b.cls != va.NEVER).sum())
    if ov is None:
        return known_a + known_b
    sb, sa = ov
    ca, cb = a.cls[sa], b.cls[sb]
    return int((ca != cb).sum()) + known_a - int((ca != va.NEVER).sum()) + known_b - int((cb != va.NEVER).sum())


def rays_rescued(window, atlas):
    """rays that the window answers LEFT_WINDOW and the atlas otherwise (result rows of rr.walk and va.walk)"""
    return int(((window[:, 0] == rr.LEFT_WINDOW) & (atlas[:, 0] != va.LEFT)).sum())


# ---- holding the GPU's products to the referee ---------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def hold_box(box, want, origin, what):
    assert box is not None, what + ": no data"
    with box:
        assert tuple(box.origin_voxels) == tuple(int(v) for v in origin), (what, box.origin_voxels, origin)
        classes, counts = box.copy_to_host()
    assert classes.dtype == np.uint8 and classes.shape == want[0].shape, what
    assert np.array_equal(classes, want[0]), "%s: %d voxels of the box differ" % (what, int((classes != want[0]).sum()))
    assert np.array_equal(counts, want[1]), "%s: box counts %r, referee %r" % (what, counts.tolist(), want[1].tolist())
    return classes, counts


def same_rays(got, want):
    """(result, position, voxel) twice: rows and voxels equal, positions by bit pattern with NaN equal to NaN"""
    (r, p, v), (wr, wp, wv) = got, want
    if r.shape != wr.shape or not np.array_equal(r, wr) or not np.array_equal(v, wv):
        return False
    return bool(((_bits(p) == _bits(wp)) | (np.isnan(p) & np.isnan(wp))).all()) and np.array_equal(np.isnan(p), np.isnan(wp))


def hold_rays(rays, want, E, what):
    assert rays is not None, what + ": no data"
    with rays:
        assert tuple(rays.extent_origin) == tuple(int(v) for v in E), (what, rays.extent_origin, E)
        got = rays.copy_to_host()
    result, position, voxel = got
    assert result.dtype == np.int32 and position.dtype == F32 and voxel.dtype == np.int32 and result.shape == want[0].shape, what
    if not np.array_equal(result, want[0]):
        bad = np.flatnonzero((result != want[0]).any(axis=1))
        raise AssertionError("%s: %d rays differ, first %d: got %r, referee %r" % (what, len(bad), bad[0], result[bad[0]], want[0][bad[0]]))
    assert same_rays(got, want), what + ": positions or voxels differ"


# ---- the cycle with a voxel atlas attached ---------------------------------------------------------------------------------------------
class AtlasCycle(qc.Cycle):
    """qc.Cycle with a voxel atlas on the handle (created before P0) and a VoxelAtlasRef beside it that only the mirror feeds.
    `offset` (fixed atlases): the extent's corner = the window origin of A - offset."""

    def __init__(self, grid, bs, mod=None, stats=False, cells=64, levels=32, follow=True, offset=None, **kw):
        qc.Cycle.__init__(self, grid, bs, mod, stats, **kw)
        xr, zr, xy, zs = rr.GRIDS[grid]
        self.res, self.window = (xr, xr, zr), (xy, xy, zs)
        E = (0, 0, 0) if follow else tuple(w - o for w, o in zip(first_window(grid), offset))
        self.ref = va.VoxelAtlasRef(cells, levels, xy, zs, follow=follow, origin=E)
        self.atlas = None
        if self.g is not None:
            self.atlas = self.g.create_voxel_atlas(cells, levels, follow=follow, origin_voxels=None if follow else np.array(E))
            assert self.atlas.extent_origin == E
        self.first = None                                     # the window origin of the first point
        self.merged = None                                    # the Map of the last integrate
        self.trail = []
        self._asked = None

    def P0(self, what):
        if self.atlas is None:
            return
        assert self.atlas.integrate() is False, what + ": integrate() merged something before the first combine"
        counts = self.atlas.counts()
        assert counts["seq"] == 0 and self.atlas.seq == 0 and not any(counts.values()), (what, counts)
        assert self.atlas.box() is None, what

    def _referee(self, which):
        """the referee's answers to the atlas half of the bundle, now: `which` of rays, viewpoints, alignments (and always the two
        boxes).  What only depends on the classes, the extent and the inputs is kept while none of them changes."""
        ref, inp = self.ref, self.cur.inputs
        kept = self._asked
        if kept is None or kept[0] is not self.cur or kept[1] != ref.E or not np.array_equal(kept[2], ref.cls):
            kept = self._asked = (self.cur, ref.E, ref.cls.copy(), {})
        w = kept[3]
        for ub in (True, False):
            if "rays" in which and ("rays", ub) not in w:
                w["rays", ub] = va.atlas_walk(ref, self.res, inp["A"], inp["B"], unknown_blocks=ub)
        if "viewpoints" in which and "viewpoints" not in w:
            d, o = vr.model(qc.MODEL)
            w["viewpoints"] = va.viewpoints(ref.dense_state(), ref.E, ref.sizes(), self.res, d, o, inp["poses"], inp["range"])
        for B in (ref.last_origin, self.first):
            if "alignments" in which and ("alignments", B) not in w:
                w["alignments", B] = vaa.score(ref, B, self.grid, inp["cloud"], inp["M"], 1)
        out = dict(w)
        out["box", None], out["box", self.first] = ref.box(), ref.box(self.first)
        return out

    def merge(self, label):
        """integrate() on the referee and on the GPU, nothing in front of it: extent_origin, seq and the eleven counts.  Returns
        (what, W, the referee's counts of this integrate, the referee as it stood before -- the census only)"""
        cur, ref = self.cur, self.ref
        W = tuple(int(v) for v in cur.W)
        assert np.array_equal(np.asarray(W, np.float64), cur.W)
        if self.first is None:
            self.first = W
        what = "%s, ring of %d, point %s (map of %s), voxel atlas" % (self.grid, self.bs, label, cur.label)
        before = copy.deepcopy(ref) if self.g is None else None
        n = ref.integrate(cur.state, W)
        if cur is self.merged:                                # B, C, "H pending", H, I: the same map again changes no class
            assert n["first_seen"] == n["free_to_occupied"] == n["occupied_to_free"] == 0, (what, n)
            assert n["cleared"] == n["cleared_observed"] == 0, (what, n)
        self.merged = cur
        if self.g is not None:
            atlas = self.atlas
            assert atlas.integrate() is True, what + ": integrate() reports no data"
            assert atlas.extent_origin == ref.E and atlas.seq == ref.seq, (what, atlas.extent_origin, ref.E, atlas.seq, ref.seq)
            got, want = atlas.counts(), ref.counts()
            assert tuple(got) == va.COUNT_NAMES and got == want, "%s: counts %r, referee %r" % (what, got, want)
        return what, W, n, before

    # the hooks of a subclass (tests/voxel_changes_cycle.py): calls in front of the parent's bundle, calls in front of the merge, points
    # without a merge, and what follows a merge in place of the atlas's own product bundle
    def before_bundle(self, label):
        pass

    def before_merge(self, label):
        pass

    def merges_at(self, label):
        return True

    def Q(self, label):
        self.before_bundle(label)
        qc.Cycle.Q(self, label)
        self.before_merge(label)
        if self.merges_at(label):
            self.after_merge(label, *self.merge(label))

    def after_merge(self, label, what, W, n, before):
        if self.g is None:
            self._census(label, before, n, W)
            return
        atlas, ref, inp = self.atlas, self.ref, self.cur.inputs
        w = self._referee(("rays", "viewpoints", "alignments"))
        hold_box(atlas.box(), w["box", None], W, what + ": box()")
        hold_box(atlas.box(np.array(self.first)), w["box", self.first], self.first, what + ": box(first window)")
        for ub in (True, False):
            hold_rays(atlas.raycast(inp["A"], inp["B"], unknown_blocks=ub), w["rays", ub], ref.E, "%s: raycast, unknown_blocks %d" % (what, ub))
        qc.hold_viewpoints(atlas.score_viewpoints(inp["poses"], inp["range"]), w["viewpoints"], np.array(ref.E, np.float64), what + ": score_viewpoints")
        r = atlas.score_alignments(inp["cloud"], inp["M"], dilate=1)
        assert r is not None and r.origin_voxels == W, (what, r)
        qc.hold_alignments(r, w["alignments", W], np.array(W, np.float64), what + ": score_alignments, default box")
        r = atlas.score_alignments(inp["cloud"], inp["M"], dilate=1, origin_voxels=np.array(self.first))
        assert r is not None and r.origin_voxels == self.first, (what, r)
        qc.hold_alignments(r, w["alignments", self.first], np.array(self.first, np.float64), what + ": score_alignments, first window")

    def integrate_first(self, label):
        """a point of its own kind: integrate() with NOTHING in front of it -- the parent's bundle would join the second stream and
        settle the combine before the atlas is asked -- then the counts and the default box"""
        self.points.append((label, self.cur, [m for m in (self.prev,) if m is not None]))
        what, W, n, before = self.merge(label)
        if self.g is None:
            self._census(label, before, n, W)
        else:
            hold_box(self.atlas.box(), self.ref.box(), W, what + ": box()")

    def _census(self, label, before, n, W):
        ref = self.ref
        others = []
        for other in self.points[-1][2]:
            wrong = copy.deepcopy(before)
            m = wrong.integrate(other.state, tuple(int(v) for v in other.W))
            others.append((other.label, m, world_difference(ref, wrong)))
        walked = self._referee(("rays",))["rays", True][0]
        self.trail.append(dict(label=label, n=n, counts=ref.counts(), W=W, E=ref.E, others=others,
                               rescued=rays_rescued(self.cur.want["rays", True][0], walked),
                               status=np.bincount(walked[:, 0], minlength=5).tolist()))


def run_async_first_script(c):
    """integrate() as the FIRST call behind a combine_maps_async() that fuses on the second stream (three scans fill a ring of 3 or
    4 slots before it begins): the join with that stream is then integrate()'s own.  In run_script the parent's bundle comes first at
    G and joins for it.  Returns c"""
    assert c.bs >= 3
    for k in range(3):
        c.scan(k)
    c.combine("sync", "first"); c.Q("first")
    c.scan(3)
    c.combine("async", "second")
    c.integrate_first("second, pending")
    c.finish("second"); c.Q("second")
    return c


# ---- the integrating thread's replay ---------------------------------------------------------------------------------------------------
def replay(kept, maps, grid, A, B, cells=64, levels=32):
    """kept: what the second thread recorded after each of its integrates -- (box origin, box classes, box counts, extent origin of the
    rays, result, position, voxel).  The box's origin names the map the integrate merged (the ten origins are distinct).  Replays
    exactly that subsequence of the mirror's maps into a fresh VoxelAtlasRef and holds every recorded answer to the referee at that
    point of the replay.  Returns the merged steps."""
    xr, zr, xy, zs = rr.GRIDS[grid]
    step_of = {tuple(int(v) for v in m.W): k for k, m in enumerate(maps)}
    assert len(step_of) == len(maps)
    ref = va.VoxelAtlasRef(cells, levels, xy, zs)
    steps, walked = [], None
    for i, (origin, classes, counts, extent, result, position, voxel) in enumerate(kept):
        assert tuple(origin) in step_of, "integrate %d: its box has an origin no map of the run has: %r" % (i, origin)
        k = step_of[tuple(origin)]
        what = "integrate %d (the map of step %d)" % (i, k)
        was = (ref.E, ref.cls.copy())
        ref.integrate(maps[k].state, tuple(origin))
        want = ref.box()
        assert np.array_equal(classes, want[0]), "%s: %d voxels of the box differ from the replay" % (what, int((classes != want[0]).sum()))
        assert np.array_equal(counts, want[1]), "%s: box counts %r, replay %r" % (what, counts.tolist(), want[1].tolist())
        assert tuple(extent) == ref.E, (what, extent, ref.E)
        if walked is None or was[0] != ref.E or not np.array_equal(was[1], ref.cls):
            walked = va.atlas_walk(ref, (xr, xr, zr), A, B, unknown_blocks=True)
        assert same_rays((result, position, voxel), walked), "%s: the rays differ from the replay" % what
        steps.append(k)
    return steps
