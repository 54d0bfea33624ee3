"""Shared by tests/test_voxel_changes_cycle.py (GPU) and tests/test_voxel_changes_cycle_cpu.py (no GPU): the voxel atlas's change query at
every point of the scan cycle.  tests/query_cycle.py has the rule, the mirror and the scripts, tests/voxel_atlas_cycle.py the cycle with a
voxel atlas attached; this file asks that atlas for its changes.

WHY: gvom_voxel_atlas_changes reads the LIVE fused buffers exactly as gvom_voxel_atlas_integrate does -- h->fused[h->cur], its state and
tile tags under the epoch of occ_params(), on the handle's stream behind its own join_second_stream() -- and tests/test_voxel_changes.py
only ever asks it directly behind a synchronous combine_maps(), with a referee fed from the same handle's read_dense().  A changes() that
compared the wrong fused buffer, or read the tags under the epoch before, could agree with that referee; in the per-scan loop (combine,
changes, integrate) it would report phantom objects or miss real ones without any error.

THE REFEREE is tests/voxel_changes_ref.py product() on tests/voxel_atlas_ref.py VoxelAtlasRef, both fed ONLY from the oracle mirror: Map.state
and Map.W of Cycle.cur -- never from the handle's read_dense().  All seven parts with tolerance 0 (voxel_changes_ref.differing_parts),
origin_voxels, n_clusters, marked_columns and dropped as tests/test_voxel_changes.py compares them.

ChangesCycle.Q(label), in this order:
  1  changes(mask 3, min_cells 2, max_clusters 1024) as the FIRST call on the handle after the scan or combine that made the point, held to
     the referee.  On rings of 3 and 4 slots the call's own join is then the one that counts at G, where combine_maps_async() is pending on
     the second stream.
  2  read-only: atlas.counts() and the default atlas.box() (origin and bytes; None before the first integrate) behind that call equal the
     ones taken at the end of the point before (in front of the first point: when the atlas was made).  A scan or a combine does not
     touch the atlas, so this is the state in front of the call -- taken THERE, counts() and box() would wait for and join the streams in
     changes()' place.
  3  the parent's window bundle (qc.Cycle.Q: raycast, viewpoints, alignments, occupancy, dense read)
  4  changes(min_cells 1, max_clusters 3, mask 2 and 1 in turn from point to point), held to the referee; parts 5 (codes) and 6 (columns)
     equal the first call's byte for byte
  5  where the point is in `integrate_at` (None: every point): merge(label) -- integrate on the referee and on the GPU; counts, seq and
     extent as in tests/voxel_atlas_cycle.py --; then words 4 and 5 of the first call's part 3 equal the integrate's free_to_occupied and
     occupied_to_free, unless a following extent moved by a whole side or more on an axis (the rule of the drive test of
     tests/test_voxel_changes.py), and for a fixed extent word 6 equals `outside`.
The atlas's own product bundle (boxes, rays, viewpoints, alignments) is not repeated: tests/test_voxel_atlas_cycle.py has it.

THE TWO SCHEDULES of run_script: EVERY_POINT merges at all twelve points -- at B, C, "H pending", H and I the referee's answer is then all
zeros, where the speculation in the spare buffer of a one-slot ring would give hundreds of codes --; LAGGING merges at A, D, F and K only --
at G, "H pending", H and I the right answer is then the same non-zero product, the map of G against the memory of F, asked four times across
a scan, the end of the asynchronous combine and two rejected scans; J's answer is against the memory of F as well.

Without a handle (g=None: the census) Q records in `trail`, per point: part 3 and the info of the first call's referee, how many clusters
the second call's referee keeps, and -- for every map a wrong answer could come from (Cycle.Q's `others`: the map before, and what a
combine at that moment would give) -- the origin and words 4 .. 6 of the product THAT map would give against the same atlas."""
import functools

import numpy as np

import query_cycle as qc
import raycast_ref as rr
import voxel_atlas_cycle as vac
import voxel_atlas_ref as va
import voxel_changes_ref as vcr

FIRST = (3, 2, 1024)                                          # mask, min_cells, max_clusters of the first call of a point
SECOND_MIN_CELLS, SECOND_CAP = 1, 3                           # of the second call; its mask is 2 and 1 in turn: appeared alone at D and F, vanished alone at G and J
EVERY_POINT = None
LAGGING = ("A", "D", "F", "K")
THREAD_ATLAS = dict(cells=128, levels=64)                     # following
THREAD_CALLS = 100


def changes(atlas, mask, min_cells, cap):
    return atlas.changes(appeared=bool(mask & 1), vanished=bool(mask & 2), min_cells=min_cells, max_clusters=cap)


def hold(ch, want, info, W, what):
    """the product `ch` against the referee's (parts, info) at the window origin W; returns the parts"""
    assert ch is not None, what + ": no data"
    with ch:
        assert tuple(ch.origin_voxels) == tuple(int(v) for v in W), "%s: origin %r, mirror %r" % (what, ch.origin_voxels, W)
        got = ch.copy_to_host()
        assert (ch.n_clusters, ch.marked_columns, ch.dropped) == tuple(info) and ch.rounds >= 1, (what, ch.n_clusters, ch.marked_columns, ch.dropped, info)
    bad = vcr.differing_parts(got, want)
    assert not bad, "%s: parts %r differ; part 3 %r, referee %r" % (what, bad, list(got[3]), list(want[3]))
    return got


def coded(parts):
    """voxels with a code: appeared + vanished (words 4 and 5 of part 3)"""
    return int(parts[3][4]) + int(parts[3][5])


class ChangesCycle(vac.AtlasCycle):
    """AtlasCycle whose points ask the atlas for its changes in front of the window bundle and in front of the merge, and merge only at
    the labels of `integrate_at` (None: everywhere)"""

    def __init__(self, grid, bs, mod=None, stats=False, integrate_at=EVERY_POINT, **kw):
        vac.AtlasCycle.__init__(self, grid, bs, mod, stats, **kw)
        self.integrate_at = integrate_at
        self.asked = 0                                        # points so far: the second call's mask
        self._wanted = {}
        self._first_parts = None                              # the first call's parts at this point (census: the referee's)
        self._extent = None                                   # the referee's extent in front of the merge
        self._snap = self._snapshot()

    # ---- the referee -------------------------------------------------------------------------------------------------------------------
    def origin(self):
        W = tuple(int(v) for v in self.cur.W)
        assert np.array_equal(np.asarray(W, np.float64), self.cur.W)
        return W

    def referee(self, mask, min_cells, cap):
        """product() of the current map against the referee atlas as it stands; kept while neither changes"""
        key = (id(self.cur), self.ref.seq, mask, min_cells, cap)
        if key not in self._wanted:
            if len(self._wanted) > 8:
                self._wanted.clear()
            self._wanted[key] = (self.cur, vcr.product(self.ref, self.cur.state, self.origin(), mask, min_cells, cap))
        return self._wanted[key][1]

    def second(self):
        return 2 - self.asked % 2, SECOND_MIN_CELLS, SECOND_CAP

    # ---- the atlas in front of and behind a call that must only read -----------------------------------------------------------------------
    def _snapshot(self):
        if self.g is None:
            return None
        counts, box = self.atlas.counts(), self.atlas.box()
        if box is None:
            return counts, None
        with box:
            return counts, (tuple(box.origin_voxels),) + tuple(a.tobytes() for a in box.copy_to_host())

    def what(self, label):
        return "%s, ring of %d, point %s (map of %s), voxel changes" % (self.grid, self.bs, label, self.cur.label)

    # ---- the hooks of AtlasCycle.Q -------------------------------------------------------------------------------------------------------
    def P0(self, what):
        vac.AtlasCycle.P0(self, what)
        if self.atlas is not None:
            assert changes(self.atlas, *FIRST) is None, what + ": changes() has data before the first combine"

    def before_bundle(self, label):
        want, info = self.referee(*FIRST)
        if self.g is None:
            self._first_parts = want
            return
        what = self.what(label)
        self._first_parts = hold(changes(self.atlas, *FIRST), want, info, self.origin(), what + ", first call")
        after = self._snapshot()
        assert after[0] == self._snap[0], "%s: changes() wrote the atlas's counts: %r, before %r" % (what, after[0], self._snap[0])
        assert after[1] == self._snap[1], "%s: changes() wrote the atlas: its default box differs from the one before the call" % what

    def before_merge(self, label):
        mask, min_cells, cap = self.second()
        want, info = self.referee(mask, min_cells, cap)
        self._extent = self.ref.E
        if self.g is None:
            self._census(label, info)
        else:
            what = "%s, second call (mask %d)" % (self.what(label), mask)
            got = hold(changes(self.atlas, mask, min_cells, cap), want, info, self.origin(), what)
            first = self._first_parts
            assert got[5].tobytes() == first[5].tobytes() and got[6].tobytes() == first[6].tobytes(), what + ": codes or columns differ from the first call's"
        self.asked += 1

    def merges_at(self, label):
        return self.integrate_at is None or label in self.integrate_at

    def after_merge(self, label, what, W, n, before):
        """the first call's totals against the counts of the integrate behind it (merge() has held the GPU's counts to the referee's)"""
        part3, ref = [int(v) for v in self._first_parts[3]], self.ref
        whole_side = any(abs(ref.E[a] - self._extent[a]) >= ref.sizes()[a] for a in range(3))
        if not whole_side:
            assert (part3[4], part3[5]) == (n["free_to_occupied"], n["occupied_to_free"]), (what, part3, n)
        if not ref.follow:
            assert part3[6] == n["outside"], (what, part3, n)
        if self.trail and self.trail[-1]["label"] == label:
            self.trail[-1].update(merged=True, n=n, whole_side=whole_side)

    def Q(self, label):
        vac.AtlasCycle.Q(self, label)
        self._snap = self._snapshot()

    def integrate_first(self, label):
        """a point of its own kind: changes() with NOTHING in front of it -- the parent's bundle would join the second stream and settle
        the combine before the atlas is asked --, then the merge"""
        self.points.append((label, self.cur, [m for m in (self.prev,) if m is not None]))
        self.before_bundle(label)
        self._extent = self.ref.E
        if self.g is None:
            self._census(label, self.referee(*self.second())[1])
        self.asked += 1
        self.after_merge(label, *self.merge(label))
        self._snap = self._snapshot()

    # ---- the census --------------------------------------------------------------------------------------------------------------------
    def _census(self, label, second_info):
        want, info = self.referee(*FIRST)
        others = []
        for other in self.points[-1][2]:
            W = tuple(int(v) for v in other.W)
            parts, _ = vcr.product(self.ref, other.state, W, *FIRST)
            others.append((other.label, W, [int(v) for v in parts[3][4:7]]))
        self.trail.append(dict(label=label, map=self.cur.label, W=self.origin(), part3=[int(v) for v in want[3]], coded=coded(want),
                               kept=info[0], dropped=info[2], kept_second=second_info[0], others=others, merged=False))


# ---- the query thread ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def changes_thread_mirror(grid, bs):
    """(maps of the ten steps of qc.thread_mirror, the ten referee products): a following 128 x 128 x 64 referee atlas is integrated ONCE,
    with the map of step 0; product k is what changes(*FIRST) must answer while the map of step k is the current one"""
    maps, _, _ = qc.thread_mirror(grid, bs)
    xr, zr, xy, zs = rr.GRIDS[grid]
    ref = va.VoxelAtlasRef(THREAD_ATLAS["cells"], THREAD_ATLAS["levels"], xy, zs)
    origins = [tuple(int(v) for v in m.W) for m in maps]
    ref.integrate(maps[0].state, origins[0])
    return maps, [vcr.product(ref, m.state, W, *FIRST) for m, W in zip(maps, origins)]
