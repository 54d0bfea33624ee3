"""The mirror of STATISTICS ON DEMAND (include/gvom_hip.h GVOM_FLAG_STATISTICS_ON_DEMAND; fuse_impl in g-vom_amd/csrc/gvom_combine.hip;
stats_demand / release_statistics_buffers in gvom_handle.hip): a subclass of oracle.OracleGvom that restates, in plain Python, when the
default `gvom.Gvom(...)` computes the per-voxel statistics, when it merges them, and what a read returns -- and the scenes and scripts
that tests/test_stats_on_demand_cpu.py (mirror alone) and tests/test_stats_on_demand.py (the library against the mirror) share.

THE RULE
  state      on (True at start), idle, has[slot] per ring slot, fused_has.
  scan       an ACCEPTED scan computes its slot's metrics iff `on` and sets has[slot] = on.  A rejected scan (empty cloud, only NaN
             returns, no overlap) changes nothing.
  combine    with a filled last slot: if on, idle += 1, and past IDLE_THRESHOLD `on`, every has[] and fused_has go False (the buffers
             are released) -- the code's test is `++stats_idle > 3`, so this is the FOURTH unread combine, and it merges none.
             It merges statistics iff on and every filled slot has its own.  With statistics: the slots through
             orc_combine_metrics_full_f64 in slot order, then the previous map -- through orc_combine_metrics_full_f32 if fused_has,
             else through orc_combine_metrics (counts and minimum height only: "restarted from the ring") -- then the eigenvalues.
             Without: the plain combine; combined_metrics, last_combined_metrics and voxels_eigenvalues are None.  fused_has = merged.
  read       idle = 0.  If `on` was False it becomes True and the read returns no data.  Otherwise it returns data iff the thing
             read -- the fused map, or that slot -- has statistics.

ROWS WITHOUT RETURNS.  A fused voxel that only a previous map WITHOUT statistics knows has an all-zero metrics row: count (column 9)
0.  The reference's merge (gvom.py:858-909) divides by the sum of the two counts, and an always-on mapper never sees 0 there (a voxel
with a hit counts itself).  After a restart it does, one combine later: such a row as the previous map's, merged into a voxel no slot
holds, is 0 / 0.  The rule: A PREVIOUS ROW OF COUNT 0 CONTRIBUTES ITS HIT COUNTS AND ITS MINIMUM HEIGHT AND NO STATISTICS, exactly like
a row of a previous map without statistics.  The mirror states it without new arithmetic: the previous map's index map is split into
the rows with returns (orc_combine_metrics_full_f32) and the rows without (orc_combine_metrics); a voxel is in one of the two.

WRONG MIRRORS (tests/test_stats_on_demand_cpu.py: what the GPU tests must be able to tell from the right one)
  "stale"    keeps and merges the statistics through the pause as if there had been none: its numbers are an always-on oracle's.
  "no_prev"  never merges a previous map's statistics at all."""
import numpy as np

from oracle import oracle

IDLE_THRESHOLD = 3            # fuse_impl: `++stats_idle > 3` -- off at combine number IDLE_THRESHOLD + 1 without a read
FUSED = "fused"
_p = oracle._p


class DemandOracle(oracle.OracleGvom):
    def __init__(self, *params, **kw):
        self.wrong = kw.pop("wrong", None)
        assert self.wrong in (None, "stale", "no_prev")
        kw["voxel_statistics"] = True
        super(DemandOracle, self).__init__(*params, **kw)
        self.on, self.idle = True, 0
        self.has = [False] * self.buffer_size
        self.fused_has = False
        self.combines = 0                                  # combines that found a filled last slot

    # ---- the three events ------------------------------------------------------------------------------------------------
    def process_pointcloud(self, pointcloud, ego_position, transform=None):
        b, before = self.buffer_index, self.origin_buffer[self.buffer_index]
        compute = self.on or self.wrong == "stale"
        self.voxel_statistics = compute
        try:
            super(DemandOracle, self).process_pointcloud(pointcloud, ego_position, transform)
        finally:
            self.voxel_statistics = True
        if self.origin_buffer[b] is before:                # rejected: the ring is untouched
            return False
        self.has[b] = self.on
        return True

    def combine_maps(self):
        if self.origin_buffer[self.last_buffer_index] is None:
            return super(DemandOracle, self).combine_maps()
        self.combines += 1
        if self.on:
            self.idle += 1
            if self.idle > IDLE_THRESHOLD:
                self.on = False
                self.has = [False] * self.buffer_size
                self.fused_has = False
                if self.wrong != "stale":
                    self.metrics_buffer = [None] * self.buffer_size
                    self.last_combined_metrics = None
        merged = self.on and all(self.has[i] for i in range(self.buffer_size) if self.origin_buffer[i] is not None)
        self.voxel_statistics = merged or self.wrong == "stale"
        try:
            out = super(DemandOracle, self).combine_maps()
        finally:
            self.voxel_statistics = True
        if not merged and self.wrong != "stale":
            self.combined_metrics = self.last_combined_metrics = self.voxels_eigenvalues = None
        self.fused_has = merged
        return out

    def read(self, which=FUSED):
        """a read of the statistics of the fused map or of ring slot `which`: True where it returns data"""
        was_on, self.idle = self.on, 0
        if not was_on:
            self.on = True
            return False
        return self.fused_has if which == FUSED else bool(self.has[which])

    # ---- the merge -------------------------------------------------------------------------------------------------------
    def _combine_with_statistics(self, Cc):
        L = oracle.lib()
        xy, zs = self.xy_size, self.z_size
        self.combined_metrics = np.zeros((Cc, 10), np.float32)
        fused = (self.combined_hit_count, self.combined_total_count, self.combined_min_height, self.combined_index_map, self.combined_origin)
        for i in range(self.buffer_size):
            if self.origin_buffer[i] is None:
                continue
            L.orc_combine_metrics_full_f64(_p(self.combined_metrics), *[_p(a) for a in fused],
                                           _p(self.metrics_buffer[i]), _p(self.hit_count_buffer[i]), _p(self.total_count_buffer[i]),
                                           _p(self.min_height_buffer[i]), _p(self.index_buffer[i]), _p(self.origin_buffer[i]), xy, zs)
        if self.last_combined_origin is not None:
            prev = (self.last_combined_hit_count, self.last_combined_total_count, self.last_combined_min_height)
            lim = self.last_combined_index_map
            with_stats = (self.fused_has and self.wrong != "no_prev") or self.wrong == "stale"
            if with_stats:
                # rows with returns merge their statistics; rows without (count 0) their hit counts and minimum height only
                empty = np.zeros(lim.shape, bool)
                occ = lim >= 0
                empty[occ] = self.last_combined_metrics[lim[occ], 9] == 0
                L.orc_combine_metrics_full_f32(_p(self.combined_metrics), *[_p(a) for a in fused], _p(self.last_combined_metrics),
                                               *[_p(a) for a in prev], _p(np.where(empty, np.int32(-1), lim)), _p(self.last_combined_origin), xy, zs)
                lim = np.where(empty, lim, np.int32(-1))
            L.orc_combine_metrics(*[_p(a) for a in fused], *[_p(a) for a in prev], _p(np.ascontiguousarray(lim)), _p(self.last_combined_origin), xy, zs)
        self.last_combined_metrics = self.combined_metrics
        self.voxels_eigenvalues = np.zeros((Cc, 3), np.float32)
        L.orc_calculate_eigenvalues(_p(self.voxels_eigenvalues), _p(self.combined_metrics), Cc)

    def make_debug_voxel_map(self):
        """(no read by itself: the tests call read() where the library's call counts as one)"""
        if self.voxels_eigenvalues is None:
            return None
        return super(DemandOracle, self).make_debug_voxel_map()


# ---- scenes ------------------------------------------------------------------------------------------------------------------
# The fusion routes are tests/test_hip_parity.py's _ROUTES, at their own shapes: the smallest at which each kernel runs.
ROUTE_SCENES = ("encfuse_64x32", "encfuse_48x20", "fuse1_36x32", "fuse4x2_64x32", "fuse4x4_64x32_b3", "fuse4x4_64x32_b4",
                "fuse_short_50x13", "fuse_tall_16x300", "descs_mem_32x16")
READS = ("make_debug_voxel_map", "voxels_eigenvalues", "metrics_buffer", "combined_metrics", "voxel_cloud_device")
SMALL = (0.4, 0.2, 32, 16)                                 # xy_res, z_res, xy, zs of the scenes of cases B to F
UNREAD = 6                                                 # unread combines of a pause in the scripts: IDLE_THRESHOLD + 1 and two more


def _hp():
    import test_hip_parity as hp                           # (_ROUTES, _surface_steps, _same_maps: the scenes and the map rule of the route matrix)
    return hp


def _scans(steps):
    return [s[1:] for s in steps if s[0] == "scan"]


def route_scene(name):
    """(params, scans, route) of a _ROUTES entry, long enough for script A"""
    hp = _hp()
    xy, zs, buf, z_res, _, route = hp._ROUTES[name]
    params = (0.4, z_res, xy, zs, buf, 0.5, 0.5, 0.5, 0.3, 2.0, 2.0, 1.0, 1, 1)
    long_ring = buf > 4
    steps = hp._surface_steps(xy * 100 + zs + buf, xy, zs, 0.4, z_res, a_length(buf), 1500 if long_ring else 4000,
                              move=(0.25, -0.15, 0.02) if long_ring else (0.45, -0.3, 0.04))
    return params, _scans(steps), route


def small_scene(bs, n_scans, seed=4):
    xr, zr, xy, zs = SMALL
    params = (xr, zr, xy, zs, bs, 0.5, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
    # (the sensor climbs a quarter as fast as in the route matrix: the longest script here has 43 scans, and the surface stays inside a 3.2 m window)
    return params, _scans(_hp()._surface_steps(seed, xy, zs, xr, zr, n_scans, 3000, move=(0.45, -0.3, 0.01)))


def a_length(bs):
    """combines of script A on a ring of bs slots: 0-2 read, 3-8 unread, 9 .. 9 + bs read (the cloud returns at 9 + bs), four more"""
    return 3 + UNREAD + bs + 1 + 4


def rows_differing(a, b, factor=10.0):
    """rows of two fused metrics arrays (same rows) that differ by more than `factor` times parity.STATS_TOL["fused"] in
    stats_deviation's measure, or in their count column; a NaN differs from everything"""
    import parity
    t, sc = parity.STATS_TOL["fused"]
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    with np.errstate(invalid="ignore"):
        d = np.abs(a[:, :9] - b[:, :9]) / (np.abs(b[:, :9]) + sc)
        far = ~(d <= factor * t)
    return int(np.count_nonzero(far.any(axis=1) | (a[:, 9] != b[:, 9])))


# ---- one run: the mirror, its followers and -- on the GPU -- the library, driven together -------------------------------------
class Run:
    """Drives the mirror `w` (a DemandOracle), the followers (name -> any OracleGvom: an always-on oracle, a plain one, wrong
    mirrors) and, where `g` is given, the library's mapper through the same scans, combines and reads.
      combine()  the mirror's maps equal every follower's bit for bit (they never depend on the statistics); the library's are held
                 as tests/test_hip_parity.py _same_maps holds them, with the fused cell count and the route where one is named
      read()     the library and the mirror agree on data or no data -- for the fused map and for every ring slot -- and where there
                 is data the library is held by parity.compare_statistics to `referee` (default: the mirror)
    `trail` records ("combine", k, merged, restarted, previous map had statistics) and ("read", k, data, slots with data)."""

    def __init__(self, params, g=None, followers=None, route=None, what=""):
        self.params, self.g, self.route, self.what = params, g, route, what
        self.w = DemandOracle(*params)
        self.followers = dict(followers or {})
        self.referee = None
        self.k = -1                                        # index of the last combine
        self.pauses = 0
        self.trail, self.last = [], None
        self.has_prev = False
        self.on_combine = None                             # hook(run), after every combine (the census)

    def _all(self):
        return [self.w] + list(self.followers.values())

    def tag(self):
        return "%s combine %d: " % (self.what, self.k)

    def scan(self, pc, ego, tf=None):
        took = [m.process_pointcloud(np.array(pc, copy=True), ego, tf) for m in self._all()]
        assert took[0] is True, self.tag() + "the scene's scan was rejected"
        if self.g is not None:
            self.g.process_pointcloud(pc, ego, tf)

    def reject(self, kind, ego):
        """a scan that must change nothing: "empty", "nan" (only NaN returns; the oracle, which ros_numpy shields from them, is
        handed the empty cloud) or "far" (no overlap)"""
        far = np.full((5, 3), 4000.0, np.float32)
        for m in self._all():
            before = (m.buffer_index, m.last_buffer_index)
            m.process_pointcloud(far.copy() if kind == "far" else np.zeros((0, 3), np.float32), ego)
            assert (m.buffer_index, m.last_buffer_index) == before
        if self.g is not None:
            before = (self.g.buffer_index, self.g.last_buffer_index)
            self.g.process_pointcloud({"empty": np.zeros((0, 3), np.float32), "nan": np.full((64, 3), np.nan, np.float32), "far": far}[kind], ego)
            assert (self.g.buffer_index, self.g.last_buffer_index) == before, self.tag() + kind

    def combine(self, form="sync", read=None):
        """form: "sync" | "async" | "async_read_first" (a read of combined_metrics before .result()) | "device" | "occupancy";
        read: None, "full" or one of READS -- made after the combine"""
        w = self.w
        was_on, prev_had = w.on, w.fused_has
        outs = [m.combine_maps() for m in self._all()]
        b = outs[0]
        assert b is not None
        self.k += 1
        for name, o in zip(self.followers, outs[1:]):
            for i in range(5):
                assert np.array_equal(b[i], o[i]), self.tag() + "map %d of %s" % (i, name)
        if was_on and not w.on:
            self.pauses += 1
        self.last = ("combine", self.k, w.fused_has, w.fused_has and self.pauses > 0, prev_had)
        self.trail.append(self.last)
        begun = self._begin_gpu(form) if self.g is not None else None
        if form == "async_read_first":                     # a read while the combine is pending
            self.read("combined_metrics")
        if self.g is not None:
            self._finish_gpu(form, begun, b)
        self.has_prev = True
        if self.on_combine is not None:
            self.on_combine(self)
        if read is not None:
            return self.read(read)

    def _begin_gpu(self, form):
        g = self.g
        if form == "sync":
            return g.combine_maps()
        if form in ("async", "async_read_first"):
            return g.combine_maps_async()
        if form == "device":
            return g.combine_maps_device()
        if form == "occupancy":
            return g.combine_maps_occupancy()
        raise ValueError(form)

    def _finish_gpu(self, form, begun, b):
        g, tag = self.g, self.tag()
        hp = _hp()
        assert begun is not None, tag + form
        a = begun
        if form in ("async", "async_read_first"):
            a = begun.result()
        elif form == "device":
            with begun as m:
                a = (m.origin, m.positive.copy_to_host(), m.negative.copy_to_host(), m.roughness.copy_to_host(), m.visibility.copy_to_host())
        elif form == "occupancy":
            assert np.array_equal(begun[0], b[0]), tag
            for name, x, y in zip(("hard", "soft", "certainty", "negative", "roughness"), begun[1:], oracle.ros_occupancy_grids(b)):
                assert x.dtype == np.int8 and np.array_equal(x, y), tag + name
            a = None
        if a is not None:
            hp._same_maps(a, b, tag + form)
        assert g.combined_cell_count_cpu == self.w.combined_cell_count_cpu, tag
        if self.route is not None and form == "sync":
            filled = sum(o is not None for o in self.w.origin_buffer)
            want = self.route(self.k, filled, self.has_prev)
            if want is not None:
                assert g.get_tuning("fuse_kernel") == want, (tag, filled, g.get_tuning("fuse_kernel"), want)

    def not_a_read(self):
        """calls that must NOT count as a read of the statistics (the mirror is told nothing)"""
        g, w = self.g, self.w
        if g is None:
            return
        import gvom
        d = g.read_dense(gvom.GVOM_WHICH_FUSED)
        import scenarios
        ws = scenarios.dense_from_compact(w.combined_index_map, w.combined_hit_count, w.combined_total_count, w.combined_min_height)
        for x, y in zip(d[:4], ws):
            assert np.array_equal(x, np.asarray(y)), self.tag() + "read_dense"
        assert g.read_dense(g.last_buffer_index) is not None
        np.testing.assert_allclose(g.make_debug_height_map(), w.make_debug_height_map(), rtol=0, atol=1e-5, err_msg=self.tag())
        occ = w.get_map_as_occupancy_grid()
        assert np.array_equal(g.get_map_as_occupancy_grid(), occ), self.tag()
        with g.occupancy_grid_device() as grid:
            assert np.array_equal(grid.copy_to_host().astype(bool), occ), self.tag()

    def read(self, how="full"):
        w = self.w
        data = w.read()
        for f in self.followers.values():
            if isinstance(f, DemandOracle):
                f.read()
        slots = tuple(bool(w.has[i]) and w.origin_buffer[i] is not None for i in range(w.buffer_size))
        self.trail.append(("read", self.k, data, slots))
        g, tag = self.g, self.tag()
        if g is None:
            return data
        ref = self.referee or w
        if how != "full":
            got = getattr(g, how)
            got = got() if callable(got) else got
            if how == "metrics_buffer":
                assert tuple(m is not None for m in got) == slots, tag + how
            else:
                assert (got is not None) == data, tag + how
                if how == "combined_metrics" and data:     # (the form that needs no fused cell count: also while an asynchronous combine is pending)
                    import parity
                    gc, wc = got.copy_to_host(), parity.voxel_order(ref.combined_index_map, ref.combined_metrics)
                    assert gc.shape == wc.shape and np.array_equal(gc[:, 9], wc[:, 9]), tag + "fused counts"
                    parity._within("fused", gc[:, :9], wc[:, :9], parity.STATS_TOL, {}, tag)
                if how == "voxel_cloud_device" and got is not None:
                    got.release()
            return data
        import parity
        cloud = g.make_debug_voxel_map()
        assert (cloud is not None) == data, tag + "make_debug_voxel_map: %s, the mirror: %s" % ("data" if cloud is not None else "none", "data" if data else "none")
        assert tuple(m is not None for m in g.metrics_buffer) == slots, tag + "metrics_buffer"
        dev_cloud = g.voxel_cloud_device()
        assert (dev_cloud is not None) == data, tag + "voxel_cloud_device"
        if data:
            with dev_cloud:
                rows = dev_cloud.copy_to_host()
            assert np.array_equal(parity.cloud_voxel_order(rows).view(np.uint32), parity.cloud_voxel_order(cloud).view(np.uint32)), tag + "voxel_cloud_device rows"
            parity.compare_statistics(g, ref, what=tag)
        else:
            assert g.combined_metrics is None and g.last_combined_metrics is None and g.voxels_eigenvalues is None, tag + "paused or restarting"
            if slots[w.last_buffer_index]:
                parity.compare_statistics(g, ref, what=tag, fused=False)
        return data


# ---- scripts -----------------------------------------------------------------------------------------------------------------
def script_a(run, scans):
    """one pause: reads after combines 0 to 2, none after 3 to 8, then after every combine; returns the data / no-data pattern of
    the reads from combine 9 on"""
    bs = run.w.buffer_size
    assert len(scans) == a_length(bs)
    pattern = []
    for k, s in enumerate(scans):
        run.scan(*s)
        unread = 3 <= k < 3 + UNREAD
        got = run.combine(read=None if unread else "full")
        if k < 3:
            assert got is True, run.tag()
        elif not unread:
            pattern.append(got)
    return pattern


def a_pattern(bs):
    """no data at combine 9 (the demand) and while the ring turns over; data from combine 9 + bs on"""
    return [False] * bs + [True] * 5


def b_length(bs):
    return 3 + len(READS) * (IDLE_THRESHOLD + 1 + bs + 1) + IDLE_THRESHOLD + 1


def script_b(run, scans):
    """what counts as a read: five pauses, each behind IDLE_THRESHOLD + 1 combines with only calls that are NOT reads in between, each
    ended by another of READS; the statistics that restart are held at every combine until they have been merged as a previous map;
    at the end the sentence of the issue: four such combines, and the next make_debug_voxel_map() returns None"""
    bs, it = run.w.buffer_size, iter(scans)
    assert len(scans) == b_length(bs)

    def step(read):
        run.scan(*next(it))
        return run.combine(read=read)

    def idle_combines():
        for _ in range(IDLE_THRESHOLD + 1):
            assert run.w.on, run.tag()
            step(None)
            run.not_a_read()
        assert not run.w.on, run.tag()

    for _ in range(3):
        assert step("full") is True
    for how in READS:
        idle_combines()
        assert run.read(how) is False and run.w.on, run.tag() + how          # the demand finds nothing and switches them on
        for j in range(bs):
            assert step("full") is (j == bs - 1), (run.tag(), how, j)
        assert step("full") is True, (run.tag(), how)
    idle_combines()
    assert run.read("make_debug_voxel_map") is False


def script_c(run, scans, period):
    """a reader of every period-th combine; returns the data / no-data pattern of its reads"""
    got = []
    for k, s in enumerate(scans):
        run.scan(*s)
        got.append(run.combine(read="full" if (k + 1) % period == 0 else None))
    return [d for d in got if d is not None]


D_AFTER = ("async", "device", "occupancy", "sync", "async_read_first", "async", "device")


def d_length(bs):
    return 3 + UNREAD + 1 + bs + 4


def script_d(run, scans):
    """every combine form through a pause and a restart; a combine with no scan in between and two rejected scans once during the
    pause and once between the demand and the next accepted scan; the demand itself is a read while an asynchronous combine is
    pending.  Returns the pattern of the full reads from the demand on."""
    bs, it = run.w.buffer_size, iter(scans)
    assert len(scans) == d_length(bs)
    ego = [None]

    def step(form, read):
        s = next(it)
        ego[0] = s[1]
        run.scan(*s)
        return run.combine(form, read)

    for _ in range(3):
        assert step("sync", "full") is True
    for form in ("async", "device", "occupancy", "sync"):                      # the fourth switches them off
        step(form, None)
    assert not run.w.on
    run.combine("sync")                                                        # paused: a combine with no scan in between,
    run.reject("nan", ego[0])                                                  # two rejected scans,
    run.reject("far", ego[0])
    step("device", None)                                                       # and two more combines nobody reads
    step("async", None)
    pattern = [step("async_read_first", "full")]                               # the demand: made while the combine is pending
    assert run.w.on and pattern == [False]
    pattern.append(run.combine("sync", "full"))                                # no scan in between: the ring still has no statistics
    run.reject("empty", ego[0])
    run.reject("far", ego[0])
    for j in range(bs + 4):
        pattern.append(step(D_AFTER[j], "full"))
    return pattern


def d_pattern(bs):
    return [False, False] + [False] * (bs - 1) + [True] * 5


def e_length(bs):
    return 3 + UNREAD + 1 + bs + 3


def script_e(run, scans, always):
    """a restart behind a jump of three window widths: the scan whose combine merges statistics again, and every scan after it, lies
    where nothing of the previous map -- nor of the slots before -- overlaps; from there on the referee is `always`, an always-on
    oracle among the followers"""
    bs = run.w.buffer_size
    assert len(scans) == e_length(bs)
    jump_at = 3 + UNREAD + bs
    width = 3.0 * run.w.xy_size * run.w.xy_resolution
    pattern = []
    for k, (pc, ego, tf) in enumerate(scans):
        if k >= jump_at:
            pc = pc + np.array([width, 0, 0], pc.dtype)
            ego = (ego[0] + width, ego[1], ego[2])
            run.referee = always
        run.scan(pc, ego, tf)
        unread = 3 <= k < 3 + UNREAD
        got = run.combine(read=None if unread else "full")
        if k >= 3 + UNREAD:
            pattern.append(got)
    return pattern


def e_pattern(bs):
    return [False] * bs + [True] * 4


def f_length(bs):
    return 2 * (UNREAD + bs) + 8


def script_f(run, scans):
    """two pauses in one run: the buffers are freed and allocated a second time"""
    bs = run.w.buffer_size
    assert len(scans) == f_length(bs)
    first = 3 + UNREAD + bs + 2                                # reads 0-2, none 3-8, reads 9 .. 9 + bs + 1
    pattern = []
    for k, s in enumerate(scans):
        run.scan(*s)
        unread = 3 <= k < 3 + UNREAD or first <= k < first + UNREAD
        got = run.combine(read=None if unread else "full")
        if got is not None:
            pattern.append(got)
    return pattern


def f_pattern(bs):
    return [True] * 3 + [False] * bs + [True] * 2 + [False] * bs + [True] * 3
