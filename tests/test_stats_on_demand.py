"""Statistics on demand -- `gvom.Gvom(...)` as every caller gets it, voxel_statistics=None -- held to the mirror of
tests/stats_demand_ref.py across pause and restart: k_stats, k_stats_gather, k_fuse_stats, k_voxel_cloud and the link table k_encfuse
writes, with the buffers released at the fourth unread combine and allocated again by the next read.

At every combine: the returned maps (tests/test_hip_parity.py _same_maps), the fused cell count and, where _ROUTES names one, the
fusion kernel launched.  At every read: first that the library and the mirror agree on data or no data, for the fused map
(make_debug_voxel_map, voxel_cloud_device, and where there is none combined_metrics / voxels_eigenvalues too) and for every ring slot
(metrics_buffer); then, where there is data, the full parity.compare_statistics with parity.STATS_TOL unchanged; where only the last
slot has statistics, its slot metrics (compare_statistics(..., fused=False)).

  A  every fusion route across one pause (script_a): the previous map comes without metrics at the first restarted combine -- behind a
     link table on the two encfuse routes -- and with restarted ones, some rows of count 0, at the four after it
  B  each of the five calls that count as a read ends a pause; read_dense, the returned maps, make_debug_height_map,
     get_map_as_occupancy_grid and occupancy_grid_device() do not keep the statistics alive
  C  reader periods 1 to 5 on rings of 1 and 3; up to period 3 every read is held to an always-on oracle
  D  combine_maps_async (read before and after .result()), combine_maps_device, combine_maps_occupancy, a combine with no scan in
     between and rejected scans, through a pause and a restart
  E  a restart behind a jump of three window widths: the always-on oracle's statistics
  F  two pauses in one run; voxel_statistics=True behind ten unread combines; voxel_statistics=False

tests/test_stats_on_demand_cpu.py shows on the mirror alone that these can fail: a library that kept merging the statistics of before
the pause, or never merged a previous map's, differs in hundreds to thousands of rows, by more than ten times the tolerance, at the
restarted combines of every script here.  These tests found one: k_fuse_stats merged previous rows of count 0 as the reference's
arithmetic has it, 0 / 0, and the NaN stayed in the map (stats_demand_ref's docstring, "ROWS WITHOUT RETURNS").  With that kernel
case A failed on all nine routes at the second restarted combine ("fused: deviation nan") and case F on both rings, on the MI355X.

Not driven here: the release deferred while another thread's scan is in flight (stats_release && !scan_inflight) -- it cannot be
reached deterministically -- and make_debug_voxel_map() while an asynchronous combine is pending (its row capacity is the fused cell
count of the combine before; the pending read here is combined_metrics, which needs none).

Wall time on the MI355X (pytest --durations, one run): case A 0.07 s (fuse1_36x32) to 0.35 s (encfuse_64x32, the first case of the
file) and 0.19 s on the ring of 20; B 0.12 and 0.13 s; C 0.06 to 0.11 s a case; D 0.06 and 0.08 s; E 0.07 and 0.08 s; F 0.07 and
0.09 s, its always / never case 0.07 s; the 28 cases 3.6 s."""
import contextlib
import io

import numpy as np
import pytest

import stats_demand_ref as sd
from oracle import oracle
from parity import compare_statistics
from test_hip_parity import gvom_mod   # noqa: F401  (the module's fixture: DefaultGvom is the class as a user gets it)

pytestmark = pytest.mark.gpu
B_RINGS, CDEF_RINGS = (1, 2), (1, 3)
C_SCANS = 16


def _quiet(fn, *a):
    with contextlib.redirect_stdout(io.StringIO()):           # (the warnings of rejected scans, on both sides)
        return fn(*a)


def _run(gvom_mod, params, what, route=None, followers=None):
    return sd.Run(params, g=gvom_mod.DefaultGvom(*params), followers=followers, route=route, what=what)


@pytest.mark.parametrize("name", sd.ROUTE_SCENES)
def test_every_fusion_route_across_a_pause(gvom_mod, name):
    """case A"""
    params, scans, route = sd.route_scene(name)
    run = _run(gvom_mod, params, name, route)
    assert _quiet(sd.script_a, run, scans) == sd.a_pattern(params[4])
    if name.startswith("encfuse"):                             # with or without statistics: every combine adopts the scan's own fusion
        assert run.g.get_tuning("eager_adopted") == len(scans)


@pytest.mark.parametrize("bs", B_RINGS)
def test_what_counts_as_a_read(gvom_mod, bs):
    """case B"""
    params, scans = sd.small_scene(bs, sd.b_length(bs), 4)
    run = _run(gvom_mod, params, "B ring %d" % bs)
    _quiet(sd.script_b, run, scans)
    assert run.pauses == len(sd.READS) + 1


@pytest.mark.parametrize("bs", CDEF_RINGS)
@pytest.mark.parametrize("period", [1, 2, 3, 4, 5])
def test_reader_periods(gvom_mod, period, bs):
    """case C.  Periods 4 and 5: the present rule -- the statistics go off at the fourth unread combine, the reader arrives behind it,
    finds nothing and switches them on for three combines nobody reads: it never sees a cloud, on any ring (ADVICE.md's first finding:
    no hysteresis).  Pinned so that a change of the rule shows; not defended."""
    params, scans = sd.small_scene(bs, C_SCANS, 8)
    always = oracle.OracleGvom(*params, voxel_statistics=True)
    run = _run(gvom_mod, params, "C period %d ring %d" % (period, bs), followers={"always": always})
    if period <= sd.IDLE_THRESHOLD:
        run.referee = always
    pattern = _quiet(sd.script_c, run, scans, period)
    assert pattern == [period <= sd.IDLE_THRESHOLD] * (C_SCANS // period)


@pytest.mark.parametrize("bs", CDEF_RINGS)
def test_every_combine_form_through_a_pause_and_a_restart(gvom_mod, bs):
    """case D"""
    params, scans = sd.small_scene(bs, sd.d_length(bs), 5)
    run = _run(gvom_mod, params, "D ring %d" % bs)
    assert _quiet(sd.script_d, run, scans) == sd.d_pattern(bs)


@pytest.mark.parametrize("bs", CDEF_RINGS)
def test_a_restart_behind_a_jump_of_three_window_widths(gvom_mod, bs):
    """case E"""
    params, scans = sd.small_scene(bs, sd.e_length(bs), 6)
    always = oracle.OracleGvom(*params, voxel_statistics=True)
    run = _run(gvom_mod, params, "E ring %d" % bs, followers={"always": always})
    assert _quiet(sd.script_e, run, scans, always) == sd.e_pattern(bs)
    assert run.referee is always


@pytest.mark.parametrize("bs", CDEF_RINGS)
def test_two_pauses_in_one_run(gvom_mod, bs):
    """case F"""
    params, scans = sd.small_scene(bs, sd.f_length(bs), 7)
    run = _run(gvom_mod, params, "F ring %d" % bs)
    assert _quiet(sd.script_f, run, scans) == sd.f_pattern(bs)
    assert run.pauses == 2


def test_always_and_never_do_not_depend_on_reads(gvom_mod):
    """case F: voxel_statistics=True gives the always-on oracle's statistics behind ten unread combines; False never gives any"""
    params, scans = sd.small_scene(1, 12, 9)
    on, off, w = gvom_mod.Gvom(*params, voxel_statistics=True), gvom_mod.Gvom(*params, voxel_statistics=False), oracle.OracleGvom(*params, voxel_statistics=True)
    for k, s in enumerate(scans):
        for m in (on, off, w):
            m.process_pointcloud(np.array(s[0], copy=True), s[1], s[2])
        b = w.combine_maps()
        for a in (on.combine_maps(), off.combine_maps()):
            for i in (0, 1, 2, 4):
                assert np.array_equal(a[i], b[i]), (k, i)
        if k in (0, 11):
            compare_statistics(on, w, what="always, combine %d: " % k)
            assert off.make_debug_voxel_map() is None and off.combined_metrics is None and off.voxels_eigenvalues is None \
                and off.voxel_cloud_device() is None and off.metrics_buffer == [None]
