"""Shared comparison rules for parity tests (fixtures vs oracle vs HIP).

Tolerances (BASELINE.json north_star): integer/index outputs bit-exact; float height /
slope / roughness within 1e-5.  In practice everything except log/atan2 results is
bit-identical, so the float maps are held to 1e-9 where both sides use the same libm and
1e-5 only across libm implementations (glibc vs ocml).
"""
import json
import os

import numpy as np

INT_KEYS = ("positive", "negative", "visibility", "fused_state", "fused_hit", "fused_total",
            "slot_state", "slot_hit", "slot_total", "cell_count", "buffer_index",
            "last_buffer_index", "slots_filled", "slot", "returned_none", "occupancy", "kind")
EXACT_FLOAT_KEYS = ("fused_min_h", "slot_min_h", "slot_origin", "origin_world", "height_map",
                    "inferred_height_map", "guessed_height_delta")
TOL_FLOAT_KEYS = ("roughness", "roughness_map", "x_slope_map", "y_slope_map", "debug_height_map",
                  "debug_inferred_height_map")
# per-voxel statistics (float accumulation order is unspecified on a GPU; eigenvalue differences of
# nearly degenerate covariances are ill-conditioned): looser, absolute + relative
STATS_KEYS = ("debug_voxel_map",)
INPUT_KEYS = ("pc", "ego", "tf")


def compare_records(got, want, float_tol=1e-5, skip=(), stats_rtol=1e-4, stats_atol=1e-5):
    """Asserts that `got` reproduces every output recorded in `want`."""
    checked = 0
    for key in want.files if hasattr(want, "files") else want.keys():
        if key in ("params", "n_steps", "ref_step_seconds"):
            continue
        base = key.split("_", 1)[1] if key[0] == "s" and "_" in key else key
        if base in INPUT_KEYS or base in skip:
            continue
        assert key in got, "missing output %s" % key   # (statistics included: a mapper without them says so through `skip`)
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.shape == b.shape, (key, a.shape, b.shape)
        if base in INT_KEYS:
            assert np.array_equal(a, b), "%s differs in %d places" % (key, int(np.sum(a != b)))
        elif base in EXACT_FLOAT_KEYS:
            assert np.array_equal(a, b), "%s differs, max |d|=%g" % (key, float(np.max(np.abs(a - b))))
        elif base in TOL_FLOAT_KEYS:
            assert a.dtype == b.dtype, (key, a.dtype, b.dtype)
            np.testing.assert_allclose(a, b, rtol=0, atol=float_tol, err_msg=key)
        elif base in STATS_KEYS:
            assert a.dtype == b.dtype, (key, a.dtype, b.dtype)
            np.testing.assert_array_equal(a[:, :3], b[:, :3], err_msg=key + " xyz")
            np.testing.assert_array_equal(a[:, 4], b[:, 4], err_msg=key + " hit")
            np.testing.assert_allclose(a[:, 3], b[:, 3], rtol=1e-6, atol=0, err_msg=key + " solid factor")
            np.testing.assert_allclose(a[:, 5:], b[:, 5:], rtol=stats_rtol, atol=stats_atol, err_msg=key + " eigen")
        else:
            raise AssertionError("no comparison rule for %s" % key)
        checked += 1
    return checked


# ---- per-voxel statistics of two live mappers (HIP and oracle), after a combine ---------------------------------------------
# A float column group g is held to |hip - oracle| <= T_g * (|oracle| + S_g): relative where the value is large, absolute
# (T_g * S_g) near zero.  The values are in voxel units (in-voxel positions of a neighbourhood's returns).  T_g is what
# stats_deviation() reports.  The bounds (at most 10x the largest deviation measured on the MI355X over every test that calls
# these helpers: route matrix, neighbourhood sizes, degenerate voxels, statistics fuzz, m256 / c3 / c4 / c5, sharded) are:
STATS_TOL = {
    "slot": (1.8e-12, 1e-2),  # metrics_buffer[last slot], float64 -- measured 1.8e-13 (c5)
    "fused": (6.6e-7, 1e-2),  # combined_metrics, float32 -- measured 6.7e-8 (c4): a float32 rounded the other way here and there
    "cloud": (5e-7, 0.2),     # debug-cloud eigenvalue columns where no fused metrics are at hand (sharded) -- measured 6.9e-8
}
# The eigenvalues themselves are NOT held to a tolerance against the oracle's: the reference's trigonometric solver is
# ill-conditioned near repeated eigenvalues (acos near +-1), and one float32 ulp in one covariance entry of a fused voxel moves
# an eigenvalue by up to 8e-5 absolute at m256 (every row of the oracle's own m256 fused map nudged by one ulp: 7.9e-5; the
# GPU against the oracle: 8e-5 in the rows whose fused metrics differ).  Instead, per row:
#   fused metrics bitwise equal to the oracle's  ->  eigenvalues equal to the solver bound (SOLVER_* below);
#   fused metrics within tol["fused"]            ->  k_voxel_cloud's eigenvalues equal to the oracle's solver applied to the
#                                                   HIP mapper's own fused metrics, to the same solver bound.
# Solver bound: 1 float32 ulp (same arithmetic; ocml's acos / cos against glibc's), or, where the smallest eigenvalues cancel
# (q + 2 p cos(phi + 2 pi / 3) of a flat or thin neighbourhood, millions of float32 ulps of a value near zero), SOLVER_CANCEL
# of the covariance's scale |q| + 2 p -- measured 4.8e-16 (m256), i.e. two float64 ulps of the terms.
SOLVER_ULPS, SOLVER_CANCEL = 1.0, 2.0 ** -48
_COUNT = 9                                               # metrics column 9: the neighbourhood's return count (exact)
_LOG = os.environ.get("GVOM_STATS_DEVIATION_LOG")        # (tolerance calibration: one JSON line per call)


def stats_deviation(a, b, scale):
    """The smallest T with |a - b| <= T (|b| + scale) everywhere (0 for empty or equal arrays)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b) / (np.abs(b) + scale)))


def voxel_order(index_map, arr):
    """rows of a compact array in voxel order (x fastest, then y, then z: the reference's numbering, gvom.py:1154-1160)"""
    im = np.asarray(index_map).reshape(-1)
    return np.asarray(arr)[im[im >= 0]]


def cloud_voxel_order(cloud):
    """make_debug_voxel_map() rows (unspecified order) sorted into voxel order by their world position"""
    cloud = np.asarray(cloud)
    return cloud[np.lexsort((cloud[:, 0], cloud[:, 1], cloud[:, 2]))]


def solver_disagreement(e, e_ref, metrics):
    """(entries beyond the solver bound, largest ulp distance, largest cancellation figure): e and e_ref are float32 eigenvalues
    (C, 3) of the same float32 metrics rows (C, 10) from two implementations of the reference's solver (gvom.py:1333-1378)"""
    a, b = np.asarray(e, np.float32).astype(np.float64), np.asarray(e_ref, np.float32).astype(np.float64)
    if a.size == 0:
        return 0, 0.0, 0.0
    gap = np.abs(a - b)
    ulps = gap / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)
    far = ulps > SOLVER_ULPS
    if not np.any(far):
        return 0, float(ulps.max()), 0.0
    m = np.asarray(metrics, np.float32).astype(np.float64)
    q = (m[:, 3] + m[:, 6] + m[:, 8]) / 3.0
    p = np.sqrt(((m[:, 3] - q) ** 2 + (m[:, 6] - q) ** 2 + (m[:, 8] - q) ** 2 + 2.0 * (m[:, 4] ** 2 + m[:, 5] ** 2 + m[:, 7] ** 2)) / 6.0)
    scale = np.broadcast_to((np.abs(q) + 2.0 * p)[:, None], gap.shape)
    cancel = gap[far] / np.maximum(scale[far], 1e-300)
    return int(np.count_nonzero(cancel > SOLVER_CANCEL)), float(ulps.max()), float(cancel.max())


def _within(name, a, b, tol, dev, what):
    t, sc = tol[name]
    d = stats_deviation(a, b, sc)
    dev[name] = max(dev.get(name, 0.0), d)
    assert d <= t, "%s%s: deviation %.3g > %.3g (|d| <= T (|oracle| + %g))" % (what, name, d, t, sc)


def _log(dev, what, rows):
    if _LOG:
        with open(_LOG, "a") as f:
            f.write(json.dumps(dict(dev, what=what, rows=int(rows))) + "\n")


def compare_cloud(cloud, want_cloud, tol=None, what="", eigen=True):
    """A debug voxel cloud (rows in any order: the ranks' clouds of a sharded map concatenated, say) against the oracle's:
    positions and hit counts exact, solid factor to 1e-6 relative, eigenvalue columns (eigen=True) to tol["cloud"].  Returns
    both in voxel order."""
    tol = STATS_TOL if tol is None else tol
    assert cloud is not None and want_cloud is not None, what + "debug voxel cloud missing"
    a, b = cloud_voxel_order(cloud), cloud_voxel_order(want_cloud)
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(a[:, :3], b[:, :3]), what + "debug voxel cloud: positions"
    assert np.array_equal(a[:, 4], b[:, 4]), what + "debug voxel cloud: hit counts"
    np.testing.assert_allclose(a[:, 3], b[:, 3], rtol=1e-6, atol=0, err_msg=what + "debug voxel cloud: solid factor")
    if eigen:
        dev = {}
        _within("cloud", a[:, 5:], b[:, 5:], tol, dev, what)
        _log(dev, what, a.shape[0])
    return a, b


def compare_statistics(g, w, tol=None, what="", fused=True):
    """Per-voxel statistics of the HIP mapper `g` against the oracle mapper `w` (both with voxel_statistics, same inputs, just
    combined), rows in voxel order on both sides (fused=False: statistics on demand that are restarting -- the last slot has its
    own, the fused map has none yet on EITHER side: the slot's are held as always, and the fused map's must be absent):
      metrics_buffer[last slot] (float64), combined_metrics and last_combined_metrics (float32): count column exact, the rest
        to tol["slot"] / tol["fused"];
      voxels_eigenvalues: see above (the oracle's where the fused metrics are the same, the oracle's solver on HIP's own fused
        metrics everywhere -- k_voxel_cloud's eigen-solver on its own, apart from the float atomic order of the merge);
      make_debug_voxel_map(): positions / hit counts exact, solid factor 1e-6; its columns 5-7 ARE the differences of the same
        mapper's voxels_eigenvalues, on both sides.
    Returns the deviations measured."""
    from oracle import oracle
    tol = STATS_TOL if tol is None else tol
    dev = {}
    slot = w.last_buffer_index
    assert g.last_buffer_index == slot, what
    wm = voxel_order(w.index_buffer[slot], w.metrics_buffer[slot])
    gm = g.metrics_buffer[slot].copy_to_host()
    assert gm.dtype == np.float64 and gm.shape == wm.shape, (what, gm.shape, wm.shape)
    assert np.array_equal(gm[:, _COUNT], wm[:, _COUNT]), what + "slot counts"
    _within("slot", gm[:, :_COUNT], wm[:, :_COUNT], tol, dev, what)
    if not fused:
        assert w.combined_metrics is None and w.voxels_eigenvalues is None, what + "the referee has fused statistics"
        assert g.combined_metrics is None and g.last_combined_metrics is None and g.voxels_eigenvalues is None \
            and g.make_debug_voxel_map() is None, what + "fused statistics where the referee has none"
        _log(dev, what, gm.shape[0])
        return dev

    wc = voxel_order(w.combined_index_map, w.combined_metrics)
    gc = g.combined_metrics.copy_to_host()
    assert gc.dtype == np.float32 and gc.shape == wc.shape, (what, gc.shape, wc.shape)
    assert np.array_equal(gc[:, _COUNT], wc[:, _COUNT]), what + "fused counts"
    _within("fused", gc[:, :_COUNT], wc[:, :_COUNT], tol, dev, what)
    assert np.array_equal(g.last_combined_metrics.copy_to_host(), gc), what + "last_combined_metrics"
    assert w.last_combined_metrics is w.combined_metrics

    a, b = compare_cloud(g.make_debug_voxel_map(), w.make_debug_voxel_map(), tol, what, eigen=False)
    we = voxel_order(w.combined_index_map, w.voxels_eigenvalues)
    ge = g.voxels_eigenvalues.copy_to_host()
    assert ge.dtype == np.float32 and ge.shape == we.shape == (a.shape[0], 3), (what, ge.shape, we.shape)
    for cloud, e, who in ((a, ge, "hip"), (b, we, "oracle")):
        assert np.array_equal(cloud[:, 5], e[:, 0] - e[:, 1]) and np.array_equal(cloud[:, 6], e[:, 1] - e[:, 2]) \
            and np.array_equal(cloud[:, 7], e[:, 2]), what + who + ": debug cloud columns 5-7 vs voxels_eigenvalues"

    same = np.all(gc.view(np.uint32) == wc.view(np.uint32), axis=1)
    bad, ulps, cancel = solver_disagreement(ge[same], we[same], gc[same])
    dev.update(eigen_rows_differing=int(np.count_nonzero(~same)), eigen_ulps=ulps, eigen_cancel=cancel,
               eigen_all=stats_deviation(ge, we, 1e-2))
    assert bad == 0, "%seigenvalues of %d rows with the oracle's fused metrics: %d entries beyond the solver bound" % (
        what, int(np.count_nonzero(same)), bad)
    se = np.zeros((gc.shape[0], 3), np.float32)
    gcc = np.ascontiguousarray(gc)
    oracle.lib().orc_calculate_eigenvalues(oracle._p(se), oracle._p(gcc), gc.shape[0])
    bad, ulps, cancel = solver_disagreement(ge, se, gc)
    dev.update(solver_ulps=ulps, solver_cancel=cancel)
    assert bad == 0, "%sk_voxel_cloud's eigenvalues against the oracle's solver on the same fused metrics: %d entries beyond the bound" % (what, bad)
    _log(dev, what, gc.shape[0])
    return dev
