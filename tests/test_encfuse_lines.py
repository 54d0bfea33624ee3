"""k_encfuse's two forms -- column blocks of 32 sx (whole 128-byte lines of the state arrays; grids with xy % 32 == 0) and of
16 sx (the other xy % 16 == 0 grids, and everywhere with tuning "encfuse" bit 5) -- against the CPU oracle after EVERY step:
the ring slot densely after each scan, the fused map densely and the four returned maps after each combine
(scenarios.run_and_record / parity.compare_records: integers bit-exact, floats within 1e-5), and against each other bit for
bit.  The shapes are the smallest at which the block -> (column, row band, level) mapping can go wrong: one block per row
band, several, a width that is no power of two, a width that must fall back, level counts that do not fill the last wave
iteration, more levels than columns; the window moves across the storage wrap of every axis and once by more than itself."""
import numpy as np
import pytest

import scenarios
from parity import compare_records
from oracle import oracle
from test_hip_parity import ENCFUSE, FUSE1, _stats_steps, _surface_steps, gvom_mod   # noqa: F401  (gvom_mod: the module's fixture)

pytestmark = pytest.mark.gpu

XY_RES, Z_RES = 0.4, 0.2
FORCE_16 = 32                                                    # tuning "encfuse" bit 5


def _params(xy, zs):
    return (XY_RES, Z_RES, xy, zs, 1, 0.5, 0.5, 0.5, 0.3, 2.0, 2.0, 1.0, 1, 1)


def _ego(xy, zs, k, step):
    """Sensor position of scan k: the window origin (floor(ego / res - size / 2), gvom.py:124) starts 4 voxels below the storage
    wrap in x (moving up), 3 above it in y (moving down) and 3 levels below it in z (moving up), `step` voxels per scan: each
    axis crosses its wrap inside the first scans."""
    return (XY_RES * (xy / 2 + xy - 4 + step * k + 0.25), XY_RES * (xy / 2 + 3 - step * k + 0.25), Z_RES * (zs / 2 + zs - 3 + step * k + 0.25))


def _cloud(rng, xy, zs, k, ego):
    n = 4 * xy * xy // 3 + 2000
    half = 0.45 * xy * XY_RES
    ground = np.stack([rng.uniform(-half, half, n) + ego[0], rng.uniform(-half, half, n) + ego[1],
                       rng.normal(-0.5, 0.12, n) + ego[2]], axis=1)
    wall = np.stack([np.full(500, 2.6 + 0.4 * (k % 2)) + ego[0], rng.uniform(-2, 2, 500) + ego[1],
                     rng.uniform(-0.3 * zs * Z_RES, 0.3 * zs * Z_RES, 500) + ego[2]], axis=1)
    return np.concatenate([ground, wall], 0).astype(np.float32 if k % 2 else np.float64)


def _both_forms(gvom_mod, sc, widths, min_arrays, statistics=False):
    """The oracle once, then the mapper with the form the grid's shape selects and with the 16-sx form forced: both equal to the
    oracle at every step and to each other bit for bit.  widths = the block widths the two mappers must report having launched."""
    want = scenarios.run_and_record(oracle.OracleGvom, sc, record_debug=False)
    made = []

    def knob(v):
        def make(*p):
            g = gvom_mod.Gvom(*p, voxel_statistics=statistics)
            g.set_tuning("eager", 1)
            g.set_tuning("encfuse", v)
            g.routes, combine = [], g.combine_maps

            def combine_and_note():                             # "fuse_kernel" behind every combine
                out = combine()
                g.routes.append(g.get_tuning("fuse_kernel"))
                return out
            g.combine_maps = combine_and_note
            made.append(g)
            return g
        return make
    recs = [scenarios.run_and_record(knob(v), sc, record_debug=False) for v in (0, FORCE_16)]
    for got in recs:
        assert compare_records(got, want, float_tol=1e-5) > min_arrays
    for key in recs[0]:
        a, b = np.asarray(recs[0][key]), np.asarray(recs[1][key])
        assert a.shape == b.shape and (np.array_equal(a, b, equal_nan=True) if a.dtype.kind in "fiub" else True), key
    assert [g.get_tuning("encfuse_width") for g in made] == list(widths)
    return want, made


@pytest.mark.parametrize("step", [1, 5])
@pytest.mark.parametrize("grid", [(32, 20), (64, 36), (96, 20), (48, 20), (32, 40)])
def test_both_forms_match_the_oracle_across_the_storage_wrap_and_a_jump(gvom_mod, grid, step):
    """Eight scans + combines with the window moving by `step` voxels in x, y and z, across the storage wrap of each axis; a
    ninth behind a jump of three window widths, so the previous map has no overlap.  xy = 32: one block per row band; 64;
    96: three blocks per band, two tile columns, the second half empty; 48: the 16-sx form whatever the knob says (read back);
    z = 20 / 36: 4 levels in the last iteration of the 32-sx form's eight waves; 40 > 32: more levels than columns."""
    xy, zs = grid
    rng = np.random.default_rng(100 * xy + zs + step)
    steps = []
    for k in range(9):
        ego = _ego(xy, zs, k, step)
        if k == 8:
            ego = (ego[0] + 3 * xy * XY_RES, ego[1] - 3 * xy * XY_RES, ego[2] + 3 * zs * Z_RES)
        steps += [("scan", _cloud(rng, xy, zs, k, ego), ego, None), ("combine",)]
    _, made = _both_forms(gvom_mod, {"params": _params(xy, zs), "steps": steps}, (32 if xy % 32 == 0 else 16, 16), 100)
    assert all(g.get_tuning("eager_adopted") == 9 and g.routes == [ENCFUSE] * 9 for g in made)
    assert made[0].get_tuning("encfuse_waves") == (8 if xy % 32 == 0 else 4) and made[1].get_tuning("encfuse_waves") == 4


def test_a_dense_slab_settles_its_occupied_voxels_in_the_middle_of_a_wave_iteration(gvom_mod):
    """More than 128 occupied voxels fall to one wave in one group of levels, so the list of occupied voxels is settled (emit())
    while the group is still being listed.  Returns fill a slab of 8 levels over the whole 32 x 32 window, about 30 per voxel.
    At least 95 % of the slab's 8192 voxels are occupied (asserted on the oracle's slot).  Whatever the storage offsets, at
    least 3 aligned level pairs x 8 row bands = 24 wave groups of 256 voxels lie inside the slab; for none of them to hold
    more than 128 occupied voxels 24 x 128 = 3072 voxels would have to be empty, and at most 410 are.  (The 16-sx form's
    groups are 4 levels x 4 rows x 16 sx: at least 1 aligned quad x 8 bands x 2 = 16 groups, 2048 > 410.)"""
    xy, zs = 32, 20
    rng = np.random.default_rng(7)
    steps = []
    for k in range(3):
        ego = (XY_RES * (xy / 2 + xy - 2 + k + 0.25), XY_RES * (xy / 2 + 1 - k + 0.25), Z_RES * 0.25)   # origin z = -10: levels -4 .. 3 are z in [-0.8, 0.8)
        n = 250000
        half = 0.5 * xy * XY_RES
        pc = np.stack([rng.uniform(-half, half, n) + ego[0], rng.uniform(-half, half, n) + ego[1], rng.uniform(-0.8, 0.8, n)], axis=1)
        steps += [("scan", pc.astype(np.float32), ego, None), ("combine",)]
    want, made = _both_forms(gvom_mod, {"params": _params(xy, zs), "steps": steps}, (32, 16), 30)
    for k in (0, 2, 4):
        assert int((np.asarray(want["s%d_slot_hit" % k]) > 0).sum()) >= 0.95 * 8192
    assert all(g.get_tuning("eager_adopted") == 3 for g in made)


def test_a_dropped_speculation_leaves_the_slot_for_k_fuse1(gvom_mod):
    """Two scans, then a combine: the first scan's speculative fusion is dropped (its slot is overwritten, its fused buffer is
    the spare one again).  Two combines behind one scan: the second fuses, with k_fuse1, the slot that k_encfuse wrote -- its
    states, compact rows and tile tags, in the form's own block order -- with the map the first combine adopted."""
    xy, zs = 64, 32                                             # (whole 16-level chunks: the one-slot fusion of the combine is k_fuse1)
    rng = np.random.default_rng(11)
    steps, k = [], 0
    for kind in "ssc scc ssc sc":
        if kind == " ":
            continue
        if kind == "c":
            steps.append(("combine",))
            continue
        ego = _ego(xy, zs, k, 2)
        steps.append(("scan", _cloud(rng, xy, zs, k, ego), ego, None))
        k += 1
    _, made = _both_forms(gvom_mod, {"params": _params(xy, zs), "steps": steps}, (32, 16), 50)
    for g in made:
        assert g.routes == [ENCFUSE, ENCFUSE, FUSE1, ENCFUSE, ENCFUSE]
        assert g.get_tuning("eager_dropped") == 2 and g.get_tuning("eager_adopted") == 4


@pytest.mark.parametrize("tune", [0, FORCE_16])
def test_voxel_statistics_through_the_link_table_of_either_form(gvom_mod, tune):
    """Statistics on: the merge of an adopted eager fusion finds the previous map's rows through the link table that k_encfuse
    writes beside its fused rows -- per-voxel statistics against the oracle after every combine of a moving window, 96 x 20."""
    xy, zs, n_scans = 96, 20, 5

    def hip(*p):
        g = gvom_mod.Gvom(*p, voxel_statistics=True)
        g.set_tuning("encfuse", tune)
        return g
    steps = _surface_steps(960 + zs, xy, zs, XY_RES, Z_RES, n_scans, 6000)
    g, _, checked = _stats_steps(gvom_mod, _params(xy, zs), steps, route=lambda k, f, p: ENCFUSE, make_hip=hip, what="encfuse %d" % tune)
    assert checked == n_scans and g.get_tuning("eager_adopted") == n_scans
    assert g.get_tuning("encfuse_width") == (16 if tune else 32)
