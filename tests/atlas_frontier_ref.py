"""Referee of the atlas frontiers (gvom_atlas_frontiers; include/gvom_hip.h "atlas frontiers"), written from the definition: the
field's c and D are atlas_field_ref.field()'s, the visibility is a THREE-VALUED plane in the field's frame built from an AtlasRef's
unwrapped extent and the offset F - E (1 known, 0 unknown, -1 outside the atlas's present extent), and frontier_ref.product() on those
three arrays is the answer; product_loops() is the second form.  frontier_ref's predicate reads `vis > 0` as known and `vis == 0` as
unknown, so a cell at -1 is neither.  Planes here are [x, y] like atlas_field_ref's; frontier_ref takes device order, their transposes.
Also here, for the census of tests/test_atlas_frontiers_cpu.py only: two deliberately WRONG twins -- one whose edge neighbours wrap
around the extent, one that reads the visibility plane at [y*A + x] without the storage phase -- and the counts the census holds."""
import copy
import functools

import numpy as np

import atlas_field_ref as afr
import costfield_ref as cf
import frontier_ref as fr

VARIANTS = (0, 1, 5)                                               # of atlas_field_ref.VARIANTS: plain, blocked unknown + inflation, nearly empty
LIMITS = ((4, 1024), (1, 8), (2, 2 ** 20))                          # (min_cells, max_clusters)


def visibility(ref, F, Af):
    """int32 [x, y], Af x Af, in the frame of a field with origin F: 1 where the AtlasRef's cell is known (visibility > 0), 0 where it
    lies in the present extent and is not, -1 outside the present extent.  The AtlasRef may have another side than the field"""
    vis = ref.i[2].T                                                # [x, y] over the present extent
    out = np.full((Af, Af), -1, np.int32)
    x0, y0 = F[0] - ref.E[0], F[1] - ref.E[1]                        # the field's corner in extent cells
    lx, hx, ly, hy = max(x0, 0), min(x0 + Af, ref.A), max(y0, 0), min(y0 + Af, ref.A)
    if lx < hx and ly < hy:
        out[lx - x0:hx - x0, ly - y0:hy - y0] = (vis[lx:hx, ly:hy] > 0).astype(np.int32)
    return out


def unphased_visibility(ref, F, Af):
    """the WRONG twin's plane: the toroidal storage read at [y*A + x] as if it were the unwrapped extent (no storage phase)"""
    A = ref.A
    twin = copy.copy(ref)
    twin.i = list(ref.i)
    twin.i[2] = np.roll(ref.i[2], (ref.E[1] & (A - 1), ref.E[0] & (A - 1)), axis=(0, 1))    # storage[(E + e) & (A-1)] = extent[e]
    return visibility(twin, F, Af)


def mask(c, vis3, D):
    """bool [x, y]: the frontier cells"""
    return fr.frontier_mask(np.asarray(c).T, np.asarray(vis3).T, np.asarray(D).T).T


def wrapping_mask(c, vis3, D):
    """the WRONG twin's cells: edge neighbours taken around the extent's edges"""
    unknown = np.asarray(vis3) == 0
    beside = np.roll(unknown, 1, 0) | np.roll(unknown, -1, 0) | np.roll(unknown, 1, 1) | np.roll(unknown, -1, 1)
    return (np.asarray(c) > 0) & (np.asarray(vis3) > 0) & beside & (np.asarray(D).astype(np.int64) < cf.UNREACHED)


def product(c, vis3, D, min_cells, cap, loops=False):
    """(clusters, sums, cluster map [x, y], counts, [n_kept, frontier cells, dropped]) of [x, y] planes"""
    f = fr.product_loops if loops else fr.product
    rows, sums, cmap, counts, info = f(np.ascontiguousarray(np.asarray(c).T), np.ascontiguousarray(np.asarray(vis3).T),
                                       np.ascontiguousarray(np.asarray(D).T), min_cells, cap)
    return rows, sums, cmap.T, counts, info


def of_field(f, ref, min_cells, cap, loops=False):
    """the product of an atlas_field_ref.field() dict (its own E is the frame) against an AtlasRef as it is NOW"""
    return product(f["c"], visibility(ref, f["E"], f["c"].shape[0]), f["D"], min_cells, cap, loops)


@functools.lru_cache(maxsize=None)
def expected(xy, A, follow, k, min_cells=4, cap=1024):
    """the referee's product of variant k of a scenario with the atlas as the scenario leaves it; shared, read-only"""
    ref, _ = afr.scenario(xy, A, follow)
    out = of_field(afr.expected(xy, A, follow, k), ref, min_cells, cap)
    for a in out[:4]:
        a.setflags(write=False)
    return out


def spanning(rows, n):
    """kept clusters among the first n rows whose box spans a 32-cell tile border"""
    r = np.asarray(rows[:n], np.int64)
    return int(((r[:, 2] // fr.TILE != r[:, 4] // fr.TILE) | (r[:, 3] // fr.TILE != r[:, 5] // fr.TILE)).sum())


def census(xy, A, follow, k):
    """what tests/test_atlas_frontiers_cpu.py holds floors on, from the referee alone"""
    ref, _ = afr.scenario(xy, A, follow)
    f = afr.expected(xy, A, follow, k)
    vis3 = visibility(ref, f["E"], A)
    rows, sums, cmap, counts, info = expected(xy, A, follow, k)
    n = min(int(counts[0]), rows.shape[0])
    m = mask(f["c"], vis3, f["D"])
    return dict(kept=int(counts[0]), dropped=int(info[2]), cells=int(counts[1]), largest=int(rows[:n, 1].max()) if n else 0,
                spanning=spanning(rows, n), wrap_differs=int((m != wrapping_mask(f["c"], vis3, f["D"])).sum()),
                unphased_differs=int((m != mask(f["c"], unphased_visibility(ref, f["E"], A), f["D"])).sum()),
                unreachable=int((mask(f["c"], vis3, np.zeros_like(f["D"])) & ~m).sum()))


def moved(xy, A, follow, shift=(20, -5)):
    """(a copy of the scenario's AtlasRef after one more integrate `shift` cells on, the (set, origin) integrated)"""
    ref, steps = afr.scenario(xy, A, follow)
    ref = copy.deepcopy(ref)
    s = afr.terrain_set(np.random.default_rng(99), xy)
    o = (steps[-1][1][0] + shift[0], steps[-1][1][1] + shift[1])
    ref.integrate(s, o)
    return ref, (s, o)


def negative_set(xy):
    """nine [y][x] maps: observed free ground in the left half, and in the right half cells of rank 1 (an inferred height) whose
    visibility is -3: UNKNOWN by the atlas-field rule, though not 0"""
    n = (xy, xy)
    vis = np.zeros(n, np.int32)
    vis[:, :xy // 2] = 4
    vis[:, xy // 2:] = -3
    inferred = np.full(n, -1000.0)
    inferred[:, xy // 2:] = -1.25
    return [np.zeros(n, np.int32), np.zeros(n, np.int32), vis, np.full(n, -1.0), np.where(vis > 0, -1.0, -1000.0), inferred, np.zeros(n),
            np.zeros(n), np.zeros(n)]
