"""Referee of gvom_voxel_atlas_score_alignments (include/gvom_hip.h "voxel atlas alignment"): gvom_score_alignments' referee
(tests/align_ref.py score) on a class grid made of the voxel atlas referee's classes (tests/voxel_atlas_ref.py VoxelAtlasRef.cls) alone --
dilated over the WHOLE extent, then cropped to the box, UNKNOWN where the box leaves the extent.  Pure numpy, not toroidal.  Also here:
the grid of the climbing drive under a name of its own in align_ref.GRIDS, the drive on the CPU referee's maps, the drive's candidates, the
boxes that the CPU census and the GPU tests share, and the count of the voxels whose class only the halo decides."""
import functools

import numpy as np

import align_ref as ar
import voxel_atlas_ref as va

GRID = "vdrive"
ar.GRIDS.setdefault(GRID, va.DRIVE_PARAMS)                     # (tests/test_voxel_atlas.py registers the same tuple under the same name)
SCANS = (4, 6, 8, 10, 16)                                      # the scans held against memory after the drive; 16 is the last
BEST = 122                                                     # the true pose among the drive's candidates: the centre of the 245
HALO_FLOOR = 100


def extent_classes(ref, dilate):
    """uint8 [Z, A, A] ([z][y][x] over the extent): the alignment class of every voxel of the extent -- OCCUPIED; NEAR where dilate and an
    occupied voxel of the extent lies within one voxel on every axis (voxels outside the extent never count); FREE; UNKNOWN"""
    occ = ref.cls == va.OCCUPIED
    near = np.zeros_like(occ)
    if dilate:
        Z, A, _ = occ.shape
        pad = np.zeros((Z + 2, A + 2, A + 2), bool)
        pad[1:-1, 1:-1, 1:-1] = occ
        for dz in range(3):
            for dy in range(3):
                for dx in range(3):
                    near |= pad[dz:dz + Z, dy:dy + A, dx:dx + A]
    return np.where(occ, ar.OCCUPIED, np.where(near, ar.NEAR, np.where(ref.cls == va.FREE, ar.FREE, ar.UNKNOWN))).astype(np.uint8)


def box_classes(ref, B, dilate):
    """uint8 [zs, xy, xy] ([z][y][x] over the box at world voxel B): extent_classes cropped to the box, UNKNOWN outside the extent"""
    out = np.full((ref.zs, ref.xy, ref.xy), ar.UNKNOWN, np.uint8)
    ov = ref._overlap(B, (ref.xy, ref.xy, ref.zs))
    if ov is not None:
        b, e = ov
        out[b] = extent_classes(ref, dilate)[e]
    return out


def box_only_classes(ref, B):
    """the same with the dilation taken inside the box alone: what k_align_field's rule ("voxels outside the window never count") would
    give on the box's own voxels, the part of the box outside the extent taken as never observed.  Differs from box_classes(ref, B, 1)
    exactly at the voxels whose class the halo or the extent's edge decides"""
    ov = ref._overlap(B, (ref.xy, ref.xy, ref.zs))
    state = np.full((ref.zs, ref.xy, ref.xy), -1, np.int32)
    if ov is not None:
        b, e = ov
        state[b] = np.where(ref.cls[e] == va.OCCUPIED, 0, np.where(ref.cls[e] == va.FREE, -2, -1))
    zs, xy = ref.zs, ref.xy
    occ = state >= 0
    pad = np.zeros((zs + 2, xy + 2, xy + 2), bool)
    pad[1:-1, 1:-1, 1:-1] = occ
    near = np.zeros_like(occ)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                near |= pad[dz:dz + zs, dy:dy + xy, dx:dx + xy]
    return np.where(occ, ar.OCCUPIED, np.where(near, ar.NEAR, np.where(state <= -2, ar.FREE, ar.UNKNOWN))).astype(np.uint8)


def halo_only(ref, B):
    """box voxels whose class the dilation decides differently over the extent than inside the box alone: NEAR by an occupied voxel beyond
    the box's faces only, or -- outside the extent, next to an occupied voxel of the box -- UNKNOWN where the box alone would say NEAR"""
    return int((box_classes(ref, B, 1) != box_only_classes(ref, B)).sum())


def score(ref, B, grid, cloud, M, dilate=0, weights=ar.DEFAULT_WEIGHTS):
    """(counts int32 [K, 6], best int32 [4]) of the cloud under the candidates M against the box at world voxel B of the atlas `ref`"""
    assert (ar.GRIDS[grid][2], ar.GRIDS[grid][3]) == (ref.xy, ref.zs)
    return ar.score(None, tuple(int(v) for v in B), grid, cloud, M, dilate, weights, cls=box_classes(ref, B, dilate))


def drive_candidates(gvom, ego):
    """float64 [245, 4, 4]: the candidates of the drive's census around the pose a scan was taken at; index BEST is the identity"""
    M = gvom.pose_candidates(np.identity(4), va.DRIVE_RES[0], ar.XY_STEPS, ar.YAW_STEP, ar.YAW_STEPS, pivot=ego)
    assert len(M) == ar.N_GRID and BEST == ar.CENTRE and np.array_equal(M[BEST], np.identity(4))
    return M


def window_sees_nothing(k, dilate, counts, best, n):
    """asserts what gvom_score_alignments' (counts, best) hold for scan k = 8 or 10 of the drive under its 245 candidates against the FINAL
    window, which that scan's returns have left.  These are facts of the inside test alone -- the clouds, the candidates and the window's
    origin -- and of the few voxels met: the same on the CPU referee's maps and on the GPU's, for rings of 1 and 2 slots.
    Scan 10: all 245 x 2,486 pairs are OUTSIDE; every score is 0 and the best is candidate 0.
    Scan 8 (6,701 returns): 231 candidates, the true pose among them, have every return OUTSIDE; 14 turned candidates bring one or two
    returns into the window, none into an occupied or a free voxel; under dilate 1 two returns of candidate 203 end next to an occupied
    voxel, so that it is the best with a score of 2; under dilate 0 every score is 0 and the best is candidate 0."""
    assert k in (8, 10) and counts.shape == (ar.N_GRID, 6)
    assert counts[BEST].tolist() == [0, 0, 0, 0, 0, n]
    inside = np.flatnonzero(counts[:, 5] != n)
    if k == 10:
        assert n == 2486 and len(inside) == 0 and (counts[:, :5] == 0).all() and best.tolist() == [0, 0, n, ar.N_GRID], (dilate, inside, best)
        return
    assert n == 6701 and len(inside) == 14 and counts[:, 5].min() == n - 2 and 203 in inside, (dilate, inside, counts[inside])
    assert (counts[:, 1] == 0).all() and (counts[:, 3] == 0).all(), dilate
    if dilate:
        assert counts[203].tolist() == [2, 0, 2, 0, 0, n - 2] and best.tolist() == [203, 2, n, ar.N_GRID], (counts[203], best)
    else:
        assert (counts[:, 0] == 0).all() and (counts[:, 2] == 0).all() and best.tolist() == [0, 0, n, ar.N_GRID], best


def drive_boxes(ref, Ws):
    """the six boxes of the halo census after the drive, (name, origin): the final window, two earlier windows, a box across the
    storage seams of x and y (world 0) and a pair boundary, a box over the extent's far corner, a box wholly outside the extent"""
    E, A, Z, xy = ref.E, ref.A, ref.Z, ref.xy
    return [("final window", Ws[16]), ("scan 8's window", Ws[8]), ("scan 4's window", Ws[4]), ("seam box", (-30, -35, -4)),
            ("corner box", (E[0] + A - 32, E[1] - 32, E[2] + Z - 4)), ("wholly outside", (E[0] + A + 7, E[1] - 2 * xy, E[2]))]


@functools.lru_cache(maxsize=None)
def cpu_drive(ring):
    """the climbing drive on the CPU referee of the whole pipeline: (atlas referee after the last integrate, window origins per scan,
    final dense state).  Following, A x A x Z = 128 x 128 x 16"""
    from oracle import oracle
    ref = va.VoxelAtlasRef(va.DRIVE_A, va.DRIVE_Z, va.DRIVE_XY, va.DRIVE_ZS)
    o = oracle.OracleGvom(*(va.DRIVE_PARAMS + (ring,) + va.DRIVE_TAIL))
    Ws = []
    for pc, ego in va.drive_scans():
        o.process_pointcloud(pc, ego)
        o.combine_maps()
        W = tuple(int(v) for v in np.asarray(o.combined_origin))
        Ws.append(W)
        ref.integrate(np.asarray(o.combined_index_map), W)
    return ref, tuple(Ws), np.array(o.combined_index_map)
