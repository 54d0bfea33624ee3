"""Referee of the voxel distance field (include/gvom_hip.h "voxel distance field"): pure numpy on a VoxelAtlasRef (tests/voxel_atlas_ref.py),
in two forms that tests/test_voxel_distance_cpu.py holds to each other bit for bit.

  brute()      the definition applied literally: for every box voxel the minimum over the list of sources of fl64(fl64(a * n) + fl64(b * m)),
               chunked.  Without the flag only (under it the sources are infinitely many); also says which source was nearest
  separable()  for the flag and large caps: the class grid padded by the halo, NEVER outside the extent; per level the exact integer
               n_min -- nearest source along y by running maxima, then along x by a loop over the offsets: the other way round than the
               kernels, which take x first --, then the float64 minimum over the levels.  A level without a source, or of sources only,
               needs neither pass

Both return (distance float32 [xy, xy, z], counts int32 [4] {at 0, finite, outside the extent, seq}): parts 0 and 1 of the product."""
import numpy as np

import voxel_atlas_ref as va

NONE = np.int64(1) << 40                                # "no source": larger than any squared offset


def halo(cap, res):
    """the largest h with fl64(a * (double)(h*h)) <= fl64(cap * cap), a = fl64(res * res): by search from 0, not from a root"""
    a, cap2 = float(res) * float(res), float(cap) * float(cap)
    h = 0
    while a * float((h + 1) * (h + 1)) <= cap2:
        h += 1
    return h


def _finish(ref, origin, d2, cap):
    """d2 float64 [z, y, x] (inf: no source) -> the product's two parts"""
    cap2 = float(cap) * float(cap)
    with np.errstate(invalid="ignore"):
        dist = np.where(d2 <= cap2, np.sqrt(d2), np.inf).astype(np.float32)
    dist = np.ascontiguousarray(dist.transpose(2, 1, 0))
    outside = int(ref.box(origin)[1][2])
    counts = np.array([(dist == 0).sum(), np.isfinite(dist).sum(), outside, ref.seq], np.int32)
    return dist, counts


def sources(ref, origin=None, box_only=False):
    """world voxels int64 [n, 3] of class OCCUPIED: every one the atlas holds, or (box_only) those inside the box at `origin`"""
    z, y, x = np.nonzero(ref.cls == va.OCCUPIED)
    s = np.stack([x, y, z], axis=1).astype(np.int64) + np.array(ref.E, np.int64)
    if box_only:
        w = s - np.array(origin, np.int64)
        s = s[((w >= 0) & (w < np.array([ref.xy, ref.xy, ref.zs]))).all(axis=1)]
    return s


def brute(ref, origin, cap, res, box_only=False, chunk=1024, with_nearest=False):
    """the definition, literally.  res = (xy_resolution, z_resolution).  with_nearest: also the offset (dx, dy, dz) int64 [z, y, x, 3] of
    a nearest source (the first of the list among equals; (0, 0, 0) where there is none)"""
    origin = tuple(int(v) for v in origin)
    a, b = float(res[0]) * float(res[0]), float(res[1]) * float(res[1])
    s = sources(ref, origin, box_only)
    z, y, x = np.indices((ref.zs, ref.xy, ref.xy))
    v = np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1).astype(np.int64) + np.array(origin, np.int64)
    d2 = np.full(len(v), np.inf)
    near = np.zeros((len(v), 3), np.int64)
    s32, v32 = s.astype(np.int32), v.astype(np.int32)       # (offsets of a few thousand voxels: their squares fit int32)
    for k in range(0, len(v) if len(s) else 0, chunk):
        dx, dy, dz = (s32[None, :, e] - v32[k:k + chunk, None, e] for e in range(3))
        n = (dx * dx + dy * dy).astype(np.float64)
        m = (dz * dz).astype(np.float64)
        t = a * n + b * m                                    # two roundings of the products, one of the sum: numpy does not contract
        j = t.argmin(axis=1)
        rows = np.arange(len(j))
        d2[k:k + chunk] = t[rows, j]
        near[k:k + chunk] = np.stack([dx[rows, j], dy[rows, j], dz[rows, j]], axis=1)
    out = _finish(ref, origin, d2.reshape(ref.zs, ref.xy, ref.xy), cap)
    return out + (near.reshape(ref.zs, ref.xy, ref.xy, 3),) if with_nearest else out


def padded_classes(ref, origin, pad):
    """the classes uint8 [z, y, x] of the box at `origin` grown by pad = (px, py, pz) on either side; NEVER outside the extent"""
    shape = (ref.xy + 2 * pad[0], ref.xy + 2 * pad[1], ref.zs + 2 * pad[2])
    lo = tuple(int(origin[k]) - pad[k] for k in range(3))
    out = np.zeros(shape[::-1], np.uint8)
    b, e = [], []
    for k in (2, 1, 0):
        r = lo[k] - ref.E[k]
        l, h = max(r, 0), min(r + shape[k], ref.sizes()[k])
        if l >= h:
            return out
        b.append(slice(l - r, h - r)); e.append(slice(l, h))
    out[tuple(b)] = ref.cls[tuple(e)]
    return out


def _nearest_along(src, axis):
    """the distance int64 from every element to the nearest True along `axis` (NONE where the line has none)"""
    n = src.shape[axis]
    shape = [1] * src.ndim
    shape[axis] = n
    at = np.arange(n, dtype=np.int64).reshape(shape)
    before = np.maximum.accumulate(np.where(src, at, -NONE), axis=axis)
    after = np.flip(np.minimum.accumulate(np.flip(np.where(src, at, NONE), axis), axis=axis), axis)
    return np.where(src.any(axis=axis, keepdims=True), np.minimum(at - before, after - at), NONE)


def separable(ref, origin, cap, res, unknown_blocks=False, box_only=False):
    origin = tuple(int(v) for v in origin)
    a, b = float(res[0]) * float(res[0]), float(res[1]) * float(res[1])
    cap2 = float(cap) * float(cap)
    hx, hz = halo(cap, res[0]), halo(cap, res[1])
    pad = (hx, hx, hz)
    xy, zs = ref.xy, ref.zs
    cls = padded_classes(ref, origin, pad)
    src = (cls == va.OCCUPIED) | ((cls == va.NEVER) if unknown_blocks else False)
    if box_only:
        keep = np.zeros_like(src)
        keep[hz:hz + zs, hx:hx + xy, hx:hx + xy] = True
        src &= keep
    # n_min int64 [padded z, y, x] over the box's rows and columns, level by level
    nmin = np.full((src.shape[0], xy, xy), NONE, np.int64)
    some, every = src.any(axis=(1, 2)), src.all(axis=(1, 2))
    nmin[every] = 0
    mixed = np.flatnonzero(some & ~every)
    if len(mixed):
        gy = _nearest_along(src[mixed], 1)[:, hx:hx + xy, :]           # along y, at the box's rows, every padded column
        gy2 = np.where(gy >= NONE, NONE, gy * gy)
        best = np.full((len(mixed), xy, xy), NONE, np.int64)
        for dx in range(-hx, hx + 1):
            np.minimum(best, gy2[:, :, hx + dx:hx + dx + xy] + dx * dx, out=best)
        nmin[mixed] = best
    # the float64 pass: every box level against every padded level
    with np.errstate(invalid="ignore", over="ignore"):
        an = np.where(nmin >= NONE, np.inf, a * nmin.astype(np.float64))
    d2 = np.full((zs, xy, xy), np.inf)
    levels = np.flatnonzero(some)
    for z in range(zs):
        dz = (levels - (z + hz)).astype(np.int64)
        t = an[levels] + (b * (dz * dz).astype(np.float64))[:, None, None]
        if len(levels):
            d2[z] = t.min(axis=0)
    return _finish(ref, origin, d2, cap)


def decided_from_outside(ref, origin, cap, res, unknown_blocks=False):
    """how many box voxels read another value where only the box's own voxels are sources"""
    whole = separable(ref, origin, cap, res, unknown_blocks)[0]
    alone = separable(ref, origin, cap, res, unknown_blocks, box_only=True)[0]
    return int((whole.view(np.uint32) != alone.view(np.uint32)).sum())


def census(dist):
    """(voxels at 0, finite and positive, infinite)"""
    return int((dist == 0).sum()), int((np.isfinite(dist) & (dist > 0)).sum()), int(np.isinf(dist).sum())


def gather(dist, origin, res, points):
    """the sample product of float32 points [n, 3] against the field `dist` of the box at `origin`: (distance float32 [n], counts int32 [4])"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    r = np.array([res[0], res[0], res[1]], np.float64)
    with np.errstate(invalid="ignore"):
        v = np.floor(p.astype(np.float64) / r) - np.array(origin, np.float64)
        inside = ((v >= 0) & (v < np.array(dist.shape, np.float64))).all(axis=1)
    out = np.full(len(p), np.nan, np.float32)
    i = v[inside].astype(np.int64)
    out[inside] = dist[i[:, 0], i[:, 1], i[:, 2]]
    got = out[inside]
    return out, np.array([inside.sum(), np.isfinite(got).sum(), (got == 0).sum(), len(p)], np.int32)


def same_bits(a, b):
    """float32 arrays equal bit for bit (+inf by position; NaN by position, whatever its payload)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
