// gvom_raywalk.h -- what the kernels that READ the fused map along a ray share (k_raycast in gvom_query.hip, k_viewpoints in
// gvom_viewpoint.hip): the status words, the number of steps in flight, and the lookup of a ray position -- window voxel, storage
// index, tile index.  One definition: a viewpoint's beam examines exactly the voxels gvom_raycast's ray examines.
#ifndef GVOM_RAYWALK_H
#define GVOM_RAYWALK_H
#include "gvom_device.h"
#include "gvom_ray.h"

#define RQ_DEPTH 4          // steps whose loads are in flight together

// status words of part 0 (include/gvom_hip.h GVOM_RAY_*)
#define RQ_CLEAR 0
#define RQ_OCCUPIED 1
#define RQ_UNKNOWN 2
#define RQ_LEFT_WINDOW 3
#define RQ_INVALID 4

// Storage index L and tile index T of the window voxel (wx, wy, wz) (gvom_internal.h "STORAGE LAYOUT", "TILES"); both 0 -- in
// bounds, the value is ignored -- where the position is outside the window.  P2: power-of-two grids wrap by mask, the others by
// compare and subtract (the unsigned minimum of s and s - size).
template <bool P2>
__device__ __forceinline__ void rq_index(bool in, uint32_t wx, uint32_t wy, uint32_t wz, uint32_t uxy, uint32_t uzs, uint32_t unseg,
                                         uint32_t om0, uint32_t om1, uint32_t om2, uint32_t &L, uint32_t &T, int32_t &vox)
{
    uint32_t sx, sy, sz;
    if (P2) { sx = (wx + om0) & (uxy - 1u); sy = (wy + om1) & (uxy - 1u); sz = (wz + om2) & (uzs - 1u); }
    else { sx = min(wx + om0, wx + om0 - uxy); sy = min(wy + om1, wy + om1 - uxy); sz = min(wz + om2, wz + om2 - uzs); }
    const uint32_t row = mad24s(sy, uzs, sz);
    L = in ? mad24s(row, uxy, sx) : 0u;
    T = in ? mad24s(row, unseg, sx >> 6) : 0u;
    vox = in ? (int32_t)mad24s(mad24s(wz, uxy, wy), uxy, wx) : -1;       // x + y * xy + z * xy * xy (gvom.py:1146)
}

// the lookups of RQ_DEPTH consecutive positions of every lane, in the integer or the literal form (window_voxel)
template <bool LIT, bool P2>
__device__ __forceinline__ void rq_lookup(const ScanParams &P, const float (&qx)[RQ_DEPTH], const float (&qy)[RQ_DEPTH],
                                          const float (&qz)[RQ_DEPTH], uint32_t (&L)[RQ_DEPTH], uint32_t (&T)[RQ_DEPTH],
                                          int32_t (&vox)[RQ_DEPTH])
{
    const uint32_t uxy = (uint32_t)P.xy, uzs = (uint32_t)P.zs, unseg = (uint32_t)P.nseg;
    const uint32_t om0 = (uint32_t)P.om[0], om1 = (uint32_t)P.om[1], om2 = (uint32_t)P.om[2];
    const uint32_t o0 = (uint32_t)(int)P.origin[0], o1 = (uint32_t)(int)P.origin[1], o2 = (uint32_t)(int)P.origin[2];
#pragma unroll
    for (int d = 0; d < RQ_DEPTH; ++d) {
        uint32_t wx, wy, wz;
        const bool in = window_voxel<LIT>(P, qx[d], qy[d], qz[d], wx, wy, wz, o0, o1, o2, uxy, uxy - uzs);
        rq_index<P2>(in, wx, wy, wz, uxy, uzs, unseg, om0, om1, om2, L[d], T[d], vox[d]);
    }
}

#endif  // GVOM_RAYWALK_H
