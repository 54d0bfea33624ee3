// gvom_raywalk.h -- what the kernels that READ voxels along a ray share: k_raycast (gvom_query.hip), k_viewpoints and k_viewpoint_best
// (gvom_viewpoint.hip) on the fused map, k_vatlas_raycast, k_vatlas_viewpoints and k_vatlas_viewpoint_best (gvom_voxel_atlas.hip) on the
// voxel atlas.  For all six: the status words, the number of steps in flight, a viewpoint's pose (rq_pose), the literal float64 voxel of
// a point in metres (rq_point_voxel), the viewpoint kernels' wave census (rq_census) and the key reduction of the *_best kernels
// (rq_best_store).  For the three on the fused map: the lookup of a ray position -- window voxel, storage index, tile index.  One
// definition: a viewpoint's beam examines exactly the voxels gvom_raycast's ray examines.  The ray start, the round of positions, the
// beam's end point and the step loop are still written out in each walk kernel: moved into functions here they compile to other code
// (DESIGN.md 9.18 has the figures), and the recorded kernel tables hold every kernel to its bytes.  Device code only, everything inlined.
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

// the pose of viewpoint k: rows 0..2 of the 4x4, wave-uniform; false where an entry is not finite
__device__ __forceinline__ bool rq_pose(const double *__restrict__ poses, uint32_t k, double (&c)[12])
{
    const double *p = poses + (size_t)k * 12;
    bool fin = true;
#pragma unroll
    for (int e = 0; e < 12; ++e) { c[e] = p[e]; fin = fin && fabs(c[e]) < INFINITY; }
    return fin;
}

// the window (or extent) voxel of a point given in metres, in the literal float64 form (gvom.py:1072-1080): a ray's end point, a pose's
// own voxel.  (0, 0, 0) -- in bounds, what is read there is ignored -- where the point is outside
__device__ __forceinline__ bool rq_point_voxel(const ScanParams &P, float x, float y, float z, uint32_t &wx, uint32_t &wy, uint32_t &wz)
{
    const double fx = floor(div_by_res<float>(x, P.xy_res, P.drcp[0], P.fastdiv & 1) - P.origin[0]);
    const double fy = floor(div_by_res<float>(y, P.xy_res, P.drcp[0], P.fastdiv & 1) - P.origin[1]);
    const double fz = floor(div_by_res<float>(z, P.z_res, P.drcp[1], P.fastdiv & 2) - P.origin[2]);
    const bool in = fx >= 0.0 && fx < (double)P.xy && fy >= 0.0 && fy < (double)P.xy && fz >= 0.0 && fz < (double)P.zs;
    wx = in ? (uint32_t)(int)fx : 0u; wy = in ? (uint32_t)(int)fy : 0u; wz = in ? (uint32_t)(int)fz : 0u;
    return in;
}

// ---- the viewpoint kernels' ends ---------------------------------------------------------------------------------------------------------------
// The census of a wave of beams into the viewpoint's row: five ballots and population counts of the beam endings (status -1: a lane
// without a beam), two wave sums, at most seven int32 atomic adds.  Integer sums: the row does not depend on the order of the waves
__device__ __forceinline__ void rq_census(int32_t st, int32_t r_unknown, int32_t r_first, uint32_t lane, int32_t *__restrict__ row)
{
    const uint32_t n_occ = (uint32_t)__builtin_popcountll(lanes(st == RQ_OCCUPIED)), n_clr = (uint32_t)__builtin_popcountll(lanes(st == RQ_CLEAR));
    const uint32_t n_left = (uint32_t)__builtin_popcountll(lanes(st == RQ_LEFT_WINDOW)), n_unk = (uint32_t)__builtin_popcountll(lanes(st == RQ_UNKNOWN));
    const uint32_t n_inv = (uint32_t)__builtin_popcountll(lanes(st == RQ_INVALID));
    const uint32_t visits = wave_sum((uint32_t)r_unknown), gain = wave_sum((uint32_t)r_first);
    if (lane == 0u) {
        if (gain) atomicAdd(row + 1, (int32_t)gain);
        if (visits) atomicAdd(row + 2, (int32_t)visits);
        if (n_occ) atomicAdd(row + 3, (int32_t)n_occ);
        if (n_clr) atomicAdd(row + 4, (int32_t)n_clr);
        if (n_left) atomicAdd(row + 5, (int32_t)n_left);
        if (n_unk) atomicAdd(row + 6, (int32_t)n_unk);
        if (n_inv) atomicAdd(row + 7, (int32_t)n_inv);
    }
}

// The end of the *_best kernels, one workgroup of BLOCK threads: the maximum of every thread's key -- ((gain + 1) << 32) | ~k over its CLEAR
// rows, 0 without one -- and part 1 = {best, gain[best], K, nb}: the lowest index of the largest gain
template <int BLOCK>
__device__ __forceinline__ void rq_best_store(unsigned long long key, const ViewQuery &Q, int32_t *__restrict__ best)
{
    __shared__ unsigned long long s_key[BLOCK / WAVE];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o);
        key = other > key ? other : key;
    }
    if ((threadIdx.x & 63u) == 0u) s_key[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0u) {
#pragma unroll
        for (int w = 1; w < BLOCK / WAVE; ++w) key = s_key[w] > key ? s_key[w] : key;
        const v4i r = {key ? (int32_t)~(uint32_t)key : -1, key ? (int32_t)((uint32_t)(key >> 32) - 1u) : 0, Q.K, Q.nb};
        *(v4i *)best = r;
    }
}

#endif  // GVOM_RAYWALK_H
