// gvom_vatlas_pairs.h -- what the kernels that read the voxel atlas's pairs share (gvom_voxel_atlas.hip has the storage layout;
// gvom_voxel_changes.hip reads it too): the pair type and address, the fused-state read of a window voxel as k_occupancy does it, and
// the mask of the 64 columns of a box row that lie inside the box and the extent.  Device code only; everything is inlined, so a
// kernel that calls these is the kernel that had the same lines written out.
#pragma once
#include "gvom_device.h"

typedef unsigned long long v2ull __attribute__((ext_vector_type(2)));      // one pair: .x observed, .y occupied

__device__ __forceinline__ unsigned long long bits_below(uint32_t n) { return n >= 64u ? ~0ull : (1ull << n) - 1ull; }    // bits 0 .. n - 1

__device__ __forceinline__ size_t va_pair(const VAtlas &V, uint32_t sx, uint32_t sy, uint32_t sz)
{
    return ((((size_t)sy << V.lgZ) | sz) << V.lgP) | (sx >> 6);
}

// the fused state at storage column fx of storage row `row` (= fy * zs + fz) of the fused map (gvom_internal.h "STORAGE LAYOUT", "TILES"):
// a stale tile reads "never observed"
__device__ __forceinline__ int32_t va_fused_state(const OccParams &F, const int32_t *__restrict__ fstate, const uint32_t *__restrict__ ftags,
                                                  size_t row, uint32_t fx)
{
    const uint32_t tg = ftags[row * (uint32_t)F.nseg + (fx >> 6)];
    const int32_t sv = fstate[row * (uint32_t)F.xy + fx];
    return tg == F.epoch ? sv : -1;
}

// box columns x0 + b, b = 0 .. 63, inside a box of n columns and inside the extent of A: 0 <= rx + x0 + b < A (|rx| <= 2^30)
__device__ __forceinline__ unsigned long long va_columns_inside(int rx, uint32_t x0, uint32_t n, uint32_t A)
{
    const int e0 = rx + (int)x0;                                                           // extent voxel of bit 0
    const int lo_b = e0 < 0 ? -e0 : 0, hi_b = min((int)(n - x0), (int)A - e0);             // bits [lo_b, hi_b)
    return hi_b > lo_b ? bits_below((uint32_t)min(hi_b, 64)) & ~bits_below((uint32_t)min(lo_b, 64)) : 0ull;
}
