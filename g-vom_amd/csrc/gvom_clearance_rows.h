// gvom_clearance_rows.h -- the row pass of the obstacle clearance map as a body of two front ends: k_clearance_rows (gvom_clearance.hip)
// reads a [y][x] map pair, k_atlas_clearance_rows (gvom_atlas_field.hip) reads the atlas's toroidal planes through their storage phase.
// What differs is where cell x of the row is loaded from, and that comes in as a callable; the ballots, the search and the store are
// one text.
#pragma once
#include "gvom_device.h"

// "no obstacle in this row": 46341^2 = 2,147,488,281 > INT32_MAX, so as an unsigned candidate it never beats a limit that
// fits int32, and 46341^2 + 4095^2 still fits 32 bits: the column pass needs no test for it
#define GVOM_CLR_NONE 46341u

// One workgroup per map row, one wave per 64 cells.  Pass 1: every wave's obstacle ballot goes to LDS (at most 64 masks:
// xy <= 4096).  Pass 2: the nearest obstacle to the left / right of a lane is found in the wave's own mask with clz / ffs on
// the bits at or below / at or above the lane; where the mask has none, in the nearest non-empty mask on that side, which one
// more ballot (over the masks themselves) names.  No loop over cells, no division.
// obstacle(x): is cell x (< xy) of this workgroup's row an obstacle; g_row: the row's gp uint16 distances; s_mask: 64 words of LDS
template <typename OB>
__device__ __forceinline__ void clearance_row(OB obstacle, const int xy, const int gp, uint16_t *__restrict__ g_row,
                                              unsigned long long *s_mask)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nchunks = gp >> 6;
    for (int c = wave; c < nchunks; c += 4) {
        const int x = c * 64 + lane;
        bool ob = false;
        if (x < xy) ob = obstacle(x);
        const unsigned long long m = __ballot(ob);
        if (lane == 0) s_mask[c] = m;
    }
    __syncthreads();
    const unsigned long long nz = __ballot(lane < nchunks && s_mask[lane < nchunks ? lane : 0] != 0ull);
    for (int c = wave; c < nchunks; c += 4) {
        const unsigned long long own = s_mask[c];
        const unsigned long long lo = nz & ((1ull << c) - 1ull);           // non-empty chunks left of c
        const unsigned long long hi = c == 63 ? 0ull : nz >> (c + 1);      // ... right of c
        int lpos = -(1 << 20), rpos = 1 << 20;                            // (wave-uniform) nearest obstacle outside the chunk
        if (lo) {
            const int cc = 63 - __clzll((long long)lo);
            lpos = cc * 64 + 63 - __clzll((long long)s_mask[cc]);
        }
        if (hi) {
            const int cc = c + __ffsll((unsigned long long)hi);
            rpos = cc * 64 + __ffsll((unsigned long long)s_mask[cc]) - 1;
        }
        const int x = c * 64 + lane;
        const unsigned long long ml = own & (~0ull >> (63 - lane));        // obstacles at or left of the lane
        const unsigned long long mr = own >> lane;                         // at or right of it
        const int dl = ml ? lane - (63 - __clzll((long long)ml)) : x - lpos;
        const int dr = mr ? __ffsll((unsigned long long)mr) - 1 : rpos - x;
        const int d = min(dl, dr);
        g_row[x] = (uint16_t)(d > 4095 ? GVOM_CLR_NONE : (unsigned)d);
    }
}
