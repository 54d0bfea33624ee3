// gvom_classgrid.h -- the CLASS GRID of scan alignment scoring (include/gvom_hip.h "scan alignment scoring"): a 2-bit code per voxel, 16
// voxels per uint32, in [z][y][x] order with rows padded to whole words.  Shared by its two writers, k_align_field (gvom_align.hip: from
// the fused state) and k_vatlas_align_field (gvom_voxel_atlas.hip: from the voxel atlas's bit planes), and read by k_align_score, so that
// the codes, the bit spreading and the sizing of the writers' workgroups cannot drift apart.
#pragma once
#include <stdint.h>

#define AL_ZC_MAX 16                // levels per workgroup of a field kernel, at most
#define AL_LDS_BUDGET (48 * 1024)   // bytes of masks a field kernel's workgroup may hold

// the 2-bit codes; count column of part 0 = 1 + code
#define AL_OCC 0u
#define AL_NEAR 1u
#define AL_FREE 2u
#define AL_UNK 3u

// bit i of the low 16 bits of v -> bit 2 i
__device__ __forceinline__ uint32_t al_spread16(uint32_t v)
{
    v &= 0xffffu;
    v = (v | (v << 8)) & 0x00ff00ffu;
    v = (v | (v << 4)) & 0x0f0f0f0fu;
    v = (v | (v << 2)) & 0x33333333u;
    v = (v | (v << 1)) & 0x55555555u;
    return v;
}
