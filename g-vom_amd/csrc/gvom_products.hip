// gvom_products.hip -- device kernels of the 3-D products (gvom_device_product, gvom_get_occupancy):
//   k_occupancy         reference gvom.py:356-361: the fused map as a dense uint8 grid out[x][y][z] (1 = occupied)
//   k_occupancy_plain   the same for grids whose z_size is not a multiple of 4
// (the voxel cloud and the height clouds are k_voxel_cloud / k_debug_height of gvom_stats.hip / gvom_map2d.hip)
#include "gvom_device.h"

// A TRANSPOSITION of a mostly empty volume: the fused states are fastest along storage x (a wave reads one 256-byte tile row),
// the grid is fastest along window z.  One workgroup (4 waves) takes one storage row sy, one tile column (64 sx) and OCC_ZC
// window levels:
//   gather   wave w takes the level quads q = w, w + 4, ...: four tile tags (wave-uniform), then -- only where a tag is live --
//            four coalesced row loads; every lane packs the 0/1 bytes of ITS voxel's four levels into one dword (byte k = level
//            4 q + k, the grid's byte order) and stores it to LDS at [lane][q].  The LDS row pitch is odd, so the 32 lanes of
//            a ds_write_b32 group hit 32 different banks.
//   scatter  the LDS row of storage column sx is the nq consecutive dwords out[x][y][z0 ..]: LPR = 2^lg >= nq lanes per row,
//            64 / LPR rows per wave instruction; consecutive lanes read consecutive LDS dwords (conflict-free) and store
//            consecutive global dwords (128-byte runs at OCC_ZC = 128).
// No division or modulo anywhere (wrap-around by compare and subtract, the lane -> (row, dword) split by shift and mask).
// SKIP: the grid was cleared beforehand (hipMemsetAsync); a workgroup whose tiles are all dead stores nothing.
template <bool SKIP>
__global__ __launch_bounds__(256) void k_occupancy(const OccParams P, const int32_t *__restrict__ fstate,
                                                   const uint32_t *__restrict__ ftags, uint32_t *__restrict__ out)
{
    __shared__ uint32_t s_tile[64 * (GVOM_OCC_ZC / 4 + 1)];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int seg = blockIdx.x, y = blockIdx.y, z0 = blockIdx.z * GVOM_OCC_ZC;
    const int nq = (min(GVOM_OCC_ZC, P.zs - z0)) >> 2;           // level quads of this workgroup (zs % 4 == 0)
    const int pitch = nq | 1;
    const int sy = wrap_add(y, P.om[1], P.xy);
    const bool mine = sy >= P.y_lo && sy < P.y_hi;               // (rows of another rank's slab read as empty)
    const int sx = seg * 64 + lane;
    const uint32_t rbase = (uint32_t)sy * P.zs;
    int any = 0;
    for (int q = wave; q < nq; q += 4) {
        uint32_t rz[4];
        bool live[4];
        bool some = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            rz[k] = rbase + (uint32_t)wrap_add(z0 + 4 * q + k, P.om[2], P.zs);
            live[k] = mine && ftags[(size_t)rz[k] * P.nseg + seg] == P.epoch;
            some |= live[k];
        }
        uint32_t d = 0;
        if (some) {                                              // (wave-uniform) four loads in flight, a dummy index where dead
            int32_t st[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) st[k] = fstate[(live[k] && sx < P.xy) ? (size_t)rz[k] * P.xy + sx : (size_t)0];
#pragma unroll
            for (int k = 0; k < 4; ++k) d |= (live[k] && sx < P.xy && st[k] >= 0) ? (1u << (8 * k)) : 0u;
            any = 1;
        }
        s_tile[lane * pitch + q] = d;
    }
    if (SKIP) {
        if (!__syncthreads_or(any)) return;
    } else {
        __syncthreads();
    }
    const int lg = nq > 1 ? 32 - __clz(nq - 1) : 0;              // lanes per LDS row: 2^lg >= nq
    const int col = lane & ((1 << lg) - 1);
    const int rpi = 64 >> lg;                                    // rows per wave instruction
    for (int r = wave * rpi + (lane >> lg); r < 64; r += 4 * rpi) {
        const int sxr = seg * 64 + r;
        if (sxr < P.xy && col < nq) {
            const int x = wrap_sub(sxr, P.om[0], P.xy);
            out[((((size_t)x * P.xy + y) * P.zs + z0) >> 2) + col] = s_tile[r * pitch + col];
        }
    }
}

// z_size % 4 != 0: rows of the grid are not dword-aligned.  One workgroup per (storage row, tile column); a wave per level,
// coalesced loads, byte stores.
__global__ __launch_bounds__(256) void k_occupancy_plain(const OccParams P, const int32_t *__restrict__ fstate,
                                                         const uint32_t *__restrict__ ftags, uint8_t *__restrict__ out)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int seg = blockIdx.x, y = blockIdx.y;
    const int sy = wrap_add(y, P.om[1], P.xy);
    const bool mine = sy >= P.y_lo && sy < P.y_hi;
    const int sx = seg * 64 + lane;
    if (sx >= P.xy) return;
    const int x = wrap_sub(sx, P.om[0], P.xy);
    uint8_t *o = out + ((size_t)x * P.xy + y) * P.zs;
    for (int z = wave; z < P.zs; z += 4) {
        const uint32_t rz = (uint32_t)sy * P.zs + (uint32_t)wrap_add(z, P.om[2], P.zs);
        uint8_t b = 0;
        if (mine && ftags[(size_t)rz * P.nseg + seg] == P.epoch) b = fstate[(size_t)rz * P.xy + sx] >= 0;
        o[z] = b;
    }
}

hipError_t gvom_launch_occupancy(hipStream_t s, const OccParams &P, const int32_t *fstate, const uint32_t *ftags, uint8_t *out,
                                 bool clear_first)
{
    if (P.xy <= 0 || P.zs <= 0) return hipErrorInvalidValue;
    if (P.zs % 4) {
        hipLaunchKernelGGL(k_occupancy_plain, dim3(P.nseg, P.xy), dim3(256), 0, s, P, fstate, ftags, out);
        return hipGetLastError();
    }
    const dim3 grid(P.nseg, P.xy, (P.zs + GVOM_OCC_ZC - 1) / GVOM_OCC_ZC);
    if (clear_first) {
        const hipError_t e = hipMemsetAsync(out, 0, (size_t)P.xy * P.xy * P.zs, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_occupancy<true>, grid, dim3(256), 0, s, P, fstate, ftags, (uint32_t *)out);
    } else {
        hipLaunchKernelGGL(k_occupancy<false>, grid, dim3(256), 0, s, P, fstate, ftags, (uint32_t *)out);
    }
    return hipGetLastError();
}
