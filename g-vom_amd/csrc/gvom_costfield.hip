// gvom_costfield.hip -- device kernels of the cost-to-go field (gvom_cost_to_go): from every cell of a 2-D cost map, the cheapest
// 8-connected way to a goal and the first step of it.  include/gvom_hip.h "cost-to-go fields" has the definition.
//   k_travcost    the uint16 cost map from a device map set (positive, negative, visibility, roughness, the clearance d2)
//   k_ctg_seed    phase 0: a caller's int32 costs -> uint16, D = UNREACHED, activity flags cleared
//                 phase 1: D = 0 at the goals on unblocked cells; their tiles, and the tiles that see them in their halo, marked active
//   k_ctg_relax   ONE ROUND: every active 32 x 32 tile relaxes in LDS to its local fixed point and marks its neighbours
//   k_ctg_dirs    the direction codes from the final D, and the number of reached cells
// WHY ANY ORDER WORKS.  D is the least fixed point of D[u] = min(D[u], D[v] + w(u, v)) over the admissible steps, reached from
// above: every value ever stored is 0 at a goal or (a stored value of a neighbour) + (the weight of the step to it), that is the
// cost of a real path, and values only go down.  A tile reads its one-cell halo from memory other workgroups of the SAME launch
// may be writing; it sees the old value or a newer one, both are costs of real paths, and the tile whose rim went down marks its
// neighbours active for the NEXT launch, which does see it.  Nothing waits on another workgroup: correctness needs only what
// EARLIER launches wrote.  Every loop has a bound fixed at launch.
// All arithmetic is unsigned 32-bit below 2^31 + 2^31 (UNREACHED + the "no step" weight): nothing wraps.
#include "gvom_device.h"
#include "gvom_travcost.h"

#define CTG_T 32                       // cells per tile side
#define CTG_P (CTG_T + 2)              // LDS pitch: the tile and its halo
#define CTG_UNREACHED 0x7fffffffu      // (GVOM_CTG_UNREACHED)
#define CTG_NOSTEP 0x7fffffffu         // weight of an inadmissible step: UNREACHED + NOSTEP fits 32 bits and beats nothing

__device__ __forceinline__ int ctg_dx(int k) { return k == 0 || k == 1 || k == 7 ? 1 : (k >= 3 && k <= 5 ? -1 : 0); }
__device__ __forceinline__ int ctg_dy(int k) { return k >= 1 && k <= 3 ? 1 : (k >= 5 ? -1 : 0); }

// the weight of the step u -> neighbour k given the costs around u (cu: u's own; at(dx, dy): a neighbour's, 0 outside the
// window), or CTG_NOSTEP: both ends unblocked, and for a diagonal both cells that share the corner
template <typename F>
__device__ __forceinline__ uint32_t ctg_weight(uint32_t cu, int k, F at)
{
    const int dx = ctg_dx(k), dy = ctg_dy(k);
    const uint32_t cv = at(dx, dy);
    bool ok = cu > 0u && cv > 0u;
    if (k & 1) ok = ok && at(dx, 0) > 0u && at(0, dy) > 0u;
    return ok ? (k & 1 ? 7u : 5u) * (cu + cv) : CTG_NOSTEP;
}

__global__ __launch_bounds__(256) void k_travcost(const int32_t *__restrict__ pos, const int32_t *__restrict__ neg,
                                                  const int32_t *__restrict__ vis, const double *__restrict__ rough,
                                                  const int32_t *__restrict__ d2, const TravParams P, const int n2,
                                                  uint16_t *__restrict__ c)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n2) return;
    c[i] = trav_cell<false>(P, pos, neg, vis, rough, d2, i, i);       // (gvom_travcost.h)
}

__global__ __launch_bounds__(256) void k_ctg_seed(const int phase, const int xy, const int n2, const int32_t *__restrict__ cost32,
                                                  uint16_t *__restrict__ c, uint32_t *__restrict__ D, uint32_t *__restrict__ flags,
                                                  const int nflags, const int32_t *__restrict__ goals, const int G,
                                                  uint32_t *__restrict__ seeded)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (phase == 0) {
        if (i < nflags) flags[i] = 0u;
        if (i >= n2) return;
        if (cost32) c[i] = (uint16_t)min(max(cost32[i], 0), 65535);
        D[i] = CTG_UNREACHED;
        return;
    }
    if (i >= G) return;
    const int gx = goals[2 * i], gy = goals[2 * i + 1];
    if (gx < 0 || gy < 0 || gx >= xy || gy >= xy) return;              // (the host has refused these)
    const int cell = gy * xy + gx;
    if (c[cell] == 0) return;                                          // a goal on a blocked cell seeds nothing
    D[cell] = 0u;
    const int ntx = (xy + CTG_T - 1) / CTG_T;
    for (int k = 0; k < 9; ++k) {                                      // its tile, and every tile that has it in its halo
        const int vx = gx + k % 3 - 1, vy = gy + k / 3 - 1;
        if (vx >= 0 && vy >= 0 && vx < xy && vy < xy) flags[(vy / CTG_T) * ntx + vx / CTG_T] = 1u;
    }
    atomicAdd(seeded, 1u);
}

// One workgroup per tile, 256 threads, 4 cells each: thread t has the cells (t & 31, (t >> 5) + 8 j), so a wave reads two
// tile rows of 32 consecutive dwords -- one bank each within a ds_read_b32 lane group.  LDS: (32 + 2)^2 uint32 of D and as
// many uint16 of cost, 6.9 KB.  The eight step weights of a thread's cells do not change while it relaxes and live in registers
// (32 of them); a sweep is eight LDS reads and eight adds per cell.  Updates are in place: a sweep may read what another wave
// has just lowered, which only gets it there sooner; the sweep that changes nothing saw constant LDS and ends the tile.
__global__ __launch_bounds__(256) void k_ctg_relax(const int xy, const uint16_t *__restrict__ c, uint32_t *D,
                                                   uint32_t *__restrict__ fcur, uint32_t *__restrict__ fnext,
                                                   uint32_t *__restrict__ activated, uint32_t *__restrict__ relaxed,
                                                   const uint32_t max_cost, const int inner)
{
    __shared__ uint32_t sD[CTG_P * CTG_P];
    __shared__ uint16_t sC[CTG_P * CTG_P];
    __shared__ uint32_t s_rim;
    const int ntx = gridDim.x, nty = gridDim.y;
    const int tile = blockIdx.y * ntx + blockIdx.x;
    if (fcur[tile] == 0u) return;                                      // (workgroup-uniform: before any barrier)
    const int t = threadIdx.x;
    const int x0 = blockIdx.x * CTG_T - 1, y0 = blockIdx.y * CTG_T - 1;   // window coordinates of LDS cell (0, 0)
    if (t == 0) { s_rim = 0u; atomicAdd(relaxed, 1u); }
    for (int i = t; i < CTG_P * CTG_P; i += 256) {
        const int ly = i / CTG_P, lx = i - ly * CTG_P;
        const int x = x0 + lx, y = y0 + ly;
        const bool in = x >= 0 && y >= 0 && x < xy && y < xy;
        const size_t g = (size_t)y * xy + x;
        sC[i] = in ? c[g] : (uint16_t)0;
        sD[i] = in ? D[g] : CTG_UNREACHED;
    }
    __syncthreads();
    const int lx = (t & 31) + 1;
    uint32_t w[4][8], d[4], d_in[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int at0 = ((t >> 5) + 8 * j + 1) * CTG_P + lx;
        const uint32_t cu = sC[at0];
#pragma unroll
        for (int k = 0; k < 8; ++k) w[j][k] = ctg_weight(cu, k, [&](int dx, int dy) { return (uint32_t)sC[at0 + dy * CTG_P + dx]; });
        d[j] = d_in[j] = sD[at0];
    }
    bool more = true;
    for (int it = 0; it < inner; ++it) {
        bool changed = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int at0 = ((t >> 5) + 8 * j + 1) * CTG_P + lx;
            uint32_t best = d[j];
#pragma unroll
            for (int k = 0; k < 8; ++k) best = min(best, sD[at0 + ctg_dy(k) * CTG_P + ctg_dx(k)] + w[j][k]);
            if (best < d[j] && best <= max_cost) { d[j] = best; sD[at0] = best; changed = true; }
        }
        if (!__syncthreads_or(changed)) { more = false; break; }
    }
    // store what went down; a lowered rim cell wakes the tiles that have it in their halo: bit (dy + 1) * 3 + (dx + 1)
    uint32_t rim = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int cx = t & 31, cy = (t >> 5) + 8 * j;
        if (d[j] >= d_in[j]) continue;
        const int x = x0 + 1 + cx, y = y0 + 1 + cy;
        if (x < xy && y < xy) D[(size_t)y * xy + x] = d[j];
        const int ex = cx == 0 ? -1 : (cx == CTG_T - 1 ? 1 : 0), ey = cy == 0 ? -1 : (cy == CTG_T - 1 ? 1 : 0);
        if (ex) rim |= 1u << (3 + ex + 1);
        if (ey) rim |= 1u << ((ey + 1) * 3 + 1);
        if (ex && ey) rim |= 1u << ((ey + 1) * 3 + ex + 1);
    }
    if (rim) atomicOr(&s_rim, rim);
    __syncthreads();
    if (t < 9) {
        const int dx = t % 3 - 1, dy = t / 3 - 1;
        const int tx = (int)blockIdx.x + dx, ty = (int)blockIdx.y + dy;
        const bool wake = t == 4 ? more : ((s_rim >> t) & 1u) != 0u && tx >= 0 && ty >= 0 && tx < ntx && ty < nty;
        if (wake) fnext[ty * ntx + tx] = 1u;
        if (__ballot(wake) != 0ull && t == 0) atomicAdd(activated, 1u);
        if (t == 0) fcur[tile] = 0u;                                   // (every wave has read it: they are past the barriers)
    }
}

__global__ __launch_bounds__(256) void k_ctg_dirs(const int xy, const uint16_t *__restrict__ c, const uint32_t *__restrict__ D,
                                                  uint8_t *__restrict__ dir, uint32_t *__restrict__ reached)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const bool in = x < xy && y < xy;
    bool got = false;
    if (in) {
        const size_t u = (size_t)y * xy + x;
        const uint32_t du = D[u];
        uint32_t code = 255u;                                          // (GVOM_CTG_NONE)
        if (du == 0u) code = 8u;                                       // (GVOM_CTG_GOAL)
        else if (du != CTG_UNREACHED) {
            code = 254u;                                               // (GVOM_CTG_UNSETTLED)
            auto at = [&](int dx, int dy) {
                const int vx = x + dx, vy = y + dy;
                return vx >= 0 && vy >= 0 && vx < xy && vy < xy ? (uint32_t)c[(size_t)vy * xy + vx] : 0u;
            };
            const uint32_t cu = c[u];
#pragma unroll
            for (int k = 7; k >= 0; --k) {
                const uint32_t wk = ctg_weight(cu, k, at);
                if (wk != CTG_NOSTEP && D[(size_t)(y + ctg_dy(k)) * xy + (x + ctg_dx(k))] + wk == du) code = (uint32_t)k;
            }
        }
        dir[u] = (uint8_t)code;
        got = du != CTG_UNREACHED;
    }
    const unsigned long long m = __ballot(got);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(reached, (uint32_t)__popcll(m));
}

int gvom_ctg_tiles(int xy) { return (xy + CTG_T - 1) / CTG_T; }

hipError_t gvom_launch_travcost(hipStream_t s, int xy, const int32_t *pos, const int32_t *neg, const int32_t *vis, const double *rough,
                                const int32_t *d2, const CtgCostParams &C, uint16_t *c)
{
    TravParams P;
    P.thr = C.density_threshold; P.rmin = C.min_roughness; P.rmax = C.max_roughness;
    P.infl2 = d2 ? C.inflation_cells2 : 0; P.base = C.base; P.soft = C.soft_weight; P.unknown = C.unknown_cost; P.rough = C.rough_weight;
    P.use_neg = C.use_negative; P.unknown_blocks = C.unknown_blocks;
    const int n2 = xy * xy;
    hipLaunchKernelGGL(k_travcost, dim3((n2 + 255) / 256), dim3(256), 0, s, pos, neg, vis, rough, d2, P, n2, c);
    return hipGetLastError();
}

hipError_t gvom_launch_ctg_seed(hipStream_t s, int xy, const int32_t *cost32, uint16_t *c, int32_t *D, uint32_t *flags,
                                const int32_t *goals, int G, uint32_t *seeded)
{
    const int n2 = xy * xy, nt = gvom_ctg_tiles(xy), nflags = 2 * nt * nt;
    hipLaunchKernelGGL(k_ctg_seed, dim3((n2 + 255) / 256), dim3(256), 0, s, 0, xy, n2, cost32, c, (uint32_t *)D, flags, nflags, goals, G, seeded);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ctg_seed, dim3((G + 255) / 256), dim3(256), 0, s, 1, xy, n2, cost32, c, (uint32_t *)D, flags, nflags, goals, G, seeded);
    return hipGetLastError();
}

hipError_t gvom_launch_ctg_relax(hipStream_t s, int xy, const uint16_t *c, int32_t *D, uint32_t *fcur, uint32_t *fnext,
                                 uint32_t *activated, uint32_t *relaxed, int32_t max_cost, int inner)
{
    const int nt = gvom_ctg_tiles(xy);
    hipLaunchKernelGGL(k_ctg_relax, dim3(nt, nt), dim3(256), 0, s, xy, c, (uint32_t *)D, fcur, fnext, activated, relaxed,
                       (uint32_t)max_cost, inner);
    return hipGetLastError();
}

hipError_t gvom_launch_ctg_dirs(hipStream_t s, int xy, const uint16_t *c, const int32_t *D, uint8_t *dir, uint32_t *reached)
{
    hipLaunchKernelGGL(k_ctg_dirs, dim3((xy + 63) / 64, (xy + 3) / 4), dim3(256), 0, s, xy, c, (const uint32_t *)D, dir, reached);
    return hipGetLastError();
}
