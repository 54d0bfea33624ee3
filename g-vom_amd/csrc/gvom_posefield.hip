// gvom_posefield.hip -- device kernels of the pose field (gvom_pose_field): the navigation function on (x, y, heading) states under the
// oriented footprint and a table of motion primitives.  include/gvom_hip.h "pose fields" has the definition; DESIGN.md 9.11 the scheme.
//   k_cspace         the pose cost volume C[h][cell]: lanes over neighbouring cells of one heading, walking that heading's footprint list
//   k_pose_seed      phase 0: a caller's int32 costs -> uint16, D = UNREACHED, activity flags cleared
//                    phase 1: D = 0 at the goal states with C != 0; their tiles, and the tiles that see them in their halo, marked active
//   k_pose_relax     ONE ROUND: every active tile (8 x 8 cells x ALL headings) relaxes in LDS to its local fixed point and marks its neighbours
//   k_pose_actions   the action codes from the final D, and the number of reached states
// WHY ANY ORDER WORKS is k_ctg_relax's argument (gvom_costfield.hip) on a directed graph: every value ever stored is 0 at a seeded
// state or (a stored value of a successor) + (the price of the primitive to it), the cost of a real drive, and values only go down.  A
// tile reads its halo -- R cells wide, R the table's largest |dx|, |dy| -- from memory other workgroups of the SAME launch may be
// writing; it sees the old value or a newer one, both costs of real drives, and the tile whose state went down marks every tile that
// has the state in its halo active for the NEXT launch, which does see it.  Nothing waits on another workgroup: correctness needs only
// what EARLIER launches wrote.  Every loop has a bound fixed at launch.
// All arithmetic is unsigned 32-bit below 2^31 + 2^31 (UNREACHED + the "no step" price; a real price is at most 255 * 131070 < 2^25
// on top of a stored value <= 2^30): nothing wraps.
#include "gvom_device.h"
#include <atomic>

#define PF_MAX_DEVICES 64              // devices the launcher remembers having raised k_pose_relax's dynamic-LDS limit on
#define PF_T 8                        // cells per tile side: the 64 lanes of a wave are the 64 cells of a tile at ONE heading
#define PF_UNREACHED 0x7fffffffu       // (GVOM_CTG_UNREACHED)
#define PF_NOSTEP 0x7fffffffu          // price of an inadmissible primitive: UNREACHED + NOSTEP fits 32 bits and beats nothing

// a primitive as the table holds it: int16 (dx, dy, h_to, w) in two little-endian words
__device__ __forceinline__ void pf_prim(const uint2 q, int &dx, int &dy, int &hto, uint32_t &w)
{
    dx = (int)(int16_t)(q.x & 0xffffu); dy = (int)(int16_t)(q.x >> 16);
    hto = (int)(q.y & 0xffffu); w = q.y >> 16;
}

// blockIdx.y = the heading (wave-uniform: the footprint list is read through scalar loads), lanes over consecutive cells of a row
__global__ __launch_bounds__(256) void k_cspace(const int xy, const int n2, const uint16_t *__restrict__ c,
                                                const int32_t *__restrict__ fstart, const uint32_t *__restrict__ foffs,
                                                uint16_t *__restrict__ C)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n2) return;
    const int h = blockIdx.y;
    const int y = i / xy, x = i - y * xy;
    const int b = fstart[h], M = fstart[h + 1] - b;
    const uint32_t uxy = (uint32_t)xy;
    uint32_t mx = 0u;
    bool bad = false;
    for (int m = 0; m < M; ++m) {
        const uint32_t o = foffs[b + m];
        const uint32_t fx = (uint32_t)(x + (int)(int16_t)(o & 0xffffu)), fy = (uint32_t)(y + (int)(int16_t)(o >> 16));
        const bool in = fx < uxy && fy < uxy;
        const uint32_t v = in ? (uint32_t)c[fy * uxy + fx] : 0u;       // (outside the window: blocked)
        bad = bad || v == 0u;
        mx = max(mx, v);
    }
    C[(size_t)h * n2 + i] = (uint16_t)(bad ? 0u : mx);
}

__global__ __launch_bounds__(256) void k_pose_seed(const int phase, const int xy, const int n2, const int H, const int R,
                                                   const int32_t *__restrict__ cost32, uint16_t *__restrict__ c16,
                                                   const uint16_t *__restrict__ C, uint32_t *__restrict__ D, uint32_t *__restrict__ flags,
                                                   const int nflags, const int32_t *__restrict__ goals, const int G,
                                                   uint32_t *__restrict__ seeded)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (phase == 0) {
        if (i < (size_t)nflags) flags[i] = 0u;
        if (cost32 && i < (size_t)n2) c16[i] = (uint16_t)min(max(cost32[i], 0), 65535);
        if (i < (size_t)H * n2) D[i] = PF_UNREACHED;
        return;
    }
    if (i >= (size_t)G) return;
    const int gx = goals[3 * i], gy = goals[3 * i + 1], gh = goals[3 * i + 2];
    if (gx < 0 || gy < 0 || gx >= xy || gy >= xy || gh >= H) return;      // (the host has refused these)
    const int h0 = gh < 0 ? 0 : gh, h1 = gh < 0 ? H : gh + 1;             // a goal without a heading seeds every heading of its cell
    const size_t cell = (size_t)gy * xy + gx;
    uint32_t n = 0u;
    for (int h = h0; h < h1; ++h) {
        const size_t s = (size_t)h * n2 + cell;
        if (C[s] == 0) continue;                                          // a goal state the footprint blocks seeds nothing
        if (atomicExch(&D[s], 0u) != 0u) ++n;                             // (a state named twice counts once)
    }
    if (n == 0u) return;
    atomicAdd(seeded, n);
    const int ntx = (xy + PF_T - 1) / PF_T;
    const int tx = gx / PF_T, ty = gy / PF_T, cx = gx - tx * PF_T, cy = gy - ty * PF_T;
    for (int k = 0; k < 9; ++k) {                                         // its tile, and every tile that has it in its halo
        const int ex = k % 3 - 1, ey = k / 3 - 1;
        const bool okx = ex == 0 || (ex < 0 ? cx < R : cx >= PF_T - R), oky = ey == 0 || (ey < 0 ? cy < R : cy >= PF_T - R);
        const int ux = tx + ex, uy = ty + ey;
        if (okx && oky && ux >= 0 && uy >= 0 && ux < ntx && uy < ntx) flags[uy * ntx + ux] = 1u;
    }
}

// One workgroup per tile, 256 threads = 4 waves.  A wave takes the headings w, w + 4, ...; its 64 lanes are the tile's 8 x 8 cells, so
// the heading -- and with it the primitive list -- is wave-uniform: start and the primitives come through scalar loads, once per wave
// and primitive.  LDS (dynamic): D (uint32) and C (uint16) of H x (8 + 2R)^2 states, the tile and its halo at every heading -- 6 bytes
// a state, 98,304 bytes at H = 64, R = 4.  A primitive costs two LDS reads (C and D of its end state), a multiply-add and a minimum.
// Updates are in place: a sweep may read what another wave has just lowered, which only gets it there sooner; the sweep in which no
// thread changed anything saw constant LDS and ends the tile.  A cell outside the window has C = 0 at every heading: never a start,
// never an end.
__global__ __launch_bounds__(256) void k_pose_relax(const int xy, const int H, const int R, const uint16_t *__restrict__ C, uint32_t *D,
                                                    const int32_t *__restrict__ pstart, const uint2 *__restrict__ prims,
                                                    uint32_t *__restrict__ fcur, uint32_t *__restrict__ fnext,
                                                    uint32_t *__restrict__ activated, uint32_t *__restrict__ relaxed,
                                                    const uint32_t max_cost, const int inner)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_pf[];
    __shared__ uint32_t s_rim;
    const int P = PF_T + 2 * R, PP = P * P, N = H * PP;
    uint32_t *const sD = s_pf;
    uint16_t *const sC = (uint16_t *)(s_pf + N);
    const int ntx = gridDim.x, nty = gridDim.y;
    const int tile = blockIdx.y * ntx + blockIdx.x;
    if (fcur[tile] == 0u) return;                                      // (workgroup-uniform: before any barrier)
    const int t = threadIdx.x;
    const int x0 = blockIdx.x * PF_T - R, y0 = blockIdx.y * PF_T - R;  // window coordinates of LDS cell (0, 0)
    const size_t n2 = (size_t)xy * xy;
    if (t == 0) { s_rim = 0u; atomicAdd(relaxed, 1u); }
    for (int i = t; i < N; i += 256) {
        const int h = i / PP, r = i - h * PP;
        const int ly = r / P, lx = r - ly * P;
        const int x = x0 + lx, y = y0 + ly;
        const bool in = x >= 0 && y >= 0 && x < xy && y < xy;
        const size_t g = (size_t)h * n2 + (size_t)y * xy + x;
        sC[i] = in ? C[g] : (uint16_t)0;
        sD[i] = in ? D[g] : PF_UNREACHED;
    }
    __syncthreads();
    const int lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int cx = lane & 7, cy = lane >> 3;
    const int at0 = (cy + R) * P + cx + R;
    unsigned long long chg = 0ull;                                     // bit h: this lane's state at heading h went down
    bool more = true;
    for (int it = 0; it < inner; ++it) {
        bool changed = false;
        for (int h = wv; h < H; h += 4) {
            const int u = h * PP + at0;
            const uint32_t cu = sC[u], d = sD[u];
            uint32_t best = d;
            const int p0 = pstart[h], p1 = pstart[h + 1];
            for (int p = p0; p < p1; ++p) {
                int dx, dy, hto;
                uint32_t w;
                pf_prim(prims[p], dx, dy, hto, w);
                const int v = hto * PP + at0 + dy * P + dx;
                const uint32_t cv = sC[v];
                best = min(best, sD[v] + (cu != 0u && cv != 0u ? w * (cu + cv) : PF_NOSTEP));
            }
            if (best < d && best <= max_cost) { sD[u] = best; chg |= 1ull << h; changed = true; }
        }
        if (!__syncthreads_or(changed)) { more = false; break; }
    }
    // store what went down; a lowered state wakes the tiles that have its cell in their halo: bit (ey + 1) * 3 + (ex + 1)
    if (chg != 0ull) {
        const size_t cell = (size_t)(y0 + R + cy) * xy + (x0 + R + cx);   // (inside the window: a state outside has C = 0 and never goes down)
        for (int h = wv; h < H; h += 4)
            if ((chg >> h) & 1ull) D[(size_t)h * n2 + cell] = sD[h * PP + at0];
        uint32_t rim = 0u;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int ex = k % 3 - 1, ey = k / 3 - 1;
            const bool okx = ex == 0 || (ex < 0 ? cx < R : cx >= PF_T - R), oky = ey == 0 || (ey < 0 ? cy < R : cy >= PF_T - R);
            if (okx && oky) rim |= 1u << k;
        }
        atomicOr(&s_rim, rim);
    }
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

// blockIdx.y = the heading, lanes over consecutive cells.  The first primitive in table order that attains D[u]: the list is walked
// backwards and the last match kept.
__global__ __launch_bounds__(256) void k_pose_actions(const int xy, const int n2, const uint16_t *__restrict__ C,
                                                      const uint32_t *__restrict__ D, const int32_t *__restrict__ pstart,
                                                      const uint2 *__restrict__ prims, uint8_t *__restrict__ action,
                                                      uint32_t *__restrict__ reached)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int h = blockIdx.y;
    bool got = false;
    if (i < n2) {
        const int y = i / xy, x = i - y * xy;
        const size_t u = (size_t)h * n2 + i;
        const uint32_t du = D[u];
        uint32_t code = 255u;                                          // (GVOM_CTG_NONE)
        if (du == 0u) code = 253u;                                     // (GVOM_POSE_GOAL: a price is at least 2, so only a seed holds 0)
        else if (du != PF_UNREACHED) {
            code = 254u;                                               // (GVOM_CTG_UNSETTLED)
            const uint32_t cu = C[u];
            const int p0 = pstart[h], p1 = pstart[h + 1];
            for (int p = p1 - 1; p >= p0; --p) {
                int dx, dy, hto;
                uint32_t w;
                pf_prim(prims[p], dx, dy, hto, w);
                const int vx = x + dx, vy = y + dy;
                if (vx < 0 || vy < 0 || vx >= xy || vy >= xy) continue;
                const size_t v = (size_t)hto * n2 + (size_t)vy * xy + vx;
                const uint32_t cv = C[v];
                if (cu != 0u && cv != 0u && D[v] + w * (cu + cv) == du) code = (uint32_t)(p - p0);
            }
        }
        action[u] = (uint8_t)code;
        got = du != PF_UNREACHED;
    }
    const unsigned long long m = __ballot(got);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(reached, (uint32_t)__popcll(m));
}

int gvom_pose_tiles(int xy) { return (xy + PF_T - 1) / PF_T; }

size_t gvom_pose_relax_lds(int H, int R) { const size_t P = PF_T + 2 * (size_t)R; return (size_t)H * P * P * 6; }

static bool pose_shape_ok(int xy, int H, int R)
{
    return xy >= 1 && xy <= 4096 && H >= 1 && H <= GVOM_POSE_MAX_HEADINGS && R >= 0 && R <= GVOM_POSE_MAX_REACH &&
           (int64_t)H * xy * xy <= GVOM_POSE_MAX_STATES;
}

hipError_t gvom_launch_cspace(hipStream_t s, int xy, int H, const uint16_t *c, const int32_t *fstart, const uint32_t *foffs, uint16_t *C)
{
    if (!pose_shape_ok(xy, H, 0)) return hipErrorInvalidValue;
    const int n2 = xy * xy;
    hipLaunchKernelGGL(k_cspace, dim3((n2 + 255) / 256, H), dim3(256), 0, s, xy, n2, c, fstart, foffs, C);
    return hipGetLastError();
}

hipError_t gvom_launch_pose_seed(hipStream_t s, int phase, int xy, int H, int R, const int32_t *cost32, uint16_t *c16, const uint16_t *C,
                                 int32_t *D, uint32_t *flags, const int32_t *goals, int G, uint32_t *seeded)
{
    if (!pose_shape_ok(xy, H, R)) return hipErrorInvalidValue;
    const int n2 = xy * xy, nt = gvom_pose_tiles(xy), nflags = 2 * nt * nt;
    const size_t states = (size_t)H * n2;
    const size_t n = phase == 0 ? (states > (size_t)nflags ? states : (size_t)nflags) : (size_t)G;
    hipLaunchKernelGGL(k_pose_seed, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, phase, xy, n2, H, R, cost32, c16, C, (uint32_t *)D,
                       flags, nflags, goals, G, seeded);
    return hipGetLastError();
}

hipError_t gvom_launch_pose_relax(hipStream_t s, int xy, int H, int R, const uint16_t *C, int32_t *D, const int32_t *pstart,
                                  const int16_t *prims, uint32_t *fcur, uint32_t *fnext, uint32_t *activated, uint32_t *relaxed,
                                  int32_t max_cost, int inner)
{
    if (!pose_shape_ok(xy, H, R)) return hipErrorInvalidValue;
    const size_t lds = gvom_pose_relax_lds(H, R);
    if (lds > 60000) {                                                 // beyond the default limit of dynamic LDS: ask, once per device, for the most a tile can need
        static std::atomic<bool> raised[PF_MAX_DEVICES];
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        const bool known = dev >= 0 && dev < PF_MAX_DEVICES;
        if (!known || !raised[dev].load(std::memory_order_acquire)) {
            e = hipFuncSetAttribute((const void *)k_pose_relax, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)gvom_pose_relax_lds(GVOM_POSE_MAX_HEADINGS, GVOM_POSE_MAX_REACH));
            if (e != hipSuccess) return e;
            if (known) raised[dev].store(true, std::memory_order_release);
        }
    }
    const int nt = gvom_pose_tiles(xy);
    hipLaunchKernelGGL(k_pose_relax, dim3(nt, nt), dim3(256), lds, s, xy, H, R, C, (uint32_t *)D, pstart, (const uint2 *)prims, fcur, fnext,
                       activated, relaxed, (uint32_t)max_cost, inner);
    return hipGetLastError();
}

hipError_t gvom_launch_pose_actions(hipStream_t s, int xy, int H, const uint16_t *C, const int32_t *D, const int32_t *pstart,
                                    const int16_t *prims, uint8_t *action, uint32_t *reached)
{
    if (!pose_shape_ok(xy, H, 0)) return hipErrorInvalidValue;
    const int n2 = xy * xy;
    hipLaunchKernelGGL(k_pose_actions, dim3((n2 + 255) / 256, H), dim3(256), 0, s, xy, n2, C, (const uint32_t *)D, pstart,
                       (const uint2 *)prims, action, reached);
    return hipGetLastError();
}
