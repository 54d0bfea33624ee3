// gvom_frontier.hip -- device kernels of frontier extraction (gvom_frontiers): the cells of a cost map that are known, drivable,
// reachable and border never-seen ground, clustered under 8-connectivity, ranked and summarised.  include/gvom_hip.h "frontier
// extraction" has the definition.
//   k_frontier_mark    L = own index at a frontier cell, NONE elsewhere; count = 0; a flag per 32 x 32 tile that holds one
//   k_frontier_relax   ONE ROUND: every flagged tile lowers its labels in LDS to its local fixed point and flags its neighbours
//   k_frontier_count   count[L[u]] += 1
//   k_frontier_rank    0: kept / dropped roots per block of 1024 cells; 1: one workgroup scans the block counts; 2: rank[root]
//                      over count[root] in label order, the row's label and size
//   k_frontier_rows    0: rows cleared and initialised; 1: rows past the kept clusters zeroed, part 3 written
//   k_frontier_stats   the cluster map, and per row the box, the sums and the best key
// WHY ANY ORDER WORKS (k_ctg_relax's argument, gvom_costfield.hip, with another equation).  L[u] = min(L[u], L[v]) over the
// frontier cells v among u's eight neighbours.  Every label ever stored is the index of a member of u's cluster: it starts as u's
// own and is only ever replaced by the stored label of a neighbour, which is one by induction.  Labels only go down and are bounded
// below by the cluster's least index.  A tile reads its one-cell halo from memory other workgroups of the SAME launch may be
// writing; it sees the old label or a newer one, both are members' indices, and the tile whose rim went down flags its neighbours
// for the NEXT launch, which does see it.  Where no relaxation changes anything, connected frontier cells agree, and the least
// member holds itself: the fixed point is the definition.  Nothing waits on another workgroup; every loop has a bound fixed at
// launch.  The ranks come from an ordered scan, not from atomics; the statistics are integer adds, minima and maxima, which
// commute: the product does not depend on scheduling.
#include "gvom_device.h"

#define FR_T 32                        // cells per tile side
#define FR_P (FR_T + 2)                // LDS pitch: the tile and its halo
#define FR_NONE 0xffffffffu            // label of a cell that is no frontier cell: loses every minimum
#define FR_UNREACHED 0x7fffffff        // (GVOM_CTG_UNREACHED)

// cell (x, y) of a 256-thread workgroup that covers 4 rows of 64 cells: a wave owns a row segment
#define FR_CELL() const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6); \
                  const bool in = x < xy && y < xy; const size_t u = (size_t)y * xy + x

// the sum of v over the workgroup's 4 waves, added to *dst once (s4: 4 words of LDS)
__device__ __forceinline__ void fr_block_add(uint32_t v, uint32_t *s4, uint32_t *dst)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) { const uint32_t t = s4[0] + s4[1] + s4[2] + s4[3]; if (t) atomicAdd(dst, t); }
}

__global__ __launch_bounds__(256) void k_frontier_mark(const int xy, const uint16_t *__restrict__ c, const int32_t *__restrict__ vis,
                                                       const int32_t *__restrict__ D, uint32_t *__restrict__ L,
                                                       uint32_t *__restrict__ count, uint32_t *__restrict__ flags,
                                                       uint32_t *__restrict__ n_frontier)
{
    __shared__ uint32_t s4[4];
    FR_CELL();
    bool f = false;
    if (in) {
        f = c[u] > 0 && vis[u] > 0 && (D == nullptr || D[u] < FR_UNREACHED);
        if (f) {                                                       // east / west: the wave's own row again (cached); north / south: a row each
            bool open = x > 0 && vis[u - 1] == 0;
            open = open || (x + 1 < xy && vis[u + 1] == 0);
            open = open || (y > 0 && vis[u - (size_t)xy] == 0);
            open = open || (y + 1 < xy && vis[u + (size_t)xy] == 0);
            f = open;
        }
        L[u] = f ? (uint32_t)u : FR_NONE;
        count[u] = 0u;
    }
    const unsigned long long m = __ballot(f);
    if (m) {                                                           // the wave's segment lies in at most two tiles
        const int ntx = (xy + FR_T - 1) / FR_T, lane = threadIdx.x & 63;
        if ((lane == 0 && (m & 0xffffffffull)) || (lane == 32 && (m >> 32))) flags[(y / FR_T) * ntx + x / FR_T] = 1u;   // (a set bit is a cell inside the window)
    }
    fr_block_add(f ? 1u : 0u, s4, n_frontier);
}

// One workgroup per tile, 256 threads, 4 cells each, as k_ctg_relax: thread t has the cells (t & 31, (t >> 5) + 8 j).  LDS: (32 + 2)^2
// uint32 of labels, 4.6 KB.  Updates are in place: a sweep may read what another wave has just lowered, which only gets it there
// sooner; the sweep that changes nothing saw constant LDS and ends the tile.
__global__ __launch_bounds__(256) void k_frontier_relax(const int xy, uint32_t *L, uint32_t *__restrict__ fcur, uint32_t *__restrict__ fnext,
                                                        uint32_t *__restrict__ activated, uint32_t *__restrict__ relaxed, const int inner)
{
    __shared__ uint32_t sL[FR_P * FR_P];
    __shared__ uint32_t s_rim;
    const int ntx = gridDim.x, nty = gridDim.y;
    const int tile = blockIdx.y * ntx + blockIdx.x;
    if (fcur[tile] == 0u) return;                                      // (workgroup-uniform: before any barrier)
    const int t = threadIdx.x;
    const int x0 = blockIdx.x * FR_T - 1, y0 = blockIdx.y * FR_T - 1;  // window coordinates of LDS cell (0, 0)
    if (t == 0) { s_rim = 0u; atomicAdd(relaxed, 1u); }
    for (int i = t; i < FR_P * FR_P; i += 256) {
        const int ly = i / FR_P, lx = i - ly * FR_P;
        const int x = x0 + lx, y = y0 + ly;
        const bool in = x >= 0 && y >= 0 && x < xy && y < xy;
        sL[i] = in ? L[(size_t)y * xy + x] : FR_NONE;
    }
    __syncthreads();
    const int lx = (t & 31) + 1;
    uint32_t l[4], l_in[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) l[j] = l_in[j] = sL[((t >> 5) + 8 * j + 1) * FR_P + lx];
    bool more = true;
    for (int it = 0; it < inner; ++it) {
        bool changed = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (l[j] == FR_NONE) continue;                             // no frontier cell: it takes no label
            const int at0 = ((t >> 5) + 8 * j + 1) * FR_P + lx;
            uint32_t best = l[j];
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) best = min(best, sL[at0 + dy * FR_P + dx]);
            if (best < l[j]) { l[j] = best; sL[at0] = best; changed = true; }
        }
        if (!__syncthreads_or(changed)) { more = false; break; }
    }
    // store what went down; a lowered rim cell wakes the tiles that have it in their halo: bit (dy + 1) * 3 + (dx + 1)
    uint32_t rim = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int cx = t & 31, cy = (t >> 5) + 8 * j;
        if (l[j] >= l_in[j]) continue;
        const int x = x0 + 1 + cx, y = y0 + 1 + cy;
        if (x < xy && y < xy) L[(size_t)y * xy + x] = l[j];
        const int ex = cx == 0 ? -1 : (cx == FR_T - 1 ? 1 : 0), ey = cy == 0 ? -1 : (cy == FR_T - 1 ? 1 : 0);
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

// The lanes of a wave that hold the same key, one group after the other: fn(lanes of the group, this lane is in it) runs in
// converged control flow for every group, at most 64 of them.  Adjacent frontier cells nearly always share a label: one group.
template <typename F>
__device__ __forceinline__ void fr_wave_groups(const bool active, const uint32_t key, F fn)
{
    unsigned long long todo = __ballot(active);
    for (int it = 0; it < 64 && todo; ++it) {
        const int lead = __ffsll((long long)todo) - 1;
        const uint32_t k = (uint32_t)__shfl((int)key, lead);
        const bool mine = active && key == k;
        const unsigned long long same = __ballot(mine);
        fn(same, mine);
        todo &= ~same;
    }
}

__global__ __launch_bounds__(256) void k_frontier_count(const int xy, const uint32_t *__restrict__ L, uint32_t *__restrict__ count)
{
    FR_CELL();
    const uint32_t lab = in ? L[u] : FR_NONE;
    const int lane = threadIdx.x & 63;
    fr_wave_groups(lab != FR_NONE, lab, [&](unsigned long long same, bool mine) {
        if (mine && lane == __ffsll((long long)same) - 1) atomicAdd(&count[lab], (uint32_t)__popcll(same));   // (lab is a cell's index: < xy * xy)
    });
}

// Ordered compaction of the kept roots.  A block is 1024 cells in index order: pass j of a workgroup has the cells base + 256 j + t,
// so (pass, wave, lane) is the index order.  phase 0: bc[b] = kept roots, bc[nb + b] = dropped roots of block b.  phase 1 (one
// workgroup): bc[0 .. nb) becomes its exclusive prefix sum; totals[0] = kept, totals[1] = dropped clusters.  phase 2: rank[root] =
// the kept roots in front of it, written over count[root]; -2 at a dropped root; the row's label and size where the rank is below cap.
__global__ __launch_bounds__(256) void k_frontier_rank(const int phase, const int n2, const int nb, const uint32_t min_cells, const int cap,
                                                       const uint32_t *__restrict__ L, uint32_t *__restrict__ count, uint32_t *__restrict__ bc,
                                                       uint32_t *__restrict__ totals, int32_t *__restrict__ rows)
{
    __shared__ uint32_t s[256];
    const int t = threadIdx.x;
    if (phase == 1) {
        const int per = (nb + 255) / 256;
        uint32_t kept = 0u, dropped = 0u;
        for (int k = 0; k < per; ++k) {
            const int b = t * per + k;
            if (b < nb) { kept += bc[b]; dropped += bc[nb + b]; }
        }
        s[t] = kept;
        __syncthreads();
        uint32_t before = 0u, all = 0u;
        for (int k = 0; k < 256; ++k) { const uint32_t v = s[k]; all += v; if (k < t) before += v; }
        for (int k = 0; k < per; ++k) {
            const int b = t * per + k;
            if (b < nb) { const uint32_t v = bc[b]; bc[b] = before; before += v; }
        }
        __syncthreads();
        s[t] = dropped;
        __syncthreads();
        if (t == 0) {
            uint32_t d = 0u;
            for (int k = 0; k < 256; ++k) d += s[k];
            totals[0] = all; totals[1] = d;
        }
        return;
    }
    const int b = blockIdx.x, lane = t & 63, w = t >> 6;
    bool keep[4];
    uint32_t cnt[4];
    uint32_t n_drop = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = b * 1024 + j * 256 + t;
        bool root = false;
        cnt[j] = 0u;
        if (i < n2 && L[i] == (uint32_t)i) { root = true; cnt[j] = count[i]; }
        keep[j] = root && cnt[j] >= min_cells;
        const bool drop = root && !keep[j];
        n_drop += drop ? 1u : 0u;
        const unsigned long long m = __ballot(keep[j]);
        if (lane == 0) s[j * 4 + w] = (uint32_t)__popcll(m);
        if (phase == 2 && drop) count[i] = 0xfffffffeu;                // (-2)
    }
    if (phase == 0) {
        n_drop = wave_sum(n_drop);
        if (lane == 0) s[16 + w] = n_drop;
        __syncthreads();
        if (t == 0) {
            uint32_t k = 0u;
            for (int q = 0; q < 16; ++q) k += s[q];
            bc[b] = k; bc[nb + b] = s[16] + s[17] + s[18] + s[19];
        }
        return;
    }
    __syncthreads();
    const uint32_t base = bc[b];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned long long m = __ballot(keep[j]);
        if (!keep[j]) continue;
        uint32_t r = base + (uint32_t)__popcll(m & lanemask_lt());
        for (int q = 0; q < j * 4 + w; ++q) r += s[q];
        const int i = b * 1024 + j * 256 + t;
        count[i] = r;
        if (r < (uint32_t)cap) { rows[(size_t)r * 8] = i; rows[(size_t)r * 8 + 1] = (int32_t)cnt[j]; }
    }
}

// phase 0: row r of part 0 = {0, 0, +max, +max, -1, -1, key all ones}, of part 1 = {0, 0}.  phase 1: rows past the kept clusters are
// zero; counts = {n_kept, frontier cells, frontier cells in kept clusters, cap} from the counters tot = {kept, dropped, in kept} and
// *n_frontier.  The best key lies in columns 6 and 7 of its row -- index in the low word, D in the high one: split as it stands.
__global__ __launch_bounds__(256) void k_frontier_rows(const int phase, const int cap, int32_t *__restrict__ rows, long long *__restrict__ sums,
                                                       const uint32_t *__restrict__ tot, const uint32_t *__restrict__ n_frontier,
                                                       int32_t *__restrict__ counts)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (phase == 1 && r == 0) { counts[0] = (int32_t)tot[0]; counts[1] = (int32_t)*n_frontier; counts[2] = (int32_t)tot[2]; counts[3] = cap; }
    if (r >= cap) return;
    int32_t *q = rows + (size_t)r * 8;
    if (phase == 0) {
        q[0] = 0; q[1] = 0; q[2] = INT_MAX; q[3] = INT_MAX; q[4] = -1; q[5] = -1; q[6] = -1; q[7] = -1;
        sums[(size_t)r * 2] = 0; sums[(size_t)r * 2 + 1] = 0;
    } else if ((uint32_t)r >= tot[0]) {
#pragma unroll
        for (int k = 0; k < 8; ++k) q[k] = 0;
        sums[(size_t)r * 2] = 0; sums[(size_t)r * 2 + 1] = 0;
    }
}

__device__ __forceinline__ uint32_t fr_wave_min(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}
__device__ __forceinline__ uint32_t fr_wave_max(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}

// Per frontier cell rank[L[u]] (k_frontier_rank left it in `rank`); the cluster map; for ranks below cap the row's box, sums and
// best key, the lanes of a wave that share a rank combined first.  A wave is 64 cells of ONE row: the group's y is the lanes' own,
// its x run from the first to the last lane of the group.
__global__ __launch_bounds__(256) void k_frontier_stats(const int xy, const int cap, const uint32_t *__restrict__ L,
                                                        const uint32_t *__restrict__ rank, const int32_t *__restrict__ D,
                                                        int32_t *__restrict__ rows, unsigned long long *__restrict__ sums,
                                                        int32_t *__restrict__ cmap, uint32_t *__restrict__ in_kept)
{
    __shared__ uint32_t s4[4];
    FR_CELL();
    int32_t r = -1;
    if (in) {
        const uint32_t lab = L[u];
        if (lab != FR_NONE) r = (int32_t)rank[lab];                    // (lab is a cell's index: < xy * xy)
        cmap[u] = r;
    }
    const bool rowed = r >= 0 && r < cap;
    const uint32_t du = rowed ? (D ? (uint32_t)D[u] : (uint32_t)FR_UNREACHED) : 0xffffffffu;
    const int lane = threadIdx.x & 63;
    fr_wave_groups(rowed, (uint32_t)r, [&](unsigned long long same, bool mine) {
        const int first = __ffsll((long long)same) - 1, last = 63 - __clzll((long long)same);
        const uint32_t n = (uint32_t)__popcll(same);
        const uint32_t sx = wave_sum(mine ? (uint32_t)x : 0u);
        // the least (D, index): the least D, and among the lanes that have it the first -- indices ascend with the lane
        const uint32_t dmin = fr_wave_min(mine ? du : 0xffffffffu);
        const unsigned long long at = __ballot(mine && du == dmin);
        if (mine && lane == first) {
            int32_t *q = rows + (size_t)r * 8;
            const int x_lo = blockIdx.x * 64 + first, x_hi = blockIdx.x * 64 + last, best = __ffsll((long long)at) - 1;
            atomicMin(&q[2], x_lo); atomicMin(&q[3], y); atomicMax(&q[4], x_hi); atomicMax(&q[5], y);
            atomicMin((unsigned long long *)(q + 6), ((unsigned long long)dmin << 32) | (unsigned long long)(u - (size_t)first + (size_t)best));
            atomicAdd(&sums[(size_t)r * 2], (unsigned long long)sx);
            atomicAdd(&sums[(size_t)r * 2 + 1], (unsigned long long)n * (unsigned long long)y);
        }
    });
    fr_block_add(r >= 0 ? 1u : 0u, s4, in_kept);
}

int gvom_frontier_tiles(int xy) { return (xy + FR_T - 1) / FR_T; }
int gvom_frontier_blocks(int xy) { return (xy * xy + 1023) / 1024; }

hipError_t gvom_launch_frontier_mark(hipStream_t s, int xy, const uint16_t *c, const int32_t *vis, const int32_t *D, uint32_t *L,
                                     uint32_t *count, uint32_t *flags, uint32_t *n_frontier)
{
    hipLaunchKernelGGL(k_frontier_mark, dim3((xy + 63) / 64, (xy + 3) / 4), dim3(256), 0, s, xy, c, vis, D, L, count, flags, n_frontier);
    return hipGetLastError();
}

hipError_t gvom_launch_frontier_relax(hipStream_t s, int xy, uint32_t *L, uint32_t *fcur, uint32_t *fnext, uint32_t *activated,
                                      uint32_t *relaxed, int inner)
{
    const int nt = gvom_frontier_tiles(xy);
    hipLaunchKernelGGL(k_frontier_relax, dim3(nt, nt), dim3(256), 0, s, xy, L, fcur, fnext, activated, relaxed, inner);
    return hipGetLastError();
}

hipError_t gvom_launch_frontier_rows(hipStream_t s, int phase, int cap, int32_t *rows, int64_t *sums, const uint32_t *totals,
                                     const uint32_t *n_frontier, int32_t *counts)
{
    hipLaunchKernelGGL(k_frontier_rows, dim3((cap + 255) / 256), dim3(256), 0, s, phase, cap, rows, (long long *)sums, totals, n_frontier, counts);
    return hipGetLastError();
}

hipError_t gvom_launch_frontier_finish(hipStream_t s, int xy, int32_t min_cells, int cap, const int32_t *D, const uint32_t *L, uint32_t *count,
                                       uint32_t *bc, uint32_t *totals, const uint32_t *n_frontier, int32_t *rows, int64_t *sums,
                                       int32_t *cmap, int32_t *counts)
{
    const int n2 = xy * xy, nb = gvom_frontier_blocks(xy);
    const dim3 cells((xy + 63) / 64, (xy + 3) / 4);
    hipLaunchKernelGGL(k_frontier_count, cells, dim3(256), 0, s, xy, L, count);
    hipError_t e = hipGetLastError();
    for (int phase = 0; phase < 3 && e == hipSuccess; ++phase) {
        hipLaunchKernelGGL(k_frontier_rank, dim3(phase == 1 ? 1 : nb), dim3(256), 0, s, phase, n2, nb, (uint32_t)min_cells, cap, L, count, bc, totals, rows);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_frontier_stats, cells, dim3(256), 0, s, xy, cap, L, count, D, rows, (unsigned long long *)sums, cmap, totals + 2);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return gvom_launch_frontier_rows(s, 1, cap, rows, sums, totals, n_frontier, counts);
}
