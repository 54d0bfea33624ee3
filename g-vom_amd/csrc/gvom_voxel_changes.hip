// gvom_voxel_changes.hip -- device kernels of the voxel atlas's change query (gvom_voxel_atlas_changes; include/gvom_hip.h "voxel atlas
// changes" has the definition): which voxels of the CURRENT fused map are OCCUPIED where the atlas remembers FREE (appeared) or FREE
// where it remembers OCCUPIED (vanished), and the 8-connected clusters of the columns that hold one (gfx950, wave64).  Read-only on the
// atlas and on the fused map.
//   k_vchange_planes    a wave takes 64 window columns of one (y, z) row at a time: the lanes read the fused state as k_vatlas_merge
//                       reads it (tile tag + state), two ballots give the row's OCCUPIED and FREE masks; the atlas's bits of the same 64
//                       world columns are assembled from one or two 16-byte pairs as k_vatlas_box assembles them (wave-uniform loads,
//                       funnel shift, extent mask); lane 0 stores the 16-byte word {appeared, vanished} of the row: 2 bits a voxel,
//                       window-ordered, word ((y * zs + z) * nseg + q).  The three totals {appeared, vanished, outside the extent} are
//                       population counts kept in registers while the wave strides over its share on a capped grid, summed over the
//                       workgroup in LDS: one 64-bit atomic per counter and workgroup
//   k_vchange_codes     k_vatlas_box's shape: a thread holds the 64 x bits of one (y, z) row from both planes and stores a byte per x;
//                       for one x the workgroup's (y, z) are consecutive bytes.  No LDS
//   k_vchange_columns   a thread per column, a wave 64 columns of one row y: it walks the levels, the words are wave-uniform per
//                       segment.  Writes part 6 (appeared / vanished voxels per column), the column's {lowest, highest} masked level,
//                       the labels / tile flags / marked-column counter exactly as k_frontier_mark leaves them, the squared distance to
//                       the window's centre cell (gvom_frontiers' D), and initialises part 4
//   k_vchange_clusters  behind the labelling (k_frontier_relax .. k_frontier_stats run unchanged): every marked column of a kept rank
//                       below cap adds its voxels and levels to its row of part 4, the lanes of a wave that share a rank combined first
//                       as in k_frontier_stats; rows past the kept clusters are zeroed; words 4 .. 7 of part 3
// Everything is an integer sum, minimum or maximum of population counts: exact whatever the schedule.
// The small wave helpers of gvom_frontier.hip are repeated here: sharing them through a header is what changed k_frontier_mark's
// registers and code size once, so that unit stays as it is.
#include "gvom_device.h"
#include "gvom_vatlas_pairs.h"
#include <algorithm>

#define VC_BLOCK 256
#define VC_WAVES (VC_BLOCK / WAVE)
#define VC_PLANE_BLOCKS 2048                               // the most workgroups of k_vchange_planes: 8 per CU, each strides over its share
#define VC_T 32                                            // cells per tile side (FR_T, gvom_frontier.hip: k_frontier_relax reads these flags)
#define VC_NONE 0xffffffffu                                // label of a column that is not marked (FR_NONE)
#define VC_NO_LEVELS 0x0000ffffu                           // {lowest, highest} of a column without a masked voxel: lowest 65535, highest 0

// ---- the bit planes ----------------------------------------------------------------------------------------------------------------------
// item = (y * zs + z) * nseg + q, wave-uniform: window row y, level z, columns 64 q .. 64 q + 63.  B is the window as a box of the atlas
// (n, zs, r*, p*).  cnt uint64 [3], CLEARED by the caller = {appeared, vanished, window voxels outside the extent}.
__global__ __launch_bounds__(VC_BLOCK) void k_vchange_planes(const VAtlas V, const VAtlasBox B, const OccParams F, const int32_t *__restrict__ fstate,
                                                             const uint32_t *__restrict__ ftags, v2ull *__restrict__ planes,
                                                             unsigned long long *__restrict__ cnt)
{
    __shared__ int32_t s_c[VC_WAVES][4];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t gw = __builtin_amdgcn_readfirstlane(blockIdx.x * VC_WAVES + wv);
    const uint32_t uA = (uint32_t)V.A, uZ = (uint32_t)V.Z, n = (uint32_t)B.n, zs = (uint32_t)B.zs, nseg = (n + 63u) >> 6;
    const uint32_t items = n * zs * nseg;                                                  // (n <= 4096, zs <= 4096: below 2^32, the launcher checks)
    int32_t c[3] = {0, 0, 0};
    for (uint32_t item = gw; item < items; item += gridDim.x * VC_WAVES) {
        const uint32_t q = item % nseg, r = item / nseg;
        const uint32_t z = r % zs, y = r / zs;
        const uint32_t x0 = q << 6, wx = x0 + lane;
        // the row of the fused map at the mapper's storage index, as k_vatlas_merge reads it
        const uint32_t my = y + (uint32_t)F.om[1], mz = z + (uint32_t)F.om[2];
        const uint32_t fy = min(my, my - n), fz = min(mz, mz - zs);
        const size_t row = (size_t)fy * zs + fz;
        const bool in = wx < n;
        const uint32_t mx = in ? wx + (uint32_t)F.om[0] : 0u;
        const uint32_t fx = min(mx, mx - n);
        int32_t s = -1;
        if (in) s = va_fused_state(F, fstate, ftags, row, fx);
        const unsigned long long m_in = lanes(in), m_occ = lanes(in && s >= 0), m_free = lanes(in && s < -1);
        // the atlas's bits of the same 64 world columns, as k_vatlas_box assembles them
        unsigned long long obs = 0ull, occ = 0ull, valid = 0ull;
        const uint32_t ey = (uint32_t)(B.ry + (int)y), ez = (uint32_t)(B.rz + (int)z);
        if (ey < uA && ez < uZ) {
            const uint32_t sy = ((uint32_t)B.py + y) & (uA - 1u), sz = ((uint32_t)B.pz + z) & (uZ - 1u);
            const uint32_t sx = ((uint32_t)B.px + x0) & (uA - 1u), sh = sx & 63u;
            const v2ull lo = ((const v2ull *)V.pairs)[va_pair(V, sx, sy, sz)];
            obs = lo.x >> sh; occ = lo.y >> sh;
            if (sh) {
                const v2ull hi = ((const v2ull *)V.pairs)[va_pair(V, (sx + 64u) & (uA - 1u), sy, sz)];
                obs |= hi.x << (64u - sh); occ |= hi.y << (64u - sh);
            }
            valid = va_columns_inside(B.rx, x0, n, uA);
            obs &= valid; occ &= valid;
        }
        v2ull w;
        w.x = m_occ & obs & ~occ;                                                          // OCCUPIED now, remembered FREE
        w.y = m_free & occ;                                                                // FREE now, remembered OCCUPIED
        if (lane == 0u) planes[item] = w;
        c[0] += __builtin_popcountll(w.x);
        c[1] += __builtin_popcountll(w.y);
        c[2] += __builtin_popcountll(m_in & ~valid);
    }
    if (lane == 0u) {
#pragma unroll
        for (int e = 0; e < 3; ++e) s_c[wv][e] = c[e];     // (a wave's share of a window of fewer than 2^32 voxels on >= 4 waves: int32 holds it)
    }
    __syncthreads();
    if (threadIdx.x < 3u) {
        long long t = 0;
#pragma unroll
        for (int w = 0; w < VC_WAVES; ++w) t += s_c[w][threadIdx.x];
        if (t != 0) atomicAdd(cnt + threadIdx.x, (unsigned long long)t);
    }
}

// ---- the codes ---------------------------------------------------------------------------------------------------------------------------
// A workgroup takes 64 columns x (blockIdx.x), yb rows y (blockIdx.y) and zc levels z (blockIdx.z): thread t = yy * zc + zz holds the word
// of its (y, z) row and stores the code of every x -- out[x][y][z], for one x the workgroup's (y, z) are one contiguous run wherever
// zc == zs.
__global__ __launch_bounds__(VC_BLOCK) void k_vchange_codes(const int n_, const int zs_, const int zc_, const int yb_, const v2ull *__restrict__ planes,
                                                            uint8_t *__restrict__ out)
{
    const uint32_t t = threadIdx.x, n = (uint32_t)n_, zs = (uint32_t)zs_, zc = (uint32_t)zc_, nseg = (n + 63u) >> 6;
    const uint32_t yy = t / zc, zz = t - yy * zc;
    const uint32_t x0 = blockIdx.x * 64u, y = blockIdx.y * (uint32_t)yb_ + yy, z = blockIdx.z * zc + zz;
    if (yy < (uint32_t)yb_ && y < n && z < zs) {
        const v2ull w = planes[((size_t)y * zs + z) * nseg + blockIdx.x];
        const uint32_t nx = min(64u, n - x0);
        uint8_t *o = out + ((size_t)x0 * n + y) * zs + z;
        const size_t pitch = (size_t)n * zs;
        for (uint32_t b = 0; b < nx; ++b) o[b * pitch] = (uint8_t)(((w.x >> b) & 1ull) + 2ull * ((w.y >> b) & 1ull));     // 0 none, 1 appeared, 2 vanished
    }
}

// ---- the columns -------------------------------------------------------------------------------------------------------------------------
// the sum of v over the workgroup's 4 waves, added to *dst once (s4: 4 words of LDS)
__device__ __forceinline__ void vc_block_add(uint32_t v, uint32_t *s4, uint32_t *dst)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) { const uint32_t t = s4[0] + s4[1] + s4[2] + s4[3]; if (t) atomicAdd(dst, t); }
}

// A 256-thread workgroup covers 4 rows of 64 columns: a wave owns a row segment, so the word of a level is the same for its 64 lanes.
// cols uint16 [2][xy][xy] (part 6: plane k at k * xy * xy, [y][x] inside), lohi uint32 [xy][xy] = lowest | highest << 16 of the levels
// whose code is in `mask`; L, count, flags, n_marked as k_frontier_mark leaves them; D int32 [xy][xy]; rows4 = part 4, cap rows of 4.
__global__ __launch_bounds__(VC_BLOCK) void k_vchange_columns(const int xy, const int zs, const int mask, const int cap, const v2ull *__restrict__ planes,
                                                              uint16_t *__restrict__ cols, uint32_t *__restrict__ lohi, uint32_t *__restrict__ L,
                                                              uint32_t *__restrict__ count, uint32_t *__restrict__ flags,
                                                              uint32_t *__restrict__ n_marked, int32_t *__restrict__ D, int32_t *__restrict__ rows4)
{
    __shared__ uint32_t s4[4];
    const int lane = threadIdx.x & 63;
    const int x = blockIdx.x * 64 + lane, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const bool in = x < xy && y < xy;
    const size_t u = (size_t)y * xy + x, n2 = (size_t)xy * xy;
    const uint32_t nseg = ((uint32_t)xy + 63u) >> 6;
    uint32_t na = 0u, nv = 0u, lo = 0xffffu, hi = 0u;
    if (y < xy) {                                                                          // (wave-uniform)
        const v2ull *row = planes + (size_t)y * zs * nseg + blockIdx.x;
        const unsigned long long ka = (mask & 1) ? ~0ull : 0ull, kv = (mask & 2) ? ~0ull : 0ull;
        for (int z = 0; z < zs; ++z) {
            const v2ull w = row[(size_t)z * nseg];
            na += (uint32_t)(w.x >> lane) & 1u;
            nv += (uint32_t)(w.y >> lane) & 1u;
            if ((((w.x & ka) | (w.y & kv)) >> lane) & 1ull) { lo = min(lo, (uint32_t)z); hi = (uint32_t)z; }
        }
    }
    const bool f = in && lo != 0xffffu;                                                    // (a bit beyond the window's last column is never set)
    if (in) {
        cols[u] = (uint16_t)na; cols[n2 + u] = (uint16_t)nv;
        lohi[u] = f ? lo | (hi << 16) : VC_NO_LEVELS;
        L[u] = f ? (uint32_t)u : VC_NONE;
        count[u] = 0u;
        const int dx = x - xy / 2, dy = y - xy / 2;
        D[u] = dx * dx + dy * dy;                                                          // (xy <= 4096: below 2^24)
    }
    const unsigned long long m = __ballot(f);
    if (m) {                                                                               // the wave's segment lies in at most two tiles
        const int ntx = (xy + VC_T - 1) / VC_T;
        if ((lane == 0 && (m & 0xffffffffull)) || (lane == 32 && (m >> 32))) flags[(y / VC_T) * ntx + x / VC_T] = 1u;   // (a set bit is a column inside the window)
    }
    vc_block_add(f ? 1u : 0u, s4, n_marked);
    // part 4 before the clusters add to it: no voxels, no levels yet
    const uint32_t gid = (blockIdx.y * gridDim.x + blockIdx.x) * VC_BLOCK + threadIdx.x, all = gridDim.x * gridDim.y * VC_BLOCK;
    const v4i none = {0, 0, INT_MAX, -1};
    for (uint32_t r = gid; r < (uint32_t)cap; r += all) *(v4i *)(rows4 + (size_t)r * 4) = none;
}

// ---- the clusters ------------------------------------------------------------------------------------------------------------------------
// The lanes of a wave that hold the same key, one group after the other (fr_wave_groups, gvom_frontier.hip): fn(lanes of the group, this
// lane is in it) runs in converged control flow for every group, at most 64 of them.
template <typename Fn>
__device__ __forceinline__ void vc_wave_groups(const bool active, const uint32_t key, Fn fn)
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
__device__ __forceinline__ uint32_t vc_wave_min(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}
__device__ __forceinline__ uint32_t vc_wave_max(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}
__device__ __forceinline__ int32_t vc_word(unsigned long long v) { return v > (unsigned long long)INT_MAX ? INT_MAX : (int32_t)v; }

// cmap = part 2 as k_frontier_stats wrote it (rank, -1 unmarked, -2 below min_cells); totals[0] = kept clusters; cnt = k_vchange_planes'
// three totals; counts = part 3, words 4 .. 7 written here.  Rows of part 4 from min(kept, cap) on are zeroed: nothing adds to them.
__global__ __launch_bounds__(VC_BLOCK) void k_vchange_clusters(const int xy, const int cap, const int seq, const int32_t *__restrict__ cmap,
                                                               const uint16_t *__restrict__ cols, const uint32_t *__restrict__ lohi,
                                                               const uint32_t *__restrict__ totals, const unsigned long long *__restrict__ cnt,
                                                               int32_t *__restrict__ rows4, int32_t *__restrict__ counts)
{
    const int lane = threadIdx.x & 63;
    const int x = blockIdx.x * 64 + lane, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const bool in = x < xy && y < xy;
    const size_t u = (size_t)y * xy + x, n2 = (size_t)xy * xy;
    const int32_t r = in ? cmap[u] : -1;
    const bool rowed = r >= 0 && r < cap;
    uint32_t a = 0u, v = 0u, lo = 0xffffffffu, hi = 0u;
    if (rowed) {
        a = cols[u]; v = cols[n2 + u];
        const uint32_t w = lohi[u];
        lo = w & 0xffffu; hi = w >> 16;
    }
    vc_wave_groups(rowed, (uint32_t)r, [&](unsigned long long same, bool mine) {
        const uint32_t sa = wave_sum(mine ? a : 0u), sv = wave_sum(mine ? v : 0u);
        const uint32_t l = vc_wave_min(mine ? lo : 0xffffffffu), h = vc_wave_max(mine ? hi : 0u);
        if (mine && lane == __ffsll((long long)same) - 1) {
            int32_t *q = rows4 + (size_t)r * 4;
            if (sa) atomicAdd(&q[0], (int32_t)sa);
            if (sv) atomicAdd(&q[1], (int32_t)sv);
            atomicMin(&q[2], (int32_t)l); atomicMax(&q[3], (int32_t)h);
        }
    });
    const uint32_t gid = (blockIdx.y * gridDim.x + blockIdx.x) * VC_BLOCK + threadIdx.x, all = gridDim.x * gridDim.y * VC_BLOCK;
    const v4i zero = {0, 0, 0, 0};
    for (uint64_t z = (uint64_t)totals[0] + gid; z < (uint64_t)cap; z += all) *(v4i *)(rows4 + (size_t)z * 4) = zero;
    if (gid == 0u) {
        const v4i tail = {vc_word(cnt[0]), vc_word(cnt[1]), vc_word(cnt[2]), seq};
        *(v4i *)(counts + 4) = tail;
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------
size_t gvom_vchange_planes_bytes(int n, int zs) { return (size_t)n * zs * ((n + 63) / 64) * 16; }

static bool vc_box_ok(const VAtlas &V, const VAtlasBox &B)
{
    const int lim = 1 << 30;
    const bool atlas = V.pairs && V.A >= GVOM_VATLAS_MIN_CELLS && V.A <= GVOM_VATLAS_MAX_CELLS && !(V.A & (V.A - 1)) && V.Z >= 1 && V.Z <= V.A &&
                       !(V.Z & (V.Z - 1)) && (1 << V.lgZ) == V.Z && (64 << V.lgP) == V.A;
    return atlas && B.n >= 1 && B.n <= GVOM_VATLAS_MAX_CELLS && B.zs >= 1 && B.zs <= GVOM_VATLAS_MAX_CELLS && B.px >= 0 && B.px < V.A && B.py >= 0 &&
           B.py < V.A && B.pz >= 0 && B.pz < V.Z && B.rx >= -lim && B.rx <= lim && B.ry >= -lim && B.ry <= lim && B.rz >= -lim && B.rz <= lim;
}

hipError_t gvom_launch_vchange_planes(hipStream_t s, const VAtlas &V, const VAtlasBox &B, const OccParams &F, const int32_t *fstate,
                                      const uint32_t *ftags, void *planes, unsigned long long *cnt)
{
    if (!vc_box_ok(V, B) || F.xy != B.n || F.zs != B.zs || F.nseg < (B.n + 63) / 64 || !fstate || !ftags || !planes || !cnt) return hipErrorInvalidValue;
    for (int k = 0; k < 3; ++k)
        if (F.om[k] < 0 || F.om[k] >= (k < 2 ? B.n : B.zs)) return hipErrorInvalidValue;
    const uint64_t items = (uint64_t)B.n * B.zs * ((B.n + 63) / 64);
    const unsigned blocks = (unsigned)std::min<uint64_t>((items + VC_WAVES - 1) / VC_WAVES, VC_PLANE_BLOCKS);
    hipLaunchKernelGGL(k_vchange_planes, dim3(blocks), dim3(VC_BLOCK), 0, s, V, B, F, fstate, ftags, (v2ull *)planes, cnt);
    return hipGetLastError();
}

hipError_t gvom_launch_vchange_codes(hipStream_t s, int n, int zs, const void *planes, uint8_t *out)
{
    if (n < 1 || n > GVOM_VATLAS_MAX_CELLS || zs < 1 || zs > GVOM_VATLAS_MAX_CELLS || !planes || !out) return hipErrorInvalidValue;
    const int zc = zs < VC_BLOCK ? zs : VC_BLOCK, yb = VC_BLOCK / zc;
    const dim3 grid((unsigned)((n + 63) / 64), (unsigned)((n + yb - 1) / yb), (unsigned)((zs + zc - 1) / zc));
    hipLaunchKernelGGL(k_vchange_codes, grid, dim3(VC_BLOCK), 0, s, n, zs, zc, yb, (const v2ull *)planes, out);
    return hipGetLastError();
}

hipError_t gvom_launch_vchange_columns(hipStream_t s, int xy, int zs, int mask, int cap, const void *planes, uint16_t *cols, uint32_t *lohi,
                                       uint32_t *L, uint32_t *count, uint32_t *flags, uint32_t *n_marked, int32_t *D, int32_t *rows4)
{
    if (xy < 1 || xy > GVOM_VATLAS_MAX_CELLS || zs < 1 || zs > GVOM_VATLAS_MAX_CELLS || mask < 1 || mask > 3 || cap < 1 || !planes || !cols || !lohi || !L ||
        !count || !flags || !n_marked || !D || !rows4)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_vchange_columns, dim3((xy + 63) / 64, (xy + 3) / 4), dim3(VC_BLOCK), 0, s, xy, zs, mask, cap, (const v2ull *)planes, cols, lohi,
                       L, count, flags, n_marked, D, rows4);
    return hipGetLastError();
}

hipError_t gvom_launch_vchange_clusters(hipStream_t s, int xy, int cap, int seq, const int32_t *cmap, const uint16_t *cols, const uint32_t *lohi,
                                        const uint32_t *totals, const unsigned long long *cnt, int32_t *rows4, int32_t *counts)
{
    if (xy < 1 || xy > GVOM_VATLAS_MAX_CELLS || cap < 1 || !cmap || !cols || !lohi || !totals || !cnt || !rows4 || !counts) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_vchange_clusters, dim3((xy + 63) / 64, (xy + 3) / 4), dim3(VC_BLOCK), 0, s, xy, cap, seq, cmap, cols, lohi, totals, cnt, rows4,
                       counts);
    return hipGetLastError();
}
