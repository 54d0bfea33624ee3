// gvom_voxel_atlas.hip -- the voxel atlas (include/gvom_hip.h "voxel atlas" defines the result): a world-anchored, toroidally stored
// grid of A x A x Z voxels at 2 bits each that remembers the classes of the fused map beyond the rolling window (gfx950, wave64).
//
// STORAGE (private to this unit): one 16-byte pair {uint64 observed, uint64 occupied} per 64 consecutive world x; world voxel (X, Y, Zv)
// has its bit X & 63 in pair ((Y & (A-1)) * Z + (Zv & (Z-1))) * (A/64) + ((X & (A-1)) >> 6).  occupied implies observed.  The kernels
// take every box RELATIVE to the extent (r = box origin - extent origin, |r| <= 2^30, the host clamps) and the storage phase of its
// first voxel (p = origin & (size - 1)): extent voxel e of an axis lies at storage coordinate (e + phase of the extent) & (size - 1).
//
//   k_vatlas_merge           integrate's hot path: a wave takes one (y, z) row of the window at a time and walks the row's pair columns; a
//                            lane reads the fused state of its world x (tile tag + state, as k_occupancy reads them), two ballots give
//                            the masks of a pair, the wave is the only writer of that pair (plain 16-byte load and store, no atomics on
//                            the planes); the census is population counts of mask combinations, kept in registers while the wave strides
//                            over its rows on a capped grid, then summed over the workgroup in LDS: one 64-bit atomic per counter and workgroup
//   k_vatlas_move            clears one slab of pairs (cyclic intervals of rows, levels and columns, the columns as edge masks)
//   k_vatlas_box             any window-sized box as the uint8 class grid out[x][y][z]: a thread holds the 64 x bits of one (y, z) row
//                            and stores a byte per x; for one x the workgroup's (y, z) are consecutive bytes.  No LDS
//   k_vatlas_align_field     any window-sized box as k_align_field's class grid (gvom_align.hip: 2-bit codes, 16 voxels per uint32, box
//                            order [z][y][x]), so that k_align_score and k_align_best run on remembered space unchanged: k_align_field's
//                            shape -- one box row and a chunk of levels per workgroup, three planes of 64-bit masks in LDS, the
//                            26-neighbourhood by ORs and shifts -- with the masks assembled from pairs as k_vatlas_box assembles its rows,
//                            no ballots; the halo rows, levels and the two x carries are the atlas's own voxels where the extent has them
//   k_vatlas_raycast         k_raycast's walk (gvom_ray.h: set-up and step count) on the atlas: one ray per lane, RQ_DEPTH 16-byte
//                            loads in flight, the lookup masks and shifts only -- no tile tags, no epoch
//   k_vatlas_viewpoints      k_viewpoints' shape on the same lookup; the distinct never-observed voxels of a pose are counted in a bitmap
//                            over a box of the pose's own that the host proves to hold every voxel its beams can examine
//   k_vatlas_viewpoint_best  k_viewpoint_best with the pose's own voxel read from the atlas
//
// Numerics as in gvom_query.hip: -ffp-contract=off, IEEE division / sqrt, every operation rounded once.  Everything that leaves the
// census kernels is an integer sum of population counts: exact whatever the schedule.
#include "gvom_device.h"
#include "gvom_ray.h"
#include "gvom_raywalk.h"
#include "gvom_classgrid.h"
#include "gvom_vatlas_pairs.h"                               // the pair type and address, the fused-state read, the extent mask
#include <algorithm>

#define VA_BLOCK 256
#define VA_WAVES (VA_BLOCK / WAVE)
#define VA_MERGE_BLOCKS 2048                              // the most workgroups of k_vatlas_merge / k_vatlas_move: 8 per CU (every wave slot), each strides over its share

// ---- integrate -------------------------------------------------------------------------------------------------------------------------
// A wave takes (window row y, window level z) = row r = yi * nz + zi at a time and walks its npx pair columns.  They are STORAGE columns --
// bx + k, at most A/64 of them -- so that no two waves share a pair even where the window's clipped x range wraps around the seam;
// the lane's world x follows from its storage x.  Lanes whose x lies outside the window stay idle.  The grid is capped (VA_MERGE_BLOCKS)
// and a wave strides over its share of the rows with the census in registers: the counters share one cache line, and one set of atomics per (row,
// pair) -- 82,000 workgroups on a 256^3 window -- ran at the rate of same-address atomics, 1 ms where the loads need 30 us.
__global__ __launch_bounds__(VA_BLOCK) void k_vatlas_merge(const VAtlas V, const VAtlasWindow D, const OccParams F,
                                                           const int32_t *__restrict__ fstate, const uint32_t *__restrict__ ftags,
                                                           unsigned long long *__restrict__ cnt)
{
    __shared__ int32_t s_c[VA_WAVES][8];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t gw = __builtin_amdgcn_readfirstlane(blockIdx.x * VA_WAVES + wv);
    int32_t c[7] = {0, 0, 0, 0, 0, 0, 0};                 // first seen, free -> occupied, occupied -> free, confirmed, uninformative, d observed, d occupied
    const uint32_t nrows = (uint32_t)D.ny * (uint32_t)D.nz;
    for (uint32_t r = gw; r < nrows; r += gridDim.x * VA_WAVES) {                          // (wave-uniform) a row, then its pair columns
        const uint32_t zi = r % (uint32_t)D.nz, yi = r / (uint32_t)D.nz;
        const uint32_t uA = (uint32_t)V.A, uZ = (uint32_t)V.Z;
        const uint32_t wy = (uint32_t)D.y0 + yi, wz = (uint32_t)D.z0 + zi;                 // window row and level, inside the extent
        const uint32_t sy = ((uint32_t)(D.ry + (int)wy) + (uint32_t)D.pey) & (uA - 1u);
        const uint32_t sz = ((uint32_t)(D.rz + (int)wz) + (uint32_t)D.pez) & (uZ - 1u);
        // the row of the fused map at the mapper's storage index (gvom_internal.h "STORAGE LAYOUT", "TILES")
        const uint32_t uxy = (uint32_t)F.xy, uzs = (uint32_t)F.zs;
        const uint32_t my = wy + (uint32_t)F.om[1], mz = wz + (uint32_t)F.om[2];
        const uint32_t fy = min(my, my - uxy), fz = min(mz, mz - uzs);
        const size_t row = (size_t)fy * uzs + fz;
        for (uint32_t k = 0; k < (uint32_t)D.npx; ++k) {
            const uint32_t sx = ((((uint32_t)D.bx + k) << 6) | lane) & (uA - 1u);
            const uint32_t ex = (sx - (uint32_t)D.pex) & (uA - 1u);                        // extent voxel of this lane's bit
            const uint32_t wx = ex - (uint32_t)D.rx;                                       // its window column (huge where outside)
            const bool in = wx < uxy;
            const uint32_t mx = in ? wx + (uint32_t)F.om[0] : 0u;
            const uint32_t fx = min(mx, mx - uxy);
            int32_t s = -1;
            if (in) s = va_fused_state(F, fstate, ftags, row, fx);
            const unsigned long long m_in = lanes(in), m_obs = lanes(in && s != -1), m_occ = lanes(in && s >= 0);
            v2ull *const pair = (v2ull *)V.pairs + va_pair(V, sx, sy, sz);
            const v2ull old = *pair;                                                       // (wave-uniform address: every lane reads the pair)
            const unsigned long long obs = old.x, occ = old.y;
            v2ull now;
            now.x = obs | m_obs;
            now.y = (occ & ~m_obs) | m_occ;
            if (lane == 0u && m_obs != 0ull) *pair = now;
            c[0] += __builtin_popcountll(m_obs & ~obs);
            c[1] += __builtin_popcountll(m_occ & obs & ~occ);
            c[2] += __builtin_popcountll(m_obs & ~m_occ & occ);
            c[3] += __builtin_popcountll(m_obs & obs & ~(m_occ ^ occ));
            c[4] += __builtin_popcountll(m_in & ~m_obs);
            c[6] += __builtin_popcountll(now.y) - __builtin_popcountll(occ);
        }
    }
    c[5] = c[0];                                          // (a wave's share of a window of fewer than 2^31 voxels: int32 holds it)
    if (lane == 0u) {
#pragma unroll
        for (int e = 0; e < 7; ++e) s_c[wv][e] = c[e];
    }
    __syncthreads();
    if (threadIdx.x < 7u) {
        int32_t t = 0;
#pragma unroll
        for (int w = 0; w < VA_WAVES; ++w) t += s_c[w][threadIdx.x];
        const int slot = threadIdx.x < 5u ? (int)threadIdx.x : (threadIdx.x == 5u ? VA_CNT_OBSERVED : VA_CNT_OCCUPIED);
        if (t != 0) atomicAdd(cnt + slot, (unsigned long long)(long long)t);               // (two's complement: a negative sum subtracts)
    }
}

// ---- move -------------------------------------------------------------------------------------------------------------------------------
// the bits of pair column p (storage x 64 p .. 64 p + 63) whose storage x lies in the cyclic interval [xs, xs + w) mod A, 0 <= w <= A
__device__ __forceinline__ unsigned long long column_mask(uint32_t p, uint32_t xs, uint32_t w, uint32_t A)
{
    const uint32_t rel = ((p << 6) - xs) & (A - 1u);                                       // the pair's first x, counted from the interval's start
    const unsigned long long head = rel < w ? bits_below(min(64u, w - rel)) : 0ull;        // rel + b < w
    const uint32_t wrap = A - rel;                                                         // b >= wrap: the pair runs over the seam of the count
    const unsigned long long tail = wrap < 64u ? bits_below(min(64u, wrap + w)) & ~bits_below(wrap) : 0ull;
    return head | tail;
}

// One thread per pair of the slab at a time: pair t = (yi * nz + zi) * (A/64) + p; a capped grid strides over them.  Counts what it clears: cnt[VA_CNT_MOVED_OBS] += observed
// voxels cleared, and the atlas's totals go down by them.
__global__ __launch_bounds__(VA_BLOCK) void k_vatlas_move(const VAtlas V, const VAtlasSlab S, unsigned long long *__restrict__ cnt)
{
    uint32_t n_obs = 0, n_occ = 0;
    for (size_t t = (size_t)blockIdx.x * VA_BLOCK + threadIdx.x; t < S.npairs; t += (size_t)gridDim.x * VA_BLOCK) {
        const uint32_t uA = (uint32_t)V.A, uZ = (uint32_t)V.Z;
        const uint32_t p = (uint32_t)t & ((uA >> 6) - 1u);
        const uint32_t r = (uint32_t)(t >> V.lgP);
        const uint32_t zi = r % (uint32_t)S.nz, yi = r / (uint32_t)S.nz;
        const uint32_t sy = ((uint32_t)S.ys + yi) & (uA - 1u), sz = ((uint32_t)S.zs + zi) & (uZ - 1u);
        const unsigned long long m = column_mask(p, (uint32_t)S.xs, (uint32_t)S.wx, uA);
        if (m != 0ull) {
            v2ull *const pair = (v2ull *)V.pairs + va_pair(V, p << 6, sy, sz);
            v2ull w = *pair;
            const uint32_t k_obs = (uint32_t)__builtin_popcountll(w.x & m);
            n_obs += k_obs;
            n_occ += (uint32_t)__builtin_popcountll(w.y & m);
            if (k_obs) { w.x &= ~m; w.y &= ~m; *pair = w; }
        }
    }
    n_obs = wave_sum(n_obs); n_occ = wave_sum(n_occ);
    if ((threadIdx.x & 63u) == 0u && n_obs) {
        atomicAdd(cnt + VA_CNT_MOVED_OBS, (unsigned long long)n_obs);
        atomicAdd(cnt + VA_CNT_OBSERVED, 0ull - (unsigned long long)n_obs);
        if (n_occ) atomicAdd(cnt + VA_CNT_OCCUPIED, 0ull - (unsigned long long)n_occ);
    }
}

// ---- box --------------------------------------------------------------------------------------------------------------------------------
// A workgroup takes 64 box columns x (blockIdx.x), VA_BLOCK / zc box rows y (blockIdx.y) and zc levels z (blockIdx.z): thread t = yy * zc + zz
// assembles the 64 bits of its (y, z) row -- two pairs, shifted together, where the box is not aligned to the pair grid --, masks what lies
// outside the extent, and stores the class of every x from its registers.  The bits are x-major and out[x][y][z] is x-outermost, yet
// nothing has to change hands between threads: for one x the workgroup's (y, z) are one contiguous run of out wherever zc == z_size,
// so consecutive threads store consecutive bytes.
__global__ __launch_bounds__(VA_BLOCK) void k_vatlas_box(const VAtlas V, const VAtlasBox B, uint8_t *__restrict__ out, int32_t *__restrict__ counts)
{
    const uint32_t t = threadIdx.x;
    const uint32_t uA = (uint32_t)V.A, uZ = (uint32_t)V.Z, n = (uint32_t)B.n, zs = (uint32_t)B.zs, zc = (uint32_t)B.zc;
    const uint32_t yy = t / zc, zz = t - yy * zc;
    const uint32_t x0 = blockIdx.x * 64u, y = blockIdx.y * (uint32_t)B.yb + yy, z = blockIdx.z * zc + zz;
    const bool mine = yy < (uint32_t)B.yb && y < n && z < zs;
    unsigned long long obs = 0ull, occ = 0ull;
    const uint32_t ey = (uint32_t)(B.ry + (int)y), ez = (uint32_t)(B.rz + (int)z);
    if (mine && ey < uA && ez < uZ) {
        const uint32_t sy = ((uint32_t)B.py + y) & (uA - 1u), sz = ((uint32_t)B.pz + z) & (uZ - 1u);
        const uint32_t sx = ((uint32_t)B.px + x0) & (uA - 1u), sh = sx & 63u;
        const v2ull lo = ((const v2ull *)V.pairs)[va_pair(V, sx, sy, sz)];
        obs = lo.x >> sh; occ = lo.y >> sh;
        if (sh) {
            const v2ull hi = ((const v2ull *)V.pairs)[va_pair(V, (sx + 64u) & (uA - 1u), sy, sz)];
            obs |= hi.x << (64u - sh); occ |= hi.y << (64u - sh);
        }
        const unsigned long long valid = va_columns_inside(B.rx, x0, n, uA);
        obs &= valid; occ &= valid;
    }
    const uint32_t c_occ = wave_sum((uint32_t)__builtin_popcountll(occ)), c_free = wave_sum((uint32_t)__builtin_popcountll(obs & ~occ));
    if ((t & 63u) == 0u) {
        if (c_occ) atomicAdd(counts, (int32_t)c_occ);
        if (c_free) atomicAdd(counts + 1, (int32_t)c_free);
    }
    if (blockIdx.x == 0u && blockIdx.y == 0u && blockIdx.z == 0u && t == 0u) { counts[2] = B.outside; counts[3] = B.seq; }
    if (mine) {
        const uint32_t nx = min(64u, n - x0);
        uint8_t *o = out + ((size_t)x0 * n + y) * zs + z;
        const size_t pitch = (size_t)n * zs;
        for (uint32_t b = 0; b < nx; ++b) o[b * pitch] = (uint8_t)(((obs >> b) & 1ull) + ((occ >> b) & 1ull));     // 0 never, 1 free, 2 occupied
    }
}

// ---- the class grid of scan alignment scoring ---------------------------------------------------------------------------------------------
// which of the 64 box columns x0 .. x0 + 63 of box row y and box level z lie inside the extent (0 where the row or the level does not)
__device__ __forceinline__ unsigned long long va_box_inside(const VAtlas &V, const VAtlasBox &B, int x0, int y, int z)
{
    const uint32_t ey = (uint32_t)(B.ry + y), ez = (uint32_t)(B.rz + z);                   // (|r| <= 2^30, |y|, |z| <= 4160: no overflow)
    const int e0 = B.rx + x0;                                                              // extent voxel of bit 0
    const int lo_b = e0 < 0 ? -e0 : 0, hi_b = min(64, V.A - e0);                           // bits [lo_b, hi_b)
    if (ey >= (uint32_t)V.A || ez >= (uint32_t)V.Z || lo_b >= hi_b) return 0ull;
    return bits_below((uint32_t)hi_b) & ~bits_below((uint32_t)lo_b);
}

// the pair of the 64 box columns x0 .. x0 + 63 (x0 a multiple of 64; -64 and past the box's last column included) of box row y and box
// level z, both possibly one outside the box: two storage pairs shifted together, the bits outside the extent cleared.  Every wrap is an AND
__device__ __forceinline__ v2ull va_box_segment(const VAtlas &V, const VAtlasBox &B, int x0, int y, int z)
{
    const uint32_t uA = (uint32_t)V.A, uZ = (uint32_t)V.Z;
    v2ull r = {0ull, 0ull};
    const unsigned long long valid = va_box_inside(V, B, x0, y, z);
    if (valid != 0ull) {
        const uint32_t sy = ((uint32_t)B.py + (uint32_t)y) & (uA - 1u), sz = ((uint32_t)B.pz + (uint32_t)z) & (uZ - 1u);
        const uint32_t sx = ((uint32_t)B.px + (uint32_t)x0) & (uA - 1u), sh = sx & 63u;
        const v2ull lo = ((const v2ull *)V.pairs)[va_pair(V, sx, sy, sz)];
        r.x = lo.x >> sh; r.y = lo.y >> sh;
        if (sh) {
            const v2ull hi = ((const v2ull *)V.pairs)[va_pair(V, (sx + 64u) & (uA - 1u), sy, sz)];
            r.x |= hi.x << (64u - sh); r.y |= hi.y << (64u - sh);
        }
        r.x &= valid; r.y &= valid;
    }
    return r;
}

// LDS: plane [0], (zc + 2) levels x (nq + 2) 64-bit words: occupied in box rows y - 1 .. y + 1, segments -1 .. nq (the two outer ones
// carry the voxels next to the box's first and last column); planes [1] and [2], (zc + 2) levels x nq words: occupied / free in row y.
// Level l of a plane is box level z0 - 1 + l.  A thread assembles one segment of one level: up to six 16-byte loads in flight, no ballots.
// dilate == 0 loads no halo: rows y +- 1, levels z0 - 1 and z0 + zc and the outer segments stay zero.
__global__ __launch_bounds__(VA_BLOCK) void k_vatlas_align_field(const VAtlas V, const VAtlasBox B, const int zc, const int nq, const int rw,
                                                                 const int dilate, uint32_t *__restrict__ grid)
{
    extern __shared__ unsigned long long s_va[];
    const int y = (int)blockIdx.x, z0 = (int)blockIdx.y * zc;
    const int nl = zc + 2, na = nq + 2;
    unsigned long long *const s_around = s_va, *const s_own = s_va + nl * na, *const s_free = s_own + nl * nq;
    const int nlev = min(zc, B.zs - z0);                                                   // the box levels this workgroup writes
    for (int it = (int)threadIdx.x; it < nl * na; it += VA_BLOCK) {
        const int l = it / na, q = it - l * na - 1;                                        // segment q = -1 .. nq
        const int z = z0 - 1 + l, x0 = q * 64;
        const bool inner = q >= 0 && q < nq && l >= 1 && l <= nlev;                        // a segment of the box itself
        unsigned long long around = 0ull, own = 0ull, fre = 0ull;
        if (dilate ? l <= nlev + 1 : inner) {
            v2ull p[3] = {{0ull, 0ull}, {0ull, 0ull}, {0ull, 0ull}};
#pragma unroll
            for (int d = 0; d < 3; ++d)                                                    // rows y - 1, y, y + 1: their loads in flight together
                if (d == 1 || dilate) p[d] = va_box_segment(V, B, x0, y + d - 1, z);
            around = p[0].y | p[1].y | p[2].y;
            const unsigned long long box = bits_below((uint32_t)min(64, max(0, B.n - x0)));   // the columns inside the box
            own = p[1].y & box; fre = p[1].x & ~p[1].y & box;
        }
        s_around[it] = around;
        if (q >= 0 && q < nq) { s_own[l * nq + q] = inner ? own : 0ull; s_free[l * nq + q] = inner ? fre : 0ull; }
    }
    __syncthreads();
    for (int it = (int)threadIdx.x; it < nlev * nq * 4; it += VA_BLOCK) {
        const int j = it & 3, lq = it >> 2;
        const int l = lq / nq + 1, q = lq - (l - 1) * nq;
        if (q * 4 + j >= rw) continue;
        const unsigned long long own = s_own[l * nq + q], fre = s_free[l * nq + q];
        unsigned long long near = 0ull;
        if (dilate) {
            unsigned long long m = 0ull, left = 0ull, right = 0ull;
#pragma unroll
            for (int dl = -1; dl <= 1; ++dl) {
                const unsigned long long *row = s_around + (l + dl) * na + q + 1;
                m |= row[0]; left |= row[-1]; right |= row[1];
            }
            near = (m | (m << 1) | (m >> 1) | (left >> 63) | (right << 63)) & va_box_inside(V, B, q * 64, y, z0 + l - 1);   // a voxel outside the extent is UNKNOWN
        }
        const uint32_t o16 = (uint32_t)(own >> (16 * j)), n16 = (uint32_t)(near >> (16 * j)), f16 = (uint32_t)(fre >> (16 * j));
        // AL_OCC 0, AL_NEAR 1, AL_FREE 2, AL_UNK 3: high bit = neither occupied nor near, low bit = not occupied and (near or not free)
        const uint32_t hi = ~o16 & ~n16, lo = ~o16 & (n16 | ~f16);
        const int z = z0 + l - 1;
        grid[((size_t)z * B.n + y) * rw + q * 4 + j] = al_spread16(lo) | (al_spread16(hi) << 1);
    }
}

// ---- the walk kernels' lookup ------------------------------------------------------------------------------------------------------------
// The frame is a ScanParams whose "window" is the extent: origin = E, xy = A, zs = Z, om = E & (size - 1).  Pair index and bit of the
// extent voxel (wx, wy, wz); pair 0 -- in bounds, the value is ignored -- where the position is outside the extent.
struct VaStep { uint32_t idx, wx, wy, wz; bool in; };

template <bool LIT>
__device__ __forceinline__ void va_lookup(const ScanParams &P, const VAtlas &V, const float (&qx)[RQ_DEPTH], const float (&qy)[RQ_DEPTH],
                                          const float (&qz)[RQ_DEPTH], VaStep (&st)[RQ_DEPTH])
{
    const uint32_t uA = (uint32_t)V.A, uZ = (uint32_t)V.Z;
    const uint32_t o0 = (uint32_t)(int)P.origin[0], o1 = (uint32_t)(int)P.origin[1], o2 = (uint32_t)(int)P.origin[2];
#pragma unroll
    for (int d = 0; d < RQ_DEPTH; ++d) {
        uint32_t wx, wy, wz;
        const bool in = window_voxel<LIT>(P, qx[d], qy[d], qz[d], wx, wy, wz, o0, o1, o2, uA, uA - uZ);
        const uint32_t sx = (wx + (uint32_t)P.om[0]) & (uA - 1u), sy = (wy + (uint32_t)P.om[1]) & (uA - 1u), sz = (wz + (uint32_t)P.om[2]) & (uZ - 1u);
        st[d].in = in; st[d].wx = wx; st[d].wy = wy; st[d].wz = wz;
        st[d].idx = in ? (uint32_t)va_pair(V, sx, sy, sz) : 0u;                            // (< 2^26 pairs)
    }
}

// the same for k_vatlas_raycast, which needs the voxel of ONE position per ray (its stop) and recomputes it there: pair index and bit in
// one word, (idx << 6) | bit, idx < 2^26
template <bool LIT>
__device__ __forceinline__ void va_lookup_packed(const ScanParams &P, const VAtlas &V, const float (&qx)[RQ_DEPTH], const float (&qy)[RQ_DEPTH],
                                                 const float (&qz)[RQ_DEPTH], uint32_t (&at)[RQ_DEPTH], bool (&in)[RQ_DEPTH])
{
    const uint32_t uA = (uint32_t)V.A, uZ = (uint32_t)V.Z;
    const uint32_t o0 = (uint32_t)(int)P.origin[0], o1 = (uint32_t)(int)P.origin[1], o2 = (uint32_t)(int)P.origin[2];
#pragma unroll
    for (int d = 0; d < RQ_DEPTH; ++d) {
        uint32_t wx, wy, wz;
        in[d] = window_voxel<LIT>(P, qx[d], qy[d], qz[d], wx, wy, wz, o0, o1, o2, uA, uA - uZ);
        const uint32_t sx = (wx + (uint32_t)P.om[0]) & (uA - 1u), sy = (wy + (uint32_t)P.om[1]) & (uA - 1u), sz = (wz + (uint32_t)P.om[2]) & (uZ - 1u);
        at[d] = in[d] ? ((uint32_t)va_pair(V, sx, sy, sz) << 6) | (sx & 63u) : 0u;
    }
}

__device__ __forceinline__ v2ull va_load(const VAtlas &V, const ScanParams &P, uint32_t wx, uint32_t wy, uint32_t wz, uint32_t &bit)
{
    const uint32_t uA = (uint32_t)V.A, uZ = (uint32_t)V.Z;
    const uint32_t sx = (wx + (uint32_t)P.om[0]) & (uA - 1u), sy = (wy + (uint32_t)P.om[1]) & (uA - 1u), sz = (wz + (uint32_t)P.om[2]) & (uZ - 1u);
    bit = sx & 63u;
    return ((const v2ull *)V.pairs)[va_pair(V, sx, sy, sz)];
}

struct __attribute__((aligned(4))) VaInt3 { int32_t a, b, c; };
struct __attribute__((aligned(4))) VaFloat3 { float x, y, z; };

// ---- rays ---------------------------------------------------------------------------------------------------------------------------------
// k_raycast's body (gvom_query.hip) with the atlas lookup: one ray per lane, a round computes RQ_DEPTH positions, issues their pair
// loads together (a load from outside the extent is pair 0: in bounds and ignored) and examines them in step order.  No LDS, no atomics.
__global__ __launch_bounds__(VA_BLOCK) void k_vatlas_raycast(const ScanParams P, const RayQuery Q, const VAtlas V, VaInt3 *__restrict__ out,
                                                             VaFloat3 *__restrict__ out_pos, VaInt3 *__restrict__ out_vox)
{
    const long i = (long)blockIdx.x * VA_BLOCK + threadIdx.x;
    const bool live = i < Q.n;
    float ax = 0.0f, ay = 0.0f, az = 0.0f, bx = 0.0f, by = 0.0f, bz = 0.0f;
    if (live) {
        const float *a = Q.from + (Q.one_origin ? 0 : 3 * i), *b = Q.to + 3 * i;
        ax = a[0]; ay = a[1]; az = a[2]; bx = b[0]; by = b[1]; bz = b[2];
    }
    const bool fin = fabsf(ax) < INFINITY && fabsf(ay) < INFINITY && fabsf(az) < INFINITY &&
                     fabsf(bx) < INFINITY && fabsf(by) < INFINITY && fabsf(bz) < INFINITY;
    int32_t r_status = RQ_INVALID, r_steps = 0, r_unknown = 0;
    uint32_t r_wx = 0, r_wy = 0, r_wz = 0;
    bool r_at = false, r_step = false;                    // stopped at a voxel; at a step's (its position is r_q)
    float r_qx = 0.0f, r_qy = 0.0f, r_qz = 0.0f;
    float r_x = NAN, r_y = NAN, r_z = NAN;
    // ray set-up (gvom.py:1097-1126): the start in voxels, increments, the steps the loop test admits
    float px = (float)div_by_res<float>(ax, P.xy_res, P.drcp[0], P.fastdiv & 1);
    float py = (float)div_by_res<float>(ay, P.xy_res, P.drcp[0], P.fastdiv & 1);
    float pz = (float)div_by_res<float>(az, P.z_res, P.drcp[1], P.fastdiv & 2);
    const RaySetup R = ray_setup<float, true>(P, bx, by, bz, px, py, pz);
    const uint32_t S = ray_steps(R.lim, R.step_len, R.inv_step, Q.cap);
    bool run = live && fin;
    if (run && S > 0u && !R.finite) {                     // the first step lands on NaN / inf: outside the extent
        r_status = RQ_LEFT_WINDOW;
        run = false;
    }
    uint32_t j = 0;                                       // steps taken so far: the same in every lane
    unsigned long long alive = lanes(run && S > 0u);
    while (alive != 0ull) {
        float qx[RQ_DEPTH], qy[RQ_DEPTH], qz[RQ_DEPTH];
        bool nz = false;
#pragma unroll
        for (int d = 0; d < RQ_DEPTH; ++d) {
            px += R.incx; py += R.incy; pz += R.incz;     // gvom.py:1128-1132
            qx[d] = px; qy[d] = py; qz[d] = pz;
            nz |= (px < 0.0f && px > -1e-4f) || (py < 0.0f && py > -1e-4f) || (pz < 0.0f && pz > -1e-4f);
        }
        uint32_t at[RQ_DEPTH];
        bool in[RQ_DEPTH];
        if (Q.lit || lanes(run && nz) != 0ull) va_lookup_packed<true>(P, V, qx, qy, qz, at, in);      // (wave-uniform)
        else va_lookup_packed<false>(P, V, qx, qy, qz, at, in);
        v2ull w[RQ_DEPTH];
#pragma unroll
        for (int d = 0; d < RQ_DEPTH; ++d) w[d] = ((const v2ull *)V.pairs)[at[d] >> 6];
#pragma unroll
        for (int d = 0; d < RQ_DEPTH; ++d) {
            const uint32_t jj = j + (uint32_t)d + 1u;
            if (run && jj <= S) {
                const uint32_t bit = at[d] & 63u;
                const bool outside = !in[d];
                const bool occ = !outside && ((w[d].y >> bit) & 1ull) != 0ull;
                const bool unk = !outside && ((w[d].x >> bit) & 1ull) == 0ull;
                r_unknown += unk ? 1 : 0;
                const bool stop = outside || occ || (unk && Q.unknown_blocks);
                if (stop) {
                    r_status = outside ? RQ_LEFT_WINDOW : (occ ? RQ_OCCUPIED : RQ_UNKNOWN);
                    r_steps = outside ? (int32_t)jj - 1 : (int32_t)jj;
                    r_step = !outside;
                    r_qx = qx[d]; r_qy = qy[d]; r_qz = qz[d];
                    run = false;
                }
            }
        }
        j += RQ_DEPTH;
        alive = lanes(run && j < S);
    }
    if (r_step) {                                         // the stop's voxel, in the literal form (what every form of the lookup equals), and its position
        r_at = window_voxel<true>(P, r_qx, r_qy, r_qz, r_wx, r_wy, r_wz);
        r_x = (float)((double)r_qx * P.xy_res); r_y = (float)((double)r_qy * P.xy_res); r_z = (float)((double)r_qz * P.z_res);
    }
    if (run) {                                            // S unstopped steps
        r_status = RQ_CLEAR; r_steps = (int32_t)S;
        if (Q.check_target) {                             // the end point's own voxel (gvom.py:1072-1080), literal form
            uint32_t wx, wy, wz, bit;
            const bool in = rq_point_voxel(P, bx, by, bz, wx, wy, wz);
            const v2ull w = va_load(V, P, wx, wy, wz, bit);                                // (voxel 0 of the extent where outside: ignored)
            const bool occ = in && ((w.y >> bit) & 1ull) != 0ull;
            const bool unk = in && ((w.x >> bit) & 1ull) == 0ull;
            r_unknown += unk ? 1 : 0;
            if (!in) r_status = RQ_LEFT_WINDOW;
            else if (occ || (unk && Q.unknown_blocks)) {
                r_status = occ ? RQ_OCCUPIED : RQ_UNKNOWN;
                r_steps = (int32_t)S + 1;
                r_at = true; r_wx = wx; r_wy = wy; r_wz = wz;
                r_x = bx; r_y = by; r_z = bz;
            }
        }
    }
    if (live) {
        const VaInt3 r = {r_status, r_steps, r_unknown};
        out[i] = r;
        const VaFloat3 q = {r_x, r_y, r_z};
        out_pos[i] = q;
        // the world voxel of the stop: E + extent voxel (|E| < 2^30, the host checks)
        const VaInt3 v = {r_at ? (int32_t)P.origin[0] + (int32_t)r_wx : 0, r_at ? (int32_t)P.origin[1] + (int32_t)r_wy : 0,
                          r_at ? (int32_t)P.origin[2] + (int32_t)r_wz : 0};
        out_vox[i] = v;
    }
}

// ---- viewpoints ---------------------------------------------------------------------------------------------------------------------------
// k_viewpoints' body (gvom_viewpoint.hip) with the atlas lookup.  boxes [K][8] int32 = {lx, ly, lz, dx, dy, dz, 0, 0}: the box of extent
// voxels of pose k, inside the extent, dx * dy * dz <= 32 * Q.bm_words; bit ((wz - lz) * dy + (wy - ly)) * dx + (wx - lx) of the pose's
// bitmap stands for extent voxel (wx, wy, wz).  The host proves that every voxel a beam of the pose examines lies in the box; a voxel
// outside it would be counted without deduplication, never written outside the bitmap.
__global__ __launch_bounds__(VA_BLOCK) void k_vatlas_viewpoints(const ScanParams P, const ViewQuery Q, const VAtlas V, const int32_t *__restrict__ boxes,
                                                                uint32_t *__restrict__ bitmaps, int32_t *__restrict__ rows)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gw = __builtin_amdgcn_readfirstlane(blockIdx.x * VA_WAVES + (threadIdx.x >> 6));
    const uint32_t hi = gw / Q.nwc, wi = (gw - hi * Q.nwc) * 64u + lane;
    if (hi >= Q.nh) return;                               // (the whole wave: the last workgroup's spare waves)
    const uint32_t k = Q.k0 + blockIdx.y;                 // < K: the grid's y extent is the batch
    double c[12];
    if (!rq_pose(Q.poses, k, c)) return;                  // an invalid pose: k_vatlas_viewpoint_best writes its row
    const bool live = wi < Q.nw;
    // the beam's end point (include/gvom_hip.h "viewpoint scoring": k_unproject's arithmetic with r = max_range)
    double d[3] = {0.0, 0.0, 0.0}, o[3] = {0.0, 0.0, 0.0};
    if (live) {
        const size_t pix = (size_t)(hi * Q.stride_h) * Q.W + (size_t)wi * Q.stride_w;     // h < H and w < W: inside the model
#pragma unroll
        for (int e = 0; e < 3; ++e) { d[e] = Q.dir[3 * pix + e]; o[e] = Q.off[3 * pix + e]; }
    }
    double p[3], q[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const double m = Q.max_range * d[e];
        p[e] = m + o[e];
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const double m0 = p[0] * c[4 * e], m1 = p[1] * c[4 * e + 1], m2 = p[2] * c[4 * e + 2];
        q[e] = ((m0 + m1) + m2) + c[4 * e + 3];
    }
    const float ax = (float)c[3], ay = (float)c[7], az = (float)c[11];
    const float bx = (float)q[0], by = (float)q[1], bz = (float)q[2];
    const bool fin = fabsf(ax) < INFINITY && fabsf(ay) < INFINITY && fabsf(az) < INFINITY &&
                     fabsf(bx) < INFINITY && fabsf(by) < INFINITY && fabsf(bz) < INFINITY;
    int32_t r_status = RQ_INVALID, r_unknown = 0, r_first = 0;
    float px = (float)div_by_res<float>(ax, P.xy_res, P.drcp[0], P.fastdiv & 1);
    float py = (float)div_by_res<float>(ay, P.xy_res, P.drcp[0], P.fastdiv & 1);
    float pz = (float)div_by_res<float>(az, P.z_res, P.drcp[1], P.fastdiv & 2);
    const RaySetup R = ray_setup<float, true>(P, bx, by, bz, px, py, pz);
    const uint32_t S = ray_steps(R.lim, R.step_len, R.inv_step, Q.cap);
    bool run = live && fin;
    if (run && S > 0u && !R.finite) {                     // the first step lands on NaN / inf: outside the extent
        r_status = RQ_LEFT_WINDOW;
        run = false;
    }
    const int32_t *const box = boxes + (size_t)k * 8;     // (wave-uniform)
    const uint32_t lx = (uint32_t)box[0], ly = (uint32_t)box[1], lz = (uint32_t)box[2];
    const uint32_t dx = (uint32_t)box[3], dy = (uint32_t)box[4], dz = (uint32_t)box[5];
    uint32_t *const bm = bitmaps + (size_t)blockIdx.y * Q.bm_words;
    uint32_t j = 0;
    unsigned long long alive = lanes(run && S > 0u);
    while (alive != 0ull) {
        float qx[RQ_DEPTH], qy[RQ_DEPTH], qz[RQ_DEPTH];
        bool nz = false;
#pragma unroll
        for (int t = 0; t < RQ_DEPTH; ++t) {
            px += R.incx; py += R.incy; pz += R.incz;     // gvom.py:1128-1132
            qx[t] = px; qy[t] = py; qz[t] = pz;
            nz |= (px < 0.0f && px > -1e-4f) || (py < 0.0f && py > -1e-4f) || (pz < 0.0f && pz > -1e-4f);
        }
        VaStep st[RQ_DEPTH];
        if (Q.lit || lanes(run && nz) != 0ull) va_lookup<true>(P, V, qx, qy, qz, st);      // (wave-uniform)
        else va_lookup<false>(P, V, qx, qy, qz, st);
        v2ull w[RQ_DEPTH];
#pragma unroll
        for (int t = 0; t < RQ_DEPTH; ++t) w[t] = ((const v2ull *)V.pairs)[st[t].idx];
#pragma unroll
        for (int t = 0; t < RQ_DEPTH; ++t) {
            const uint32_t jj = j + (uint32_t)t + 1u;
            if (run && jj <= S) {
                const uint32_t bit = (st[t].wx + (uint32_t)P.om[0]) & 63u;
                const bool outside = !st[t].in;
                const bool occ = !outside && ((w[t].y >> bit) & 1ull) != 0ull;
                const bool unk = !outside && ((w[t].x >> bit) & 1ull) == 0ull;
                if (unk) {
                    const uint32_t ux = st[t].wx - lx, uy = st[t].wy - ly, uz = st[t].wz - lz;
                    r_unknown += 1;
                    if (ux < dx && uy < dy && uz < dz) {
                        const uint32_t v = (uz * dy + uy) * dx + ux;                        // < 2^31: inside the bitmap
                        const uint32_t b = 1u << (v & 31u);
                        const uint32_t old = atomicOr(bm + (v >> 5), b);
                        r_first += (old & b) ? 0 : 1;                                       // exactly one lane finds the bit clear
                    } else r_first += 1;
                }
                if (outside || occ || (unk && Q.unknown_blocks)) {
                    r_status = outside ? RQ_LEFT_WINDOW : (occ ? RQ_OCCUPIED : RQ_UNKNOWN);
                    run = false;
                }
            }
        }
        j += RQ_DEPTH;
        alive = lanes(run && j < S);
    }
    if (run) r_status = RQ_CLEAR;                         // S unstopped steps
    rq_census(live ? r_status : -1, r_unknown, r_first, lane, rows + (size_t)k * 8);
}

// k_viewpoint_best (gvom_viewpoint.hip) with the class of the pose's own voxel read from the atlas: column 0 of every row, the whole row
// of an invalid pose, and part 1 = {best, gain[best], K, nb}.  One workgroup, behind the last batch.
__global__ __launch_bounds__(VA_BLOCK) void k_vatlas_viewpoint_best(const ScanParams P, const ViewQuery Q, const VAtlas V, int32_t *__restrict__ rows,
                                                                    int32_t *__restrict__ best)
{
    unsigned long long key = 0ull;
    for (uint32_t k = threadIdx.x; k < (uint32_t)Q.K; k += VA_BLOCK) {
        double c[12];
        int32_t *row = rows + (size_t)k * 8;
        if (!rq_pose(Q.poses, k, c)) {
            const v4i lo = {RQ_INVALID, 0, 0, 0}, hi = {0, 0, 0, Q.nb};
            *(v4i *)row = lo; *(v4i *)(row + 4) = hi;
            continue;
        }
        uint32_t wx, wy, wz, bit;
        const bool in = rq_point_voxel(P, (float)c[3], (float)c[7], (float)c[11], wx, wy, wz);
        const v2ull w = va_load(V, P, wx, wy, wz, bit);
        const bool occ = ((w.y >> bit) & 1ull) != 0ull, obs = ((w.x >> bit) & 1ull) != 0ull;
        const int32_t status = !in ? RQ_LEFT_WINDOW : (occ ? RQ_OCCUPIED : (!obs ? RQ_UNKNOWN : RQ_CLEAR));
        row[0] = status;
        if (status == RQ_CLEAR) {
            const unsigned long long cand = ((unsigned long long)((uint32_t)row[1] + 1u) << 32) | (unsigned long long)(~k);
            key = cand > key ? cand : key;
        }
    }
    rq_best_store<VA_BLOCK>(key, Q, best);
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------------
static bool va_ok(const VAtlas &V)
{
    return V.pairs && V.A >= GVOM_VATLAS_MIN_CELLS && V.A <= GVOM_VATLAS_MAX_CELLS && !(V.A & (V.A - 1)) && V.Z >= 1 && V.Z <= V.A && !(V.Z & (V.Z - 1)) &&
           (1 << V.lgZ) == V.Z && (64 << V.lgP) == V.A;
}

hipError_t gvom_launch_vatlas_merge(hipStream_t s, const VAtlas &V, const VAtlasWindow &D, const OccParams &F, const int32_t *fstate,
                                    const uint32_t *ftags, unsigned long long *cnt)
{
    if (!va_ok(V) || F.xy <= 0 || F.zs <= 0 || D.ny < 0 || D.nz < 0 || D.npx < 0 || D.npx > V.A / 64) return hipErrorInvalidValue;
    if (D.y0 < 0 || D.y0 + D.ny > F.xy || D.z0 < 0 || D.z0 + D.nz > F.zs) return hipErrorInvalidValue;      // rows and levels of the window
    if (D.ny && (D.ry + D.y0 < 0 || D.ry + D.y0 + D.ny > V.A)) return hipErrorInvalidValue;                  // ... that lie inside the extent
    if (D.nz && (D.rz + D.z0 < 0 || D.rz + D.z0 + D.nz > V.Z)) return hipErrorInvalidValue;
    if ((uint64_t)D.ny * (uint64_t)D.nz * (uint64_t)D.npx != D.npairs) return hipErrorInvalidValue;
    if (D.npairs == 0) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<uint64_t>(((uint64_t)D.ny * (uint64_t)D.nz + VA_WAVES - 1) / VA_WAVES, VA_MERGE_BLOCKS);
    hipLaunchKernelGGL(k_vatlas_merge, dim3(blocks), dim3(VA_BLOCK), 0, s, V, D, F, fstate, ftags, cnt);
    return hipGetLastError();
}

hipError_t gvom_launch_vatlas_move(hipStream_t s, const VAtlas &V, const VAtlasSlab &S, unsigned long long *cnt)
{
    if (!va_ok(V) || S.ny < 0 || S.ny > V.A || S.nz < 0 || S.nz > V.Z || S.wx < 0 || S.wx > V.A) return hipErrorInvalidValue;
    if (S.ys < 0 || S.ys >= V.A || S.zs < 0 || S.zs >= V.Z || S.xs < 0 || S.xs >= V.A) return hipErrorInvalidValue;
    if ((uint64_t)S.ny * (uint64_t)S.nz * (uint64_t)(V.A / 64) != S.npairs) return hipErrorInvalidValue;
    if (S.npairs == 0 || S.wx == 0) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<uint64_t>((S.npairs + VA_BLOCK - 1) / VA_BLOCK, VA_MERGE_BLOCKS);
    hipLaunchKernelGGL(k_vatlas_move, dim3(blocks), dim3(VA_BLOCK), 0, s, V, S, cnt);
    return hipGetLastError();
}

hipError_t gvom_launch_vatlas_box(hipStream_t s, const VAtlas &V, VAtlasBox B, uint8_t *out, int32_t *counts)
{
    if (!va_ok(V) || B.n < 1 || B.zs < 1 || !out || !counts) return hipErrorInvalidValue;
    B.zc = B.zs < VA_BLOCK ? B.zs : VA_BLOCK;
    B.yb = VA_BLOCK / B.zc;
    const dim3 grid((unsigned)((B.n + 63) / 64), (unsigned)((B.n + B.yb - 1) / B.yb), (unsigned)((B.zs + B.zc - 1) / B.zc));
    hipLaunchKernelGGL(k_vatlas_box, grid, dim3(VA_BLOCK), 0, s, V, B, out, counts);
    return hipGetLastError();
}

// levels per workgroup of k_vatlas_align_field: what fits the LDS budget ((zc + 2) levels of 3 nq + 2 64-bit words), at most AL_ZC_MAX
hipError_t gvom_launch_vatlas_align_field(hipStream_t s, const VAtlas &V, const VAtlasBox &B, int dilate, uint32_t *grid)
{
    if (!va_ok(V) || B.n < 1 || B.n > GVOM_VATLAS_MAX_CELLS || B.zs < 1 || B.zs > GVOM_VATLAS_MAX_CELLS || !grid || (dilate != 0 && dilate != 1))
        return hipErrorInvalidValue;
    if (B.px < 0 || B.px >= V.A || B.py < 0 || B.py >= V.A || B.pz < 0 || B.pz >= V.Z) return hipErrorInvalidValue;
    const int lim = 1 << 30;
    if (B.rx < -lim || B.rx > lim || B.ry < -lim || B.ry > lim || B.rz < -lim || B.rz > lim) return hipErrorInvalidValue;
    const int nq = (B.n + 63) / 64, rw = (B.n + 15) / 16;
    int zc = AL_LDS_BUDGET / (8 * (3 * nq + 2)) - 2;
    zc = zc > AL_ZC_MAX ? AL_ZC_MAX : zc;
    zc = zc > B.zs ? B.zs : zc;
    if (zc < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_vatlas_align_field, dim3((unsigned)B.n, (unsigned)((B.zs + zc - 1) / zc)), dim3(VA_BLOCK), (size_t)(zc + 2) * (3 * nq + 2) * 8, s,
                       V, B, zc, nq, rw, dilate, grid);
    return hipGetLastError();
}

hipError_t gvom_launch_vatlas_raycast(hipStream_t s, const ScanParams &P, const RayQuery &Q, const VAtlas &V, int32_t *out3, float *pos3, int32_t *vox3)
{
    if (!va_ok(V) || Q.n < 1 || P.xy != V.A || P.zs != V.Z) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((Q.n + VA_BLOCK - 1) / VA_BLOCK);
    hipLaunchKernelGGL(k_vatlas_raycast, dim3(blocks), dim3(VA_BLOCK), 0, s, P, Q, V, (VaInt3 *)out3, (VaFloat3 *)pos3, (VaInt3 *)vox3);
    return hipGetLastError();
}

hipError_t gvom_launch_vatlas_viewpoints(hipStream_t s, const ScanParams &P, const ViewQuery &Q, const VAtlas &V, int batch, const int32_t *boxes,
                                         uint32_t *bitmaps, int32_t *rows)
{
    if (!va_ok(V) || P.xy != V.A || P.zs != V.Z || batch < 1 || batch > GVOM_VIEWPOINT_MAX_BATCH || Q.k0 < 0 || Q.k0 + batch > Q.K || Q.nh < 1 || Q.nw < 1 ||
        Q.nwc < 1 || !boxes)
        return hipErrorInvalidValue;
    const unsigned waves = (unsigned)Q.nh * (unsigned)Q.nwc;
    const dim3 grid((waves + VA_WAVES - 1) / VA_WAVES, (unsigned)batch);
    hipLaunchKernelGGL(k_vatlas_viewpoints, grid, dim3(VA_BLOCK), 0, s, P, Q, V, boxes, bitmaps, rows);
    return hipGetLastError();
}

hipError_t gvom_launch_vatlas_viewpoint_best(hipStream_t s, const ScanParams &P, const ViewQuery &Q, const VAtlas &V, int32_t *rows, int32_t *best)
{
    if (!va_ok(V) || P.xy != V.A || P.zs != V.Z || Q.K < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_vatlas_viewpoint_best, dim3(1), dim3(VA_BLOCK), 0, s, P, Q, V, rows, best);
    return hipGetLastError();
}
