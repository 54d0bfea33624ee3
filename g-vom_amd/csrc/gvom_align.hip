// gvom_align.hip -- scan alignment scoring (gfx950, wave64): K candidate rigid transforms of one float32 cloud of n returns held
// against the fused map -- per candidate, how many returns end in an occupied voxel, next to one, in a free one, in a never-observed
// one, outside the window (include/gvom_hip.h "scan alignment scoring" defines the result).
//
//   k_align_field   one pass over the fused state and its tile tags: the CLASS GRID, a 2-bit code per voxel (AL_OCC, AL_NEAR, AL_FREE,
//                   AL_UNK), 16 voxels per uint32, in WINDOW order [z][y][x] with rows padded to whole words.  A workgroup takes one
//                   window row y and AL_ZC levels; per level and 64-voxel segment a wave makes, with ballots, the bitmask of the
//                   occupied voxels of the rows y - 1, y, y + 1 OR-ed together and the occupied / free masks of row y itself, all in
//                   LDS.  Behind a barrier the 26-neighbourhood is three levels OR-ed and the x neighbours by shifts (the bit carried
//                   over from the neighbouring 64-bit words); the codes are interleaved into words by bit spreading.
//   k_align_score   the hot path, K * n pairs.  A workgroup takes AL_PTS_BLOCK returns -- AL_PTS per lane, widened to float64 once and
//                   kept in registers -- and a group of AL_CG candidates.  A candidate's twelve doubles are wave-uniform (scalar
//                   loads); per pair the scan's own transform (float64, source order, rounded once to float32: load_return of
//                   gvom_trace.hip) and endpoint rule (div_by_res, the literal float64 window test: endpoint_of) give the voxel, ONE
//                   load of the class grid its code.  AL_UNROLL candidates x AL_PTS returns of loads are in flight per lane; an
//                   OUTSIDE pair loads word 0 and ignores it.  Classes are counted by ballots and population counts, summed per
//                   candidate in LDS over the workgroup's waves and added to the product's count columns by int32 atomics (exact,
//                   order-independent).  No early exit; every loop is bounded at launch.
//   k_align_best    the weights: outside = n - the four counted classes, score = sum of weight * count, and the lowest index whose
//                   score is the maximum.  One workgroup.
//
// READ-ONLY on the map.  No scratch.  Numerics as in gvom_trace.hip: -ffp-contract=off, every operation rounded once; the explicit
// fma() calls of div_by_res are its own.
#include "gvom_device.h"
#include "gvom_ray.h"
#include "gvom_classgrid.h"           // the codes, al_spread16 and the field kernels' sizing: shared with k_vatlas_align_field

#define AL_BLOCK 256
#define AL_PTS 4                    // returns per lane of k_align_score
#define AL_UNROLL 2                 // candidates whose loads are in flight together

static_assert(GVOM_ALIGN_PTS_BLOCK == AL_BLOCK * AL_PTS, "points per block");
static_assert(GVOM_ALIGN_CAND_GROUP % AL_UNROLL == 0, "candidate group");

// LDS: three planes of (zc + 2) levels x nq 64-bit words -- [0] occupied in rows y - 1 .. y + 1, [1] occupied in row y, [2] free in row y.
// Level l of a plane is window level z0 - 1 + l.
__global__ __launch_bounds__(AL_BLOCK) void k_align_field(const OccParams P, const int zc, const int nq, const int rw, const int dilate,
                                                          const int32_t *__restrict__ fstate, const uint32_t *__restrict__ ftags,
                                                          uint32_t *__restrict__ grid)
{
    extern __shared__ unsigned long long s_mask[];
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int y = (int)blockIdx.x, z0 = (int)blockIdx.y * zc;
    const int nl = zc + 2, plane = nl * nq;
    for (int it = wave; it < plane; it += AL_BLOCK / WAVE) {
        const int l = it / nq, q = it - l * nq;                     // (wave-uniform)
        const int z = z0 - 1 + l, x = q * 64 + lane;
        unsigned long long around = 0ull, own = 0ull, fre = 0ull;
        if (z >= 0 && z < P.zs && (dilate || (l >= 1 && l <= zc))) {
            const int sz = wrap_add(z, P.om[2], P.zs), sx = wrap_add(x < P.xy ? x : 0, P.om[0], P.xy);
            uint32_t tg[3];
            int32_t st[3];
            bool ok[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {                           // rows y - 1, y, y + 1: three tag and three state loads in flight
                const int yy = y + d - 1;
                ok[d] = yy >= 0 && yy < P.xy && x < P.xy && (d == 1 || dilate);
                const int sy = wrap_add(ok[d] ? yy : 0, P.om[1], P.xy);
                ok[d] = ok[d] && sy >= P.y_lo && sy < P.y_hi;
                const size_t row = (size_t)sy * P.zs + sz;
                tg[d] = ok[d] ? ftags[row * P.nseg + (sx >> 6)] : 0u;
                st[d] = ok[d] ? fstate[row * P.xy + sx] : -1;
            }
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const int32_t s = (ok[d] && tg[d] == P.epoch) ? st[d] : -1;        // a stale tile reads "never observed"
                const unsigned long long o = lanes(s >= 0);
                around |= o;
                if (d == 1) { own = o; fre = lanes(s <= -2); }
            }
        }
        if (lane == 0) { s_mask[it] = around; s_mask[plane + it] = own; s_mask[2 * plane + it] = fre; }
    }
    __syncthreads();
    const int nlev = min(zc, P.zs - z0);
    for (int it = (int)threadIdx.x; it < nlev * nq * 4; it += AL_BLOCK) {
        const int j = it & 3, lq = it >> 2;
        const int l = lq / nq + 1, q = lq - (l - 1) * nq;
        if (q * 4 + j >= rw) continue;
        const unsigned long long own = s_mask[plane + l * nq + q], fre = s_mask[2 * plane + l * nq + q];
        unsigned long long near = 0ull;
        if (dilate) {
            unsigned long long m = 0ull, left = 0ull, right = 0ull;
#pragma unroll
            for (int dl = -1; dl <= 1; ++dl) {
                const unsigned long long *row = s_mask + (l + dl) * nq;
                m |= row[q];
                if (q > 0) left |= row[q - 1];
                if (q + 1 < nq) right |= row[q + 1];
            }
            near = m | (m << 1) | (m >> 1) | (left >> 63) | (right << 63);
        }
        const uint32_t o16 = (uint32_t)(own >> (16 * j)), n16 = (uint32_t)(near >> (16 * j)), f16 = (uint32_t)(fre >> (16 * j));
        // AL_OCC 0, AL_NEAR 1, AL_FREE 2, AL_UNK 3: high bit = neither occupied nor near, low bit = not occupied and (near or not free)
        const uint32_t hi = ~o16 & ~n16, lo = ~o16 & (n16 | ~f16);
        const int z = z0 + l - 1;
        grid[((size_t)z * P.xy + y) * rw + q * 4 + j] = al_spread16(lo) | (al_spread16(hi) << 1);
    }
}

// word of the class grid and the shift of the code in it for the return (x, y, z) under the candidate M; word 0 and inside = false
// for an OUTSIDE pair.  FAST: both resolutions divide by their verified reciprocals (ScanParams::fastdiv == 3, the usual case) -- as a
// template argument, so that the IEEE divides are not compiled in beside them
template <bool FAST>
__device__ __forceinline__ void al_pair(const AlignParams &P, const double (&M)[12], double x, double y, double z, uint32_t &word,
                                        uint32_t &shift, bool &inside)
{
    // load_return (gvom.py:1044-1052): float64, source order, rounded once to the cloud's type
    const float w0 = (float)(((x * M[0] + y * M[1]) + z * M[2]) + M[3]);
    const float w1 = (float)(((x * M[4] + y * M[5]) + z * M[6]) + M[7]);
    const float w2 = (float)(((x * M[8] + y * M[9]) + z * M[10]) + M[11]);
    // endpoint_of (gvom.py:1072-1080): the literal float64 lookup
    const double fx = floor(div_by_res<float>(w0, P.xy_res, P.drcp[0], FAST || (P.fastdiv & 1)) - P.origin[0]);
    const double fy = floor(div_by_res<float>(w1, P.xy_res, P.drcp[0], FAST || (P.fastdiv & 1)) - P.origin[1]);
    const double fz = floor(div_by_res<float>(w2, P.z_res, P.drcp[1], FAST || (P.fastdiv & 2)) - P.origin[2]);
    inside = fx >= 0.0 && fx < (double)P.xy && fy >= 0.0 && fy < (double)P.xy && fz >= 0.0 && fz < (double)P.zs;
    const uint32_t vx = inside ? (uint32_t)(int)fx : 0u, vy = inside ? (uint32_t)(int)fy : 0u, vz = inside ? (uint32_t)(int)fz : 0u;
    word = (vz * (uint32_t)P.xy + vy) * (uint32_t)P.rw + (vx >> 4);
    shift = (vx & 15u) << 1;
}

template <bool FAST>
__global__ __launch_bounds__(AL_BLOCK) void k_align_score(const AlignParams P, const float *__restrict__ cloud,
                                                          const double *__restrict__ tf, const uint32_t *__restrict__ grid,
                                                          int32_t *__restrict__ counts)
{
    __shared__ uint32_t s_cnt[GVOM_ALIGN_CAND_GROUP * 4];
    const int lane = (int)(threadIdx.x & 63u);
    for (int t = (int)threadIdx.x; t < GVOM_ALIGN_CAND_GROUP * 4; t += AL_BLOCK) s_cnt[t] = 0u;
    double px[AL_PTS], py[AL_PTS], pz[AL_PTS];
#pragma unroll
    for (int p = 0; p < AL_PTS; ++p) {                              // a return that does not exist: NaN, OUTSIDE under every candidate, never counted
        const long i = (long)blockIdx.x * GVOM_ALIGN_PTS_BLOCK + p * AL_BLOCK + (long)threadIdx.x;
        const bool live = i < P.n;
        const float *c = cloud + 3 * (live ? i : 0);
        px[p] = live ? (double)c[0] : (double)NAN; py[p] = live ? (double)c[1] : (double)NAN; pz[p] = live ? (double)c[2] : (double)NAN;
    }
    __syncthreads();
    const int k0 = (int)blockIdx.y * GVOM_ALIGN_CAND_GROUP;
    for (int g = 0; g < GVOM_ALIGN_CAND_GROUP; g += AL_UNROLL) {
        uint32_t word[AL_UNROLL][AL_PTS], shift[AL_UNROLL][AL_PTS], code[AL_UNROLL][AL_PTS];
        bool in[AL_UNROLL][AL_PTS];
#pragma unroll
        for (int u = 0; u < AL_UNROLL; ++u) {
            const int k = min(k0 + g + u, P.K - 1);                 // (wave-uniform; a candidate beyond K is computed and dropped)
            double M[12];
#pragma unroll
            for (int e = 0; e < 12; ++e) M[e] = tf[(size_t)k * 12 + e];
#pragma unroll
            for (int p = 0; p < AL_PTS; ++p) al_pair<FAST>(P, M, px[p], py[p], pz[p], word[u][p], shift[u][p], in[u][p]);
        }
#pragma unroll
        for (int u = 0; u < AL_UNROLL; ++u)
#pragma unroll
            for (int p = 0; p < AL_PTS; ++p) code[u][p] = grid[word[u][p]];
#pragma unroll
        for (int u = 0; u < AL_UNROLL; ++u) {
            uint32_t c0 = 0u, c1 = 0u, c2 = 0u, c3 = 0u;
#pragma unroll
            for (int p = 0; p < AL_PTS; ++p) {
                const uint32_t c = (code[u][p] >> shift[u][p]) & 3u;
                c0 += (uint32_t)__builtin_popcountll(lanes(in[u][p] && c == AL_OCC));
                c1 += (uint32_t)__builtin_popcountll(lanes(in[u][p] && c == AL_NEAR));
                c2 += (uint32_t)__builtin_popcountll(lanes(in[u][p] && c == AL_FREE));
                c3 += (uint32_t)__builtin_popcountll(lanes(in[u][p] && c == AL_UNK));
            }
            if (k0 + g + u < P.K && lane < 4) {
                const uint32_t v = lane == 0 ? c0 : (lane == 1 ? c1 : (lane == 2 ? c2 : c3));
                if (v) atomicAdd(&s_cnt[(g + u) * 4 + lane], v);
            }
        }
    }
    __syncthreads();
    for (int t = (int)threadIdx.x; t < GVOM_ALIGN_CAND_GROUP * 4; t += AL_BLOCK) {
        const int k = k0 + (t >> 2);
        const uint32_t v = s_cnt[t];
        if (k < P.K && v) atomicAdd(&counts[(size_t)k * 6 + 1 + (t & 3)], (int32_t)v);
    }
}

// counts [K][6]: columns 1 .. 4 hold the counted classes; writes columns 0 (score) and 5 (outside) and best[4]
__global__ __launch_bounds__(1024) void k_align_best(const AlignParams P, int32_t *__restrict__ counts, int32_t *__restrict__ best)
{
    __shared__ long long s_key[16];
    long long key = LLONG_MIN;                                      // (score << 32) | (2^32 - 1 - k): the maximum is the lowest k of the best score
    for (int k = (int)threadIdx.x; k < P.K; k += (int)blockDim.x) {
        int32_t *r = counts + (size_t)k * 6;
        const int32_t occ = r[1], near = r[2], fre = r[3], unk = r[4];
        const int32_t out = (int32_t)P.n - occ - near - fre - unk;
        const int32_t score = P.w[0] * occ + P.w[1] * near + P.w[2] * fre + P.w[3] * unk + P.w[4] * out;    // |score| <= 1024 * 2^20
        r[0] = score; r[5] = out;
        const long long kk = ((long long)score << 32) | (long long)(0xffffffffu - (uint32_t)k);
        key = kk > key ? kk : key;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) { const long long o = __shfl_xor(key, s); key = o > key ? o : key; }
    if ((threadIdx.x & 63u) == 0u) s_key[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (unsigned w = 1; w < (blockDim.x >> 6); ++w) key = s_key[w] > key ? s_key[w] : key;
        best[0] = (int32_t)(0xffffffffu - (uint32_t)(key & 0xffffffffll));
        best[1] = (int32_t)(key >> 32);
        best[2] = (int32_t)P.n;
        best[3] = P.K;
    }
}

// levels per workgroup of k_align_field: what fits the LDS budget (three planes of (zc + 2) * nq 64-bit words), at most AL_ZC_MAX
static int al_zc(int xy, int zs)
{
    const int nq = (xy + 63) / 64;
    int zc = AL_LDS_BUDGET / (24 * nq) - 2;
    zc = zc > AL_ZC_MAX ? AL_ZC_MAX : zc;
    return zc > zs ? zs : zc;
}

size_t gvom_align_grid_bytes(int xy, int zs)
{
    return (size_t)zs * (size_t)xy * (size_t)((xy + 15) / 16) * 4;
}

static bool al_ok(const AlignParams &P)
{
    if (P.n < 1 || P.n > GVOM_ALIGN_MAX_POINTS || P.K < 1 || P.K > GVOM_ALIGN_MAX_CANDIDATES || P.xy < 1 || P.zs < 1 ||
        P.rw != (P.xy + 15) / 16 || (P.dilate != 0 && P.dilate != 1))
        return false;
    return gvom_align_grid_bytes(P.xy, P.zs) / 4 <= 0xffffffffull;                                // (word indices are 32 bits)
}

hipError_t gvom_launch_align(hipStream_t s, const OccParams &F, const AlignParams &P, const int32_t *fstate, const uint32_t *ftags,
                             const float *cloud, const double *tf, uint32_t *grid, int32_t *counts, int32_t *best)
{
    if (!al_ok(P) || P.xy != F.xy || P.zs != F.zs) return hipErrorInvalidValue;
    const int zc = al_zc(P.xy, P.zs), nq = (P.xy + 63) / 64;
    if (zc < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_align_field, dim3((unsigned)P.xy, (unsigned)((P.zs + zc - 1) / zc)), dim3(AL_BLOCK), (size_t)3 * (zc + 2) * nq * 8, s,
                       F, zc, nq, P.rw, P.dilate, fstate, ftags, grid);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : gvom_launch_align_grid(s, P, cloud, tf, grid, counts, best);
}

hipError_t gvom_launch_align_grid(hipStream_t s, const AlignParams &P, const float *cloud, const double *tf, const uint32_t *grid,
                                  int32_t *counts, int32_t *best)
{
    if (!al_ok(P) || !grid) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)P.K * 24, s);
    if (e != hipSuccess) return e;
    const dim3 sg((unsigned)((P.n + GVOM_ALIGN_PTS_BLOCK - 1) / GVOM_ALIGN_PTS_BLOCK), (unsigned)((P.K + GVOM_ALIGN_CAND_GROUP - 1) / GVOM_ALIGN_CAND_GROUP));
    if ((P.fastdiv & 3) == 3) hipLaunchKernelGGL(k_align_score<true>, sg, dim3(AL_BLOCK), 0, s, P, cloud, tf, grid, counts);
    else hipLaunchKernelGGL(k_align_score<false>, sg, dim3(AL_BLOCK), 0, s, P, cloud, tf, grid, counts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_align_best, dim3(1), dim3(1024), 0, s, P, counts, best);
    return hipGetLastError();
}
