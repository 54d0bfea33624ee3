// gvom_voxel_distance.hip -- voxel distance fields (include/gvom_hip.h "voxel distance field" defines the result): the truncated, exact,
// anisotropic Euclidean distance from every voxel of a window-sized box to the nearest source voxel of the voxel atlas, and the gather
// that samples such a field at world points (gfx950, wave64).  The atlas's storage is gvom_voxel_atlas.hip's (pairs {observed, occupied}
// of 64 consecutive world x); the box arrives as that unit's VAtlasBox, relative to the extent, with its storage phase.
//
// THE GROWN BOX.  A source beyond the box decides distances inside it, so the first two passes run on the box grown by the halo in y and
// z -- hby rows below, nyg rows in all; hbz levels below, nzg levels in all -- clipped to where a source can lie (the host: the extent,
// one row further under GVOM_DISTANCE_UNKNOWN_BLOCKS, never less than the box).  Grown row j is box row j - hby, grown level l box
// level l - hbz.  x needs no halo: the row pass looks across the box's faces in the bit planes themselves.
//
//   k_vdist_rows    x pass, integer, on the bit planes: a wave takes 64 box columns of one grown (row, level); the 64-bit source mask of
//                   its own columns and of the kx words on either side are assembled from pairs as k_vatlas_box assembles its rows (the
//                   addresses are wave-uniform), and a lane's nearest source at or left of / right of it is clz / ffs of the masks:
//                   no loop over voxels.  Writes g = |dx| as uint16 (VD_NO16: none within kx words), [level][row][x], x padded to words
//   k_vdist_cols    y pass, integer: n_min = min over dy of g^2 + dy^2 by k_clearance_cols' outward walk with its exact early exit
//                   (dy^2 >= best), capped at the halo.  Lanes along x: every load and store is a run of consecutive elements.  Writes
//                   uint32 [level][y][x] for the box's own rows (VD_NO32: no source in reach)
//   k_vdist_levels  z pass, float64: a workgroup takes one box row y and TX box columns; the columns' n_min over every grown level go
//                   to LDS TRANSPOSED ([x][level], the one transposition between the x-major bits and the z-contiguous output), then a
//                   thread per (x, z) walks outward over fl64(a * n_min(dz)) + fl64(b * dz^2) until fl64(b * dz^2) alone is no smaller
//                   than the best or exceeds cap2 -- exact: the sum is monotone in both terms -- and stores (float)sqrt along z.
//                   Counts by ballots, summed over the workgroup in LDS: one integer atomic per counter and workgroup
//   k_vdist_sample  one gather per lane: the voxel of a point by float64 division and floor, the field's value there or NaN; counts by ballots
//
// No scratch, no persistent kernel, no wait on another workgroup, every loop bounded at launch, no atomics on the field.  LDS: only
// k_vdist_levels', at most VD_LDS_BYTES.  Numerics: -ffp-contract=off, IEEE division / sqrt, every operation rounded once; the minimum
// of a set of doubles does not depend on the order they are met in.
#include "gvom_device.h"
#include <algorithm>

#define VD_BLOCK 256
#define VD_WAVES (VD_BLOCK / WAVE)
#define VD_NO16 0xffffu
#define VD_NO32 0xffffffffu
#define VD_TX 32                                          // box columns per k_vdist_levels workgroup: 128-byte runs of the y pass's output
#define VD_LDS_BYTES (48 * 1024)

typedef unsigned long long v2ull __attribute__((ext_vector_type(2)));      // one pair: .x observed, .y occupied

// ---- the source mask of 64 box columns (the pair arithmetic of gvom_voxel_atlas.hip: va_pair, va_box_inside, va_box_segment) ---------------
__device__ __forceinline__ unsigned long long vd_below(uint32_t n) { return n >= 64u ? ~0ull : (1ull << n) - 1ull; }       // bits 0 .. n - 1

// The sources among the box columns x0 .. x0 + 63 (x0 a multiple of 64, any sign) of box row y and box level z, both possibly outside the
// box: two storage pairs shifted together.  A voxel outside the extent is NEVER: a source under `unknown`, none otherwise.
__device__ __forceinline__ unsigned long long vd_sources(const VAtlas &V, const VAtlasBox &B, int unknown, int x0, int y, int z)
{
    const uint32_t uA = (uint32_t)V.A, uZ = (uint32_t)V.Z;
    const uint32_t ey = (uint32_t)(B.ry + y), ez = (uint32_t)(B.rz + z);                   // (|r| <= 2^30, |x0|, |y|, |z| < 2^17: no overflow)
    const int e0 = B.rx + x0;                                                              // extent voxel of bit 0
    const int lo_b = e0 < 0 ? -e0 : 0, hi_b = min(64, V.A - e0);                           // bits [lo_b, hi_b) lie inside the extent
    unsigned long long obs = 0ull, occ = 0ull;
    if (ey < uA && ez < uZ && lo_b < hi_b) {
        const unsigned long long valid = vd_below((uint32_t)hi_b) & ~vd_below((uint32_t)lo_b);
        const uint32_t sy = ((uint32_t)B.py + (uint32_t)y) & (uA - 1u), sz = ((uint32_t)B.pz + (uint32_t)z) & (uZ - 1u);
        const uint32_t sx = ((uint32_t)B.px + (uint32_t)x0) & (uA - 1u), sh = sx & 63u;
        const v2ull *const pairs = (const v2ull *)V.pairs;
        const v2ull lo = pairs[((((size_t)sy << V.lgZ) | sz) << V.lgP) | (sx >> 6)];
        obs = lo.x >> sh; occ = lo.y >> sh;
        if (sh) {
            const v2ull hi = pairs[((((size_t)sy << V.lgZ) | sz) << V.lgP) | (((sx + 64u) & (uA - 1u)) >> 6)];
            obs |= hi.x << (64u - sh); occ |= hi.y << (64u - sh);
        }
        obs &= valid; occ &= valid;
    }
    return unknown ? (occ | ~obs) : occ;
}

// ---- x pass -------------------------------------------------------------------------------------------------------------------------------
// Wave gw = (level l * nyg + row j) * nw + word q; lane = the column's bit.  After the words at distance < k have been examined, a source
// in word q - k or q + k lies at least 64 (k - 1) + 1 columns away: the search ends once no lane is further than that from its best, at
// the latest after kx words.
__global__ __launch_bounds__(VD_BLOCK) void k_vdist_rows(const VAtlas V, const VDistFrame F, uint16_t *__restrict__ g)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gw = __builtin_amdgcn_readfirstlane(blockIdx.x * VD_WAVES + (threadIdx.x >> 6));
    const uint32_t nw = (uint32_t)F.nw, rows = (uint32_t)F.nyg * (uint32_t)F.nzg;
    const uint32_t row = gw / nw, q = gw - row * nw;
    if (row >= rows) return;                              // (the whole wave: the last workgroup's spare waves)
    const uint32_t l = row / (uint32_t)F.nyg, j = row - l * (uint32_t)F.nyg;
    const int y = (int)j - F.hby, z = (int)l - F.hbz;
    const unsigned long long own = vd_sources(V, F.B, F.unknown, (int)q * 64, y, z);
    uint32_t d = VD_NO16;
    const unsigned long long left = own & vd_below(lane + 1u), right = own >> lane;        // sources at or left of / at or right of the lane
    if (left) d = lane - (63u - (uint32_t)__builtin_clzll(left));
    if (right) d = min(d, (uint32_t)__builtin_ctzll(right));
    for (int k = 1; k <= F.kx; ++k) {
        if (lanes(d > 64u * (uint32_t)(k - 1)) == 0ull) break;                             // (wave-uniform)
        const unsigned long long wl = vd_sources(V, F.B, F.unknown, ((int)q - k) * 64, y, z);
        const unsigned long long wr = vd_sources(V, F.B, F.unknown, ((int)q + k) * 64, y, z);
        if (wl) d = min(d, lane + 64u * (uint32_t)k - (63u - (uint32_t)__builtin_clzll(wl)));
        if (wr) d = min(d, 64u * (uint32_t)k - lane + (uint32_t)__builtin_ctzll(wr));
    }
    g[((size_t)row * nw + q) * 64u + lane] = (uint16_t)min(d, VD_NO16);
}

// ---- y pass -------------------------------------------------------------------------------------------------------------------------------
// Wave gw = (level l * n + box row y) * nw + word q.  The walk visits grown rows j0 - k and j0 + k, j0 = y + hby, for k = 1 .. min(hxy,
// the further end of the grown box); a lane is done once k^2 >= its best, the wave once every lane is.
__global__ __launch_bounds__(VD_BLOCK) void k_vdist_cols(const VDistFrame F, const uint16_t *__restrict__ g, uint32_t *__restrict__ nmin)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gw = __builtin_amdgcn_readfirstlane(blockIdx.x * VD_WAVES + (threadIdx.x >> 6));
    const uint32_t nw = (uint32_t)F.nw, n = (uint32_t)F.B.n, rows = n * (uint32_t)F.nzg;
    const uint32_t row = gw / nw, q = gw - row * nw;
    if (row >= rows) return;                              // (the whole wave)
    const uint32_t l = row / n, y = row - l * n;
    const uint32_t x = q * 64u + lane, pitch = nw * 64u;
    const int j0 = (int)y + F.hby;
    const uint16_t *const col = g + (size_t)l * (uint32_t)F.nyg * pitch + x;               // this lane's column of level l
    const uint32_t g0 = col[(size_t)j0 * pitch];
    uint32_t best = g0 == VD_NO16 ? VD_NO32 : g0 * g0;    // (g <= 32895: g^2 + k^2 < 2^32)
    const int kmax = min(F.hxy, max(j0, F.nyg - 1 - j0));
    for (int k = 1; k <= kmax; ++k) {
        const uint32_t k2 = (uint32_t)k * (uint32_t)k;
        if (lanes(k2 < best) == 0ull) break;                                               // (wave-uniform) the exact early exit
        if (j0 - k >= 0) {
            const uint32_t v = col[(size_t)(j0 - k) * pitch];
            if (v != VD_NO16) best = min(best, v * v + k2);
        }
        if (j0 + k < F.nyg) {
            const uint32_t v = col[(size_t)(j0 + k) * pitch];
            if (v != VD_NO16) best = min(best, v * v + k2);
        }
    }
    nmin[(size_t)row * pitch + x] = best;
}

// ---- z pass -------------------------------------------------------------------------------------------------------------------------------
// blockIdx.x = the tile of tx box columns, blockIdx.y = the box row.  LDS: s_n[xi * S + l], S = nzg | 1 (odd: the transposing stores of
// one level go to distinct banks), then the workgroup's counts.  Work item it = xi * zs + z: consecutive lanes store consecutive floats.
__global__ __launch_bounds__(VD_BLOCK) void k_vdist_levels(const VDistFrame F, const int tx, const uint32_t *__restrict__ nmin,
                                                           float *__restrict__ out, int32_t *__restrict__ counts)
{
    extern __shared__ uint32_t s_n[];
    __shared__ int32_t s_c[VD_WAVES][2];
    const uint32_t n = (uint32_t)F.B.n, zs = (uint32_t)F.B.zs, nzg = (uint32_t)F.nzg, S = nzg | 1u, pitch = (uint32_t)F.nw * 64u;
    const uint32_t x0 = blockIdx.x * (uint32_t)tx, y = blockIdx.y, utx = (uint32_t)tx;
    for (uint32_t it = threadIdx.x; it < nzg * utx; it += VD_BLOCK) {
        const uint32_t l = it / utx, xi = it - l * utx;
        s_n[xi * S + l] = x0 + xi < n ? nmin[((size_t)l * n + y) * pitch + x0 + xi] : VD_NO32;
    }
    __syncthreads();
    int32_t c_zero = 0, c_fin = 0;
    const uint32_t items = utx * zs;
    for (uint32_t base = 0; base < items; base += VD_BLOCK) {                              // (uniform: the ballots want every lane)
        const uint32_t it = base + threadIdx.x;
        const uint32_t xi = it / zs, z = it - xi * zs;
        const bool live = it < items && x0 + xi < n;
        const uint32_t *const col = s_n + (live ? xi : 0u) * S;
        const int j0 = (int)(live ? z : 0u) + F.hbz;
        double best = INFINITY;
        const int kmax = max(j0, (int)nzg - 1 - j0);
        bool run = live;
        for (int k = 0; k <= kmax; ++k) {
            const double tz = F.b * (double)((int64_t)k * k);
            run = run && tz < best && tz <= F.cap2;                                        // fl64(b dz^2) alone decides: the sum is monotone
            if (lanes(run) == 0ull) break;
            if (run) {
                if (j0 - k >= 0) {
                    const uint32_t v = col[j0 - k];
                    if (v != VD_NO32) { const double t = F.a * (double)v; best = fmin(best, t + tz); }
                }
                if (k > 0 && j0 + k < (int)nzg) {
                    const uint32_t v = col[j0 + k];
                    if (v != VD_NO32) { const double t = F.a * (double)v; best = fmin(best, t + tz); }
                }
            }
        }
        const bool fin = live && best <= F.cap2;
        c_zero += __builtin_popcountll(lanes(fin && best == 0.0));
        c_fin += __builtin_popcountll(lanes(fin));
        if (live) out[((size_t)(x0 + xi) * n + y) * zs + z] = fin ? (float)sqrt(best) : INFINITY;
    }
    if ((threadIdx.x & 63u) == 0u) { s_c[threadIdx.x >> 6][0] = c_zero; s_c[threadIdx.x >> 6][1] = c_fin; }
    __syncthreads();
    if (threadIdx.x < 2u) {
        int32_t t = 0;
#pragma unroll
        for (int w = 0; w < VD_WAVES; ++w) t += s_c[w][threadIdx.x];
        if (t) atomicAdd(counts + threadIdx.x, t);
    }
    if (blockIdx.x == 0u && blockIdx.y == 0u && threadIdx.x == 0u) { counts[2] = F.B.outside; counts[3] = F.B.seq; }
}

// ---- sample -------------------------------------------------------------------------------------------------------------------------------
struct __attribute__((aligned(4))) VdFloat3 { float x, y, z; };

// field: float32 [n][n][zs] of the box whose corner is world voxel `origin`.  counts += {inside the box, of those finite, of those 0}
__global__ __launch_bounds__(VD_BLOCK) void k_vdist_sample(const VDistSample Q, const VdFloat3 *__restrict__ pts, const float *__restrict__ field,
                                                           float *__restrict__ out, int32_t *__restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * VD_BLOCK + threadIdx.x;
    const bool live = i < Q.npts;
    VdFloat3 p = {NAN, NAN, NAN};
    if (live) p = pts[i];
    // floor((double)p / resolution) - origin: NaN and +-inf fail every comparison
    const double fx = floor((double)p.x / Q.xy_res) - Q.origin[0], fy = floor((double)p.y / Q.xy_res) - Q.origin[1];
    const double fz = floor((double)p.z / Q.z_res) - Q.origin[2];
    const bool in = live && fx >= 0.0 && fx < (double)Q.n && fy >= 0.0 && fy < (double)Q.n && fz >= 0.0 && fz < (double)Q.zs;
    float v = NAN;
    if (in) v = field[((size_t)(int)fx * (uint32_t)Q.n + (uint32_t)(int)fy) * (uint32_t)Q.zs + (uint32_t)(int)fz];
    if (live) out[i] = v;
    const uint32_t c_in = (uint32_t)__builtin_popcountll(lanes(in)), c_fin = (uint32_t)__builtin_popcountll(lanes(in && v < INFINITY));
    const uint32_t c_zero = (uint32_t)__builtin_popcountll(lanes(in && v == 0.0f));
    if ((threadIdx.x & 63u) == 0u) {
        if (c_in) atomicAdd(counts, (int32_t)c_in);
        if (c_fin) atomicAdd(counts + 1, (int32_t)c_fin);
        if (c_zero) atomicAdd(counts + 2, (int32_t)c_zero);
    }
    if (i == 0) counts[3] = (int32_t)Q.npts;
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------------
size_t gvom_vdist_rows_bytes(const VDistFrame &F) { return (size_t)F.nzg * (size_t)F.nyg * (size_t)F.nw * 64 * 2; }
size_t gvom_vdist_cols_bytes(const VDistFrame &F) { return (size_t)F.nzg * (size_t)F.B.n * (size_t)F.nw * 64 * 4; }

// work: gvom_vdist_rows_bytes(F), 256-byte aligned, then gvom_vdist_cols_bytes(F).  counts [4] must be zero.
hipError_t gvom_launch_vdist_field(hipStream_t s, const VAtlas &V, const VDistFrame &F, void *work, float *out, int32_t *counts)
{
    const VAtlasBox &B = F.B;
    const int lim = 1 << 30;
    if (!V.pairs || V.A < GVOM_VATLAS_MIN_CELLS || V.A > GVOM_VATLAS_MAX_CELLS || (V.A & (V.A - 1)) || V.Z < 1 || V.Z > V.A || (V.Z & (V.Z - 1)) ||
        (1 << V.lgZ) != V.Z || (64 << V.lgP) != V.A)
        return hipErrorInvalidValue;
    if (B.n < 1 || B.n > GVOM_VATLAS_MAX_CELLS || B.zs < 1 || B.zs > GVOM_VATLAS_MAX_CELLS || !work || !out || !counts) return hipErrorInvalidValue;
    if (B.px < 0 || B.px >= V.A || B.py < 0 || B.py >= V.A || B.pz < 0 || B.pz >= V.Z) return hipErrorInvalidValue;
    if (B.rx < -lim || B.rx > lim || B.ry < -lim || B.ry > lim || B.rz < -lim || B.rz > lim) return hipErrorInvalidValue;
    if (F.nw != (B.n + 63) / 64 || F.hxy < 0 || F.hxy > GVOM_VDIST_MAX_HALO || F.kx < 0 || F.kx > GVOM_VDIST_MAX_HALO / 64 + 2) return hipErrorInvalidValue;
    if (F.hby < 0 || F.hby > GVOM_VDIST_MAX_HALO || F.nyg < F.hby + B.n || F.nyg > F.hby + B.n + GVOM_VDIST_MAX_HALO) return hipErrorInvalidValue;
    if (F.hbz < 0 || F.hbz > GVOM_VDIST_MAX_HALO || F.nzg < F.hbz + B.zs || F.nzg > F.hbz + B.zs + GVOM_VDIST_MAX_HALO) return hipErrorInvalidValue;
    if (!(F.a > 0.0) || !(F.b > 0.0) || !(F.cap2 > 0.0)) return hipErrorInvalidValue;
    const size_t S = (size_t)(F.nzg | 1);
    if (S * 4 > VD_LDS_BYTES) return hipErrorInvalidValue;
    const uint64_t w_rows = (uint64_t)F.nzg * (uint64_t)F.nyg * (uint64_t)F.nw, w_cols = (uint64_t)F.nzg * (uint64_t)B.n * (uint64_t)F.nw;
    if (w_rows >= ((uint64_t)1 << 31) || w_cols >= ((uint64_t)1 << 31)) return hipErrorInvalidValue;
    uint16_t *const g = (uint16_t *)work;
    uint32_t *const nmin = (uint32_t *)((char *)work + ((gvom_vdist_rows_bytes(F) + 255) & ~(size_t)255));
    hipLaunchKernelGGL(k_vdist_rows, dim3((unsigned)((w_rows + VD_WAVES - 1) / VD_WAVES)), dim3(VD_BLOCK), 0, s, V, F, g);
    hipLaunchKernelGGL(k_vdist_cols, dim3((unsigned)((w_cols + VD_WAVES - 1) / VD_WAVES)), dim3(VD_BLOCK), 0, s, F, g, nmin);
    const int tx = (int)std::max<size_t>(1, std::min<size_t>(VD_TX, VD_LDS_BYTES / (S * 4)));
    hipLaunchKernelGGL(k_vdist_levels, dim3((unsigned)((B.n + tx - 1) / tx), (unsigned)B.n), dim3(VD_BLOCK), (size_t)tx * S * 4, s, F, tx, nmin, out, counts);
    return hipGetLastError();
}

// counts [4] must be zero
hipError_t gvom_launch_vdist_sample(hipStream_t s, const VDistSample &Q, const float *pts, const float *field, float *out, int32_t *counts)
{
    if (Q.npts < 1 || Q.npts > ((int64_t)1 << 26) || Q.n < 1 || Q.zs < 1 || !(Q.xy_res > 0.0) || !(Q.z_res > 0.0) || !pts || !field || !out || !counts)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_vdist_sample, dim3((unsigned)((Q.npts + VD_BLOCK - 1) / VD_BLOCK)), dim3(VD_BLOCK), 0, s, Q, (const VdFloat3 *)pts, field, out, counts);
    return hipGetLastError();
}
