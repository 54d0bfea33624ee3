// gvom_clearance.hip -- device kernels of the obstacle clearance map (gvom_clearance): the exact squared Euclidean distance, in
// cells, from every cell of a 2-D map to the nearest hard-obstacle cell, and that distance in metres.
//   k_clearance_rows   along x (the contiguous axis of the [y][x] maps): g[y][x] = cells to the nearest obstacle of the SAME row
//   k_clearance_cols   along y: d2[y][x] = min over rows j of g[j][x]^2 + (y - j)^2, then the two outputs
// The transform is separable because the squared distance is: min over (ox, oy) of (x - ox)^2 + (y - oy)^2 is the minimum over
// rows oy of (the smallest (x - ox)^2 of that row) + (y - oy)^2, and the first term is g[oy][x]^2.  Everything is integer
// arithmetic below 2^31 (xy <= 4096: at most 2 * 4095^2), so the result is exact; the metres are one float64 square root and one
// float64 multiply rounded once to float32 (the build has no contraction and no fast math).
#include "gvom_device.h"
#include "gvom_clearance_rows.h"

// the row pass over a [y][x] map pair (gvom_clearance_rows.h has the body)
__global__ __launch_bounds__(256) void k_clearance_rows(const int32_t *__restrict__ pos, const int32_t *__restrict__ neg,
                                                        const double thr, const int xy, const int gp, uint16_t *__restrict__ g)
{
    __shared__ unsigned long long s_mask[64];
    const int y = blockIdx.x;
    clearance_row([&](int x) {
        bool ob = (double)pos[(size_t)y * xy + x] > thr;
        if (neg) ob = ob || neg[(size_t)y * xy + x] > 0;
        return ob;
    }, xy, gp, g + (size_t)y * gp, s_mask);
}

// One workgroup per strip of W = 2^lgw columns and T output rows.  The rows of g the strip can need -- all of them, or the
// output rows and `halo` rows either side when the squared distance is capped (rows further away are beyond the cap whatever
// they hold) -- go to LDS as W uint16 per row: a wave reads 64 consecutive uint16 (W = 64) or 64 / W runs of neighbouring
// rows, one bank per dword either way.  A lane walks outwards from its own row, one row above and one below per step, and stops
// once the vertical term alone is no better than what it has (or than the cap): exact, and short wherever obstacles are near.
// dy^2 is carried along by addition; no division, no multiply but g * g.  Both outputs are stored as runs of W dwords.
__global__ __launch_bounds__(256) void k_clearance_cols(const uint32_t *__restrict__ g32, const int gp, const int xy, const int lgw,
                                                        const int T, const int halo, const uint32_t lim, const double res,
                                                        float *__restrict__ out_dist, int32_t *__restrict__ out_d2)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_g[];
    const int W = 1 << lgw, hw = W >> 1;
    const int x0 = blockIdx.x << lgw;
    const int y0 = blockIdx.y * T, y1 = min(y0 + T, xy);
    const int r0 = halo < 0 ? 0 : max(0, y0 - halo), r1 = halo < 0 ? xy : min(xy, y1 + halo);
    const int total = (r1 - r0) * hw;
    const uint32_t *src = g32 + (((size_t)r0 * gp + x0) >> 1);
    for (int i = threadIdx.x; i < total; i += 256) s_g[i] = src[(size_t)(i >> (lgw - 1)) * (gp >> 1) + (i & (hw - 1))];
    __syncthreads();
    const int cx = threadIdx.x & (W - 1), x = x0 + cx;
    if (x >= xy) return;
    const uint16_t *col = (const uint16_t *)s_g + cx;
    for (int y = y0 + (threadIdx.x >> lgw); y < y1; y += 256 >> lgw) {
        const uint32_t g0 = col[(y - r0) << lgw];
        uint32_t best = min(lim, g0 * g0);
        const int dmax = max(y - r0, r1 - 1 - y);
        uint32_t dy2 = 1;
        for (int dy = 1; dy <= dmax && dy2 < best; ++dy) {
            const int ju = y - dy, jd = y + dy;
            const uint32_t gu = ju >= r0 ? col[(ju - r0) << lgw] : GVOM_CLR_NONE;
            const uint32_t gd = jd < r1 ? col[(jd - r0) << lgw] : GVOM_CLR_NONE;
            best = min(best, min(gu * gu, gd * gd) + dy2);
            dy2 += 2u * (uint32_t)dy + 1u;
        }
        const size_t o = (size_t)y * xy + x;
        const bool far_ = best >= lim;
        out_d2[o] = far_ ? INT32_MAX : (int32_t)best;              // (GVOM_CLEARANCE_FAR)
        out_dist[o] = far_ ? __builtin_inff() : (float)(sqrt((double)best) * res);
    }
}

size_t gvom_clearance_scratch_bytes(int xy) { return (size_t)((xy + 63) & ~63) * (size_t)xy * sizeof(uint16_t); }

hipError_t gvom_launch_clearance_cols(hipStream_t s, int xy, double res, int32_t max_cells2, const uint16_t *g, float *out_dist,
                                      int32_t *out_d2, int shape[4])
{
    if (xy <= 0 || xy > GVOM_CLEARANCE_MAX_XY) return hipErrorInvalidValue;
    const int gp = (xy + 63) & ~63;
    const bool capped = max_cells2 > 0 && max_cells2 < INT32_MAX;
    const uint32_t lim = capped ? (uint32_t)max_cells2 + 1u : (uint32_t)INT32_MAX;
    int halo = -1;
    if (capped) {                                                // floor(sqrt(cap)), exactly
        long long r = (long long)sqrt((double)max_cells2);
        while (r * r > max_cells2) --r;
        while ((r + 1) * (r + 1) <= max_cells2) ++r;
        if (r < xy) halo = (int)r;
    }
    // shape: T output rows per workgroup (a sixteenth of the map: the strip is loaded 16 times over all), columns per strip
    // 64 -> 16 until there are workgroups for every CU, then down to what 64 KB of LDS hold
    const int T = max(16, (xy / 16 + 15) & ~15);
    const int ytiles = (xy + T - 1) / T;
    const int nrows = halo < 0 ? xy : min(xy, T + 2 * halo);
    int lgw = 6;
    while (lgw > 4 && ((xy + (1 << lgw) - 1) >> lgw) * ytiles < 256) --lgw;
    while (lgw > 3 && ((size_t)nrows << lgw) * 2 > 65536) --lgw;
    const size_t lds = ((size_t)nrows << lgw) * 2;
    if (lds > 65536) return hipErrorInvalidValue;
    if (shape) { shape[0] = lgw; shape[1] = T; shape[2] = (int)lds; shape[3] = gp >> 6; }
    hipLaunchKernelGGL(k_clearance_cols, dim3((xy + (1 << lgw) - 1) >> lgw, ytiles), dim3(256), lds, s, (const uint32_t *)g, gp, xy, lgw,
                       T, halo, lim, res, out_dist, out_d2);
    return hipGetLastError();
}

hipError_t gvom_launch_clearance(hipStream_t s, int xy, double res, const int32_t *pos, const int32_t *neg, double thr,
                                 int32_t max_cells2, uint16_t *g, float *out_dist, int32_t *out_d2, int shape[4])
{
    if (xy <= 0 || xy > GVOM_CLEARANCE_MAX_XY) return hipErrorInvalidValue;
    const int gp = (xy + 63) & ~63;
    hipLaunchKernelGGL(k_clearance_rows, dim3(xy), dim3(256), 0, s, pos, neg, thr, xy, gp, g);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return gvom_launch_clearance_cols(s, xy, res, max_cells2, g, out_dist, out_d2, shape);
}
