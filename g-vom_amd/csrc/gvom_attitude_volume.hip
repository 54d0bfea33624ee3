// gvom_attitude_volume.hip -- attitude volumes (gfx950, wave64): how the vehicle would sit on the ground at EVERY state (cell centre,
// heading) of the window -- the status and the tilt of "terrain attitude scoring" as two uint8 volumes [h][y][x] --, and the kernel
// that takes such a volume into a pose field's cost volume (include/gvom_hip.h "attitude volumes" defines the result).
//
//   k_volume_attitude_table  what depends on (heading, footprint cell) only, once per footprint table and chassis: U = u - am and V = v
//                            of every footprint cell (the header's du, dv, u, v with fx = fy = 0.5, the same IEEE operations in the
//                            same order), and per heading the four wheels' cell offsets floor(0.5 + w / res) and the footprint's box.
//   k_volume_attitude        k_cspace's shape: blockIdx.y is the heading, the lanes run over consecutive cells of a row.  The wheel
//                            offsets, the footprint list and the (U, V) table are wave-uniform and come through scalar loads; a lane
//                            loads its four wheel heights (gvom_rollouts.h at_state_wheels, at_stance: k_attitude's text) and tests the footprint's box against the window once, then per footprint
//                            cell ONE coalesced 8-byte ground height at (a uniform address) + (its own cell), AV_DEPTH of them in
//                            flight, and keeps the least of ((z0 + sp*U) + sr*V + belly_height) - g.  A wave ends in at_tally: one ballot
//                            and one population count per status, at most six int32 atomics per wave, integer sums.
//   k_cspace_attitude        elementwise over a pose cost volume: C' = 0 where C == 0 or the state's status is one of block_mask's,
//                            min(65535, C + tilt_weight * tilt) elsewhere.
//
// READ-ONLY on the ground map.  No load without its bounds test in front of it: a wheel outside the window reads nothing, a state
// whose wheels stand outside the window or on unknown ground reads no footprint cell.  No scratch, no LDS, no wait on another
// workgroup; every loop is bounded at launch (<= 16384 cells per heading).  Every float64 operation is one IEEE operation in the
// header's order (-ffp-contract=off): the result is exact.
#include "gvom_rollouts.h"                                  // (the status words, the wheels, the stance and the census: AT_*, at_*)

#define AV_DEPTH 4          // footprint cells per lane whose loads are in flight together
#define AV_FAR (1 << 20)    // a wheel offset that lies outside every window (xy <= 4096)

// floor(0.5 + w / res), +-AV_FAR where that is no cell of any window
__device__ __forceinline__ int av_wheel_offset(double w, double res)
{
    const double q = 0.5 + w / res;
    if (!(fabs(q) < (double)AV_FAR)) return q < 0.0 ? -AV_FAR : AV_FAR;
    return (int)floor(q);
}

__global__ __launch_bounds__(256) void k_volume_attitude_table(const int H, const int total, const double res, const double axle_mid,
                                                               const int32_t *__restrict__ fstart, const uint32_t *__restrict__ foffs,
                                                               const double *__restrict__ wheels, const double *__restrict__ cos_sin,
                                                               double2 *__restrict__ uv, int32_t *__restrict__ wcell)
{
    const int m = (int)(blockIdx.x * 256 + threadIdx.x);
    if (m < 8 * H) wcell[(m >> 3) * 12 + (m & 7)] = av_wheel_offset(wheels[m], res);   // [H][12]: 4 x (dx, dy) like the wheel table, then the box
    if (m < H) {                                                          // the footprint's box: the least and the largest dx and dy of heading m
        int lo_x = INT_MAX, hi_x = INT_MIN, lo_y = INT_MAX, hi_y = INT_MIN;
        for (int k = fstart[m]; k < fstart[m + 1]; ++k) {                 // (<= 16384 cells)
            const uint32_t o = foffs[k];
            const int dx = (int)(int16_t)(o & 0xffffu), dy = (int)(int16_t)(o >> 16);
            lo_x = min(lo_x, dx); hi_x = max(hi_x, dx); lo_y = min(lo_y, dy); hi_y = max(hi_y, dy);
        }
        wcell[m * 12 + 8] = lo_x; wcell[m * 12 + 9] = hi_x; wcell[m * 12 + 10] = lo_y; wcell[m * 12 + 11] = hi_y;
    }
    if (m >= total) return;
    int h = 0;
    while (h + 1 < H && fstart[h + 1] <= m) ++h;                          // (H <= 64)
    const uint32_t o = foffs[m];
    const double c = cos_sin[2 * h], s = cos_sin[2 * h + 1];
    const double du = (((double)(int)(int16_t)(o & 0xffffu) + 0.5) - 0.5) * res;
    const double dv = (((double)(int)(int16_t)(o >> 16) + 0.5) - 0.5) * res;
    const double u = du * c + dv * s;
    const double v = dv * c - du * s;
    uv[m] = make_double2(u - axle_mid, v);
}

// (float)t as the tilt's share of a limit: 0 .. 100, 0 for a limit that is not finite
__device__ __forceinline__ double av_share(float a, float limit)
{
    return isfinite(limit) ? (double)fabsf(a) / (double)limit * 100.0 : 0.0;
}

__global__ __launch_bounds__(256) void k_volume_attitude(const AttitudeVolumeParams P, const int32_t *__restrict__ fstart,
                                                         const uint32_t *__restrict__ foffs, const double2 *__restrict__ uv,
                                                         const int32_t *__restrict__ wcell, const double *__restrict__ G,
                                                         uint8_t *__restrict__ status, uint8_t *__restrict__ tilt, int32_t *__restrict__ counts)
{
    const int n2 = P.xy * P.xy;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    const bool live = i < n2;                                             // (no early return: the ballots below take whole waves)
    const int h = blockIdx.y;
    const int y = i / P.xy, x = i - y * P.xy;
    const uint32_t uxy = (uint32_t)P.xy;
    if (blockIdx.x == 0 && h == 0 && threadIdx.x == 0) counts[7] = P.H;
    const AtWheels W = at_state_wheels(wcell, G, h, x, y, uxy, live);
    const bool wheel_out = W.out, wheel_unknown = W.unknown, ok = W.ok;
    const AtStance a = at_stance(W.z, P.wheelbase, P.track);
    const double sp = a.sp, sr = a.sr, z0 = a.z0;
    // a footprint cell lies outside the window iff the footprint's box does (its corners are offsets of the list): ONE test per state
    // instead of one per cell, and the states that pass it read every cell of the list unconditionally
    const int lo_x = wcell[h * 12 + 8], hi_x = wcell[h * 12 + 9], lo_y = wcell[h * 12 + 10], hi_y = wcell[h * 12 + 11];
    const bool out = !(x + lo_x >= 0 && x + hi_x < P.xy && y + lo_y >= 0 && y + hi_y < P.xy);
    double belly = (double)INFINITY;
    const int b = fstart[h], M = fstart[h + 1] - b;
    if (ok && !out) {
        int m = 0;
        for (; m + AV_DEPTH <= M; m += AV_DEPTH) {
            double g[AV_DEPTH];
#pragma unroll
            for (int d = 0; d < AV_DEPTH; ++d) {
                const uint32_t o = foffs[b + m + d];
                const double *Gm = G + ((int)(int16_t)(o >> 16) * P.xy + (int)(int16_t)(o & 0xffffu));   // (wave-uniform)
                g[d] = Gm[i];
            }
#pragma unroll
            for (int d = 0; d < AV_DEPTH; ++d) {
                const double2 q = uv[b + m + d];
                const double clr = (((z0 + sp * q.x) + sr * q.y) + P.belly_height) - g[d];
                if (at_known(g[d]) && clr < belly) belly = clr;           // (a NaN clearance is skipped)
            }
        }
        for (; m < M; ++m) {
            const uint32_t o = foffs[b + m];
            const double *Gm = G + ((int)(int16_t)(o >> 16) * P.xy + (int)(int16_t)(o & 0xffffu));
            const double g = Gm[i];
            const double2 q = uv[b + m];
            const double clr = (((z0 + sp * q.x) + sr * q.y) + P.belly_height) - g;
            if (at_known(g) && clr < belly) belly = clr;
        }
    }
    const float p = (float)sp, r = (float)sr, bl = (float)belly;
    int st;
    if (wheel_out || out) st = AT_LEFT_WINDOW;
    else if (wheel_unknown) st = AT_UNKNOWN_GROUND;
    else if (fabsf(p) > P.max_pitch) st = AT_PITCH;
    else if (fabsf(r) > P.max_roll) st = AT_ROLL;
    else if (bl < P.min_clearance) st = AT_BELLY;
    else st = AT_OK;
    uint32_t tl = 0u;
    if (st < AT_UNKNOWN_GROUND) {
        const double tp = av_share(p, P.max_pitch), tr = av_share(r, P.max_roll);
        const double t = tp > tr ? tp : tr;
        tl = !(t > 0.0) ? 0u : (t >= 100.0 ? 100u : (uint32_t)floor(t));
    }
    if (live) {
        const size_t at = (size_t)h * (size_t)n2 + (size_t)i;
        status[at] = (uint8_t)st;
        tilt[at] = (uint8_t)tl;
    }
    at_tally(counts, AT_LEFT_WINDOW, live, st);
}

__global__ __launch_bounds__(256) void k_cspace_attitude(const size_t n, const uint8_t *__restrict__ status, const uint8_t *__restrict__ tilt,
                                                         const uint32_t block_mask, const uint32_t tilt_weight, uint16_t *__restrict__ C)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = C[i];
    const bool blocked = c == 0u || ((block_mask >> status[i]) & 1u) != 0u;
    C[i] = (uint16_t)(blocked ? 0u : min(65535u, c + tilt_weight * (uint32_t)tilt[i]));
}

static bool volume_shape_ok(int xy, int H)
{
    return xy >= 1 && xy <= 4096 && H >= 1 && H <= GVOM_POSE_MAX_HEADINGS && (int64_t)H * xy * xy <= GVOM_POSE_MAX_STATES;
}

hipError_t gvom_launch_attitude_volume_table(hipStream_t s, int H, int total, double res, double axle_mid, const int32_t *fstart,
                                             const uint32_t *foffs, const double *wheels, const double *cos_sin, double *uv, int32_t *wcell)
{
    if (H < 1 || H > GVOM_POSE_MAX_HEADINGS || total < H || total > GVOM_ROLLOUT_MAX_TABLE) return hipErrorInvalidValue;
    const int n = total > 8 * H ? total : 8 * H;
    hipLaunchKernelGGL(k_volume_attitude_table, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, H, total, res, axle_mid, fstart, foffs,
                       wheels, cos_sin, (double2 *)uv, wcell);
    return hipGetLastError();
}

hipError_t gvom_launch_attitude_volume(hipStream_t s, const AttitudeVolumeParams &P, const int32_t *fstart, const uint32_t *foffs,
                                       const double *uv, const int32_t *wcell, const double *ground, uint8_t *status, uint8_t *tilt,
                                       int32_t *counts)
{
    if (!volume_shape_ok(P.xy, P.H)) return hipErrorInvalidValue;
    const int n2 = P.xy * P.xy;
    hipLaunchKernelGGL(k_volume_attitude, dim3((unsigned)((n2 + 255) / 256), (unsigned)P.H), dim3(256), 0, s, P, fstart, foffs,
                       (const double2 *)uv, wcell, ground, status, tilt, counts);
    return hipGetLastError();
}

hipError_t gvom_launch_cspace_attitude(hipStream_t s, int xy, int H, const uint8_t *status, const uint8_t *tilt, uint32_t block_mask,
                                       uint32_t tilt_weight, uint16_t *C)
{
    if (!volume_shape_ok(xy, H) || block_mask > 0x7fu || tilt_weight > 255u) return hipErrorInvalidValue;
    const size_t n = (size_t)H * xy * xy;
    hipLaunchKernelGGL(k_cspace_attitude, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, status, tilt, block_mask, tilt_weight, C);
    return hipGetLastError();
}
