// gvom_body.hip -- body clearance scoring (gfx950, wave64): where a body made of spheres lies in 3-D once the vehicle sits on the ground at
// each pose of K candidate trajectories of T poses, and how close it comes to anything a voxel distance field remembers
// (include/gvom_hip.h "body clearance scoring" defines the result).
//
//   k_body   one workgroup per rollout, ONE POSE PER LANE (k_volume_attitude's shape, not k_attitude's: a pose's work is S gathers, not a
//            footprint of thousands of cells).  A lane makes its pose's frame once -- the pose frame, the four wheel heights and the
//            stance of gvom_rollouts.h (k_attitude's text), then e1, e2, n and q0 -- and keeps it in registers.  The sphere table is
//            walked by a wave-uniform index, so (bx, by, bz, r) are scalar loads; each lane issues one 4-byte gather per sphere,
//            BD_DEPTH spheres' gathers in flight.  Status, clearance and tightest sphere go to LDS, 6 bytes per pose; behind one barrier
//            wave 0 makes the four summary words -- a ballot finds the first bad pose, a shuffle the least clearance in front of it --
//            and all waves store parts 1 and 2, coalesced.
//
// READ-ONLY on the ground map and the field.  No load without its bounds test in front of it: invalid poses, wheels outside the window and
// spheres outside the box read nothing, and a pose whose wheels stand outside or on unknown ground reads no field value.  No scratch, no
// atomics, no cross-lane reduction per pose, no wait on another workgroup; every loop is bounded at launch (T <= 4096 poses, S <= 256
// spheres).  Every float64 operation is one IEEE operation in the header's order (-ffp-contract=off): the result is exact.
#include "gvom_bodyframe.h"

#define BD_WAVES 4          // waves per workgroup (fewer where T is smaller)
#define BD_DEPTH 4          // spheres per lane whose gathers are in flight together

__global__ __launch_bounds__(BD_WAVES * WAVE) void k_body(const BodyParams P, const float *__restrict__ poses, const double *__restrict__ wheels,
                                                          const double *__restrict__ cos_sin, const double *__restrict__ G,
                                                          const float4 *__restrict__ body, const float *__restrict__ field,
                                                          int32_t *__restrict__ summary, float *__restrict__ clearance, uint16_t *__restrict__ pairs)
{
    extern __shared__ float s_clr[];                          // [T] clearance, then [T] uint16 {status, tightest << 8}
    const int T = P.R.T, S = P.S;
    uint16_t *s_pr = (uint16_t *)(s_clr + T);
    const int lane = (int)(threadIdx.x & 63u);
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t k = blockIdx.x;
    const float *pk = poses + k * (size_t)T * 3;
    for (int t = (int)threadIdx.x; t < T; t += (int)blockDim.x) {
        int cx, cy, h;
        const bool valid = ro_pose(P.R, pk + 3 * t, cx, cy, h);
        int st = valid ? BD_OK : BD_INVALID;
        const double x = (double)pk[3 * t], y = (double)pk[3 * t + 1];
        double z[4] = {0.0, 0.0, 0.0, 0.0}, c = 1.0, s = 0.0;
        if (valid) {
            AtCells wc;
            if (at_pose_cells(P.R, wheels, h, x, y, wc)) st = BD_LEFT_WINDOW;
            else if (at_pose_heights(G, (uint32_t)P.R.xy, wc, z)) st = BD_UNKNOWN_GROUND;
            c = cos_sin[2 * h]; s = cos_sin[2 * h + 1];
        }
        const bool ok = st == BD_OK;
        const BdFrame F = bd_frame(at_stance(z, P.wheelbase, P.track), P.axle_mid);      // FRAME (gvom_bodyframe.h)
        float clr = INFINITY;
        int tight = -1;
        bool left = false;
        for (int s0 = 0; s0 < S; s0 += BD_DEPTH) {
            float d[BD_DEPTH], r[BD_DEPTH];
#pragma unroll
            for (int j = 0; j < BD_DEPTH; ++j) {
                d[j] = NAN; r[j] = 0.0f;                      // (a sphere that is not read: skipped by the minimum)
                if (s0 + j < S) {                             // (wave-uniform)
                    const float4 b = body[s0 + j];
                    uint32_t vx, vy, vz;
                    const bool in = bd_sphere(P, F, b, x, y, c, s, vx, vy, vz);
                    left = left || !in;
                    if (ok && in) d[j] = field[bd_at(P, vx, vy, vz)];
                    r[j] = b.w;
                }
            }
#pragma unroll
            for (int j = 0; j < BD_DEPTH; ++j) bd_margin(clr, tight, d[j], r[j], s0 + j);
        }
        if (ok) st = left ? BD_LEFT_BOX : (clr < P.min_margin ? BD_COLLISION : BD_OK);
        if (st >= BD_LEFT_BOX) { clr = 0.0f; tight = 0; }
        s_clr[t] = clr;
        s_pr[t] = (uint16_t)((uint32_t)st | ((uint32_t)(tight < 0 ? 255 : tight) << 8));
    }
    __syncthreads();
    if (w == 0) {                                             // the summary: the first bad pose, the least clearance in front of it
        const int first = at_first_bad(T, lane, [=](int t) { return (s_pr[t] & 0xffu) != BD_OK; });
        float kc = -INFINITY;
        int tc = INT_MAX;
        for (int t = lane; t < first; t += WAVE) at_better(kc, tc, -s_clr[t], t);        // (a clearance is never NaN)
        tc = at_arg_wave(kc, tc);
        if (lane < 4) {
            const int st = first < T ? (int)(s_pr[first] & 0xffu) : BD_OK;
            const int none = first == 0;
            const int word = lane == 0 ? st : (lane == 1 ? first : (none ? -1 : (lane == 2 ? tc : (int)(s_pr[tc] >> 8))));
            summary[k * 4 + lane] = word;
        }
    }
    float *pc = clearance + k * (size_t)T;
    uint16_t *pp = pairs + k * (size_t)T;
    for (int t = (int)threadIdx.x; t < T; t += (int)blockDim.x) { pc[t] = s_clr[t]; pp[t] = s_pr[t]; }
}

hipError_t gvom_launch_body(hipStream_t s, const BodyParams &P, const float *poses, const double *wheels, const double *cos_sin,
                            const double *ground, const float *body, const float *field, int32_t *summary, float *clearance, uint8_t *pairs)
{
    const RolloutParams &R = P.R;
    const long long far = 1ll << 40;
    if (R.K < 1 || R.K > GVOM_ROLLOUT_MAX_POSES || R.T < 1 || R.T > GVOM_ROLLOUT_MAX_T || R.xy < 1 || R.xy > 4096 || R.H < 1 ||
        R.H > GVOM_ROLLOUT_MAX_HEADINGS || P.S < 1 || P.S > GVOM_BODY_MAX_SPHERES || P.n < 1 || P.n > 4096 || P.zs < 1 || P.zs > 4096)
        return hipErrorInvalidValue;
    if (P.bx < -far || P.bx > far || P.by < -far || P.by > far || P.bz < -far || P.bz > far) return hipErrorInvalidValue;
    const int nw = (R.T + WAVE - 1) / WAVE < BD_WAVES ? (R.T + WAVE - 1) / WAVE : BD_WAVES;
    const size_t lds = (size_t)R.T * 6;                       // <= 24,576 bytes
    hipLaunchKernelGGL(k_body, dim3((unsigned)R.K), dim3((unsigned)(nw * WAVE)), lds, s, P, poses, wheels, cos_sin, ground, (const float4 *)body,
                       field, summary, clearance, (uint16_t *)pairs);
    return hipGetLastError();
}
