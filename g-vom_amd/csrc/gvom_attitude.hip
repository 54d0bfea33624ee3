// gvom_attitude.hip -- terrain attitude scoring (gfx950, wave64): how the vehicle would sit on the ground at each pose of K candidate
// trajectories of T poses -- pitch and roll from the ground under its four wheels, and the least clearance between the plane
// through them (raised by the belly's height) and the ground under the footprint (include/gvom_hip.h "terrain attitude scoring"
// defines the result).
//
//   k_attitude_ground   the map-set route only: one pass over the set's height and inferred-height maps writes the ONE float64 ground
//                       map k_attitude gathers from (height where it is known, else the inferred height or -1000).
//   k_attitude          one workgroup per rollout, shaped like k_rollouts.  The waves take the rollout's poses in turn; the pose
//                       frame, the four wheel heights and the plane's coefficients are wave-uniform; the 64 lanes run over the
//                       footprint cells of ONE pose, AT_DEPTH cells per lane in flight.  A pose ends in a ballot (a cell outside the
//                       window) and a 64-bit shuffle minimum; its status and three values go to LDS.  Behind one barrier wave 0 makes
//                       the five summary words -- a ballot finds the first bad pose, shuffles the three arg-extremes in front of it
//                       -- and all waves store parts 1 and 2.
//
// READ-ONLY on the ground map.  No load without its bounds test in front of it: invalid poses, wheels outside the window and cells
// outside the window read nothing, and a pose whose wheels stand on unknown ground reads no footprint cell.  No scratch, no atomics,
// no wait on another workgroup; every loop is bounded at launch (T <= 4096 poses, <= 16384 cells per heading).  Every float64
// operation is one IEEE operation in the header's order (-ffp-contract=off): the result is exact.
#include "gvom_rollouts.h"                                  // (the one text of the vehicle on the ground and of a rollout's summary: AT_*, at_*)

#define AT_WAVES 4          // waves per workgroup (fewer where T is smaller)
#define AT_DEPTH 4          // footprint cells per lane whose loads are in flight together

__global__ __launch_bounds__(256) void k_attitude_ground(int n2, int inferred, const double *__restrict__ height,
                                                         const double *__restrict__ inferred_height, double *__restrict__ ground)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n2) return;
    const double hgt = height[i];
    ground[i] = hgt > -1000.0 ? hgt : (inferred ? inferred_height[i] : -1000.0);
}

__global__ __launch_bounds__(AT_WAVES * WAVE) void k_attitude(const AttitudeParams P, const float *__restrict__ poses,
                                                              const int32_t *__restrict__ fstart, const uint32_t *__restrict__ foffs,
                                                              const double *__restrict__ wheels, const double *__restrict__ cos_sin,
                                                              const double *__restrict__ G, int32_t *__restrict__ summary,
                                                              float *__restrict__ attitude, uint8_t *__restrict__ status)
{
    extern __shared__ float s_att[];                          // [T][3] {pitch, roll, belly}, then [T] status bytes
    uint8_t *s_st = (uint8_t *)(s_att + 3 * P.R.T);
    const int lane = (int)(threadIdx.x & 63u);
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), nw = (int)(blockDim.x >> 6);
    const size_t k = blockIdx.x;
    const int T = P.R.T;
    const float *pk = poses + k * (size_t)T * 3;
    const uint32_t uxy = (uint32_t)P.R.xy;
    for (int t = w; t < T; t += nw) {
        int cx, cy, h;
        const bool valid = ro_pose(P.R, pk + 3 * t, cx, cy, h);       // (wave-uniform: one pose per wave)
        bool wheel_out = false, wheel_unknown = false, out = false;
        double sp = 0.0, sr = 0.0, belly = (double)INFINITY;
        if (valid) {
            const double x = (double)pk[3 * t], y = (double)pk[3 * t + 1];
            AtCells wc;
            wheel_out = at_pose_cells(P.R, wheels, h, x, y, wc);
            if (!wheel_out) {
                double z[4];
                wheel_unknown = at_pose_heights(G, uxy, wc, z);
                const bool ok = !wheel_unknown;
                const AtStance a = at_stance(z, P.wheelbase, P.track);
                sp = a.sp;
                sr = a.sr;
                const double z0 = a.z0;
                const double qx = x / P.R.res, qy = y / P.R.res;
                const double fx = qx - floor(qx), fy = qy - floor(qy);
                const double c = cos_sin[2 * h], s = cos_sin[2 * h + 1];
                const int b = fstart[h], M = fstart[h + 1] - b;
                for (int m0 = 0; m0 < M; m0 += AT_DEPTH * WAVE) {
                    uint32_t o[AT_DEPTH];
                    double g[AT_DEPTH];
#pragma unroll
                    for (int d = 0; d < AT_DEPTH; ++d) {
                        const int m = m0 + d * WAVE + lane;
                        o[d] = m < M ? foffs[b + m] : 0u;
                    }
#pragma unroll
                    for (int d = 0; d < AT_DEPTH; ++d) {
                        const int m = m0 + d * WAVE + lane;
                        const uint32_t X = (uint32_t)(cx + (int)(int16_t)(o[d] & 0xffffu)), Y = (uint32_t)(cy + (int)(int16_t)(o[d] >> 16));
                        const bool live = m < M, in = live && X < uxy && Y < uxy;
                        out = out || (live && !in);
                        g[d] = (in && ok) ? G[mad24s(Y, uxy, X)] : -1000.0;      // (a cell that is not read: unknown)
                    }
#pragma unroll
                    for (int d = 0; d < AT_DEPTH; ++d) {
                        const double du = (((double)(int)(int16_t)(o[d] & 0xffffu) + 0.5) - fx) * P.R.res;
                        const double dv = (((double)(int)(int16_t)(o[d] >> 16) + 0.5) - fy) * P.R.res;
                        const double u = du * c + dv * s;
                        const double v = dv * c - du * s;
                        const double plane = (z0 + sp * (u - P.axle_mid)) + sr * v;
                        const double clr = (plane + P.belly_height) - g[d];
                        if (at_known(g[d]) && clr < belly) belly = clr;          // (a NaN clearance is skipped)
                    }
                }
            }
        }
        const bool any_out = lanes(out) != 0ull;
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const double o = __shfl_xor(belly, s);
            belly = o < belly ? o : belly;
        }
        if (lane == 0) {
            float p = (float)sp, r = (float)sr, bl = (float)belly;
            int st;
            if (!valid) st = AT_INVALID;
            else if (wheel_out || any_out) st = AT_LEFT_WINDOW;
            else if (wheel_unknown) st = AT_UNKNOWN_GROUND;
            else if (fabsf(p) > P.max_pitch) st = AT_PITCH;
            else if (fabsf(r) > P.max_roll) st = AT_ROLL;
            else if (bl < P.min_clearance) st = AT_BELLY;
            else st = AT_OK;
            if (st >= AT_UNKNOWN_GROUND) p = r = bl = 0.0f;
            s_att[3 * t] = p; s_att[3 * t + 1] = r; s_att[3 * t + 2] = bl;
            s_st[t] = (uint8_t)st;
        }
    }
    __syncthreads();
    if (w == 0) {                                             // the summary: the first bad pose, the three arg-extremes in front of it
        const int first = at_first_bad(T, lane, [=](int t) { return s_st[t] != AT_OK; });
        float kp = -INFINITY, kr = -INFINITY, kb = -INFINITY;
        int tp = INT_MAX, tr = INT_MAX, tb = INT_MAX;
        for (int t = lane; t < first; t += WAVE) {
            const float p = s_att[3 * t], r = s_att[3 * t + 1], bl = s_att[3 * t + 2];
            at_better(kp, tp, p == p ? fabsf(p) : -1.0f, t);  // (a NaN tangent -- heights whose sums overflow -- ranks below every number)
            at_better(kr, tr, r == r ? fabsf(r) : -1.0f, t);
            at_better(kb, tb, -bl, t);
        }
        tp = at_arg_wave(kp, tp); tr = at_arg_wave(kr, tr); tb = at_arg_wave(kb, tb);
        if (lane < 5) {
            const int st = first < T ? (int)s_st[first] : AT_OK;
            const int none = first == 0;
            const int word = lane == 0 ? st : (lane == 1 ? first : (none ? -1 : (lane == 2 ? tp : (lane == 3 ? tr : tb))));
            summary[k * 5 + lane] = word;
        }
    }
    float *pa = attitude + k * (size_t)T * 3;
    for (int i = (int)threadIdx.x; i < 3 * T; i += (int)blockDim.x) pa[i] = s_att[i];
    uint8_t *ps = status + k * (size_t)T;
    for (int t = (int)threadIdx.x; t < T; t += (int)blockDim.x) ps[t] = s_st[t];
}

hipError_t gvom_launch_attitude_ground(hipStream_t s, int xy, int inferred, const double *height, const double *inferred_height, double *ground)
{
    if (xy < 1 || xy > 4096) return hipErrorInvalidValue;
    const int n2 = xy * xy;
    hipLaunchKernelGGL(k_attitude_ground, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, s, n2, inferred, height, inferred_height, ground);
    return hipGetLastError();
}

hipError_t gvom_launch_attitude(hipStream_t s, const AttitudeParams &P, const float *poses, const int32_t *fstart, const uint32_t *foffs,
                                const double *wheels, const double *cos_sin, const double *ground, int32_t *summary, float *attitude,
                                uint8_t *status)
{
    const RolloutParams &R = P.R;
    if (R.K < 1 || R.K > GVOM_ROLLOUT_MAX_POSES || R.T < 1 || R.T > GVOM_ROLLOUT_MAX_T || R.xy < 1 || R.xy > 4096 || R.H < 1 ||
        R.H > GVOM_ROLLOUT_MAX_HEADINGS)
        return hipErrorInvalidValue;
    const int nw = R.T < AT_WAVES ? R.T : AT_WAVES;
    const size_t lds = (size_t)R.T * 13;                      // <= 53,248 bytes
    hipLaunchKernelGGL(k_attitude, dim3((unsigned)R.K), dim3((unsigned)(nw * WAVE)), lds, s, P, poses, fstart, foffs, wheels, cos_sin, ground,
                       summary, attitude, status);
    return hipGetLastError();
}
