// gvom_rollouts.hip -- rollout scoring (gfx950, wave64): what the vehicle's footprint, turned to each pose's heading, touches on a
// cost map, for K candidate trajectories of T poses each (include/gvom_hip.h "rollout scoring" defines the result).
//
//   k_rollouts   ONE kernel, one workgroup per rollout.  The waves of the workgroup take the rollout's poses in turn; the 64 lanes
//                of a wave run over the footprint cells of ONE pose -- a compact patch of the map, so a wave's 64 two-byte reads fall
//                into a few cache lines, and the next pose (a cell further on) reads the same lines again.  A pose ends in two
//                ballots (a blocked cell inside the window, a cell outside it) and a shuffle maximum; its cost and status go to
//                LDS.  Behind a barrier wave 0 makes the rollout's summary from LDS -- first blocked pose, the sum in front of it,
//                the cost-to-go under the last free pose -- and all waves store the pose costs.  The geometry is the table's: the
//                kernel only walks it.
//
// READ-ONLY on the maps.  No scratch, no atomics, no wave waits on another workgroup; every loop is bounded at launch (T <= 4096
// poses, <= 16384 cells per heading).  Integer arithmetic throughout but the pose's two divisions (float64, IEEE) and one float32
// multiply (-ffp-contract=off): the result is exact.
#include "gvom_rollouts.h"       // RO_FAR, ro_cell, ro_pose: the pose frame, shared with gvom_attitude.hip

#define RO_WAVES 4          // waves per workgroup (fewer where T is smaller)
#define RO_DEPTH 4          // footprint cells per lane whose loads are in flight together
// status words (include/gvom_hip.h GVOM_ROLLOUT_*)
#define RO_CLEAR 0
#define RO_COLLISION 1
#define RO_LEFT_WINDOW 2
#define RO_INVALID 3

__global__ __launch_bounds__(RO_WAVES * WAVE) void k_rollouts(const RolloutParams P, const float *__restrict__ poses,
                                                              const int32_t *__restrict__ fstart, const uint32_t *__restrict__ foffs,
                                                              const uint16_t *__restrict__ c, const int32_t *__restrict__ D,
                                                              v4i *__restrict__ summary, uint16_t *__restrict__ pose_cost)
{
    __shared__ uint16_t s_cost[GVOM_ROLLOUT_MAX_T];
    __shared__ uint8_t s_st[GVOM_ROLLOUT_MAX_T];
    const int lane = (int)(threadIdx.x & 63u);
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), nw = (int)(blockDim.x >> 6);
    const size_t k = blockIdx.x;
    const float *pk = poses + k * (size_t)P.T * 3;
    const uint32_t uxy = (uint32_t)P.xy;
    for (int t = w; t < P.T; t += nw) {
        int cx, cy, h;
        const bool valid = ro_pose(P, pk + 3 * t, cx, cy, h);
        bool out = false, zero = false;
        uint32_t mx = 0u;
        if (valid) {                                          // (wave-uniform: one pose per wave)
            const int b = fstart[h], M = fstart[h + 1] - b;
            for (int m0 = 0; m0 < M; m0 += RO_DEPTH * WAVE) {
                uint32_t o[RO_DEPTH], v[RO_DEPTH];
#pragma unroll
                for (int d = 0; d < RO_DEPTH; ++d) {
                    const int m = m0 + d * WAVE + lane;
                    o[d] = m < M ? foffs[b + m] : 0u;
                }
#pragma unroll
                for (int d = 0; d < RO_DEPTH; ++d) {
                    const int m = m0 + d * WAVE + lane;
                    const uint32_t x = (uint32_t)(cx + (int)(int16_t)(o[d] & 0xffffu)), y = (uint32_t)(cy + (int)(int16_t)(o[d] >> 16));
                    const bool live = m < M, in = live && x < uxy && y < uxy;
                    out = out || (live && !in);
                    v[d] = in ? (uint32_t)c[mad24s(y, uxy, x)] : 0x10000u;      // (a cell that is not read: neither blocked nor a maximum)
                }
#pragma unroll
                for (int d = 0; d < RO_DEPTH; ++d) { zero = zero || v[d] == 0u; mx = max(mx, v[d] & 0xffffu); }
            }
        }
        const bool any_zero = lanes(zero) != 0ull, any_out = lanes(out) != 0ull;
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, s));
        if (lane == 0) {
            const bool blocked = !valid || any_zero || any_out;
            s_cost[t] = (uint16_t)(blocked ? 0u : mx);
            s_st[t] = (uint8_t)(!valid ? RO_INVALID : (any_zero ? RO_COLLISION : (any_out ? RO_LEFT_WINDOW : RO_CLEAR)));
        }
    }
    __syncthreads();
    if (w == 0) {                                             // the summary: first blocked pose, the sum in front of it, the terminal
        int first = P.T;
        uint32_t acc = 0u;
        for (int t0 = 0; t0 < P.T; t0 += WAVE) {
            const int t = t0 + lane;
            const uint32_t v = t < P.T ? (uint32_t)s_cost[t] : 0x10000u;
            const unsigned long long z = lanes(v == 0u);
            if (z != 0ull) {
                const int f = __builtin_ctzll(z);
                first = t0 + f;
                acc += lane < f ? v : 0u;
                break;
            }
            acc += v & 0xffffu;
        }
        const uint32_t path = wave_sum(acc);                 // (at most 4096 * 65535 < 2^31)
        if (lane == 0) {
            const int status = first < P.T ? (int)s_st[first] : RO_CLEAR;
            int terminal = INT_MAX;                           // GVOM_CTG_UNREACHED
            if (D != nullptr && first > 0) {
                int cx, cy, h;
                ro_pose(P, pk + 3 * (first - 1), cx, cy, h);
                if ((uint32_t)cx < uxy && (uint32_t)cy < uxy) terminal = D[(uint32_t)cy * uxy + (uint32_t)cx];
            }
            const v4i r = {status, first, (int)path, terminal};
            summary[k] = r;
        }
    }
    uint16_t *pc = pose_cost + k * (size_t)P.T;
    for (int t = (int)threadIdx.x; t < P.T; t += (int)blockDim.x) pc[t] = s_cost[t];
}

hipError_t gvom_launch_rollouts(hipStream_t s, const RolloutParams &P, const float *poses, const int32_t *fstart, const uint32_t *foffs,
                                const uint16_t *cell_cost, const int32_t *cost_to_go, int32_t *summary, uint16_t *pose_cost)
{
    if (P.K < 1 || P.K > GVOM_ROLLOUT_MAX_POSES || P.T < 1 || P.T > GVOM_ROLLOUT_MAX_T || P.xy < 1 || P.xy > 4096 || P.H < 1 ||
        P.H > GVOM_ROLLOUT_MAX_HEADINGS)
        return hipErrorInvalidValue;
    const int nw = P.T < RO_WAVES ? P.T : RO_WAVES;
    hipLaunchKernelGGL(k_rollouts, dim3((unsigned)P.K), dim3((unsigned)(nw * WAVE)), 0, s, P, poses, fstart, foffs, cell_cost, cost_to_go,
                       (v4i *)summary, pose_cost);
    return hipGetLastError();
}
