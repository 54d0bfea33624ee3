// gvom_rollouts.h -- the pose frame of rollout scoring, shared by the kernels that place a footprint at a pose: k_rollouts
// (gvom_rollouts.hip), k_attitude (gvom_attitude.hip) and k_body (gvom_body.hip).  include/gvom_hip.h "rollout scoring" defines CENTRE,
// HEADING and INVALID.  Behind it: the ONE text of the vehicle on the ground ("terrain attitude scoring") for k_attitude, k_body,
// k_volume_attitude and k_volume_body -- the status words, the wheels of a pose and of a state, the stance, a volume's census -- and of a
// rollout's summary: the first bad pose and the arg-extreme.
#pragma once
#include "gvom_device.h"

#define RO_FAR 100000       // a centre this far out has every footprint cell (|offset| < 2^15) outside any window (xy <= 4096)

// floor((double)x / res) - o, clamped to +-RO_FAR; -RO_FAR for NaN, an infinity and |x / res| >= 2^30
__device__ __forceinline__ int ro_cell(float x, double res, long long o)
{
    const double q = (double)x / res;
    if (!(fabs(q) < 1073741824.0)) return -RO_FAR;
    const long long c = (long long)floor(q) - o;
    return (int)max(min(c, (long long)RO_FAR), (long long)-RO_FAR);
}

// centre cell, heading and validity of a pose (x, y, yaw)
__device__ __forceinline__ bool ro_pose(const RolloutParams &P, const float *__restrict__ p, int &cx, int &cy, int &h)
{
    const float x = p[0], y = p[1], yaw = p[2];
    const float a = yaw * P.s;
    const bool valid = fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(yaw) < INFINITY && fabsf(a) < 16777216.0f;
    cx = ro_cell(x, P.res, P.ox); cy = ro_cell(y, P.res, P.oy);
    const int r = valid ? (int)rintf(a) % P.H : 0;          // (|a| < 2^24: the conversion is exact)
    h = r < 0 ? r + P.H : r;
    return valid;
}

// ---- terrain attitude scoring's GROUND, wheel cells and ATTITUDE (include/gvom_hip.h) ----------------------------------------------------
__device__ __forceinline__ bool at_known(double g) { return g > -1000.0 && g < (double)INFINITY; }

// floor(xx / res) - o, clamped to +-RO_FAR; -RO_FAR unless |xx / res| < 2^30 (NaN included)
__device__ __forceinline__ int at_cell(double xx, double res, long long o)
{
    const double q = xx / res;
    if (!(fabs(q) < 1073741824.0)) return -RO_FAR;
    const long long c = (long long)floor(q) - o;
    return (int)max(min(c, (long long)RO_FAR), (long long)-RO_FAR);
}

// status words (include/gvom_hip.h GVOM_ATTITUDE_*; body clearance's are gvom_bodyframe.h's BD_*)
#define AT_OK 0
#define AT_PITCH 1
#define AT_ROLL 2
#define AT_BELLY 3
#define AT_UNKNOWN_GROUND 4
#define AT_LEFT_WINDOW 5
#define AT_INVALID 6

// the wheel cells {FL, FR, RL, RR} of the pose (x, y) at heading h, through the chassis table wheels [H][4][2]: true where one lies
// outside the window (k_attitude, k_body)
struct AtCells { uint32_t x[4], y[4]; };
__device__ __forceinline__ bool at_pose_cells(const RolloutParams &R, const double *__restrict__ wheels, int h, double x, double y, AtCells &c)
{
    const uint32_t uxy = (uint32_t)R.xy;
    bool out = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        c.x[i] = (uint32_t)at_cell(x + wheels[(h * 4 + i) * 2], R.res, R.ox);
        c.y[i] = (uint32_t)at_cell(y + wheels[(h * 4 + i) * 2 + 1], R.res, R.oy);
        out = out || !(c.x[i] < uxy && c.y[i] < uxy);
    }
    return out;
}

// the ground heights z at the wheel cells of a pose, all INSIDE the window: true where one is unknown
__device__ __forceinline__ bool at_pose_heights(const double *__restrict__ G, uint32_t uxy, const AtCells &c, double z[4])
{
    bool unknown = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        z[i] = G[mad24s(c.y[i], uxy, c.x[i])];
        unknown = unknown || !at_known(z[i]);
    }
    return unknown;
}

// the wheels of the state (cell (x, y), heading h), through the attitude volume table's wheel offsets wcell [H][12]: their heights,
// whether one stands outside the window or on unknown ground, and ok = neither and the state is `live` (k_volume_attitude,
// k_volume_body).  A wheel that is not read -- the state is not live or has a wheel outside the window -- is unknown
struct AtWheels { double z[4]; bool out, unknown, ok; };
__device__ __forceinline__ AtWheels at_state_wheels(const int32_t *__restrict__ wcell, const double *__restrict__ G, int h, int x, int y,
                                                    uint32_t uxy, bool live)
{
    AtWheels W;
    W.out = W.unknown = false;
    uint32_t wi[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t X = (uint32_t)(x + wcell[h * 12 + 2 * k]), Y = (uint32_t)(y + wcell[h * 12 + 2 * k + 1]);
        W.out = W.out || !(X < uxy && Y < uxy);
        wi[k] = Y * uxy + X;
    }
    const bool wheels_in = live && !W.out;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        W.z[k] = wheels_in ? G[wi[k]] : -1000.0;
        W.unknown = W.unknown || !at_known(W.z[k]);
    }
    W.ok = wheels_in && !W.unknown;
    return W;
}

// the census of a volume: counts[s] += the wave's live states of status s, for s = 0 .. last -- one ballot, one population count and
// at most one int32 atomic per status and wave
__device__ __forceinline__ void at_tally(int32_t *__restrict__ counts, const int last, bool live, int st)
{
    const int lane = (int)(threadIdx.x & 63u);
#pragma unroll
    for (int s = 0; s <= last; ++s) {
        const int n = __builtin_popcountll(lanes(live && st == s));
        if (n != 0 && lane == 0) atomicAdd(&counts[s], n);
    }
}

// a rollout's first pose t < T with bad(t), T where there is none: one ballot per 64 poses (called by a whole wave)
template <class Bad> __device__ __forceinline__ int at_first_bad(int T, int lane, Bad bad)
{
    int first = T;
    for (int t0 = 0; t0 < T; t0 += WAVE) {
        const int t = t0 + lane;
        const unsigned long long b = lanes(t < T && bad(t));
        if (b != 0ull) { first = t0 + __builtin_ctzll(b); break; }
    }
    return first;
}

// ATTITUDE: the pitch and roll tangents and the mean height of the four wheel heights z = {zFL, zFR, zRL, zRR}
struct AtStance { double sp, sr, z0; };
__device__ __forceinline__ AtStance at_stance(const double z[4], double wheelbase, double track)
{
    const double zF = 0.5 * (z[0] + z[1]), zR = 0.5 * (z[2] + z[3]), zL = 0.5 * (z[0] + z[2]), zT = 0.5 * (z[1] + z[3]);
    AtStance a;
    a.sp = (zF - zR) / wheelbase;
    a.sr = (zL - zT) / track;
    a.z0 = 0.25 * ((z[0] + z[1]) + (z[2] + z[3]));
    return a;
}

// the better of two candidates for an arg-extreme: the larger key, the lower pose where the keys are equal (keys are never NaN)
__device__ __forceinline__ void at_better(float &key, int &t, float ko, int to)
{
    if (ko > key || (ko == key && to < t)) { key = ko; t = to; }
}

__device__ __forceinline__ int at_arg_wave(float key, int t)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const float ko = __shfl_xor(key, s);
        const int to = __shfl_xor(t, s);
        at_better(key, t, ko, to);
    }
    return t;
}
