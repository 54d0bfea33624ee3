// gvom_rollouts.h -- the pose frame of rollout scoring, shared by the kernels that place a footprint at a pose: k_rollouts
// (gvom_rollouts.hip), k_attitude (gvom_attitude.hip) and k_body (gvom_body.hip).  include/gvom_hip.h "rollout scoring" defines CENTRE,
// HEADING and INVALID.  Behind it: the wheel and plane arithmetic of "terrain attitude scoring" that k_attitude and k_body share, and the
// arg-extreme of a rollout's summary.
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
