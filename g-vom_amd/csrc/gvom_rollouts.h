// gvom_rollouts.h -- the pose frame of rollout scoring, shared by the kernels that place a footprint at a pose: k_rollouts
// (gvom_rollouts.hip) and k_attitude (gvom_attitude.hip).  include/gvom_hip.h "rollout scoring" defines CENTRE, HEADING and INVALID.
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
