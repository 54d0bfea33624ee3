// gvom_bodyframe.h -- the one text of body clearance scoring's FRAME, SPHERE CENTRE, voxel and MARGIN (include/gvom_hip.h "body clearance
// scoring"), shared by the kernels that place the sphere body on the ground: k_body (gvom_body.hip, at the poses of rollouts) and
// k_volume_body (gvom_body_volume.hip, at every state of the window).  Every float64 operation is one IEEE operation in the header's order.
#pragma once
#include "gvom_rollouts.h"

// status words (include/gvom_hip.h GVOM_BODY_*)
#define BD_OK 0
#define BD_COLLISION 1
#define BD_LEFT_BOX 2
#define BD_UNKNOWN_GROUND 3
#define BD_LEFT_WINDOW 4
#define BD_INVALID 5

#define BD_OUT 0xffffffffu

// floor(xx / res) - o where that lies in [0, n), else BD_OUT; BD_OUT unless |xx / res| < 2^30 (NaN included).  |o| <= 2^40: no overflow
__device__ __forceinline__ uint32_t bd_voxel(double xx, double res, long long o, int n)
{
    const double q = xx / res;
    if (!(fabs(q) < 1073741824.0)) return BD_OUT;
    const long long c = (long long)floor(q) - o;
    return c >= 0 && c < (long long)n ? (uint32_t)c : BD_OUT;
}

// FRAME: e1 along the chassis, n its normal, e2 = n x e1, q0 the contact plane's height under the pose
struct BdFrame { double e1u, e1w, nu, nv, nw, e2u, e2v, e2w, q0; };
__device__ __forceinline__ BdFrame bd_frame(const AtStance &a, double axle_mid)
{
    const double sp = a.sp, sr = a.sr, z0 = a.z0;
    const double one = 1.0 + sp * sp;
    const double lu = sqrt(one), ln = sqrt(one + sr * sr);
    BdFrame F;
    F.e1u = 1.0 / lu; F.e1w = sp / lu;
    F.nu = -sp / ln; F.nv = -sr / ln; F.nw = 1.0 / ln;
    F.e2u = F.nv * F.e1w; F.e2v = F.nw * F.e1u - F.nu * F.e1w; F.e2w = -(F.nv * F.e1u);
    F.q0 = z0 - sp * axle_mid;
    return F;
}

// SPHERE CENTRE of b = (bx, by, bz, r) at the pose (x, y) of heading (c, s), and its voxel (vx, vy, vz) in the box of P: false where it
// is OUTSIDE (a coordinate is BD_OUT)
__device__ __forceinline__ bool bd_sphere(const BodyParams &P, const BdFrame &F, const float4 b, double x, double y, double c, double s,
                                          uint32_t &vx, uint32_t &vy, uint32_t &vz)
{
    const double bx = (double)b.x, by = (double)b.y, bz = (double)b.z;
    const double Cu = (bx * F.e1u + by * F.e2u) + bz * F.nu;
    const double Cv = by * F.e2v + bz * F.nv;
    const double Cw = ((bx * F.e1w + by * F.e2w) + bz * F.nw) + F.q0;
    const double X = x + (Cu * c - Cv * s);
    const double Y = y + (Cu * s + Cv * c);
    vx = bd_voxel(X, P.R.res, P.bx, P.n); vy = bd_voxel(Y, P.R.res, P.by, P.n); vz = bd_voxel(Cw, P.z_res, P.bz, P.zs);
    return vx != BD_OUT && vy != BD_OUT && vz != BD_OUT;
}

// where the field holds voxel (vx, vy, vz) of its box: out[x][y][z]
__device__ __forceinline__ size_t bd_at(const BodyParams &P, uint32_t vx, uint32_t vy, uint32_t vz)
{
    return ((size_t)vx * (uint32_t)P.n + vy) * (uint32_t)P.zs + vz;
}

// MARGIN: m = d - r taken into (clearance, tightest) as sphere i; a NaN margin is skipped
__device__ __forceinline__ void bd_margin(float &clr, int &tight, float d, float r, int i)
{
    const float m = d - r;
    if (m < clr || (tight < 0 && m == m)) { clr = m; tight = i; }
}
