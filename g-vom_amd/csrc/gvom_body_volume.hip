// gvom_body_volume.hip -- body volumes (gfx950, wave64): where the sphere body lies in 3-D once the vehicle sits on the ground at EVERY
// state (cell centre, heading) of the window, and how close it comes to anything a voxel distance field remembers -- k_body's arithmetic
// without a pose array (include/gvom_hip.h "body volumes" defines the result).
//
//   k_volume_body   a workgroup takes a 16 x 16 TILE of cells at one heading (blockIdx.z), ONE STATE PER LANE, x the fast lane index: a
//                   wave is 16 cells of x by 4 of y.  The field is out[x][y][z], so one sphere's 256 gathers of a workgroup fall into a
//                   (16 + tilt spread)^2 x few-levels neighbourhood instead of a whole row's xy*zs*4-byte stride.  The four wheel gathers
//                   come through the attitude volume's per-heading wheel-offset table (wcell; gvom_rollouts.h at_state_wheels:
//                   k_volume_attitude's text), the stance and the frame are made once per lane (gvom_bodyframe.h: k_body's text), the sphere table is walked by a wave-uniform index -- (bx, by, bz, r) are
//                   scalar loads --, one 4-byte gather per sphere, BV_DEPTH in flight.  A wave none of whose states stands on known
//                   ground inside the window walks no sphere.  With x the fast lane index the three stores are already runs along x (16
//                   bytes of status, 16 of squeeze, 64 of clearance per tile row): no LDS.  A wave ends in at_tally: one ballot and one
//                   population count per status, at most five int32 atomics per wave (INVALID cannot occur), integer sums.
//
// READ-ONLY on the ground map and the field.  No load without its bounds test in front of it: a wheel outside the window reads nothing,
// a sphere outside the box reads nothing, and a state whose wheels stand outside or on unknown ground reads no field value.  No scratch,
// no LDS, no wait on another workgroup; every loop is bounded at launch (S <= 256 spheres).  Every float64 operation is one IEEE
// operation in the header's order (-ffp-contract=off): the result is exact.
#include "gvom_bodyframe.h"

#define BV_TILE 16          // cells per tile side: 256 lanes
#define BV_DEPTH 4          // spheres per lane whose gathers are in flight together

__global__ __launch_bounds__(BV_TILE * BV_TILE) void k_volume_body(const BodyParams P, const float soft_margin, const int32_t *__restrict__ wcell,
                                                                   const double *__restrict__ cos_sin, const double *__restrict__ G,
                                                                   const float4 *__restrict__ body, const float *__restrict__ field,
                                                                   uint8_t *__restrict__ status, uint8_t *__restrict__ squeeze,
                                                                   float *__restrict__ clearance, int32_t *__restrict__ counts)
{
    const int xy = P.R.xy, S = P.S;
    const int h = blockIdx.z;
    const int cx = (int)(blockIdx.x * BV_TILE + (threadIdx.x & (BV_TILE - 1))), cy = (int)(blockIdx.y * BV_TILE + threadIdx.x / BV_TILE);
    const bool live = cx < xy && cy < xy;                                // (no early return: the ballots below take whole waves)
    const uint32_t uxy = (uint32_t)xy;
    if (blockIdx.x == 0 && blockIdx.y == 0 && h == 0 && threadIdx.x == 0) { counts[6] = P.R.H; counts[7] = S; }
    const AtWheels W = at_state_wheels(wcell, G, h, cx, cy, uxy, live);
    const bool wheel_out = W.out, wheel_unknown = W.unknown, ok = W.ok;
    const double c = cos_sin[2 * h], s = cos_sin[2 * h + 1];
    const double x = ((double)(P.R.ox + cx) + 0.5) * P.R.res, y = ((double)(P.R.oy + cy) + 0.5) * P.R.res;
    const BdFrame F = bd_frame(at_stance(W.z, P.wheelbase, P.track), P.axle_mid);      // FRAME (gvom_bodyframe.h)
    float clr = INFINITY;
    int tight = -1;
    bool left = false;
    if (lanes(ok) != 0ull) {                                             // (wave-uniform)
        for (int s0 = 0; s0 < S; s0 += BV_DEPTH) {
            float d[BV_DEPTH], r[BV_DEPTH];
#pragma unroll
            for (int j = 0; j < BV_DEPTH; ++j) {
                d[j] = NAN; r[j] = 0.0f;                                 // (a sphere that is not read: skipped by the minimum)
                if (s0 + j < S) {                                        // (wave-uniform)
                    const float4 b = body[s0 + j];
                    uint32_t vx, vy, vz;
                    const bool in = bd_sphere(P, F, b, x, y, c, s, vx, vy, vz);
                    left = left || !in;
                    if (ok && in) d[j] = field[bd_at(P, vx, vy, vz)];
                    r[j] = b.w;
                }
            }
#pragma unroll
            for (int j = 0; j < BV_DEPTH; ++j) bd_margin(clr, tight, d[j], r[j], s0 + j);
        }
    }
    int st = wheel_out ? BD_LEFT_WINDOW : (wheel_unknown ? BD_UNKNOWN_GROUND : (left ? BD_LEFT_BOX : (clr < P.min_margin ? BD_COLLISION : BD_OK)));
    if (st >= BD_LEFT_BOX) clr = 0.0f;
    uint32_t sq = 0u;
    if (st < BD_LEFT_BOX) {                                              // SQUEEZE: the share of the band soft_margin .. min_margin that is used up
        const float m = P.min_margin, f = soft_margin;
        if (clr >= f) sq = 0u;
        else if (clr <= m || f == m) sq = 100u;
        else {
            const double t = ((double)f - (double)clr) / ((double)f - (double)m) * 100.0;
            sq = !(t > 0.0) ? 0u : (t >= 100.0 ? 100u : (uint32_t)floor(t));
        }
    }
    if (live) {
        const size_t at = (size_t)h * (size_t)(xy * xy) + (size_t)(cy * xy + cx);
        status[at] = (uint8_t)st;
        squeeze[at] = (uint8_t)sq;
        clearance[at] = clr;
    }
    at_tally(counts, BD_LEFT_WINDOW, live, st);
}

hipError_t gvom_launch_body_volume(hipStream_t s, const BodyParams &P, float soft_margin, const int32_t *wcell, const double *cos_sin,
                                   const double *ground, const float *body, const float *field, uint8_t *status, uint8_t *squeeze,
                                   float *clearance, int32_t *counts)
{
    const RolloutParams &R = P.R;
    const long long far = 1ll << 40;
    if (R.xy < 1 || R.xy > 4096 || R.H < 1 || R.H > GVOM_POSE_MAX_HEADINGS || (int64_t)R.H * R.xy * R.xy > GVOM_POSE_MAX_STATES || P.S < 1 ||
        P.S > GVOM_BODY_MAX_SPHERES || P.n < 1 || P.n > 4096 || P.zs < 1 || P.zs > 4096)
        return hipErrorInvalidValue;
    if (P.bx < -far || P.bx > far || P.by < -far || P.by > far || P.bz < -far || P.bz > far || R.ox < -far || R.ox > far || R.oy < -far || R.oy > far)
        return hipErrorInvalidValue;
    const unsigned nt = (unsigned)((R.xy + BV_TILE - 1) / BV_TILE);
    hipLaunchKernelGGL(k_volume_body, dim3(nt, nt, (unsigned)R.H), dim3(BV_TILE * BV_TILE), 0, s, P, soft_margin, wcell, cos_sin, ground,
                       (const float4 *)body, field, status, squeeze, clearance, counts);
    return hipGetLastError();
}
