// gvom_query.hip -- queries against the fused map (gfx950, wave64); "gvom.py:NNN" = the reference, as in gvom_trace.hip:
//
//   k_raycast   gvom_raycast: walks n segments through the fused map with the mapper's own ray rule (gvom_ray.h: the set-up and
//               step count of gvom.py:1093-1127, the three float32 additions per step of :1128-1132, the window lookup of
//               :1134-1146) and reports where each one stops -- the first occupied voxel, optionally the first voxel nobody
//               has observed, the window's face, or nowhere.  READ-ONLY: it changes nothing of the map.
//
// Numerics as in gvom_trace.hip: -ffp-contract=off, IEEE division / sqrt, every operation rounded once.  For a float32-representable
// start and end the voxels examined are exactly those k_trace adds a ray pass to.
#include "gvom_device.h"
#include "gvom_ray.h"
#include "gvom_raywalk.h"

#define RQ_BLOCK 256

struct __attribute__((aligned(4))) RqPos { float x, y, z; };

// One ray per lane.  A ray's positions depend on nothing it loads: a round computes RQ_DEPTH positions, issues their tile-tag and
// state loads together (a state load from a dead tile is in bounds and ignored) and then examines them in step order.  The loop
// ends when no lane of the wave is running.  No LDS, no atomics; results leave as one 16-byte and one 12-byte store per lane.
template <bool P2>
__global__ __launch_bounds__(RQ_BLOCK) void k_raycast(const ScanParams P, const RayQuery Q, const int32_t *__restrict__ fstate,
                                                      const uint32_t *__restrict__ ftags, v4i *__restrict__ out,
                                                      float *__restrict__ out_pos)
{
    const long i = (long)blockIdx.x * RQ_BLOCK + threadIdx.x;
    const bool live = i < Q.n;
    float ax = 0.0f, ay = 0.0f, az = 0.0f, bx = 0.0f, by = 0.0f, bz = 0.0f;
    if (live) {
        const float *a = Q.from + (Q.one_origin ? 0 : 3 * i), *b = Q.to + 3 * i;
        ax = a[0]; ay = a[1]; az = a[2]; bx = b[0]; by = b[1]; bz = b[2];
    }
    const bool fin = fabsf(ax) < INFINITY && fabsf(ay) < INFINITY && fabsf(az) < INFINITY &&
                     fabsf(bx) < INFINITY && fabsf(by) < INFINITY && fabsf(bz) < INFINITY;
    int32_t r_status = RQ_INVALID, r_steps = 0, r_vox = -1, r_unknown = 0;
    float r_x = NAN, r_y = NAN, r_z = NAN;
    // ray set-up (gvom.py:1097-1126): the start in voxels, increments, the steps the loop test admits
    float px = (float)div_by_res<float>(ax, P.xy_res, P.drcp[0], P.fastdiv & 1);
    float py = (float)div_by_res<float>(ay, P.xy_res, P.drcp[0], P.fastdiv & 1);
    float pz = (float)div_by_res<float>(az, P.z_res, P.drcp[1], P.fastdiv & 2);
    const RaySetup R = ray_setup<float, true>(P, bx, by, bz, px, py, pz);
    const uint32_t S = ray_steps(R.lim, R.step_len, R.inv_step, Q.cap);
    bool run = live && fin;
    if (run && S > 0u && !R.finite) {                     // the first step lands on NaN / inf: outside the window
        r_status = RQ_LEFT_WINDOW;
        run = false;
    }
    uint32_t j = 0;                                       // steps taken so far: the same in every lane
    unsigned long long alive = lanes(run && S > 0u);
    while (alive != 0ull) {
        float qx[RQ_DEPTH], qy[RQ_DEPTH], qz[RQ_DEPTH];
        bool nz = false;
#pragma unroll
        for (int d = 0; d < RQ_DEPTH; ++d) {
            px += R.incx; py += R.incy; pz += R.incz;     // gvom.py:1128-1132
            qx[d] = px; qy[d] = py; qz[d] = pz;
            // the integer lookup differs from the literal one only for a coordinate just below zero (window_voxel)
            nz |= (px < 0.0f && px > -1e-4f) || (py < 0.0f && py > -1e-4f) || (pz < 0.0f && pz > -1e-4f);
        }
        uint32_t L[RQ_DEPTH], T[RQ_DEPTH];
        int32_t vox[RQ_DEPTH];
        if (Q.lit || lanes(run && nz) != 0ull) rq_lookup<true, P2>(P, qx, qy, qz, L, T, vox);      // (wave-uniform)
        else rq_lookup<false, P2>(P, qx, qy, qz, L, T, vox);
        uint32_t tg[RQ_DEPTH];
        int32_t st[RQ_DEPTH];
#pragma unroll
        for (int d = 0; d < RQ_DEPTH; ++d) { tg[d] = ftags[T[d]]; st[d] = fstate[L[d]]; }
#pragma unroll
        for (int d = 0; d < RQ_DEPTH; ++d) {
            const uint32_t jj = j + (uint32_t)d + 1u;
            if (run && jj <= S) {
                const int32_t s = tg[d] == P.epoch ? st[d] : -1;            // a stale tile reads "never observed"
                const bool outside = vox[d] < 0;
                const bool unk = !outside && s == -1;
                r_unknown += unk ? 1 : 0;
                const bool stop = outside || s >= 0 || (unk && Q.unknown_blocks);
                if (stop) {
                    r_status = outside ? RQ_LEFT_WINDOW : (s >= 0 ? RQ_OCCUPIED : RQ_UNKNOWN);
                    r_steps = outside ? (int32_t)jj - 1 : (int32_t)jj;
                    r_vox = vox[d];
                    if (!outside) {
                        r_x = (float)((double)qx[d] * P.xy_res); r_y = (float)((double)qy[d] * P.xy_res); r_z = (float)((double)qz[d] * P.z_res);
                    }
                    run = false;
                }
            }
        }
        j += RQ_DEPTH;
        alive = lanes(run && j < S);
    }
    if (run) {                                            // S unstopped steps
        r_status = RQ_CLEAR; r_steps = (int32_t)S;
        if (Q.check_target) {                             // the end point's own voxel (gvom.py:1072-1080), literal form
            uint32_t wx, wy, wz;
            const bool in = rq_point_voxel(P, bx, by, bz, wx, wy, wz);
            uint32_t L, T;
            int32_t vox;
            rq_index<P2>(in, wx, wy, wz, (uint32_t)P.xy, (uint32_t)P.zs, (uint32_t)P.nseg, (uint32_t)P.om[0], (uint32_t)P.om[1], (uint32_t)P.om[2], L, T, vox);
            const uint32_t tg = ftags[T];
            const int32_t sv = fstate[L];
            const int32_t s = tg == P.epoch ? sv : -1;
            const bool unk = in && s == -1;
            r_unknown += unk ? 1 : 0;
            if (!in) r_status = RQ_LEFT_WINDOW;
            else if (s >= 0 || (unk && Q.unknown_blocks)) {
                r_status = s >= 0 ? RQ_OCCUPIED : RQ_UNKNOWN;
                r_steps = (int32_t)S + 1; r_vox = vox;
                r_x = bx; r_y = by; r_z = bz;
            }
        }
    }
    if (live) {
        const v4i r = {r_status, r_steps, r_vox, r_unknown};
        out[i] = r;
        RqPos q;
        q.x = r_x; q.y = r_y; q.z = r_z;
        *(RqPos *)(out_pos + 3 * i) = q;
    }
}

hipError_t gvom_launch_raycast(hipStream_t s, const ScanParams &P, const RayQuery &Q, const int32_t *fstate, const uint32_t *ftags,
                               int32_t *out4, float *out3)
{
    if (Q.n < 1 || P.xy <= 0 || P.zs <= 0) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((Q.n + RQ_BLOCK - 1) / RQ_BLOCK);
    const bool p2 = ((P.xy & (P.xy - 1)) | (P.zs & (P.zs - 1))) == 0;
    if (p2) hipLaunchKernelGGL(k_raycast<true>, dim3(blocks), dim3(RQ_BLOCK), 0, s, P, Q, fstate, ftags, (v4i *)out4, out3);
    else hipLaunchKernelGGL(k_raycast<false>, dim3(blocks), dim3(RQ_BLOCK), 0, s, P, Q, fstate, ftags, (v4i *)out4, out3);
    return hipGetLastError();
}
