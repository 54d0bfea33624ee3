// gvom_viewpoint.hip -- viewpoint scoring (gvom_score_viewpoints; include/gvom_hip.h "viewpoint scoring" defines the result): how many
// never-observed voxels the handle's sensor would see from each of K poses (gfx950, wave64).
//
//   k_viewpoints      one beam per lane, one viewpoint per blockIdx.y.  The beam's end point is computed in registers from the sensor
//                     model (k_unproject's float64 arithmetic with r = max_range) and the ray is walked exactly as k_raycast walks it
//                     (gvom_raywalk.h, gvom_ray.h).  A never-observed voxel a beam examines sets its bit in the viewpoint's bitmap; the
//                     lane that finds the bit clear counts it.  READ-ONLY on the map.
//   k_viewpoint_best  one workgroup: the status of every viewpoint's own voxel, the rows of invalid poses, the best viewpoint.
//
// Numerics as in gvom_query.hip: -ffp-contract=off, IEEE division / sqrt, every operation rounded once.  Everything that leaves is an
// integer sum or a bit-OR: the product does not depend on the order in which waves run.
#include "gvom_device.h"
#include "gvom_ray.h"
#include "gvom_raywalk.h"

#define VP_BLOCK 256
#define VP_WAVES (VP_BLOCK / WAVE)

// A wave is 64 consecutive selected columns of one selected row of the model: its beams point almost the same way, share cache
// lines of the map and words of the bitmap, and finish together.  The step body is k_raycast's: a round computes RQ_DEPTH positions,
// issues their tile-tag and state loads together and examines them in step order.  Per wave: ballots and population counts of the
// beam endings, wave sums of the counts, at most seven int32 atomic adds into the viewpoint's row.  No LDS, no float atomics, no wait
// on another workgroup; every loop is bounded by S <= xy + z + 1.
template <bool P2>
__global__ __launch_bounds__(VP_BLOCK) void k_viewpoints(const ScanParams P, const ViewQuery Q, const int32_t *__restrict__ fstate,
                                                         const uint32_t *__restrict__ ftags, uint32_t *__restrict__ bitmaps,
                                                         int32_t *__restrict__ rows)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gw = __builtin_amdgcn_readfirstlane(blockIdx.x * VP_WAVES + (threadIdx.x >> 6));
    const uint32_t hi = gw / Q.nwc, wi = (gw - hi * Q.nwc) * 64u + lane;
    if (hi >= Q.nh) return;                               // (the whole wave: the last workgroup's spare waves)
    const uint32_t k = Q.k0 + blockIdx.y;                 // < K: the grid's y extent is the batch
    double c[12];
    if (!rq_pose(Q.poses, k, c)) return;                  // an invalid pose: k_viewpoint_best writes its row
    const bool live = wi < Q.nw;
    // the beam's end point (include/gvom_hip.h "viewpoint scoring": k_unproject's arithmetic with r = max_range)
    double d[3] = {0.0, 0.0, 0.0}, o[3] = {0.0, 0.0, 0.0};
    if (live) {
        const size_t pix = (size_t)(hi * Q.stride_h) * Q.W + (size_t)wi * Q.stride_w;     // h < H and w < W: inside the model
#pragma unroll
        for (int e = 0; e < 3; ++e) { d[e] = Q.dir[3 * pix + e]; o[e] = Q.off[3 * pix + e]; }
    }
    double p[3], q[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const double m = Q.max_range * d[e];
        p[e] = m + o[e];
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const double m0 = p[0] * c[4 * e], m1 = p[1] * c[4 * e + 1], m2 = p[2] * c[4 * e + 2];
        q[e] = ((m0 + m1) + m2) + c[4 * e + 3];
    }
    const float ax = (float)c[3], ay = (float)c[7], az = (float)c[11];
    const float bx = (float)q[0], by = (float)q[1], bz = (float)q[2];
    const bool fin = fabsf(ax) < INFINITY && fabsf(ay) < INFINITY && fabsf(az) < INFINITY &&
                     fabsf(bx) < INFINITY && fabsf(by) < INFINITY && fabsf(bz) < INFINITY;
    int32_t r_status = RQ_INVALID, r_unknown = 0, r_first = 0;
    // ray set-up (gvom.py:1097-1126), as k_raycast
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
    uint32_t *const bm = bitmaps + (size_t)blockIdx.y * Q.bm_words;      // this viewpoint's bitmap: bit x + y * xy + z * xy * xy
    uint32_t j = 0;
    unsigned long long alive = lanes(run && S > 0u);
    while (alive != 0ull) {
        float qx[RQ_DEPTH], qy[RQ_DEPTH], qz[RQ_DEPTH];
        bool nz = false;
#pragma unroll
        for (int t = 0; t < RQ_DEPTH; ++t) {
            px += R.incx; py += R.incy; pz += R.incz;     // gvom.py:1128-1132
            qx[t] = px; qy[t] = py; qz[t] = pz;
            nz |= (px < 0.0f && px > -1e-4f) || (py < 0.0f && py > -1e-4f) || (pz < 0.0f && pz > -1e-4f);
        }
        uint32_t L[RQ_DEPTH], T[RQ_DEPTH];
        int32_t vox[RQ_DEPTH];
        if (Q.lit || lanes(run && nz) != 0ull) rq_lookup<true, P2>(P, qx, qy, qz, L, T, vox);      // (wave-uniform)
        else rq_lookup<false, P2>(P, qx, qy, qz, L, T, vox);
        uint32_t tg[RQ_DEPTH];
        int32_t st[RQ_DEPTH];
#pragma unroll
        for (int t = 0; t < RQ_DEPTH; ++t) { tg[t] = ftags[T[t]]; st[t] = fstate[L[t]]; }
#pragma unroll
        for (int t = 0; t < RQ_DEPTH; ++t) {
            const uint32_t jj = j + (uint32_t)t + 1u;
            if (run && jj <= S) {
                const int32_t s = tg[t] == P.epoch ? st[t] : -1;            // a stale tile reads "never observed"
                const bool outside = vox[t] < 0;
                const bool unk = !outside && s == -1;
                if (unk) {                                                  // 0 <= vox < xy * xy * z: inside the bitmap
                    const uint32_t bit = 1u << ((uint32_t)vox[t] & 31u);
                    const uint32_t old = atomicOr(bm + ((uint32_t)vox[t] >> 5), bit);
                    r_unknown += 1;
                    r_first += (old & bit) ? 0 : 1;                         // exactly one lane finds the bit clear
                }
                if (outside || s >= 0 || (unk && Q.unknown_blocks)) {
                    r_status = outside ? RQ_LEFT_WINDOW : (s >= 0 ? RQ_OCCUPIED : RQ_UNKNOWN);
                    run = false;
                }
            }
        }
        j += RQ_DEPTH;
        alive = lanes(run && j < S);
    }
    if (run) r_status = RQ_CLEAR;                         // S unstopped steps
    rq_census(live ? r_status : -1, r_unknown, r_first, lane, rows + (size_t)k * 8);
}

// Column 0 of every row: the GVOM_RAY_* code of the viewpoint's own voxel floor((double)a / res - W) (the literal float64 lookup), the
// whole row of an invalid pose, and part 1 = {best, gain[best], K, nb}: the lowest index of the largest gain among the rows whose
// status is CLEAR, as one unsigned 64-bit maximum over ((gain + 1) << 32) | ~k.  One workgroup, behind the last batch.
template <bool P2>
__global__ __launch_bounds__(VP_BLOCK) void k_viewpoint_best(const ScanParams P, const ViewQuery Q, const int32_t *__restrict__ fstate,
                                                             const uint32_t *__restrict__ ftags, int32_t *__restrict__ rows,
                                                             int32_t *__restrict__ best)
{
    unsigned long long key = 0ull;
    for (uint32_t k = threadIdx.x; k < (uint32_t)Q.K; k += VP_BLOCK) {
        double c[12];
        int32_t *row = rows + (size_t)k * 8;
        if (!rq_pose(Q.poses, k, c)) {
            const v4i lo = {RQ_INVALID, 0, 0, 0}, hi = {0, 0, 0, Q.nb};
            *(v4i *)row = lo; *(v4i *)(row + 4) = hi;
            continue;
        }
        uint32_t wx, wy, wz;
        const bool in = rq_point_voxel(P, (float)c[3], (float)c[7], (float)c[11], wx, wy, wz);
        uint32_t L, T;
        int32_t vox;
        rq_index<P2>(in, wx, wy, wz, (uint32_t)P.xy, (uint32_t)P.zs, (uint32_t)P.nseg, (uint32_t)P.om[0], (uint32_t)P.om[1], (uint32_t)P.om[2], L, T, vox);
        const uint32_t tg = ftags[T];
        const int32_t sv = fstate[L];
        const int32_t s = tg == P.epoch ? sv : -1;
        const int32_t status = !in ? RQ_LEFT_WINDOW : (s >= 0 ? RQ_OCCUPIED : (s == -1 ? RQ_UNKNOWN : RQ_CLEAR));
        row[0] = status;
        if (status == RQ_CLEAR) {
            const unsigned long long cand = ((unsigned long long)((uint32_t)row[1] + 1u) << 32) | (unsigned long long)(~k);
            key = cand > key ? cand : key;
        }
    }
    rq_best_store<VP_BLOCK>(key, Q, best);
}

hipError_t gvom_launch_viewpoints(hipStream_t s, const ScanParams &P, const ViewQuery &Q, int batch, const int32_t *fstate, const uint32_t *ftags,
                                  uint32_t *bitmaps, int32_t *rows)
{
    if (batch < 1 || batch > GVOM_VIEWPOINT_MAX_BATCH || Q.k0 < 0 || Q.k0 + batch > Q.K || Q.nh < 1 || Q.nw < 1 || Q.nwc < 1 || P.xy <= 0 || P.zs <= 0)
        return hipErrorInvalidValue;
    const unsigned waves = (unsigned)Q.nh * (unsigned)Q.nwc;
    const dim3 grid((waves + VP_WAVES - 1) / VP_WAVES, (unsigned)batch);
    const bool p2 = ((P.xy & (P.xy - 1)) | (P.zs & (P.zs - 1))) == 0;
    if (p2) hipLaunchKernelGGL(k_viewpoints<true>, grid, dim3(VP_BLOCK), 0, s, P, Q, fstate, ftags, bitmaps, rows);
    else hipLaunchKernelGGL(k_viewpoints<false>, grid, dim3(VP_BLOCK), 0, s, P, Q, fstate, ftags, bitmaps, rows);
    return hipGetLastError();
}

hipError_t gvom_launch_viewpoint_best(hipStream_t s, const ScanParams &P, const ViewQuery &Q, const int32_t *fstate, const uint32_t *ftags,
                                      int32_t *rows, int32_t *best)
{
    if (Q.K < 1 || P.xy <= 0 || P.zs <= 0) return hipErrorInvalidValue;
    const bool p2 = ((P.xy & (P.xy - 1)) | (P.zs & (P.zs - 1))) == 0;
    if (p2) hipLaunchKernelGGL(k_viewpoint_best<true>, dim3(1), dim3(VP_BLOCK), 0, s, P, Q, fstate, ftags, rows, best);
    else hipLaunchKernelGGL(k_viewpoint_best<false>, dim3(1), dim3(VP_BLOCK), 0, s, P, Q, fstate, ftags, rows, best);
    return hipGetLastError();
}
