// gvom_ingest.hip -- range-image ingest: the organised scan of a spinning multi-beam lidar (H beams x W columns of raw
// ranges, 0 = no return) unprojected into the handle's staging cloud, in front of the unchanged scan kernels.
//
// Arithmetic (include/gvom_hip.h "range images", normative): float64, every operation rounded once, in this order
//   r = (double)raw * scale;  p[k] = r * dir[k] + off[k];  q[k] = ((p0 * C[4k] + p1 * C[4k+1]) + p2 * C[4k+2]) + C[4k+3]
// and ONE rounding to the cloud type at the end.  The library is built with -ffp-contract=off and nothing here asks for a
// fused multiply-add, so a numpy restatement (gvom.unproject_range_image) gives the same bits.
//
// Memory: one pixel per lane, consecutive lanes = consecutive pixels of a row.  dir / off / the output are 24-byte (or
// 12-byte) records: a lane reading "its" record would make every load instruction a strided pass over three times the
// lines it uses.  A workgroup's 256 records are one contiguous run instead, so it is moved as such -- lane t takes
// elements t, t + 256, t + 512 of the run (full 8-byte-per-lane rows) -- and the records are re-dealt through LDS.  A
// column's pose is 96 bytes shared by the H pixels of the column: a lane fetches it once, as six 16-byte loads into
// registers, for all three components.
#include "gvom_ingest.h"
#include "gvom_device.h"
#include "../../include/gvom_hip.h"

namespace {

typedef double v2d __attribute__((ext_vector_type(2)));
#define UB GVOM_UNPROJECT_BLOCK

// the workgroup's records, re-dealt in LDS (element e of the run), to global memory in 8-byte units
__device__ __forceinline__ void store_run(double *g, const double *s, uint32_t t, uint32_t cnt)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t e = t + UB * k;
        if (e < cnt) g[e] = s[e];
    }
}
__device__ __forceinline__ void store_run(float *g, const float *s, uint32_t t, uint32_t cnt)
{
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const uint32_t e = 2 * (t + UB * k);               // 3 * UB floats = 1.5 * UB pairs
        if (e + 1 < cnt) *(v2f *)(g + e) = *(const v2f *)(s + e);
        else if (e < cnt) g[e] = s[e];                     // (an odd number of pixels in the image's last workgroup)
    }
}

template <typename R, typename T>
__global__ __launch_bounds__(UB) void k_unproject(const UnprojectParams P)
{
    __shared__ __attribute__((aligned(16))) double s_dir[3 * UB], s_off[3 * UB];
    __shared__ __attribute__((aligned(16))) T s_out[3 * UB];
    const uint32_t t = threadIdx.x;
    const uint32_t i0 = blockIdx.x * UB;                   // (n < 2^31: no overflow)
    const uint32_t i = i0 + t;
    const uint32_t pixels = P.n - i0 < UB ? P.n - i0 : UB;
    const uint32_t cnt = 3 * pixels;                       // elements of this workgroup's run of records
    const bool live = t < pixels;
    {
        const double *gd = P.dir + (size_t)i0 * 3, *go = P.off + (size_t)i0 * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t e = t + UB * k;
            if (e < cnt) { s_dir[e] = gd[e]; s_off[e] = go[e]; }
        }
    }
    const uint32_t h = live ? i / P.W : 0u, w = live ? i - h * P.W : 0u;
    R raw = (R)0;
    if (live) raw = *(const R *)((const char *)P.raw + (size_t)h * P.row_stride + (size_t)w * sizeof(R));
    v2d c[6];
    const bool posed = P.poses != nullptr;                 // (uniform)
    if (posed && live) {
        const v2d *pc = (const v2d *)(P.poses + (size_t)w * 12);
#pragma unroll
        for (int k = 0; k < 6; ++k) c[k] = pc[k];
    }
    __syncthreads();
    if (live) {
        const double r = (double)raw * P.scale;
        const bool valid = raw != (R)0 && __builtin_isfinite(r) && P.min_range <= r && r <= P.max_range;
        double p[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double m = r * s_dir[3 * t + k];
            p[k] = m + s_off[3 * t + k];
        }
        double q[3] = {p[0], p[1], p[2]};
        if (posed) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const v2d a = c[2 * k], b = c[2 * k + 1];   // row k of the 3x4: a = {C[4k], C[4k+1]}, b = {C[4k+2], C[4k+3]}
                const double m0 = p[0] * a.x, m1 = p[1] * a.y, m2 = p[2] * b.x;
                q[k] = ((m0 + m1) + m2) + b.y;
            }
        }
        const double nan = __builtin_nan("");
#pragma unroll
        for (int k = 0; k < 3; ++k) s_out[3 * t + k] = (T)(valid ? q[k] : nan);
    }
    __syncthreads();
    store_run((T *)P.out + (size_t)i0 * 3, s_out, t, cnt);
}

template <typename R>
hipError_t launch_r(hipStream_t s, const UnprojectParams &P, int cloud_dtype, unsigned blocks)
{
    if (cloud_dtype == GVOM_DTYPE_F32) hipLaunchKernelGGL((k_unproject<R, float>), dim3(blocks), dim3(UB), 0, s, P);
    else hipLaunchKernelGGL((k_unproject<R, double>), dim3(blocks), dim3(UB), 0, s, P);
    return hipGetLastError();
}

}  // namespace

hipError_t gvom_launch_unproject(hipStream_t s, const UnprojectParams &P, int range_dtype, int cloud_dtype)
{
    if (P.n == 0 || P.W == 0 || P.n >= 0x80000000u) return hipErrorInvalidValue;
    if (cloud_dtype != GVOM_DTYPE_F32 && cloud_dtype != GVOM_DTYPE_F64) return hipErrorInvalidValue;
    const unsigned blocks = (P.n + UB - 1) / UB;
    switch (range_dtype) {
    case GVOM_RANGE_U16: return launch_r<uint16_t>(s, P, cloud_dtype, blocks);
    case GVOM_RANGE_U32: return launch_r<uint32_t>(s, P, cloud_dtype, blocks);
    case GVOM_RANGE_F32: return launch_r<float>(s, P, cloud_dtype, blocks);
    }
    return hipErrorInvalidValue;
}
