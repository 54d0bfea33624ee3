// gvom_ray.h -- the reference's ray arithmetic (gvom.py:1093-1150), shared by the kernels that walk rays through the window:
// k_trace (gvom_trace.hip), which adds a ray pass to every voxel it visits, and k_raycast (gvom_query.hip), which reads the
// fused state of the same voxels.  One definition: a query's ray visits exactly the voxels the mapper's ray marks.
//   div_by_res     (double)x / resolution of a float32 coordinate, bit for bit, without the divide
//   window_voxel   window voxel of a ray position and the inside test (integer or literal float64 form)
//   ray_setup      per-step increments, step length and length limit of one ray
//   ray_steps      how many steps the reference's loop test lets the ray take
#ifndef GVOM_RAY_H
#define GVOM_RAY_H
#include "gvom_device.h"

// Window voxel of a ray position (gvom.py:1121-1144: floor((f64)p - origin), inside test).
// LIT = false: the window origin is an integer (gvom.py:124-126 floors it), so
// floor((double)p - origin) == (int)floorf(p) - origin -- no f64 in the lookup.  The f64 subtraction
// rounds across an integer only when p lies within half an f64 ulp BELOW an integer, which an f32 p
// can only do just below 0 (|p| < 2^-23, given |origin| < 2^30, which the host checks before selecting
// the integer form); callers use LIT = true (the reference's literal f64 expression) wherever a
// coordinate may come that close to zero, and always when |origin| >= 2^30.
// Returns "inside the window"; wx/wy/wz are only meaningful then.
// (o0..o2, uxy, zpad: the integer form's wave-uniform constants -- (int)origin, xy, xy - zs -- handed in by walk_steps,
// which pins them in scalar registers across its loop; the literal form reads P)
template <bool LIT>
__device__ __forceinline__ bool window_voxel(const ScanParams &P, float px, float py, float pz,
                                             uint32_t &wx, uint32_t &wy, uint32_t &wz,
                                             uint32_t o0 = 0, uint32_t o1 = 0, uint32_t o2 = 0, uint32_t uxy_ = 0, uint32_t zpad = 0)
{
    if (LIT) {
        const double fx = floor((double)px - P.origin[0]);
        const double fy = floor((double)py - P.origin[1]);
        const double fz = floor((double)pz - P.origin[2]);
        const bool in = fx >= 0.0 && fx < (double)P.xy && fy >= 0.0 && fy < (double)P.xy && fz >= 0.0 && fz < (double)P.zs;
        wx = in ? (uint32_t)(int)fx : 0u; wy = in ? (uint32_t)(int)fy : 0u; wz = in ? (uint32_t)(int)fz : 0u;
        return in;
    }
    wx = (uint32_t)cvt_floor_i32(px) - o0;
    wy = (uint32_t)cvt_floor_i32(py) - o1;
    wz = (uint32_t)cvt_floor_i32(pz) - o2;
    // ONE compare for the three axes (its result is the lane mask the step body needs, no boolean to
    // re-materialise): z is padded up to the xy bound with a saturating add ("negative" differences are
    // huge unsigned values and stay huge).  Requires z_size <= xy_size: callers take the literal form for
    // grids taller than wide.
    return max(max(wx, wy), __builtin_elementwise_add_sat(wz, zpad)) < uxy_;
}
// Number of DDA steps the reference's length test lets a ray take (gvom.py:1127,1149):
//   length_0 = 0, length_j = fl(length_{j-1} + step_len) in f64; step j runs iff length_{j-1} < lim,
// i.e. n = the smallest j with length_j >= lim (0 if lim <= 0), capped at `cap` + 1 (callers only need
// to know "more than cap").  The accumulated sum differs from j * step_len by at most j^2 * step_len *
// 2^-53, so n = ceil(lim / step_len) unless lim lies within that band of a multiple of step_len; only
// then (probability ~1e-12 per ray) the sum is accumulated literally.
__device__ __forceinline__ uint32_t ray_steps(double lim, double step_len, double inv_step, uint32_t cap)
{
    if (!(0.0 < lim)) return 0u;
    const double q = lim * inv_step;                      // ~ lim / step_len (inv_step ~ 1 / step_len: any error is caught by the band test)
    if (!(q < (double)cap + 2.0)) return cap + 1u;                        // also inf / NaN quotients: literal path below never needed
    const double jc = ceil(q);
    const double e = (jc * jc) * step_len * 0x1p-51 + step_len * 0x1p-50;
    const double lo = (jc - 1.0) * step_len, hi = jc * step_len;
    if (lo + e < lim && hi - e >= lim) return (uint32_t)jc;
    uint32_t n = 0;
    double length = 0.0;
    while (length < lim && n <= cap) { length += step_len; ++n; }
    return n;
}

// (double)x / d for a FLOAT32 coordinate x and a wave-uniform divisor d (xy_res, z_res), bit for bit, without the divide
// (an IEEE f64 division is ~15 instructions on gfx950: v_div_scale x2, v_rcp_f64, four Newton v_fma_f64, v_div_fmas,
// v_div_fixup ...): with r = RN(1 / d) from the host, q = x * r is within an ulp of the quotient, e = fma(-q, d, x) is its
// EXACT residual and fma(e, r, q) the correctly rounded quotient (Markstein's correction step).  Whether that holds for a
// given d is not taken from a theorem but CHECKED: rounding depends on the significands only (scaling x by a power of two
// scales q, e and the result exactly; no float32 x brings any of them near the ends of the f64 range for 2^-64 < d < 2^64), and
// a float32 has 2^23 significands -- gvom_create tries them all against the divide (verify_fastdiv, once per divisor and
// process) and clears the bit in P.fastdiv if one differs.  Zeros and non-finite x keep x * r, which is the quotient there
// (signed zero, inf, NaN).  Explicit fma() calls are not subject to -ffp-contract=off.  T = double (clouds handed over in
// float64): the IEEE divide, always.
template <typename T>
__device__ __forceinline__ double div_by_res(T x, double d, double r, bool fast)
{
    if (sizeof(T) == 4 && fast) {
        const double xd = (double)x;
        const double q = xd * r;
        const double e = __builtin_fma(-q, d, xd);
        const double q2 = __builtin_fma(e, r, q);
        return (fabs(xd) < INFINITY && xd != 0.0) ? q2 : q;
    }
    return (double)x / d;
}

// Ray set-up of one return (gvom.py:1093-1118): per-step increments in natural (x, y, z) order, the
// f64 step length and the length limit of the reference's loop test.
struct RaySetup { float incx, incy, incz; double step_len, inv_step, lim; bool finite; };
// (MO: the ray starts at the lane's own (o0, o1, o2) -- its row of the origin table, trace_item -- instead of at ScanParams::pt0)
template <typename T, bool MO>
__device__ __forceinline__ RaySetup ray_setup(const ScanParams &P, T x, T y, T z, float o0, float o1, float o2)
{
    const float e0 = (float)div_by_res<T>(x, P.xy_res, P.drcp[0], P.fastdiv & 1);
    const float e1 = (float)div_by_res<T>(y, P.xy_res, P.drcp[0], P.fastdiv & 1);
    const float e2 = (float)div_by_res<T>(z, P.z_res, P.drcp[1], P.fastdiv & 2);
    float s0 = e0 - (MO ? o0 : P.pt0[0]), s1 = e1 - (MO ? o1 : P.pt0[1]), s2 = e2 - (MO ? o2 : P.pt0[2]);
    const float ss = (s0 * s0 + s1 * s1) + s2 * s2;
    // math.sqrt -> f64; GVOM_FLAG_CUDA_F32_SQRT: sqrt of the f32 sum in f32, as real
    // Numba-CUDA types it (gvom.py:1109-1114)
    const double ray_length = P.f32_sqrt ? (double)sqrtf(ss) : sqrt((double)ss);
    s0 = (float)((double)s0 / ray_length);
    s1 = (float)((double)s1 / ray_length);
    s2 = (float)((double)s2 / ray_length);
    const float a0 = fabsf(s0), a1 = fabsf(s1), a2 = fabsf(s2);
    const float smax = py_maxf(a0, py_maxf(a1, a2));
    int si = 0;
    if (smax == a1) si = 1;
    if (smax == a2) si = 2;                              // ties: z over y over x
    const float sd  = si == 0 ? s0 : (si == 1 ? s1 : s2);
    const float so1 = si == 0 ? s1 : (si == 1 ? s2 : s0);
    const float so2 = si == 0 ? s2 : (si == 1 ? s0 : s1);
    const float adom = fabsf(sd);
    const float dir = sd / adom;
    const float inc1 = so1 / adom;
    const float inc2 = so2 / adom;
    const double step_len = fabs(1.0 / (double)sd);
    const double lim = ray_length - 1.0;
    // natural (x, y, z) order: the same three f32 additions per step as the reference's
    // (dominant, other, other) triple, without the axis permutation
    const float incx = si == 0 ? dir : (si == 1 ? inc2 : inc1);
    const float incy = si == 0 ? inc1 : (si == 1 ? dir : inc2);
    const float incz = si == 0 ? inc2 : (si == 1 ? inc1 : dir);
    // non-finite increments (degenerate returns): the reference's first step lands on NaN/inf,
    // which is outside the grid, and the ray ends without an update
    const bool finite = fabsf(incx) < INFINITY && fabsf(incy) < INFINITY && fabsf(incz) < INFINITY;
    RaySetup R;
    R.incx = incx; R.incy = incy; R.incz = incz; R.step_len = step_len; R.inv_step = fabs((double)sd); R.lim = lim; R.finite = finite;
    return R;
}

#endif  // GVOM_RAY_H
