// gvom_atlas_field.hip -- device kernels of the atlas fields (gvom_atlas_cost_to_go, gvom_atlas_field_window; include/gvom_hip.h
// "atlas fields" has the definition): the front ends that let the 2-D solver of gvom_costfield.hip run on the atlas's toroidal planes
// IN PLACE, and the crop that brings a part of the result back as a window-sized cost field.
//   k_atlas_clearance_rows   the row pass of the clearance transform (gvom_clearance_rows.h) over one row of the EXTENT: two coalesced
//                            runs of a storage row, the AND with A-1 gives the address; writes unwrapped uint16 row distances
//   k_atlas_travcost         the uint16 cost map of the extent, unwrapped, from the toroidal positive / negative / visibility /
//                            roughness planes and the unwrapped d2 (gvom_travcost.h has the cell rule)
//   k_atlas_field_window     n x n cells of a field's three planes into a cost field's; the outside values beyond the field's edge
// Everything between them -- k_clearance_cols, k_ctg_seed, k_ctg_relax, k_ctg_dirs -- runs unchanged at side A on unwrapped arrays,
// so the graph is the FLAT A x A grid: cells on opposite edges of the extent are neighbours in storage and nowhere else.  A workgroup
// is 4 waves, a wave one row, its lanes along x (as gvom_atlas.hip).  No LDS but the row pass's 64 masks, no scratch, nothing waits
// on another workgroup, no loop but the row pass's over at most 64 chunks.
#include "gvom_device.h"
#include "gvom_clearance_rows.h"
#include "gvom_travcost.h"

static constexpr int AF_ROWS = 4;                                  // rows (= waves) per workgroup

__global__ __launch_bounds__(256) void k_atlas_clearance_rows(const int32_t *__restrict__ pos, const int32_t *__restrict__ neg,
                                                              const double thr, const int A, const int px, const int py,
                                                              uint16_t *__restrict__ g)
{
    __shared__ unsigned long long s_mask[64];
    const int y = blockIdx.x;
    const size_t row = (size_t)((py + y) & (A - 1)) * A;
    clearance_row([&](int x) {
        const size_t c = row + ((px + x) & (A - 1));
        bool ob = (double)pos[c] > thr;
        if (neg) ob = ob || neg[c] > 0;
        return ob;
    }, A, A, g + (size_t)y * A, s_mask);
}

__global__ __launch_bounds__(64 * AF_ROWS) void k_atlas_travcost(const int32_t *__restrict__ pos, const int32_t *__restrict__ neg,
                                                                 const int32_t *__restrict__ vis, const double *__restrict__ rough,
                                                                 const int32_t *__restrict__ d2, const TravParams P, const int A,
                                                                 const int px, const int py, uint16_t *__restrict__ c)
{
    const int x = (int)blockIdx.x * 64 + (int)threadIdx.x, y = (int)blockIdx.y * AF_ROWS + (int)threadIdx.y;
    if (x >= A || y >= A) return;
    const size_t s = (size_t)((py + y) & (A - 1)) * A + ((px + x) & (A - 1)), u = (size_t)y * A + x;
    c[u] = trav_cell<true>(P, pos, neg, vis, rough, d2, s, u);
}

// D is stored as dwords; the uint8 and uint16 planes of a window whose side is odd have rows that start at any byte, so they go
// element by element (3 of the 7 bytes a cell has, of a window-sized array)
__global__ __launch_bounds__(64 * AF_ROWS) void k_atlas_field_window(const int32_t *__restrict__ fD, const uint8_t *__restrict__ fdir,
                                                                     const uint16_t *__restrict__ fc, const int A, const int n,
                                                                     const int rx, const int ry, int32_t *__restrict__ oD,
                                                                     uint8_t *__restrict__ odir, uint16_t *__restrict__ oc)
{
    const int x = (int)blockIdx.x * 64 + (int)threadIdx.x, y = (int)blockIdx.y * AF_ROWS + (int)threadIdx.y;
    if (x >= n || y >= n) return;
    const bool inside = (unsigned)(rx + x) < (unsigned)A && (unsigned)(ry + y) < (unsigned)A;
    const size_t s = inside ? (size_t)(ry + y) * A + (rx + x) : 0, o = (size_t)y * n + x;
    oD[o] = inside ? fD[s] : INT32_MAX;                            // (GVOM_CTG_UNREACHED)
    odir[o] = inside ? fdir[s] : (uint8_t)255;                     // (GVOM_CTG_NONE)
    oc[o] = inside ? fc[s] : (uint16_t)0;
}

static bool af_size_ok(int A) { return A >= GVOM_ATLAS_MIN_CELLS && A <= GVOM_ATLAS_MAX_CELLS && (A & (A - 1)) == 0; }
static dim3 af_grid(int n) { return dim3((unsigned)((n + 63) / 64), (unsigned)((n + AF_ROWS - 1) / AF_ROWS)); }

// the planes of the atlas these kernels read (gvom_internal.h "map atlas"): roughness is the first f64 plane, the i32 planes follow the six
struct AfPlanes { const int32_t *pos, *neg, *vis; const double *rough; };
static AfPlanes af_planes(const char *atlas, int A)
{
    const size_t n2 = (size_t)A * A;
    const int32_t *ints = (const int32_t *)((const double *)atlas + 6 * n2);
    return AfPlanes{ints, ints + n2, ints + 2 * n2, (const double *)atlas};
}

hipError_t gvom_launch_atlas_clearance_rows(hipStream_t s, const char *atlas, int A, int px, int py, bool use_negative, double thr,
                                            uint16_t *g)
{
    if (!atlas || !g || !af_size_ok(A) || px < 0 || px >= A || py < 0 || py >= A) return hipErrorInvalidValue;
    const AfPlanes P = af_planes(atlas, A);
    hipLaunchKernelGGL(k_atlas_clearance_rows, dim3(A), dim3(256), 0, s, P.pos, use_negative ? P.neg : nullptr, thr, A, px, py, g);
    return hipGetLastError();
}

hipError_t gvom_launch_atlas_travcost(hipStream_t s, const char *atlas, int A, int px, int py, const int32_t *d2, const CtgCostParams &C,
                                      uint16_t *c)
{
    if (!atlas || !c || !af_size_ok(A) || px < 0 || px >= A || py < 0 || py >= A) return hipErrorInvalidValue;
    TravParams T;
    T.thr = C.density_threshold; T.rmin = C.min_roughness; T.rmax = C.max_roughness;
    T.infl2 = d2 ? C.inflation_cells2 : 0; T.base = C.base; T.soft = C.soft_weight; T.unknown = C.unknown_cost; T.rough = C.rough_weight;
    T.use_neg = C.use_negative; T.unknown_blocks = C.unknown_blocks;
    const AfPlanes P = af_planes(atlas, A);
    hipLaunchKernelGGL(k_atlas_travcost, af_grid(A), dim3(64, AF_ROWS), 0, s, P.pos, P.neg, P.vis, P.rough, d2, T, A, px, py, c);
    return hipGetLastError();
}

// |rx|, |ry| <= 2^30 and n <= 4096: rx + x cannot overflow
hipError_t gvom_launch_atlas_field_window(hipStream_t s, int A, const int32_t *fD, const uint8_t *fdir, const uint16_t *fc, int n, int rx,
                                          int ry, int32_t *oD, uint8_t *odir, uint16_t *oc)
{
    const int lim = 1 << 30;
    if (!fD || !fdir || !fc || !oD || !odir || !oc || !af_size_ok(A) || n < 1 || n > GVOM_ATLAS_MAX_CELLS || rx < -lim || rx > lim ||
        ry < -lim || ry > lim)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_atlas_field_window, af_grid(n), dim3(64, AF_ROWS), 0, s, fD, fdir, fc, A, n, rx, ry, oD, odir, oc);
    return hipGetLastError();
}
