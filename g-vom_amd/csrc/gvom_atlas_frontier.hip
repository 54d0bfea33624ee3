// gvom_atlas_frontier.hip -- the one device kernel of the atlas frontiers (gvom_atlas_frontiers; include/gvom_hip.h "atlas frontiers" has
// the definition): the marking pass of gvom_frontier.hip on an atlas FIELD's unwrapped cost map and cost to go, with the visibility read
// IN PLACE from the atlas's toroidal plane as the atlas is now.
//   k_atlas_frontier_mark   L = own index at a frontier cell of the field's frame, NONE elsewhere; count = 0; a flag per 32 x 32 tile
// Everything behind it -- k_frontier_relax, _count, _rank, _rows, _stats -- runs unchanged at the field's side on the flat grid.
// Field cell (x, y) is extent cell (ox + x, oy + y) of the atlas's present extent, (ox, oy) = the field's origin minus the extent's,
// clamped like a window's offset; inside the extent its visibility lies at [((py + oy + y) & (A-1)) * A + ((px + ox + x) & (A-1))], (px,
// py) the extent's storage phase.  A wave is 64 cells of one field row: c and D are read coalesced from the unwrapped field; its own,
// east and west visibility come from one storage row in at most two coalesced runs (the AND wraps once at most, as in
// k_atlas_clearance_rows), north and south from one storage row each.  A cell outside the extent is neither known nor unknown: it is
// no frontier cell and makes none.  The ballot-to-tile flags and the wave-combined counter are k_frontier_mark's.  No scratch, no LDS
// beyond the 4-word block sum, no loop, nothing waits on another workgroup.
#include "gvom_device.h"

#define AFR_T 32                       // cells per tile side (FR_T, gvom_frontier.hip: k_frontier_relax reads these flags)
#define AFR_NONE 0xffffffffu           // label of a cell that is no frontier cell (FR_NONE)
#define AFR_UNREACHED 0x7fffffff       // (GVOM_CTG_UNREACHED)

// k_frontier_mark's job written out: sharing its cell rule through a header with the visibility lookup as a functor changed
// k_frontier_mark's registers and code size, so that kernel stays as it is and this one repeats the rule.
__global__ __launch_bounds__(256) void k_atlas_frontier_mark(const int xy, const uint16_t *__restrict__ c, const int32_t *__restrict__ D,
                                                             const int32_t *__restrict__ vis, const int A, const int ox, const int oy,
                                                             const int px, const int py, uint32_t *__restrict__ L,
                                                             uint32_t *__restrict__ count, uint32_t *__restrict__ flags,
                                                             uint32_t *__restrict__ n_frontier)
{
    __shared__ uint32_t s4[4];
    // cell (x, y) of a 256-thread workgroup that covers 4 rows of 64 cells: a wave owns a row segment
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const bool in = x < xy && y < xy;
    const size_t u = (size_t)y * xy + x;
    // field cell (fx, fy): 1 KNOWN, 0 UNKNOWN, -1 outside the atlas's present extent (nothing is read there)
    auto state = [&](int fx, int fy) {
        const int ex = ox + fx, ey = oy + fy;
        if ((unsigned)ex >= (unsigned)A || (unsigned)ey >= (unsigned)A) return -1;
        return vis[(size_t)((py + ey) & (A - 1)) * A + ((px + ex) & (A - 1))] > 0 ? 1 : 0;
    };
    bool f = false;
    if (in) {
        f = c[u] > 0 && D[u] < AFR_UNREACHED && state(x, y) == 1;
        if (f) {                                                       // east / west: the wave's own storage row again (cached); north / south: a row each
            bool open = x > 0 && state(x - 1, y) == 0;
            open = open || (x + 1 < xy && state(x + 1, y) == 0);
            open = open || (y > 0 && state(x, y - 1) == 0);
            open = open || (y + 1 < xy && state(x, y + 1) == 0);
            f = open;
        }
        L[u] = f ? (uint32_t)u : AFR_NONE;
        count[u] = 0u;
    }
    const unsigned long long m = __ballot(f);
    const int lane = threadIdx.x & 63;
    if (m) {                                                           // the wave's segment lies in at most two tiles
        const int ntx = (xy + AFR_T - 1) / AFR_T;
        if ((lane == 0 && (m & 0xffffffffull)) || (lane == 32 && (m >> 32))) flags[(y / AFR_T) * ntx + x / AFR_T] = 1u;   // (a set bit is a cell inside the field)
    }
    // the workgroup's frontier cells, added to *n_frontier once
    const uint32_t n = (uint32_t)__popcll(m);
    if (lane == 0) s4[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) { const uint32_t t = s4[0] + s4[1] + s4[2] + s4[3]; if (t) atomicAdd(n_frontier, t); }
}

// |ox|, |oy| <= 2^30 and xy <= 4096: ox + x cannot overflow; 0 <= px, py < A
hipError_t gvom_launch_atlas_frontier_mark(hipStream_t s, int xy, const uint16_t *c, const int32_t *D, const char *atlas, int A, int ox,
                                           int oy, int px, int py, uint32_t *L, uint32_t *count, uint32_t *flags, uint32_t *n_frontier)
{
    const int lim = 1 << 30;
    const auto side_ok = [](int n) { return n >= GVOM_ATLAS_MIN_CELLS && n <= GVOM_ATLAS_MAX_CELLS && (n & (n - 1)) == 0; };
    if (!c || !D || !atlas || !L || !count || !flags || !n_frontier || !side_ok(xy) || !side_ok(A) || ox < -lim || ox > lim || oy < -lim ||
        oy > lim || px < 0 || px >= A || py < 0 || py >= A)
        return hipErrorInvalidValue;
    // the visibility plane (gvom_internal.h "map atlas"): the third int32 plane behind the six f64 planes
    const size_t a2 = (size_t)A * A;
    const int32_t *vis = (const int32_t *)((const double *)atlas + 6 * a2) + 2 * a2;
    hipLaunchKernelGGL(k_atlas_frontier_mark, dim3((xy + 63) / 64, (xy + 3) / 4), dim3(256), 0, s, xy, c, D, vis, A, ox, oy, px, py, L, count,
                       flags, n_frontier);
    return hipGetLastError();
}
