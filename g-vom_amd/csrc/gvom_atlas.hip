// gvom_atlas.hip -- the map atlas (include/gvom_hip.h "map atlas" defines the result; gvom_internal.h has the storage and the
// launchers' contracts): k_atlas_fill, k_atlas_move, k_atlas_merge, k_atlas_recall.  Four copy kernels: a workgroup is 4 waves, one
// wave per row of the window and its 64 lanes along x, so that a row is read and written in coalesced runs -- two where it crosses
// the storage seam, which the AND with A-1 gives without a division.  No LDS, no scratch, nothing waits on another workgroup.  The
// f64 maps travel as 64-bit integers: a copy keeps every bit pattern, NaN payloads included.  Counters are integer sums of a wave's
// ballots, one atomic per wave and counter: exact, whatever the schedule.
#include "gvom_internal.h"

static constexpr int ATL_ROWS = 4;                                 // rows (= waves) per workgroup

// the bit patterns of the UNKNOWN cell's f64 values (maps 3 .. 8): roughness -1.0, height and inferred height -1000.0, the rest +0.0
static __device__ __forceinline__ unsigned long long atl_unknown_f(int k)
{
    return k == 0 ? 0xBFF0000000000000ull : (k <= 2 ? 0xC08F400000000000ull : 0ull);
}

// 2 observed, 1 inferred, 0 nothing -- from the three values that decide it
static __device__ __forceinline__ int atl_rank(int32_t vis, int32_t neg, unsigned long long inferred)
{
    if (vis > 0) return 2;
    return (neg > 0 || __longlong_as_double((long long)inferred) > -1000.0) ? 1 : 0;
}

// the whole wave arrives here (no lane has left): one add of the lanes that hold `p`
static __device__ __forceinline__ void atl_count(bool p, int32_t *c, int by = 1)
{
    const unsigned long long m = __ballot(p);
    if (threadIdx.x == 0 && m != 0ull) atomicAdd(c, by * (int)__popcll(m));
}

struct AtlasPlanes {
    unsigned long long *f[6];
    int32_t *i[3];
    int32_t *stamp;
};
static __host__ __device__ __forceinline__ AtlasPlanes atl_planes(char *atlas, int A)
{
    const size_t n2 = (size_t)A * A;
    AtlasPlanes P;
    for (int k = 0; k < 6; ++k) P.f[k] = (unsigned long long *)atlas + k * n2;
    int32_t *ints = (int32_t *)((unsigned long long *)atlas + 6 * n2);
    for (int k = 0; k < 3; ++k) P.i[k] = ints + k * n2;
    P.stamp = ints + 3 * n2;
    return P;
}

__global__ __launch_bounds__(256) void k_atlas_fill(AtlasPlanes P, size_t first, size_t n)
{
    for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (size_t)gridDim.x * blockDim.x) {
#pragma unroll
        for (int k = 0; k < 6; ++k) P.f[k][first + c] = atl_unknown_f(k);
#pragma unroll
        for (int k = 0; k < 3; ++k) P.i[k][first + c] = 0;
        P.stamp[first + c] = 0;
    }
}

// the rectangle of w x hgt cells whose first cell has the storage phase (px, py): cells that entered the extent
__global__ __launch_bounds__(64 * ATL_ROWS) void k_atlas_move(AtlasPlanes P, int A, int px, int py, int w, int hgt, int32_t *cnt)
{
    const int x = (int)blockIdx.x * 64 + (int)threadIdx.x, y = (int)blockIdx.y * ATL_ROWS + (int)threadIdx.y;
    const bool in = x < w && y < hgt;
    const size_t c = (size_t)((py + y) & (A - 1)) * A + ((px + x) & (A - 1));
    bool known = false;
    if (in) {
        known = atl_rank(P.i[2][c], P.i[1][c], P.f[2][c]) >= 1;
#pragma unroll
        for (int k = 0; k < 6; ++k) P.f[k][c] = atl_unknown_f(k);
#pragma unroll
        for (int k = 0; k < 3; ++k) P.i[k][c] = 0;
        P.stamp[c] = 0;
    }
    atl_count(in, cnt + 4);
    atl_count(known, cnt + 5);
    atl_count(known, cnt + 6, -1);
}

__global__ __launch_bounds__(64 * ATL_ROWS) void k_atlas_merge(AtlasPlanes P, int A, AtlasMaps in, int n, int rx, int ry, int px, int py,
                                                               int32_t seq, int32_t *cnt)
{
    const int x = (int)blockIdx.x * 64 + (int)threadIdx.x, y = (int)blockIdx.y * ATL_ROWS + (int)threadIdx.y;
    const bool cell = x < n && y < n;
    const bool inside = cell && (unsigned)(rx + x) < (unsigned)A && (unsigned)(ry + y) < (unsigned)A;
    bool written = false, kept = false, fresh = false, nothing = false;
    if (inside) {
        const size_t s = (size_t)y * n + x;
        const size_t c = (size_t)((py + y) & (A - 1)) * A + ((px + x) & (A - 1));
        const int32_t vis = in.i[2][s], neg = in.i[1][s];
        const unsigned long long inf = in.f[2][s];
        const int r_new = atl_rank(vis, neg, inf);
        nothing = r_new == 0;
        if (r_new >= 1) {
            const int r_old = atl_rank(P.i[2][c], P.i[1][c], P.f[2][c]);     // the old cell: only what decides its rank
            written = r_new >= r_old;
            kept = !written;
            fresh = written && r_old == 0;
            if (written) {
                P.i[0][c] = in.i[0][s]; P.i[1][c] = neg; P.i[2][c] = vis;
                P.f[0][c] = in.f[0][s]; P.f[1][c] = in.f[1][s]; P.f[2][c] = inf;
                P.f[3][c] = in.f[3][s]; P.f[4][c] = in.f[4][s]; P.f[5][c] = in.f[5][s];
                P.stamp[c] = seq;
            }
        }
    }
    atl_count(written, cnt + 0);
    atl_count(kept, cnt + 1);
    atl_count(nothing, cnt + 2);
    atl_count(cell && !inside, cnt + 3);
    atl_count(fresh, cnt + 6);
}

// n x n cells from (rx, ry) relative to the extent on: the recall (a map set and its stamps) and the extent export (n = A, rx = ry = 0)
__global__ __launch_bounds__(64 * ATL_ROWS) void k_atlas_recall(AtlasPlanes P, int A, AtlasMaps out, int n, int rx, int ry, int px, int py,
                                                                int32_t seq, int32_t *counts)
{
    const int x = (int)blockIdx.x * 64 + (int)threadIdx.x, y = (int)blockIdx.y * ATL_ROWS + (int)threadIdx.y;
    const bool cell = x < n && y < n;
    const bool inside = cell && (unsigned)(rx + x) < (unsigned)A && (unsigned)(ry + y) < (unsigned)A;
    int rank = 0;
    if (cell) {
        const size_t s = (size_t)y * n + x;
        const size_t c = (size_t)((py + y) & (A - 1)) * A + ((px + x) & (A - 1));
        const int32_t vis = inside ? P.i[2][c] : 0, neg = inside ? P.i[1][c] : 0;
        const unsigned long long inf = inside ? P.f[2][c] : atl_unknown_f(2);
        rank = atl_rank(vis, neg, inf);
        if (out.i[0]) out.i[0][s] = inside ? P.i[0][c] : 0;
        if (out.i[1]) out.i[1][s] = neg;
        if (out.i[2]) out.i[2][s] = vis;
        if (out.f[2]) out.f[2][s] = inf;
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (k != 2 && out.f[k]) out.f[k][s] = inside ? P.f[k][c] : atl_unknown_f(k);
        if (out.stamp) out.stamp[s] = inside ? P.stamp[c] : 0;
    }
    if (counts) {
        atl_count(rank == 2, counts + 0);
        atl_count(rank == 1, counts + 1);
        atl_count(cell && !inside, counts + 2);
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0) counts[3] = seq;
    }
}

static bool atl_size_ok(int A) { return A >= GVOM_ATLAS_MIN_CELLS && A <= GVOM_ATLAS_MAX_CELLS && (A & (A - 1)) == 0; }
static dim3 atl_grid(int w, int hgt) { return dim3((unsigned)((w + 63) / 64), (unsigned)((hgt + ATL_ROWS - 1) / ATL_ROWS)); }

hipError_t gvom_launch_atlas_fill(hipStream_t s, char *atlas, int A, size_t first, size_t n)
{
    if (!atlas || !atl_size_ok(A) || first + n > (size_t)A * A) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_atlas_fill, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, s, atl_planes(atlas, A), first, n);
    return hipGetLastError();
}

hipError_t gvom_launch_atlas_move(hipStream_t s, char *atlas, int A, int px, int py, int w, int hgt, int32_t *cnt)
{
    if (!atlas || !cnt || !atl_size_ok(A) || w < 0 || w > A || hgt < 0 || hgt > A || px < 0 || px >= A || py < 0 || py >= A) return hipErrorInvalidValue;
    if (w == 0 || hgt == 0) return hipSuccess;
    hipLaunchKernelGGL(k_atlas_move, atl_grid(w, hgt), dim3(64, ATL_ROWS), 0, s, atl_planes(atlas, A), A, px, py, w, hgt, cnt);
    return hipGetLastError();
}

// |rx|, |ry| <= 2^30: rx + x cannot overflow; px, py in 0 .. A-1
static bool atl_window_ok(int A, int n, int rx, int ry, int px, int py)
{
    const int lim = 1 << 30;
    return atl_size_ok(A) && n >= 1 && n <= GVOM_ATLAS_MAX_CELLS && rx >= -lim && rx <= lim && ry >= -lim && ry <= lim && px >= 0 && px < A &&
           py >= 0 && py < A;
}

hipError_t gvom_launch_atlas_merge(hipStream_t s, char *atlas, int A, const AtlasMaps &in, int n, int rx, int ry, int px, int py,
                                   int32_t seq, int32_t *cnt)
{
    if (!atlas || !cnt || !atl_window_ok(A, n, rx, ry, px, py) || n > A) return hipErrorInvalidValue;
    for (int k = 0; k < 3; ++k) if (!in.i[k]) return hipErrorInvalidValue;
    for (int k = 0; k < 6; ++k) if (!in.f[k]) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_atlas_merge, atl_grid(n, n), dim3(64, ATL_ROWS), 0, s, atl_planes(atlas, A), A, in, n, rx, ry, px, py, seq, cnt);
    return hipGetLastError();
}

hipError_t gvom_launch_atlas_recall(hipStream_t s, const char *atlas, int A, const AtlasMaps &out, int n, int rx, int ry, int px, int py,
                                    int32_t seq, int32_t *counts)
{
    if (!atlas || !atl_window_ok(A, n, rx, ry, px, py)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_atlas_recall, atl_grid(n, n), dim3(64, ATL_ROWS), 0, s, atl_planes((char *)atlas, A), A, out, n, rx, ry, px, py, seq, counts);
    return hipGetLastError();
}
