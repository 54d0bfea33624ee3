// seg_shape.hip -- what a wave instruction's ACCESS SHAPE costs on streams that miss every cache: a copy (equal bytes
// read and written, 16 bytes per lane) whose wave instruction covers 1024 bytes as
//   (a) 16 x  64-byte pieces, 1 KB apart                       -- k_encfuse's 16-sx state access
//   (b)  8 x 128-byte pieces, 1 KB apart                       -- the 32-sx form: whole lines
//   (c)  4 x 256-byte pieces, 1 KB apart
//   (d) as (a), the other half of every 128-byte line touched by the workgroup eight dispatch slots later (k_encfuse's
//       XCD pairing remap); in (a) it is the NEXT dispatch slot, i.e. another XCD.
//   (e) as (b), but with k_encfuse's ACCUMULATOR lane order: consecutive lanes step through 4 rows first, so every 16-lane
//       group of the instruction holds 4 x 64 bytes and the two halves of a line sit in different 16-lane groups.
// In (a) - (d) consecutive lanes run along a piece.
// The buffers are rows of 1 KB (a 256-voxel x row of 32-bit states).  A workgroup of 4 waves owns one column of pieces
// over 64 wave instructions (16 per wave, the waves interleaved as k_encfuse's are), 64 KB read and 64 KB written.
// Timed with HIP events around the kernel alone; best and median of 11 launches.
//   hipcc --offload-arch=gfx950 -O3 -o seg_shape seg_shape.hip;  ./seg_shape [MB per buffer, default 1024]
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

// PIECE = bytes per piece (64 / 128 / 256); PAIR = the XCD pairing remap of the dispatch slot; ROWS_FIRST = lane order (e)
template <int PIECE, bool PAIR, bool ROWS_FIRST = false>
__global__ __launch_bounds__(256) void k_copy(const uint4 *__restrict__ src, uint4 *__restrict__ dst, uint32_t rows)
{
    constexpr uint32_t NPC = 1024 / PIECE;                  // piece columns of a row = pieces (rows) per wave instruction
    constexpr uint32_t LPP = PIECE / 16;                    // lanes per piece
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t M = blockIdx.x;
    if (PAIR) { const uint32_t slot = M >> 3, xcd = M & 7u; M = ((slot >> 1) << 4) + (xcd << 1) + (slot & 1u); }
    const uint32_t pc = M % NPC, rg = M / NPC;              // piece column, row group of 64 * NPC rows
    const uint32_t prow = ROWS_FIRST ? (lane & 3u) + 4u * (lane / (4u * LPP)) : lane / LPP;   // piece of the instruction
    const uint32_t pcol = ROWS_FIRST ? (lane >> 2) % LPP : lane % LPP;                         // 16-byte unit of the piece
    const uint32_t row0 = rg * 64u * NPC + prow;
    const uint32_t col = pc * LPP + pcol;                   // in 16-byte units inside the 1 KB row
#pragma unroll 4
    for (uint32_t it = 0; it < 16u; ++it) {
        const uint32_t row = row0 + (it * 4u + w) * NPC;
        if (row < rows) {
            const size_t i = (size_t)row * 64u + col;
            dst[i] = src[i];
        }
    }
}

template <int PIECE, bool PAIR, bool ROWS_FIRST = false>
static int run(const char *name, const uint4 *src, uint4 *dst, size_t bytes, hipEvent_t e0, hipEvent_t e1)
{
    const uint32_t rows = (uint32_t)(bytes / 1024);
    const uint32_t npc = 1024 / PIECE;
    const uint32_t blocks = npc * (rows / (64u * npc));     // (rows is a multiple of 1024: whole row groups, blocks % 16 == 0)
    float t[11];
    for (int it = -2; it < 11; ++it) {
        CHECK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL((k_copy<PIECE, PAIR, ROWS_FIRST>), dim3(blocks), dim3(256), 0, 0, src, dst, rows);
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (it >= 0) t[it] = ms;
    }
    std::sort(t, t + 11);
    printf("%-44s best %8.1f us  median %8.1f us  = %.2f TB/s (read + write, median)\n", name, t[0] * 1e3, t[5] * 1e3,
           2.0 * (double)bytes / (t[5] * 1e-3) / 1e12);
    return 0;
}

int main(int argc, char **argv)
{
    const size_t mb = argc > 1 ? (size_t)atol(argv[1]) : 1024;
    if (mb < 1 || mb > 2048) { fprintf(stderr, "MB per buffer: 1 .. 2048\n"); return 1; }
    const size_t bytes = mb << 20;                          // a multiple of 1 MiB = 1024 rows
    uint4 *src, *dst;
    CHECK(hipMalloc(&src, bytes));
    CHECK(hipMalloc(&dst, bytes));
    CHECK(hipMemset(src, 1, bytes));
    CHECK(hipMemset(dst, 0, bytes));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    printf("seg_shape: %zu MB read + %zu MB written per launch\n", mb, mb);
    if (run<64, false>("(a) 16 x  64 B per wave instruction", src, dst, bytes, e0, e1)) return 1;
    if (run<128, false>("(b)  8 x 128 B", src, dst, bytes, e0, e1)) return 1;
    if (run<256, false>("(c)  4 x 256 B", src, dst, bytes, e0, e1)) return 1;
    if (run<64, true>("(d) 16 x  64 B, line halves 8 slots apart", src, dst, bytes, e0, e1)) return 1;
    if (run<128, false, true>("(e)  8 x 128 B, lanes step through rows first", src, dst, bytes, e0, e1)) return 1;
    if (run<64, false>("(a) again", src, dst, bytes, e0, e1)) return 1;
    if (run<128, false>("(b) again", src, dst, bytes, e0, e1)) return 1;
    CHECK(hipDeviceSynchronize());
    CHECK(hipFree(src));
    CHECK(hipFree(dst));
    return 0;
}
