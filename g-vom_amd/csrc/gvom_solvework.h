// gvom_solvework.h -- the arithmetic of the calls that WAIT (gvom_cost_to_go, gvom_frontiers, gvom_pose_field and their atlas forms):
// how many relaxation rounds the next batch holds, what the host reads off a batch's counters, and where the parts of a work buffer
// lie.  No HIP and no handle, like gvom_setlayout.h and gvom_outrec.h: tests/solvework_host_test.cpp holds it under sanitizers on a
// machine without a GPU.  solve_rounds (gvom_product_calls.hip) is the loop that uses it.
#pragma once
#include "gvom_setlayout.h"

namespace gvom_host {
#define GVOM_CTG_MAX_BATCH 16                   // rounds enqueued between two looks at the counters: at most
#define GVOM_CTG_MAX_GOALS 65536
// a work buffer begins with 256 bytes of counters (uint32): [r] tiles that flagged any in round r of the batch, [16 + r] tiles that
// ran in it, from [32] what each solver counts besides (CTG_CNT_*, FR_CNT_*: gvom_host.h)
#define SOLVE_CNT_RAN GVOM_CTG_MAX_BATCH
#define SOLVE_CNT_BATCH_BYTES (2 * GVOM_CTG_MAX_BATCH * 4)

// rounds in the next batch: a whole one, or what the limit leaves
inline int solve_batch_len(int batch, int64_t limit, int64_t rounds) { return (int)(limit - rounds < batch ? limit - rounds : batch); }

// the look at the pinned counters of a batch of nb rounds: the first round that flagged no tile ends the solve (the rounds enqueued
// behind it found nothing to do and do not count); the tiles that ran are summed up to and including that round
struct SolveLook { bool converged; int ran; int64_t tiles; };
inline SolveLook solve_look(const uint32_t *pin, int nb)
{
    SolveLook k = {false, nb, 0};
    for (int r = 0; r < nb; ++r) {
        k.tiles += pin[SOLVE_CNT_RAN + r];
        if (pin[r] == 0) { k.converged = true; k.ran = r + 1; break; }
    }
    return k;
}

// the work buffer of a goal solver: counters | the two halves of the tiles' activity flags | the staged goals (GVOM_CTG_MAX_GOALS of
// goal_bytes each) | tail_bytes of the caller's (gvom_pose_field's converted cost map)
struct GoalWork { size_t flags, goals, tail, end; };
inline GoalWork goal_work(int ntiles, size_t goal_bytes, size_t tail_bytes)
{
    GoalWork o;
    o.flags = 256; o.goals = o.flags + align256((size_t)2 * ntiles * 4);
    o.tail = o.goals + align256((size_t)GVOM_CTG_MAX_GOALS * goal_bytes); o.end = o.tail + tail_bytes;
    return o;
}

// the work buffer of the frontier labelling on n x n cells with nt x nt tiles and nb ranking blocks: counters | flags | block counts
// | labels | counts / ranks, int32 per cell each
struct FrOffsets { size_t flags, bc, L, count, end; };
inline FrOffsets fr_offsets(int n, int nt, int nb)
{
    const size_t n2 = (size_t)n * n;
    FrOffsets o;
    o.flags = 256; o.bc = o.flags + align256((size_t)2 * nt * nt * 4); o.L = o.bc + align256((size_t)2 * nb * 4);
    o.count = o.L + align256(n2 * 4); o.end = o.count + n2 * 4;
    return o;
}
}  // namespace gvom_host
