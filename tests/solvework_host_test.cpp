// Stand-alone check of g-vom_amd/csrc/gvom_solvework.h, the arithmetic of the calls that wait: no GPU, no HIP.
// The look at a batch's counters (the first round that flagged no tile at r = 0, in the middle, at nb - 1, or none; nb = 1 and 16; the
// tiles summed through the converging round and not beyond), the batch lengths under a limit below one batch, one that is no multiple
// of the batch and one that is, and the work buffers' layouts for sides 16, 33, 129 and 4096 -- the goal solvers' (goals of 8 and 12
// bytes, with and without a tail) and the frontier labelling's -- against the formulas the entry points used to spell out, written
// out here independently: every part on a 256-byte boundary, apart from the others, in order and inside the total.  The tile and
// block counts are passed in as numbers: 32-cell tiles (cost-to-go, frontiers), 8-cell tiles (pose fields), 1024-cell ranking blocks.
// Built with -fsanitize=address,undefined by tests/test_frontier_cpu.py.
#include "../g-vom_amd/csrc/gvom_solvework.h"

#include <stdio.h>
#include <stdlib.h>
#include <vector>

using namespace gvom_host;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed (%s)\n", __FILE__, __LINE__, #c, what); exit(1); } } while (0)

static size_t up256(size_t b) { return (b + 255) / 256 * 256; }

static void look_cases()
{
    char what[64];
    for (int nb : {1, 2, 8, 16})
        for (int zero = -1; zero < nb; ++zero) {                            // -1: no round of the batch converged
            snprintf(what, sizeof what, "nb %d, first zero at %d", nb, zero);
            std::vector<uint32_t> pin(64, 0xdeadbeefu);                     // (what lies behind the batch is never read as a counter)
            int64_t want = 0;
            for (int r = 0; r < GVOM_CTG_MAX_BATCH; ++r) {
                pin[r] = (r == zero || (zero >= 0 && r == zero + 2)) ? 0 : 5 + r;     // (a second zero behind the first plays no part)
                pin[SOLVE_CNT_RAN + r] = 100 + 7 * r;
                if (r < nb && (zero < 0 || r <= zero)) want += 100 + 7 * r;
            }
            const SolveLook k = solve_look(pin.data(), nb);
            CHECK(k.converged == (zero >= 0));
            CHECK(k.ran == (zero >= 0 ? zero + 1 : nb));
            CHECK(k.tiles == want);
        }
    snprintf(what, sizeof what, "the counters' places");
    CHECK(SOLVE_CNT_RAN == 16 && GVOM_CTG_MAX_BATCH == 16 && SOLVE_CNT_BATCH_BYTES == 128 && 2 * GVOM_CTG_MAX_BATCH <= 32);   // (the solvers' own counters start at [32])
}

static void batch_cases()
{
    const struct { int batch; int64_t limit; int n; int want[4]; } cases[] = {
        {8, 3, 1, {3}}, {8, 17, 3, {8, 8, 1}}, {8, 16, 2, {8, 8}}, {8, 8, 1, {8}}, {1, 3, 3, {1, 1, 1}}, {16, 33, 3, {16, 16, 1}}};
    char what[64];
    for (const auto &c : cases) {
        snprintf(what, sizeof what, "batch %d, limit %lld", c.batch, (long long)c.limit);
        int64_t rounds = 0;
        for (int k = 0; k < c.n; ++k) {                                     // no round converges: every batch runs whole
            const int nb = solve_batch_len(c.batch, c.limit, rounds);
            CHECK(nb == c.want[k]);
            rounds += nb;
        }
        CHECK(rounds == c.limit);
    }
    snprintf(what, sizeof what, "limits beyond 2^31");
    CHECK(solve_batch_len(8, (int64_t)1 << 29, 0) == 8 && solve_batch_len(16, ((int64_t)1 << 40) + 1, (int64_t)1 << 40) == 1);
    CHECK(solve_batch_len(8, (int64_t)4096 * 4096 + 1, (int64_t)4096 * 4096 - 3) == 4);
}

static void in_order(const size_t *at, const size_t *len, int n, size_t end, const char *what)
{
    for (int k = 0; k < n; ++k) {
        CHECK(at[k] % 256 == 0);
        CHECK(at[k] + len[k] <= (k + 1 < n ? at[k + 1] : end));
    }
}

static void layout_cases()
{
    char what[64];
    for (int n : {16, 33, 129, 4096}) {
        const size_t n2 = (size_t)n * n;
        // the goal solvers: gvom_cost_to_go / gvom_atlas_cost_to_go (32-cell tiles, goals of 2 int32, no tail), gvom_pose_field (8-cell
        // tiles, goals of 3 int32, the uint16 cost map as the tail), and the two crossed
        const struct { int tile; size_t goal, tail; } solvers[] = {{32, 8, 0}, {8, 12, n2 * 2}, {32, 12, n2 * 2}, {8, 8, 0}};
        for (const auto &sv : solvers) {
            snprintf(what, sizeof what, "goal solver, side %d, tiles of %d, goals of %zu", n, sv.tile, sv.goal);
            const int nt = (n + sv.tile - 1) / sv.tile, ntiles = nt * nt;
            const GoalWork o = goal_work(ntiles, sv.goal, sv.tail);
            const size_t flags_off = 256, goals_off = flags_off + up256((size_t)2 * ntiles * 4);             // the entry points' formulas
            const size_t tail_off = goals_off + up256((size_t)65536 * sv.goal), total = sv.tail ? tail_off + sv.tail : goals_off + (size_t)65536 * sv.goal;
            CHECK(o.flags == flags_off && o.goals == goals_off && o.tail == tail_off && o.end == total);
            const size_t at[4] = {0, o.flags, o.goals, o.tail}, len[4] = {256, (size_t)2 * ntiles * 4, (size_t)GVOM_CTG_MAX_GOALS * sv.goal, sv.tail};
            in_order(at, len, 4, o.end, what);
        }
        // the frontier labelling: 32-cell tiles, ranking blocks of 1024 cells
        snprintf(what, sizeof what, "frontier labelling, side %d", n);
        const int nt = (n + 31) / 32, nb = (int)((n2 + 1023) / 1024);
        const FrOffsets f = fr_offsets(n, nt, nb);
        const size_t bc = 256 + up256((size_t)2 * nt * nt * 4), L = bc + up256((size_t)2 * nb * 4), count = L + up256(n2 * 4);
        CHECK(f.flags == 256 && f.bc == bc && f.L == L && f.count == count && f.end == count + n2 * 4);
        const size_t at[5] = {0, f.flags, f.bc, f.L, f.count}, len[5] = {256, (size_t)2 * nt * nt * 4, (size_t)2 * nb * 4, n2 * 4, n2 * 4};
        in_order(at, len, 5, f.end, what);
    }
}

int main()
{
    look_cases();
    batch_cases();
    layout_cases();
    printf("solvework host test ok\n");
    return 0;
}
