// Stand-alone check of the output buffers' content-record table (g-vom_amd/csrc/gvom_outrec.h): no GPU, no HIP.  The table only
// decides which slot of the handle's bitmap allocation a host pointer gets and whether that slot must be reset; this program plays
// the host layer around it -- a heap block per slot stands for the device bitmap -- and walks insert, re-use, forget, size change,
// eviction of the entry used longest ago, and destroy.  Built with -fsanitize=address,undefined by tests/test_outrec_host.py.
#include "../g-vom_amd/csrc/gvom_outrec.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

struct Host {                                   // what map2d_impl does with the table
    OutRecTable t;
    std::vector<uint8_t *> slots;
    size_t slot_bytes = 0;
    int resets = 0;
    explicit Host(int max_xy) : slot_bytes(gvom_outrec_bytes(max_xy))
    {
        for (int k = 0; k < GVOM_OUTREC_MAX; ++k) slots.push_back((uint8_t *)calloc(slot_bytes, 1));
    }
    ~Host() { t.clear(); for (uint8_t *p : slots) free(p); }
    uint8_t *use(void *host, int xy)
    {
        bool fresh = false;
        const int k = t.use(host, xy, &fresh);
        CHECK(k >= 0 && k < GVOM_OUTREC_MAX);
        CHECK(gvom_outrec_bytes(xy) <= slot_bytes);
        if (fresh) { memset(slots[k], 0xFF, gvom_outrec_bytes(xy)); ++resets; }
        return slots[k];
    }
};

int main()
{
    CHECK(gvom_outrec_bytes(256) == 8 * 32 * 8);             // 8 x 32 tiles, 8 waves each
    CHECK(gvom_outrec_bytes(64) == 2 * 8 * 8);
    CHECK(gvom_outrec_bytes(33) == 2 * 5 * 8);               // partial tiles count whole
    char bufs[GVOM_OUTREC_MAX + 3][4];
    Host h(256);

    // insert: an unseen pointer starts with every bit set; the kernel's writes stay with the pointer
    uint8_t *a = h.use(bufs[0], 64);
    CHECK(h.resets == 1 && a[0] == 0xFF && a[gvom_outrec_bytes(64) - 1] == 0xFF);
    memset(a, 0x05, gvom_outrec_bytes(64));
    const uint64_t gen_a = h.t.generation(bufs[0]);
    CHECK(gen_a != 0);
    CHECK(h.use(bufs[0], 64) == a && h.resets == 1 && a[3] == 0x05 && h.t.generation(bufs[0]) == gen_a);
    // two buffers do not alias
    uint8_t *b = h.use(bufs[1], 64);
    CHECK(b != a && h.resets == 2 && b[0] == 0xFF && a[0] == 0x05 && h.t.size() == 2);

    // forget: gone, the others untouched, and the pointer starts over; unknown and null pointers are fine
    CHECK(h.t.forget(bufs[0]) && !h.t.forget(bufs[0]) && !h.t.forget(bufs[5]) && !h.t.forget(nullptr));
    CHECK(h.t.find(bufs[0]) < 0 && h.t.generation(bufs[0]) == 0 && h.t.size() == 1);
    memset(b, 0x0A, gvom_outrec_bytes(64));
    CHECK(h.use(bufs[1], 64) == b && b[0] == 0x0A && h.resets == 2);
    a = h.use(bufs[0], 64);
    CHECK(h.resets == 3 && a[0] == 0xFF && h.t.generation(bufs[0]) != gen_a);

    // size change: same pointer, another grid -> reset, same slot
    memset(a, 0, gvom_outrec_bytes(64));
    uint8_t *a2 = h.use(bufs[0], 256);
    CHECK(a2 == a && h.resets == 4 && a2[gvom_outrec_bytes(256) - 1] == 0xFF);
    CHECK(h.use(bufs[0], 256) == a && h.resets == 4);

    // eviction: fill the table, touch the oldest, add one more -- the entry used longest ago goes, nobody else
    for (int k = 2; k < GVOM_OUTREC_MAX; ++k) h.use(bufs[k], 64);
    CHECK(h.t.size() == GVOM_OUTREC_MAX);
    const int before = h.resets;
    h.use(bufs[1], 64);                                      // bufs[1] was the oldest; now bufs[0] is
    CHECK(h.resets == before);
    uint8_t *n = h.use(bufs[GVOM_OUTREC_MAX], 64);
    CHECK(h.resets == before + 1 && n == a && n[0] == 0xFF);   // took bufs[0]'s slot, reset
    CHECK(h.t.find(bufs[0]) < 0 && h.t.find(bufs[1]) >= 0 && h.t.size() == GVOM_OUTREC_MAX);
    for (int k = 1; k <= GVOM_OUTREC_MAX; ++k) CHECK(h.t.find(bufs[k]) >= 0);
    // many more pointers than slots: every one starts fresh, the table stays full and consistent
    for (int r = 0; r < 100; ++r) {
        uint8_t *p = h.use(bufs[r % (GVOM_OUTREC_MAX + 3)], 64);
        int owners = 0;
        for (int k = 0; k < GVOM_OUTREC_MAX; ++k) owners += h.slots[k] == p ? 1 : 0;
        CHECK(owners == 1 && h.t.size() == GVOM_OUTREC_MAX);
        for (int i = 0; i < GVOM_OUTREC_MAX; ++i)
            for (int j = i + 1; j < GVOM_OUTREC_MAX; ++j) CHECK(h.t.e[i].host != h.t.e[j].host);
    }
    // destroy (clear): nothing is known any more
    h.t.clear();
    CHECK(h.t.size() == 0 && h.t.find(bufs[1]) < 0);
    h.use(bufs[1], 64);
    CHECK(h.t.size() == 1);
    printf("outrec host test ok (%d resets)\n", h.resets);
    return 0;
}
