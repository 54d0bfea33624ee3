// gvom_outrec.h -- the CONTENT RECORD of the caller's output buffers (host side; no HIP in here: tests/outrec_host_test.cpp compiles
// it alone).  k_map2d's host-output [y][x] form skips a store run (32 cells in x of one map) that holds only default values now and
// held only default values the last time the library wrote the same buffer; what it wrote there is kept per buffer as a device
// bitmap (a set bit: "the library last stored non-default values in this run").  This table says WHICH bitmap belongs to a host
// pointer: a handful of entries keyed by pointer, entry k owning slot k of the handle's one bitmap allocation.
//   * a pointer the table has not seen, one whose entry was dropped (forget, eviction) and one whose grid size differs from the
//     entry's come back `fresh`: the caller fills the slot with ones (every run is stored) before the kernel reads it;
//   * a full table evicts the entry that was used longest ago;
//   * `gen` counts the fresh starts the table has handed out: an entry's generation changes exactly when its bitmap was reset.
// A bitmap is only as good as the rule that the library is the buffer's sole writer: whoever else writes the buffer (another
// output form of the library included) calls forget().
#pragma once
#include <stddef.h>
#include <stdint.h>

#define GVOM_OUTREC_MAX 8       // buffers with a record per handle (gvom.py's pool holds one per result the caller keeps alive)
// k_map2d's workgroup is a 32 (x) x 8 (y) tile of two roles x four waves; a wave owns the two runs of its two rows in the two maps
// of its role -- four bits -- and is the one writer of ONE byte: bit 2 m + (row & 1), m = 0 / 1 the role's first / second map
// (role A: visibility, roughness; role B: positive, negative).  Byte (tile * 8 + wave); the upper four bits stay clear.
static inline size_t gvom_outrec_bytes(int xy) { return (size_t)((xy + 31) / 32) * (size_t)((xy + 7) / 8) * 8; }

struct OutRecTable {
    struct Entry { void *host = nullptr; int xy = 0; uint64_t gen = 0, used = 0; };   // host null: a free slot
    Entry e[GVOM_OUTREC_MAX];
    uint64_t clock = 0, gens = 0;

    int find(const void *host) const
    {
        for (int k = 0; host && k < GVOM_OUTREC_MAX; ++k) if (e[k].host == host) return k;
        return -1;
    }
    // the slot of `host`'s bitmap; *fresh: the slot's contents are not this buffer's (fill it with ones first)
    int use(void *host, int xy, bool *fresh)
    {
        int k = find(host);
        *fresh = k < 0 || e[k].xy != xy;
        if (k < 0) {                                        // a free slot, else the entry used longest ago
            k = 0;
            for (int j = 0; j < GVOM_OUTREC_MAX; ++j) {
                if (!e[j].host) { k = j; break; }
                if (e[j].used < e[k].used) k = j;
            }
        }
        if (*fresh) { e[k].host = host; e[k].xy = xy; e[k].gen = ++gens; }
        e[k].used = ++clock;
        return k;
    }
    // drops `host`'s entry; returns whether there was one
    bool forget(const void *host)
    {
        const int k = find(host);
        if (k >= 0) e[k] = Entry();
        return k >= 0;
    }
    int size() const { int c = 0; for (const Entry &x : e) c += x.host ? 1 : 0; return c; }
    uint64_t generation(const void *host) const { const int k = find(host); return k < 0 ? 0 : e[k].gen; }
    void clear() { for (Entry &x : e) x = Entry(); }
};
