// Stand-alone check of the frontier product's layout (kind GVOM_PRODUCT_FRONTIERS of g-vom_amd/csrc/gvom_setlayout.h): no GPU, no HIP.
// For caps 1, 7 and 1024 on maps of 16, 33 and 129 cells -- and the largest call, 2^20 rows on 4096 cells -- part 0 (int32 [cap, 8]),
// part 1 (int64 [cap, 2]), part 2 (int32 [xy, xy], strides (1, xy)) and part 3 (int32 [4]) lie inside set_bytes(), each on a 256-byte
// boundary, apart from one another and as long as their shapes say; there is no part 4 and no part -1; kinds 15 and 17 have no
// parts.  Built with -fsanitize=address,undefined by tests/test_frontier_cpu.py.
#include "../g-vom_amd/csrc/gvom_setlayout.h"

#include <stdio.h>
#include <stdlib.h>

using namespace gvom_host;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed (cap %lld xy %d)\n", __FILE__, __LINE__, #c, (long long)s.cap, \
                                          s.xy); exit(1); } } while (0)

int main()
{
    const int64_t shapes[10][2] = {{1, 16}, {7, 16}, {1024, 16}, {1, 33}, {7, 33}, {1024, 33}, {1, 129}, {7, 129}, {1024, 129}, {1 << 20, 4096}};
    char *const base = (char *)(uintptr_t)0x10000000;          // (never dereferenced: the table only does arithmetic on it)
    static_assert(GVOM_PRODUCT_FRONTIERS == 16, "the kind's number is part of the interface");
    for (const auto &cx : shapes) {
        const size_t cap = (size_t)cx[0], n2 = (size_t)cx[1] * (size_t)cx[1];
        SetShape s;
        s.mem = base; s.kind = GVOM_PRODUCT_FRONTIERS; s.xy = (int)cx[1]; s.zs = 8; s.cap = cx[0];
        const size_t bytes = set_bytes(s.kind, s.xy, s.zs, s.cap);
        CHECK(bytes >= cap * 48 + n2 * 4 + 16);
        CHECK(bytes == set_bytes(s.kind, s.xy, 0, s.cap, 99));             // z_size and cols play no part
        SetPart d[4], none;
        for (int k = 0; k < 4; ++k) CHECK(set_part(&s, k, &d[k]));
        CHECK(!set_part(&s, 4, &none) && !set_part(&s, -1, &none));
        size_t o[4];
        for (int k = 0; k < 4; ++k) { o[k] = (size_t)((char *)d[k].ptr - base); CHECK(o[k] % 256 == 0); }
        CHECK(o[0] + d[0].bytes <= o[1] && o[1] + d[1].bytes <= o[2] && o[2] + d[2].bytes <= o[3] && o[3] + d[3].bytes <= bytes);   // disjoint, in order, inside
        CHECK(d[0].ndim == 2 && d[0].code == kDLInt && d[0].bits == 32 && d[0].shape[0] == cx[0] && d[0].shape[1] == 8 && d[0].shape[2] == 1);
        CHECK(d[0].strides[0] == 8 && d[0].strides[1] == 1 && d[0].bytes == cap * 32);
        CHECK(d[1].ndim == 2 && d[1].code == kDLInt && d[1].bits == 64 && d[1].shape[0] == cx[0] && d[1].shape[1] == 2 && d[1].shape[2] == 1);
        CHECK(d[1].strides[0] == 2 && d[1].strides[1] == 1 && d[1].bytes == cap * 16);
        CHECK(d[2].ndim == 2 && d[2].code == kDLInt && d[2].bits == 32 && d[2].shape[0] == cx[1] && d[2].shape[1] == cx[1] && d[2].shape[2] == 1);
        CHECK(d[2].strides[0] == 1 && d[2].strides[1] == cx[1] && d[2].bytes == n2 * 4);
        CHECK(d[3].ndim == 1 && d[3].code == kDLInt && d[3].bits == 32 && d[3].shape[0] == 4 && d[3].strides[0] == 1 && d[3].bytes == 16);
        CHECK((o[0] + 24) % 8 == 0);                                       // the best key of a row, columns 6 and 7, is one aligned 64-bit word
    }
    SetShape s;
    SetPart d;
    s.mem = base; s.xy = 16; s.zs = 1; s.cap = 1; s.cols = 1;
    s.kind = 15; CHECK(!set_part(&s, 0, &d) && set_bytes(15, 16, 1, 1, 1) == 0);    // kinds 15 and 17 are not assigned
    s.kind = 17; CHECK(!set_part(&s, 0, &d) && set_bytes(17, 16, 1, 1, 1) == 0);
    printf("frontier layout host test ok\n");
    return 0;
}
