// Stand-alone check of the alignment product's layout (kind GVOM_PRODUCT_ALIGNMENT of g-vom_amd/csrc/gvom_setlayout.h): no GPU, no HIP.
// For K = 1, 3, 257 and 65536 -- the most a call takes -- part 0 (int32 [K, 6]) and part 1 (int32 [4]) lie inside set_bytes(), each on
// a 256-byte boundary, apart from one another and as long as their shapes say; there is no part 2 and no part -1.  Built with
// -fsanitize=address,undefined by tests/test_align_cpu.py.
#include "../g-vom_amd/csrc/gvom_setlayout.h"

#include <stdio.h>
#include <stdlib.h>

using namespace gvom_host;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed (K %lld)\n", __FILE__, __LINE__, #c, (long long)s.cap); exit(1); } } while (0)

int main()
{
    const int64_t Ks[4] = {1, 3, 257, 65536};
    char *const base = (char *)(uintptr_t)0x10000000;          // (never dereferenced: the table only does arithmetic on it)
    static_assert(GVOM_PRODUCT_ALIGNMENT == 12, "the kind's number is part of the interface");
    for (const int64_t K : Ks) {
        SetShape s;
        s.mem = base; s.kind = GVOM_PRODUCT_ALIGNMENT; s.xy = 64; s.zs = 8; s.cap = K;
        const size_t bytes = set_bytes(s.kind, s.xy, s.zs, s.cap);
        CHECK(bytes >= (size_t)K * 24 + 16);
        CHECK(bytes == set_bytes(s.kind, 0, 0, s.cap));                     // the map's size plays no part
        SetPart d0, d1, none;
        CHECK(set_part(&s, 0, &d0) && set_part(&s, 1, &d1));
        CHECK(!set_part(&s, 2, &none) && !set_part(&s, -1, &none));
        const size_t o0 = (size_t)((char *)d0.ptr - base), o1 = (size_t)((char *)d1.ptr - base);
        CHECK(o0 % 256 == 0 && o1 % 256 == 0);
        CHECK(o0 + d0.bytes <= o1 && o1 + d1.bytes <= bytes);               // disjoint, in order, inside
        CHECK(d0.ndim == 2 && d0.code == kDLInt && d0.bits == 32 && d0.shape[0] == K && d0.shape[1] == 6);
        CHECK(d0.strides[0] == 6 && d0.strides[1] == 1 && d0.bytes == (size_t)K * 24);
        CHECK(d1.ndim == 1 && d1.code == kDLInt && d1.bits == 32 && d1.shape[0] == 4 && d1.strides[0] == 1 && d1.bytes == 16);
        CHECK(d0.shape[2] == 1 && d1.shape[1] == 1 && d1.shape[2] == 1);
    }
    SetShape s;
    SetPart d;
    s.mem = base; s.xy = 16; s.zs = 1; s.cap = 1; s.cols = 1;
    s.kind = 11; CHECK(!set_part(&s, 0, &d) && set_bytes(11, 16, 1, 1, 1) == 0);    // kinds 8, 9 and 11 are not assigned
    s.kind = 9; CHECK(!set_part(&s, 0, &d) && set_bytes(9, 16, 1, 1, 1) == 0);
    s.kind = 8; CHECK(!set_part(&s, 0, &d) && set_bytes(8, 16, 1, 1, 1) == 0);
    s.kind = 13; CHECK(!set_part(&s, 0, &d) && set_bytes(13, 16, 1, 1, 1) == 0);
    printf("align layout host test ok\n");
    return 0;
}
