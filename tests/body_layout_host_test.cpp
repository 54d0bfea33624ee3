// Stand-alone check of the body product's layout (kind GVOM_PRODUCT_BODY of g-vom_amd/csrc/gvom_setlayout.h): no GPU, no HIP.
// For (K, T) = (1, 1), (3, 63), (2, 65), (2, 257), (2, 4096) and (16384, 4096) -- K * T = 2^26, the most a call takes -- part 0 (int32
// [K, 4]), part 1 (float32 [K, T]) and part 2 (uint8 [K, T, 2]) lie inside set_bytes(), each on a 256-byte boundary, apart from one
// another and as long as their shapes say; there is no part 3 and no part -1; kind 43 is no kind.  Built with
// -fsanitize=address,undefined by tests/test_body_cpu.py.
#include "../g-vom_amd/csrc/gvom_setlayout.h"

#include <stdio.h>
#include <stdlib.h>

using namespace gvom_host;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed (K %lld T %lld)\n", __FILE__, __LINE__, #c, (long long)s.cap, \
                                          (long long)s.cols); exit(1); } } while (0)

int main()
{
    const int64_t shapes[6][2] = {{1, 1}, {3, 63}, {2, 65}, {2, 257}, {2, 4096}, {16384, 4096}};
    char *const base = (char *)(uintptr_t)0x10000000;          // (never dereferenced: the table only does arithmetic on it)
    static_assert(GVOM_PRODUCT_BODY == 44, "the kind's number is part of the interface");
    for (const auto &kt : shapes) {
        const size_t K = (size_t)kt[0], T = (size_t)kt[1];
        SetShape s;
        s.mem = base; s.kind = GVOM_PRODUCT_BODY; s.xy = 64; s.zs = 8; s.cap = kt[0]; s.cols = kt[1];
        const size_t bytes = set_bytes(s.kind, s.xy, s.zs, s.cap, s.cols);
        CHECK(bytes >= K * 16 + K * T * 6);
        CHECK(bytes == set_bytes(s.kind, 0, 0, s.cap, s.cols));            // the map's size plays no part
        SetPart d0, d1, d2, none;
        CHECK(set_part(&s, 0, &d0) && set_part(&s, 1, &d1) && set_part(&s, 2, &d2));
        CHECK(!set_part(&s, 3, &none) && !set_part(&s, -1, &none));
        const size_t o0 = (size_t)((char *)d0.ptr - base), o1 = (size_t)((char *)d1.ptr - base), o2 = (size_t)((char *)d2.ptr - base);
        CHECK(o0 % 256 == 0 && o1 % 256 == 0 && o2 % 256 == 0);
        CHECK(o0 + d0.bytes <= o1 && o1 + d1.bytes <= o2 && o2 + d2.bytes <= bytes);   // disjoint, in order, inside
        CHECK(d0.ndim == 2 && d0.code == kDLInt && d0.bits == 32 && d0.shape[0] == kt[0] && d0.shape[1] == 4 && d0.shape[2] == 1);
        CHECK(d0.strides[0] == 4 && d0.strides[1] == 1 && d0.bytes == K * 16);
        CHECK(d1.ndim == 2 && d1.code == kDLFloat && d1.bits == 32 && d1.shape[0] == kt[0] && d1.shape[1] == kt[1] && d1.shape[2] == 1);
        CHECK(d1.strides[0] == kt[1] && d1.strides[1] == 1 && d1.bytes == K * T * 4);
        CHECK(d2.ndim == 3 && d2.code == kDLUInt && d2.bits == 8 && d2.shape[0] == kt[0] && d2.shape[1] == kt[1] && d2.shape[2] == 2);
        CHECK(d2.strides[0] == kt[1] * 2 && d2.strides[1] == 2 && d2.strides[2] == 1 && d2.bytes == K * T * 2);
    }
    SetShape s;
    SetPart d;
    s.mem = base; s.xy = 16; s.zs = 1; s.cap = 1; s.cols = 1;
    s.kind = 43; CHECK(!set_part(&s, 0, &d) && set_bytes(43, 16, 1, 1, 1) == 0);    // kinds 43 and 45 are not assigned
    s.kind = 45; CHECK(!set_part(&s, 0, &d) && set_bytes(45, 16, 1, 1, 1) == 0);
    printf("body layout host test ok\n");
    return 0;
}
