// Stand-alone check of the atlas alignment product's layout (kind GVOM_PRODUCT_VOXEL_ATLAS_ALIGNMENT of g-vom_amd/csrc/gvom_setlayout.h):
// no GPU, no HIP.  For K = 1, 3, 10, 11, 43, 1000 and the largest call, 65536: part 0 (int32 [K, 6]) and part 1 (int32 [4]) lie inside
// set_bytes(), each on a 256-byte boundary, apart from one another and as long as their shapes say; the size is align256(K * 24) + 16 and
// depends on nothing but K; every figure equals kind 12's (GVOM_PRODUCT_ALIGNMENT), whose two parts these are; there is no part 2 and no
// part -1; kind 37, which stays unassigned, has no parts.  Built with -fsanitize=address,undefined by tests/test_voxel_atlas_align_cpu.py
// and run as a program.
#include "../g-vom_amd/csrc/gvom_setlayout.h"

#include <stdio.h>
#include <stdlib.h>

using namespace gvom_host;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed (cap %lld)\n", __FILE__, __LINE__, #c, (long long)s.cap); exit(1); } } while (0)

int main()
{
    const int64_t caps[7] = {1, 3, 10, 11, 43, 1000, 65536};
    char *const base = (char *)(uintptr_t)0x10000000;          // (never dereferenced: the table only does arithmetic on it)
    static_assert(GVOM_PRODUCT_VOXEL_ATLAS_ALIGNMENT == 38, "the kind's number is part of the interface");
    for (const int64_t cap : caps) {
        SetShape s, w;
        s.mem = base; s.kind = GVOM_PRODUCT_VOXEL_ATLAS_ALIGNMENT; s.xy = 48; s.zs = 20; s.cap = cap;
        w = s; w.kind = GVOM_PRODUCT_ALIGNMENT;
        const size_t bytes = set_bytes(s.kind, s.xy, s.zs, s.cap);
        CHECK(bytes == (((size_t)cap * 24 + 255) & ~(size_t)255) + 16);
        CHECK(bytes == set_bytes(s.kind, 0, 0, s.cap, 99));                // the map's size and cols play no part
        CHECK(bytes == set_bytes(w.kind, w.xy, w.zs, w.cap));              // kind 12's size
        SetPart d[2], e[2], none;
        for (int k = 0; k < 2; ++k) CHECK(set_part(&s, k, &d[k]) && set_part(&w, k, &e[k]));
        CHECK(!set_part(&s, 2, &none) && !set_part(&s, -1, &none));
        size_t o[2];
        for (int k = 0; k < 2; ++k) { o[k] = (size_t)((char *)d[k].ptr - base); CHECK(o[k] % 256 == 0); }
        CHECK(o[0] == 0 && o[0] + d[0].bytes <= o[1] && o[1] + d[1].bytes <= bytes);       // disjoint, in order, inside
        CHECK(d[0].ndim == 2 && d[0].code == kDLInt && d[0].bits == 32 && d[0].shape[0] == cap && d[0].shape[1] == 6 && d[0].shape[2] == 1);
        CHECK(d[0].strides[0] == 6 && d[0].strides[1] == 1 && d[0].bytes == (size_t)cap * 24);
        CHECK(d[1].ndim == 1 && d[1].code == kDLInt && d[1].bits == 32 && d[1].shape[0] == 4 && d[1].strides[0] == 1 && d[1].bytes == 16);
        CHECK(o[1] % 16 == 0);
        for (int k = 0; k < 2; ++k) {                                      // the two parts of kind 12, field for field
            CHECK(d[k].ptr == e[k].ptr && d[k].ndim == e[k].ndim && d[k].code == e[k].code && d[k].bits == e[k].bits && d[k].bytes == e[k].bytes);
            for (int a = 0; a < 3; ++a) CHECK(d[k].shape[a] == e[k].shape[a] && d[k].strides[a] == e[k].strides[a]);
        }
    }
    SetShape s;
    SetPart d;
    s.mem = base; s.xy = 16; s.zs = 1; s.cap = 1; s.cols = 1;
    s.kind = 37; CHECK(!set_part(&s, 0, &d) && set_bytes(37, 16, 1, 1, 1) == 0);    // kind 37 stays unassigned
    printf("voxel atlas alignment layout host test ok\n");
    return 0;
}
