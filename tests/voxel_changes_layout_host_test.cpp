// Stand-alone check of the voxel changes' layout (kind GVOM_PRODUCT_VOXEL_CHANGES of g-vom_amd/csrc/gvom_setlayout.h): no GPU, no HIP.
// For (cap, xy, z) = (1, 1, 1), (3, 33, 5), (1024, 64, 8), (7, 255, 48), (1 << 20, 16, 32) and (1024, 4096, 4) the seven parts -- int32
// [cap, 8], int64 [cap, 2], int32 [xy, xy] strides (1, xy), int32 [8], int32 [cap, 4], uint8 [xy, xy, z] in the occupancy grid's layout,
// uint16 [2, xy, xy] strides (xy*xy, 1, xy) -- lie inside set_bytes(), each on a 256-byte boundary, apart from one another, in order and
// as long as their shapes say; parts 0 .. 2 lie where kind 16 (frontiers) has them; there is no part 7 and no part -1; kind 47 is no
// kind.  Built with -fsanitize=address,undefined by tests/test_voxel_changes_cpu.py.
#include "../g-vom_amd/csrc/gvom_setlayout.h"

#include <stdio.h>
#include <stdlib.h>

using namespace gvom_host;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed (cap %lld xy %d z %d)\n", __FILE__, __LINE__, #c, (long long)s.cap, s.xy, s.zs); \
                                  exit(1); } } while (0)

int main()
{
    const int64_t shapes[6][3] = {{1, 1, 1}, {3, 33, 5}, {1024, 64, 8}, {7, 255, 48}, {1 << 20, 16, 32}, {1024, 4096, 4}};
    char *const base = (char *)(uintptr_t)0x10000000;          // (never dereferenced: the table only does arithmetic on it)
    static_assert(GVOM_PRODUCT_VOXEL_CHANGES == 48, "the kind's number is part of the interface");
    static_assert(GVOM_CHANGE_APPEARED == 1 && GVOM_CHANGE_VANISHED == 2, "the codes are the bits of the mask");
    for (const auto &c : shapes) {
        const size_t cap = (size_t)c[0], n2 = (size_t)c[1] * (size_t)c[1], zs = (size_t)c[2];
        SetShape s;
        s.mem = base; s.kind = GVOM_PRODUCT_VOXEL_CHANGES; s.xy = (int)c[1]; s.zs = (int)c[2]; s.cap = c[0]; s.cols = 0;
        const size_t bytes = set_bytes(s.kind, s.xy, s.zs, s.cap, s.cols);
        CHECK(bytes >= cap * 64 + n2 * 8 + n2 * zs + 32);
        CHECK(bytes == set_bytes(s.kind, s.xy, s.zs, s.cap, 99));           // cols play no part
        SetPart d[7], none;
        for (int p = 0; p < 7; ++p) CHECK(set_part(&s, p, &d[p]));
        CHECK(!set_part(&s, 7, &none) && !set_part(&s, -1, &none));
        size_t o[7];
        for (int p = 0; p < 7; ++p) { o[p] = (size_t)((char *)d[p].ptr - base); CHECK(o[p] % 256 == 0); }
        CHECK(o[0] == 0);
        for (int p = 0; p < 6; ++p) CHECK(o[p] + d[p].bytes <= o[p + 1]);   // disjoint, in order
        CHECK(o[6] + d[6].bytes <= bytes);                                  // inside
        SetShape f = s;                                                     // parts 0 .. 2: where the frontier kernels write them
        f.kind = GVOM_PRODUCT_FRONTIERS;
        for (int p = 0; p < 3; ++p) {
            SetPart e;
            CHECK(set_part(&f, p, &e) && e.ptr == d[p].ptr && e.bytes == d[p].bytes && e.code == d[p].code && e.bits == d[p].bits);
            CHECK(e.strides[0] == d[p].strides[0] && e.strides[1] == d[p].strides[1]);
        }
        CHECK(d[0].ndim == 2 && d[0].code == kDLInt && d[0].bits == 32 && d[0].shape[0] == c[0] && d[0].shape[1] == 8 && d[0].bytes == cap * 32);
        CHECK(d[1].ndim == 2 && d[1].code == kDLInt && d[1].bits == 64 && d[1].shape[0] == c[0] && d[1].shape[1] == 2 && d[1].bytes == cap * 16);
        CHECK(d[2].ndim == 2 && d[2].code == kDLInt && d[2].bits == 32 && d[2].shape[0] == c[1] && d[2].shape[1] == c[1]);
        CHECK(d[2].strides[0] == 1 && d[2].strides[1] == c[1] && d[2].bytes == n2 * 4);
        CHECK(d[3].ndim == 1 && d[3].code == kDLInt && d[3].bits == 32 && d[3].shape[0] == 8 && d[3].strides[0] == 1 && d[3].bytes == 32);
        CHECK(d[4].ndim == 2 && d[4].code == kDLInt && d[4].bits == 32 && d[4].shape[0] == c[0] && d[4].shape[1] == 4 && d[4].strides[0] == 4 && d[4].bytes == cap * 16);
        CHECK(d[5].ndim == 3 && d[5].code == kDLUInt && d[5].bits == 8 && d[5].shape[0] == c[1] && d[5].shape[1] == c[1] && d[5].shape[2] == c[2]);
        CHECK(d[5].strides[0] == c[1] * c[2] && d[5].strides[1] == c[2] && d[5].strides[2] == 1 && d[5].bytes == n2 * zs);
        SetShape b = s;                                                     // part 5: a voxel box's class grid, stride for stride
        b.kind = GVOM_PRODUCT_VOXEL_BOX;
        SetPart e;
        CHECK(set_part(&b, 0, &e) && e.bytes == d[5].bytes && e.strides[0] == d[5].strides[0] && e.strides[1] == d[5].strides[1] && e.strides[2] == d[5].strides[2]);
        CHECK(d[6].ndim == 3 && d[6].code == kDLUInt && d[6].bits == 16 && d[6].shape[0] == 2 && d[6].shape[1] == c[1] && d[6].shape[2] == c[1]);
        CHECK(d[6].strides[0] == (int64_t)n2 && d[6].strides[1] == 1 && d[6].strides[2] == c[1] && d[6].bytes == n2 * 4);
    }
    SetShape s;
    SetPart d;
    s.mem = base; s.xy = 16; s.zs = 1; s.cap = 1; s.cols = 1;
    s.kind = 47; CHECK(!set_part(&s, 0, &d) && set_bytes(47, 16, 1, 1, 1) == 0);    // kinds 47 and 49 are not assigned
    s.kind = 49; CHECK(!set_part(&s, 0, &d) && set_bytes(49, 16, 1, 1, 1) == 0);
    printf("voxel changes layout host test ok\n");
    return 0;
}
