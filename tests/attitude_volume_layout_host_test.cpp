// Stand-alone check of the attitude volume product's layout (kind GVOM_PRODUCT_ATTITUDE_VOLUME of g-vom_amd/csrc/gvom_setlayout.h): no
// GPU, no HIP.  For H = 1, 4, 16 and 64 on maps of 7, 33 and 256 cells -- and the largest volume, 64 headings on 2048 cells, 2^28
// states -- part 0 (status) and part 1 (tilt), uint8 [H, xy, xy] with strides (xy*xy, 1, xy), and part 2, int32 [8], lie inside
// set_bytes(), each on a 256-byte boundary, apart from one another and as long as their shapes say; there is no part 3 and no part
// -1; kind 29, which stays unassigned, has no parts.  Built with -fsanitize=address,undefined by tests/test_attitude_volume_cpu.py and
// run as a program.
#include "../g-vom_amd/csrc/gvom_setlayout.h"

#include <stdio.h>
#include <stdlib.h>

using namespace gvom_host;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed (H %lld, xy %d)\n", __FILE__, __LINE__, #c, (long long)s.cap, s.xy); exit(1); } } while (0)

int main()
{
    const int64_t shapes[13][2] = {{1, 7}, {4, 7}, {16, 7}, {64, 7}, {1, 33}, {4, 33}, {16, 33}, {64, 33}, {1, 256}, {4, 256}, {16, 256}, {64, 256}, {64, 2048}};
    char *const base = (char *)(uintptr_t)0x10000000;          // (never dereferenced: the table only does arithmetic on it)
    static_assert(GVOM_PRODUCT_ATTITUDE_VOLUME == 30, "the kind's number is part of the interface");
    for (const auto &hx : shapes) {
        SetShape s;
        s.mem = base; s.kind = GVOM_PRODUCT_ATTITUDE_VOLUME; s.xy = (int)hx[1]; s.zs = 8; s.cap = hx[0];
        const size_t n2 = (size_t)s.xy * s.xy, vol = (size_t)s.cap * n2;
        const size_t bytes = set_bytes(s.kind, s.xy, s.zs, s.cap);
        CHECK(bytes >= vol * 2 + 32 && bytes <= vol * 2 + 32 + 512);
        CHECK(bytes == set_bytes(s.kind, s.xy, 0, s.cap, 99));             // z_size and cols play no part
        SetPart d[3], none;
        for (int k = 0; k < 3; ++k) CHECK(set_part(&s, k, &d[k]));
        CHECK(!set_part(&s, 3, &none) && !set_part(&s, -1, &none));
        size_t o[3];
        for (int k = 0; k < 3; ++k) {
            o[k] = (size_t)((char *)d[k].ptr - base);
            CHECK(o[k] % 256 == 0);
        }
        for (int k = 0; k < 2; ++k) {
            CHECK(d[k].ndim == 3 && d[k].bits == 8 && d[k].code == kDLUInt);
            CHECK(d[k].shape[0] == s.cap && d[k].shape[1] == s.xy && d[k].shape[2] == s.xy);
            CHECK(d[k].strides[0] == (int64_t)n2 && d[k].strides[1] == 1 && d[k].strides[2] == s.xy);
            CHECK(d[k].bytes == vol);
        }
        CHECK(d[2].ndim == 1 && d[2].bits == 32 && d[2].code == kDLInt && d[2].shape[0] == 8 && d[2].strides[0] == 1 && d[2].bytes == 32);
        CHECK(o[0] == 0 && o[0] + d[0].bytes <= o[1] && o[1] + d[1].bytes <= o[2] && o[2] + d[2].bytes <= bytes);   // disjoint, in order, inside
    }
    SetShape s;
    SetPart d;
    s.mem = base; s.xy = 16; s.zs = 1; s.cap = 1; s.cols = 1;
    s.kind = 29; CHECK(!set_part(&s, 0, &d) && set_bytes(29, 16, 1, 1, 1) == 0);    // kind 29 stays unassigned: no such kind
    s.kind = 31; CHECK(!set_part(&s, 0, &d) && set_bytes(31, 16, 1, 1, 1) == 0);
    printf("attitude volume layout host test ok\n");
    return 0;
}
