// Stand-alone check of the body volume's layout (kind GVOM_PRODUCT_BODY_VOLUME of g-vom_amd/csrc/gvom_setlayout.h): no GPU, no HIP.
// For (H, xy) = (1, 1), (7, 33), (16, 40), (64, 255), (64, 2048) and (16, 4096) -- H * xy^2 = 2^28, the most a call takes -- part 0 (uint8
// status), part 1 (uint8 squeeze) and part 2 (float32 clearance), each [H, xy, xy] with strides (xy*xy, 1, xy), and part 3 (int32 [8]) lie
// inside set_bytes(), each on a 256-byte boundary, apart from one another and as long as their shapes say; there is no part 4 and no
// part -1; kind 45 is no kind.  Built with -fsanitize=address,undefined by tests/test_body_volume_cpu.py.
#include "../g-vom_amd/csrc/gvom_setlayout.h"

#include <stdio.h>
#include <stdlib.h>

using namespace gvom_host;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed (H %lld xy %d)\n", __FILE__, __LINE__, #c, (long long)s.cap, s.xy); \
                                  exit(1); } } while (0)

int main()
{
    const int64_t shapes[6][2] = {{1, 1}, {7, 33}, {16, 40}, {64, 255}, {64, 2048}, {16, 4096}};
    char *const base = (char *)(uintptr_t)0x10000000;          // (never dereferenced: the table only does arithmetic on it)
    static_assert(GVOM_PRODUCT_BODY_VOLUME == 46, "the kind's number is part of the interface");
    for (const auto &hx : shapes) {
        const size_t H = (size_t)hx[0], n2 = (size_t)hx[1] * (size_t)hx[1];
        SetShape s;
        s.mem = base; s.kind = GVOM_PRODUCT_BODY_VOLUME; s.xy = (int)hx[1]; s.zs = 8; s.cap = hx[0]; s.cols = 0;
        const size_t bytes = set_bytes(s.kind, s.xy, s.zs, s.cap, s.cols);
        CHECK(bytes >= H * n2 * 6 + 32);
        CHECK(bytes == set_bytes(s.kind, s.xy, 0, s.cap));                 // z_size and cols play no part
        SetPart d[4], none;
        for (int p = 0; p < 4; ++p) CHECK(set_part(&s, p, &d[p]));
        CHECK(!set_part(&s, 4, &none) && !set_part(&s, -1, &none));
        size_t o[4];
        for (int p = 0; p < 4; ++p) { o[p] = (size_t)((char *)d[p].ptr - base); CHECK(o[p] % 256 == 0); }
        CHECK(o[0] == 0 && o[0] + d[0].bytes <= o[1] && o[1] + d[1].bytes <= o[2] && o[2] + d[2].bytes <= o[3] && o[3] + d[3].bytes <= bytes);   // disjoint, in order, inside
        for (int p = 0; p < 3; ++p) {
            CHECK(d[p].ndim == 3 && d[p].shape[0] == hx[0] && d[p].shape[1] == hx[1] && d[p].shape[2] == hx[1]);
            CHECK(d[p].strides[0] == (int64_t)n2 && d[p].strides[1] == 1 && d[p].strides[2] == hx[1]);
        }
        CHECK(d[0].code == kDLUInt && d[0].bits == 8 && d[0].bytes == H * n2);
        CHECK(d[1].code == kDLUInt && d[1].bits == 8 && d[1].bytes == H * n2);
        CHECK(d[2].code == kDLFloat && d[2].bits == 32 && d[2].bytes == H * n2 * 4);
        CHECK(d[3].ndim == 1 && d[3].code == kDLInt && d[3].bits == 32 && d[3].shape[0] == 8 && d[3].strides[0] == 1 && d[3].bytes == 32);
    }
    SetShape s;
    SetPart d;
    s.mem = base; s.xy = 16; s.zs = 1; s.cap = 1; s.cols = 1;
    s.kind = 45; CHECK(!set_part(&s, 0, &d) && set_bytes(45, 16, 1, 1, 1) == 0);    // kinds 45 and 47 are not assigned
    s.kind = 47; CHECK(!set_part(&s, 0, &d) && set_bytes(47, 16, 1, 1, 1) == 0);
    printf("body volume layout host test ok\n");
    return 0;
}
