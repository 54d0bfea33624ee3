// Stand-alone check of the two layouts the atlas fields use (g-vom_amd/csrc/gvom_setlayout.h): no GPU, no HIP.  An atlas field (kind 26)
// is three planes of cap x cap cells, cap the side of the atlas; its window (kind 7, a cost field) three planes of xy x xy.  Over
// small, odd and the largest shapes: every part inside the allocation, on a 256-byte boundary, apart from the others, as long as its
// shape and element type say, [x, y]-indexed with strides (1, side); parts the kind does not have are refused; and the crop's
// addressing -- window cell (x, y) of a window at (rx, ry) relative to the field reads field cell [(ry + y) * A + rx + x] -- stays
// inside the field's planes for every window the entry point lets through.  Built with -fsanitize=address,undefined by
// tests/test_atlas_field_cpu.py.
#include "../g-vom_amd/csrc/gvom_setlayout.h"

#include <stdio.h>
#include <stdlib.h>
#include <vector>

using namespace gvom_host;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed (kind %d xy %d cap %lld part %d)\n", __FILE__, __LINE__, #c, \
                                          s.kind, s.xy, (long long)s.cap, part); exit(1); } } while (0)

static int check_set(SetShape s, size_t bytes, int64_t side)
{
    int part = -1;
    SetPart d;
    static const int bits[3] = {32, 8, 16};
    static const int code[3] = {kDLInt, kDLUInt, kDLUInt};
    CHECK(bytes > 0);
    CHECK(!set_part(&s, -1, &d));
    CHECK(!set_part(&s, 3, &d));
    std::vector<SetPart> parts;
    for (part = 0; part < 3; ++part) {
        CHECK(set_part(&s, part, &d));
        const size_t off = (size_t)((char *)d.ptr - s.mem);
        CHECK((char *)d.ptr >= s.mem && off % 256 == 0);
        CHECK(off + d.bytes <= bytes);
        CHECK(d.ndim == 2 && d.bits == bits[part] && d.code == code[part]);
        CHECK(d.shape[0] == side && d.shape[1] == side && d.shape[2] == 1);
        CHECK(d.strides[0] == 1 && d.strides[1] == side);
        CHECK(d.bytes == (size_t)side * (size_t)side * (size_t)(d.bits / 8));
        for (const SetPart &o : parts) CHECK((char *)d.ptr >= (char *)o.ptr + o.bytes || (char *)o.ptr >= (char *)d.ptr + d.bytes);
        parts.push_back(d);
    }
    return (int)parts.size();
}

// the cells of a window's row that the crop reads from the field: all of them inside [0, A*A)
static long crop_reads(int64_t A, int64_t n, int64_t rx, int64_t ry)
{
    long reads = 0;
    for (int64_t y = 0; y < n; y += (n > 64 ? n - 1 : 1))
        for (int64_t x = 0; x < n; x += (n > 64 ? n - 1 : 1)) {
            const bool inside = (uint64_t)(rx + x) < (uint64_t)A && (uint64_t)(ry + y) < (uint64_t)A;
            if (!inside) continue;
            const int64_t at = (ry + y) * A + rx + x;
            if (at < 0 || at >= A * A) { fprintf(stderr, "crop reads outside the field: A %lld n %lld r (%lld, %lld)\n", (long long)A, (long long)n, (long long)rx, (long long)ry); exit(1); }
            ++reads;
        }
    return reads;
}

int main()
{
    char *const base = (char *)(uintptr_t)0x10000000;          // (never dereferenced: the table only does arithmetic on it)
    int sets = 0, parts = 0;
    const int sides[] = {64, 128, 512, 4096};                   // an atlas field: the sides an atlas can have
    for (int A : sides) {
        SetShape s;
        s.mem = base; s.xy = 33; s.kind = GVOM_PRODUCT_ATLAS_FIELD; s.cap = A;
        const size_t bytes = set_bytes(s.kind, 0, 0, A);
        if (bytes != (((size_t)A * A * 4 + 255) & ~(size_t)255) + (((size_t)A * A + 255) & ~(size_t)255) + (size_t)A * A * 2) { fprintf(stderr, "kind 26: %zu bytes at %d\n", bytes, A); return 1; }
        parts += check_set(s, bytes, A);
        ++sets;
    }
    const int xys[] = {1, 15, 16, 33, 64, 4095, 4096};           // its window: a cost field of any window side
    for (int xy : xys) {
        SetShape s;
        s.mem = base; s.xy = xy; s.kind = GVOM_PRODUCT_COSTFIELD;
        parts += check_set(s, set_bytes(s.kind, xy, 0, 0), xy);
        ++sets;
    }
    long reads = 0;
    const int64_t lim = (int64_t)1 << 30;
    for (int A : sides)
        for (int xy : xys) {
            if (xy > A) continue;
            const int64_t at[] = {-lim, -(int64_t)xy, -(int64_t)xy + 1, -1, 0, 1, A - xy, A - xy + 1, A - 1, A, lim};
            for (int64_t rx : at)
                for (int64_t ry : at) reads += crop_reads(A, xy, rx, ry);
        }
    if (reads == 0) return 1;
    printf("atlas field layout host test ok: %d sets, %d parts, %ld crop reads\n", sets, parts, reads);
    return 0;
}
