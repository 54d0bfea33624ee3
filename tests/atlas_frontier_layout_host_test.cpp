// Stand-alone check of the layout the atlas frontiers use (g-vom_amd/csrc/gvom_setlayout.h): no GPU, no HIP.  A product of kind 28 is the
// four parts of kind 16 (frontiers) with the window's side replaced by cols, the side of the atlas field: over small and the largest caps
// and every side an atlas can have, every part inside the allocation, on a 256-byte boundary, apart from the others, with the shape,
// strides and element type the header says; parts the kind does not have are refused; and, part for part, the same offsets as kind 16 of
// a window of that side.  Also the marking kernel's visibility address -- field cell (x, y) at offset (ox, oy) from the extent of an
// atlas of side A with storage phase (px, py) reads [((py + oy + y) & (A-1)) * A + ((px + ox + x) & (A-1))] only where it lies in the
// extent -- in the kernel's own int arithmetic, for every offset the entry point lets through: no overflow, every read inside the plane.
// Built with -fsanitize=address,undefined by tests/test_atlas_frontiers_cpu.py.
#include "../g-vom_amd/csrc/gvom_setlayout.h"

#include <stdio.h>
#include <stdlib.h>
#include <vector>

using namespace gvom_host;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed (cap %lld side %lld part %d)\n", __FILE__, __LINE__, #c, \
                                          (long long)s.cap, (long long)s.cols, part); exit(1); } } while (0)

static int check_set(SetShape s, size_t bytes)
{
    int part = -1;
    SetPart d, w;
    const int64_t side = s.cols, cap = s.cap;
    SetShape win;                                               // kind 16 of a window of that side
    win.mem = s.mem; win.xy = (int)side; win.kind = GVOM_PRODUCT_FRONTIERS; win.cap = cap;
    CHECK(bytes > 0 && bytes == set_bytes(GVOM_PRODUCT_FRONTIERS, (int)side, 0, cap));
    CHECK(!set_part(&s, -1, &d));
    CHECK(!set_part(&s, 4, &d));
    std::vector<SetPart> parts;
    for (part = 0; part < 4; ++part) {
        CHECK(set_part(&s, part, &d) && set_part(&win, part, &w));
        const size_t off = (size_t)((char *)d.ptr - s.mem);
        CHECK((char *)d.ptr >= s.mem && off % 256 == 0 && d.ptr == w.ptr && d.bytes == w.bytes);
        CHECK(off + d.bytes <= bytes);
        CHECK(d.code == kDLInt && d.bits == (part == 1 ? 64 : 32));
        if (part == 0) CHECK(d.ndim == 2 && d.shape[0] == cap && d.shape[1] == 8 && d.strides[0] == 8 && d.strides[1] == 1);
        if (part == 1) CHECK(d.ndim == 2 && d.shape[0] == cap && d.shape[1] == 2 && d.strides[0] == 2 && d.strides[1] == 1);
        if (part == 2) CHECK(d.ndim == 2 && d.shape[0] == side && d.shape[1] == side && d.strides[0] == 1 && d.strides[1] == side);
        if (part == 3) CHECK(d.ndim == 1 && d.shape[0] == 4 && d.strides[0] == 1 && d.bytes == 16);
        for (const SetPart &o : parts) CHECK((char *)d.ptr >= (char *)o.ptr + o.bytes || (char *)o.ptr >= (char *)d.ptr + d.bytes);
        parts.push_back(d);
    }
    return (int)parts.size();
}

// the visibility reads of the field cells (x, y), x and y in {0, Af - 1} and their edge neighbours inside the field
static long mark_reads(int Af, int A, int ox, int oy, int px, int py)
{
    long reads = 0;
    const int at[] = {0, 1, Af / 2, Af - 2, Af - 1};
    for (int y : at)
        for (int x : at) {
            const int ex = ox + x, ey = oy + y;
            if ((unsigned)ex >= (unsigned)A || (unsigned)ey >= (unsigned)A) continue;
            const size_t a = (size_t)((py + ey) & (A - 1)) * A + ((px + ex) & (A - 1));
            if (a >= (size_t)A * A) { fprintf(stderr, "the marking reads outside the plane: Af %d A %d o (%d, %d) p (%d, %d)\n", Af, A, ox, oy, px, py); exit(1); }
            ++reads;
        }
    return reads;
}

int main()
{
    char *const base = (char *)(uintptr_t)0x10000000;          // (never dereferenced: the table only does arithmetic on it)
    int sets = 0, parts = 0;
    const int sides[] = {64, 128, 512, 4096};
    const int64_t caps[] = {1, 7, 8, 1024, (int64_t)1 << 20};
    for (int A : sides)
        for (int64_t cap : caps) {
            SetShape s;
            s.mem = base; s.xy = 33; s.kind = GVOM_PRODUCT_ATLAS_FRONTIERS; s.cap = cap; s.cols = A;
            parts += check_set(s, set_bytes(s.kind, 0, 0, cap, A));
            ++sets;
        }
    long reads = 0;
    const int lim = 1 << 30;
    for (int Af : sides)
        for (int A : sides) {
            const int at[] = {-lim, -Af, -Af + 1, -1, 0, 1, A - Af, A - 1, A, lim};
            const int phase[] = {0, 1, A / 2, A - 1};
            for (int ox : at)
                for (int oy : at)
                    for (int px : phase)
                        for (int py : phase) reads += mark_reads(Af, A, ox, oy, px, py);
        }
    if (reads == 0) return 1;
    printf("atlas frontier layout host test ok: %d sets, %d parts, %ld visibility reads\n", sets, parts, reads);
    return 0;
}
