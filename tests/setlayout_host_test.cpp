// Stand-alone check of the device sets' layout table (g-vom_amd/csrc/gvom_setlayout.h): no GPU, no HIP.  set_bytes() sizes the one
// allocation of a set and set_part() places its parts in it; this program walks a map set (kind 0) and every product kind over small,
// odd, tile-sized and the largest shapes and checks that every part lies inside the allocation, on the boundary its consumers
// count on, apart from every other part, and is as long as its shape and element type say -- and that a part the kind does not have
// is refused.  Built with -fsanitize=address,undefined by tests/test_setlayout_host.py.
#include "../g-vom_amd/csrc/gvom_setlayout.h"

#include <stdio.h>
#include <stdlib.h>
#include <vector>

using namespace gvom_host;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed (kind %d xy %d zs %d cap %lld part %d)\n", __FILE__, __LINE__, #c, \
                                          s.kind, s.xy, s.zs, (long long)s.cap, part); exit(1); } } while (0)

static const int n_parts[8] = {9, 1, 3, 1, 1, 2, 2, 3};      // kind 0 (the nine maps), then GVOM_PRODUCT_* 1 .. 7

static int check_set(SetShape s, size_t bytes)
{
    int part = -1;
    SetPart d;
    CHECK(bytes > 0);
    CHECK(!set_part(&s, -1, &d));
    CHECK(!set_part(&s, n_parts[s.kind], &d));
    std::vector<SetPart> parts;
    for (part = 0; part < n_parts[s.kind]; ++part) {
        CHECK(set_part(&s, part, &d));
        const size_t off = (size_t)((char *)d.ptr - s.mem);
        // every part starts on a 256-byte boundary of the set, but the int32 maps of a map set: they follow one another at
        // dev_map_stride(xy) elements, a multiple of 32 -- 128 bytes
        const size_t boundary = (s.kind == 0 && part < 3) ? 128 : 256;
        CHECK((char *)d.ptr >= s.mem && off % boundary == 0);
        CHECK(off + d.bytes <= bytes);
        CHECK(d.ndim >= 1 && d.ndim <= 3 && (d.bits == 8 || d.bits == 16 || d.bits == 32 || d.bits == 64));
        int64_t n = 1;
        for (int k = 0; k < 3; ++k) { CHECK(d.shape[k] >= 1 && d.strides[k] >= 1); n *= d.shape[k]; }
        for (int k = d.ndim; k < 3; ++k) CHECK(d.shape[k] == 1);
        CHECK(d.bytes == (size_t)n * (d.bits / 8));
        // the strides address exactly the part: its last element ends where the part does
        int64_t last = 0;
        for (int k = 0; k < d.ndim; ++k) last += (d.shape[k] - 1) * d.strides[k];
        CHECK((size_t)(last + 1) * (d.bits / 8) == d.bytes);
        for (const SetPart &o : parts) CHECK((char *)d.ptr >= (char *)o.ptr + o.bytes || (char *)o.ptr >= (char *)d.ptr + d.bytes);
        parts.push_back(d);
    }
    return (int)parts.size();
}

int main()
{
    const int xys[] = {1, 15, 16, 64, 4096}, zss[] = {1, 32};
    const int64_t caps[] = {1, 3, (int64_t)1 << 26};
    char *const base = (char *)(uintptr_t)0x10000000;          // (never dereferenced: the table only does arithmetic on it)
    int sets = 0, parts = 0;
    for (int kind = 0; kind <= 7; ++kind)
        for (int xy : xys)
            for (int zs : zss)
                for (int64_t c : caps) {
                    const bool has_cap = kind == GVOM_PRODUCT_VOXEL_CLOUD || kind == GVOM_PRODUCT_RAYCAST;
                    if (!has_cap && c != caps[0]) continue;
                    SetShape s;
                    s.mem = base; s.kind = kind; s.xy = xy; s.zs = zs;
                    // a map set's `cap` is the distance between its maps: dev_map_stride(xy), xy*xy rounded up to 32 elements
                    s.cap = kind == 0 ? (int64_t)(((size_t)xy * xy + 31) & ~(size_t)31) : (has_cap ? c : 0);
                    parts += check_set(s, set_bytes(kind, xy, zs, s.cap));
                    ++sets;
                }
    SetShape s;
    SetPart d;
    int part = 0;
    s.mem = base; s.xy = 16; s.zs = 1; s.cap = 1;
    s.kind = 8; CHECK(!set_part(&s, 0, &d) && set_bytes(8, 16, 1, 1) == 0);      // no such kind
    s.kind = -1; CHECK(!set_part(&s, 0, &d) && set_bytes(-1, 16, 1, 1) == 0);
    printf("setlayout host test ok (%d sets, %d parts)\n", sets, parts);
    return 0;
}
