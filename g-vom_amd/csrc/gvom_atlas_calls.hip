// gvom_atlas_calls.hip -- the map atlas's entry points (include/gvom_hip.h "map atlas"): gvom_atlas_configure, _integrate, _recall,
// _extent, _clear and _counts.  The kernels are gvom_atlas.hip's; everything runs on the handle's stream -- behind the combine that
// wrote the set an integrate reads, in front of whatever recycles that set later -- and only gvom_atlas_counts waits for it.  A recall
// writes a map set of the pool gvom_combine_maps_device takes its sets from (map_set_acquire, gvom_sets.hip) and a product set for the
// stamps; the extent export is a product like the others.
#include "gvom_host.h"

namespace {
const int64_t AT_FAR = (int64_t)1 << 40;                   // origins beyond this are refused, as in the other calls that take one
const int64_t AT_REL = (int64_t)1 << 30;                   // a window this far from the extent lies outside it wherever it is

struct Window { int rx, ry, px, py; };                     // a window as the kernels take it: relative to the extent, and its storage phase
Window window_of(const gvom_handle *h, const int64_t origin[2])
{
    const int64_t m = h->atl_A - 1;
    const int64_t rx = std::max(-AT_REL, std::min(AT_REL, origin[0] - h->atl_E[0])), ry = std::max(-AT_REL, std::min(AT_REL, origin[1] - h->atl_E[1]));
    return Window{(int)rx, (int)ry, (int)(origin[0] & m), (int)(origin[1] & m)};
}

// the nine maps of a set (any part of kind 0 exists: the layout table says where)
AtlasMaps maps_of_set(const DevSet *s)
{
    AtlasMaps M;
    SetPart d;
    for (int k = 0; k < 9; ++k) {
        set_part(s, k, &d);
        if (k < 3) M.i[k] = (int32_t *)d.ptr; else M.f[k - 3] = (unsigned long long *)d.ptr;
    }
    M.stamp = nullptr;
    return M;
}

bool origin_ok(const int64_t o[2]) { return o[0] >= -AT_FAR && o[0] <= AT_FAR && o[1] >= -AT_FAR && o[1] <= AT_FAR; }

// follow mode: the extent goes to `to`; the cells that entered it become UNKNOWN -- a strip of columns over every row, then a strip
// of rows over the remaining columns; a move of A or more on an axis is the first strip alone, A wide
int move_extent(gvom_handle *h, const int64_t to[2])
{
    const int A = h->atl_A;
    const int64_t m = A - 1, dx = to[0] - h->atl_E[0], dy = to[1] - h->atl_E[1];
    const int64_t ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
    const int wx = (ax >= A || ay >= A) ? A : (int)ax, wy = wx == A ? 0 : (int)ay;
    const int64_t sx = (dx > 0 && wx < A) ? to[0] + A - wx : to[0];                  // the strip of columns: [sx, sx + wx)
    const int64_t ox = (dx > 0 || wx == A) ? to[0] : to[0] + wx;                     // the other columns: [ox, ox + A - wx)
    const int64_t sy = dy > 0 ? to[1] + A - wy : to[1];                              // the strip of rows: [sy, sy + wy)
    HIPCHK(h, gvom_launch_atlas_move(h->stream, h->atl_mem, A, (int)(sx & m), (int)(to[1] & m), wx, A, h->atl_cnt));
    HIPCHK(h, gvom_launch_atlas_move(h->stream, h->atl_mem, A, (int)(ox & m), (int)(sy & m), A - wx, wy, h->atl_cnt));
    h->atl_E[0] = to[0]; h->atl_E[1] = to[1];
    return GVOM_OK;
}

int need_atlas(gvom_handle *h, const char *fn)
{
    if (h->sharded) { h->err = std::string(fn) + ": sharded handles are not supported"; return GVOM_ERR_INVALID; }
    if (!h->atl_A) { h->err = std::string(fn) + ": no atlas is configured (gvom_atlas_configure)"; return GVOM_ERR_INVALID; }
    return GVOM_OK;
}
}  // namespace

extern "C" {
VIS int gvom_atlas_configure(gvom_t *h, int32_t cells, int mode, const int64_t fixed_origin[2])
{
    if (!h) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->sharded) { h->err = "gvom_atlas_configure: sharded handles are not supported"; return GVOM_ERR_INVALID; }
    if (cells != 0) {
        if (cells < GVOM_ATLAS_MIN_CELLS || cells > GVOM_ATLAS_MAX_CELLS || (cells & (cells - 1))) { h->err = "gvom_atlas_configure: the side must be a power of two in 64 .. 4096"; return GVOM_ERR_INVALID; }
        if (cells < h->prm.xy_size) { h->err = "gvom_atlas_configure: the atlas must be at least as large as the window (xy_size)"; return GVOM_ERR_INVALID; }
        if (mode != GVOM_ATLAS_FOLLOW && mode != GVOM_ATLAS_FIXED) { h->err = "gvom_atlas_configure: unknown mode"; return GVOM_ERR_INVALID; }
        if (fixed_origin && !origin_ok(fixed_origin)) { h->err = "gvom_atlas_configure: an origin beyond 2^40 cells"; return GVOM_ERR_INVALID; }
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (cells != h->atl_A) {                                                // another size, or none: the kernels that use the old one first
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (h->atl_mem) HIPCHK(h, hipFree(h->atl_mem));
        h->atl_mem = nullptr; h->atl_A = 0;
        if (cells == 0) return GVOM_OK;
        HIPCHK(h, hipMalloc((void **)&h->atl_mem, gvom_atlas_bytes(cells)));
        ++h->atl_allocs;
    }
    if (cells == 0) return GVOM_OK;
    if (!h->atl_cnt) { HIPCHK(h, hipMalloc((void **)&h->atl_cnt, 256)); ++h->atl_allocs; }
    if (!h->atl_pin) HIPCHK(h, hipHostMalloc((void **)&h->atl_pin, 256, hipHostMallocDefault));
    h->atl_A = cells; h->atl_follow = mode == GVOM_ATLAS_FOLLOW ? 1 : 0;
    h->atl_E[0] = fixed_origin ? fixed_origin[0] : 0; h->atl_E[1] = fixed_origin ? fixed_origin[1] : 0;
    h->atl_seq = 0;
    for (int k = 0; k < 3; ++k) h->atl_last[k] = 0;
    HIPCHK(h, join_second_stream(h));
    HIPCHK(h, hipMemsetAsync(h->atl_cnt, 0, 256, h->stream));
    HIPCHK(h, gvom_launch_atlas_fill(h->stream, h->atl_mem, cells, 0, (size_t)cells * cells));
    return GVOM_OK;
}

VIS int gvom_atlas_clear(gvom_t *h)
{
    if (!h) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    const int rc = need_atlas(h, "gvom_atlas_clear");
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, join_second_stream(h));
    HIPCHK(h, hipMemsetAsync(h->atl_cnt, 0, 256, h->stream));
    HIPCHK(h, gvom_launch_atlas_fill(h->stream, h->atl_mem, h->atl_A, 0, (size_t)h->atl_A * h->atl_A));
    return GVOM_OK;
}

VIS int gvom_atlas_integrate(gvom_t *h, int64_t map_set_id, const void *const maps[9], int on_device, const int64_t origin_cells[2])
{
    if (!h) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    int rc = need_atlas(h, "gvom_atlas_integrate");
    if (rc) return rc;
    if (map_set_id >= 0 && (maps || origin_cells)) { h->err = "gvom_atlas_integrate: give a map set id or nine maps and their origin, not both"; return GVOM_ERR_INVALID; }
    if (map_set_id < 0 && (!maps || !origin_cells)) { h->err = "gvom_atlas_integrate: give a map set id or nine maps and their origin"; return GVOM_ERR_INVALID; }
    const int xy = h->prm.xy_size;
    const size_t n2 = (size_t)xy * xy;
    int64_t O[3] = {0, 0, h->atl_last[2]};
    AtlasMaps in;
    if (map_set_id >= 0) {
        DevSet *m = find_set(h->dsets, map_set_id);
        if (!m) { h->err = "unknown or stale device map set id"; return GVOM_ERR_INVALID; }
        in = maps_of_set(m);
        for (int k = 0; k < 3; ++k) O[k] = m->origin[k];
    } else {
        for (int k = 0; k < 9; ++k)
            if (!maps[k]) { h->err = "gvom_atlas_integrate: one of the nine maps is NULL"; return GVOM_ERR_INVALID; }
        if (!origin_ok(origin_cells)) { h->err = "gvom_atlas_integrate: an origin beyond 2^40 cells"; return GVOM_ERR_INVALID; }
        O[0] = origin_cells[0]; O[1] = origin_cells[1];
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, join_second_stream(h));
    if (map_set_id < 0 && !on_device) {                                     // host maps: staged, and up before the call returns
        if (h->atl_stage.bytes < n2 * 60) {
            if ((rc = ensure(h, h->atl_stage, n2 * 60))) return rc;
            ++h->atl_allocs;
        }
        char *st = (char *)h->atl_stage.p;
        for (int k = 0; k < 9; ++k) {
            char *at = k >= 3 ? st + (size_t)(k - 3) * n2 * 8 : st + 6 * n2 * 8 + (size_t)k * n2 * 4;
            HIPCHK(h, hipMemcpyAsync(at, maps[k], n2 * (k >= 3 ? 8 : 4), hipMemcpyHostToDevice, h->stream));
            if (k < 3) in.i[k] = (int32_t *)at; else in.f[k - 3] = (unsigned long long *)at;
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
    } else if (map_set_id < 0) {
        for (int k = 0; k < 9; ++k)
            if (k < 3) in.i[k] = (int32_t *)maps[k]; else in.f[k - 3] = (unsigned long long *)maps[k];
    }
    in.stamp = nullptr;
    HIPCHK(h, hipMemsetAsync(h->atl_cnt, 0, 24, h->stream));                // the six counters of the last integrate
    if (h->atl_follow) {
        const int64_t to[2] = {O[0] + xy / 2 - h->atl_A / 2, O[1] + xy / 2 - h->atl_A / 2};
        if ((rc = move_extent(h, to))) return rc;
    }
    const Window w = window_of(h, O);
    ++h->atl_seq;
    for (int k = 0; k < 3; ++k) h->atl_last[k] = O[k];
    HIPCHK(h, gvom_launch_atlas_merge(h->stream, h->atl_mem, h->atl_A, in, xy, w.rx, w.ry, w.px, w.py, h->atl_seq, h->atl_cnt));
    return GVOM_OK;
}

VIS int gvom_atlas_recall(gvom_t *h, const int64_t origin_cells[2], int64_t *set_id, int64_t *product_id, double origin_world[3])
{
    if (!h || !set_id || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *set_id = *product_id = -1;
    int rc = need_atlas(h, "gvom_atlas_recall");
    if (rc) return rc;
    if (origin_cells && !origin_ok(origin_cells)) { h->err = "gvom_atlas_recall: an origin beyond 2^40 cells"; return GVOM_ERR_INVALID; }
    const int64_t R[2] = {origin_cells ? origin_cells[0] : h->atl_last[0], origin_cells ? origin_cells[1] : h->atl_last[1]};
    const int xy = h->prm.xy_size;
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *set = nullptr, *pset = nullptr;
    if ((rc = map_set_acquire(h, "gvom_atlas_recall", &set))) return rc;
    const size_t bytes = set_bytes(GVOM_PRODUCT_ATLAS_RECALL, xy, 0, 0);
    if ((rc = product_acquire(h, GVOM_PRODUCT_ATLAS_RECALL, bytes, bytes, "gvom_atlas_recall", &h->atl_allocs, &pset))) return rc;
    HIPCHK(h, join_second_stream(h));
    if ((rc = set_wait_releases(h, set)) || (rc = set_wait_releases(h, pset))) return rc;
    AtlasMaps out = maps_of_set(set);
    SetPart d;
    set_part(pset, 0, &d); out.stamp = (int32_t *)d.ptr;
    set_part(pset, 1, &d);
    HIPCHK(h, hipMemsetAsync(d.ptr, 0, 16, h->stream));
    const Window w = window_of(h, R);
    HIPCHK(h, gvom_launch_atlas_recall(h->stream, h->atl_mem, h->atl_A, out, xy, w.rx, w.ry, w.px, w.py, h->atl_seq, (int32_t *)d.ptr));
    HIPCHK(h, hipEventRecord(set->ready, h->stream));
    if ((rc = product_publish(h, pset, product_id))) return rc;
    set->origin[0] = R[0]; set->origin[1] = R[1]; set->origin[2] = h->atl_last[2];
    set->id = ++h->dset_seq;
    *set_id = set->id;
    if (origin_world) {
        origin_world[0] = (double)R[0] * h->prm.xy_resolution; origin_world[1] = (double)R[1] * h->prm.xy_resolution;
        origin_world[2] = (double)h->atl_last[2] * h->prm.z_resolution;
    }
    return GVOM_OK;
}

VIS int gvom_atlas_extent(gvom_t *h, int64_t *product_id, int64_t extent_origin[2])
{
    if (!h || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *product_id = -1;
    int rc = need_atlas(h, "gvom_atlas_extent");
    if (rc) return rc;
    const int A = h->atl_A;
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *pset = nullptr;
    const size_t bytes = set_bytes(GVOM_PRODUCT_ATLAS_EXTENT, 0, 0, A);
    if ((rc = product_acquire(h, GVOM_PRODUCT_ATLAS_EXTENT, bytes, bytes, "gvom_atlas_extent", &h->atl_allocs, &pset))) return rc;
    pset->cap = A;
    HIPCHK(h, join_second_stream(h));
    if ((rc = set_wait_releases(h, pset))) return rc;
    AtlasMaps out;
    memset(&out, 0, sizeof out);
    SetPart d;
    for (int k = 0; k < 3; ++k) { set_part(pset, k, &d); out.i[k] = (int32_t *)d.ptr; }
    for (int k = 0; k < 2; ++k) { set_part(pset, 3 + k, &d); out.f[k] = (unsigned long long *)d.ptr; }
    set_part(pset, 5, &d); out.stamp = (int32_t *)d.ptr;
    const Window w = window_of(h, h->atl_E);
    HIPCHK(h, gvom_launch_atlas_recall(h->stream, h->atl_mem, A, out, A, 0, 0, w.px, w.py, h->atl_seq, nullptr));
    if (extent_origin) { extent_origin[0] = h->atl_E[0]; extent_origin[1] = h->atl_E[1]; }
    return product_publish(h, pset, product_id);
}

VIS int gvom_atlas_counts(gvom_t *h, int64_t out[8])
{
    if (!h || !out) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    const int rc = need_atlas(h, "gvom_atlas_counts");
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(h->atl_pin, h->atl_cnt, 32, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int k = 0; k < 7; ++k) out[k] = h->atl_pin[k];
    out[7] = h->atl_seq;
    return GVOM_OK;
}
}  // extern "C"
