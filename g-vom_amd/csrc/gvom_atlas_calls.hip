// gvom_atlas_calls.hip -- the map atlas's entry points (include/gvom_hip.h "map atlas"): gvom_atlas_configure, _integrate, _recall,
// _extent, _clear and _counts.  The kernels are gvom_atlas.hip's; everything runs on the handle's stream -- behind the combine that
// wrote the set an integrate reads, in front of whatever recycles that set later -- and only gvom_atlas_counts waits for it.  A recall
// writes a map set of the pool gvom_combine_maps_device takes its sets from (map_set_acquire, gvom_sets.hip) and a product set for the
// stamps; the extent export is a product like the others.  Below them the atlas fields (include/gvom_hip.h "atlas fields"):
// gvom_atlas_cost_to_go, which waits like gvom_cost_to_go, and gvom_atlas_field_window; their kernels are gvom_atlas_field.hip's.  Last
// the atlas frontiers (include/gvom_hip.h "atlas frontiers"): gvom_atlas_frontiers, which waits like gvom_frontiers.  The checks, the work
// buffers, the solves and their epilogues that these share with the window's calls are gvom_product_calls.hip's (gvom_host.h lists them).
#include "gvom_host.h"

namespace {
const int64_t AT_FAR = (int64_t)1 << 40;                   // origins beyond this are refused, as in the other calls that take one
const int64_t AT_REL = (int64_t)1 << 30;                   // a window this far from the extent lies outside it wherever it is

struct Window { int rx, ry, px, py; };                     // a window as the kernels take it: relative to the extent, and its storage phase
Window window_of(const gvom_handle *h, const int64_t origin[2])
{
    const int64_t m = h->atlas.A - 1;
    const int64_t rx = std::max(-AT_REL, std::min(AT_REL, origin[0] - h->atlas.E[0])), ry = std::max(-AT_REL, std::min(AT_REL, origin[1] - h->atlas.E[1]));
    return Window{(int)rx, (int)ry, (int)(origin[0] & m), (int)(origin[1] & m)};
}

// the nine maps of a set (any part of kind 0 exists: the layout table says where)
AtlasMaps maps_of_set(const DevSet *s)
{
    AtlasMaps M;
    for (int k = 0; k < 3; ++k) M.i[k] = part_ptr<int32_t>(s, k);
    for (int k = 3; k < 9; ++k) M.f[k - 3] = part_ptr<unsigned long long>(s, k);
    M.stamp = nullptr;
    return M;
}

bool origin_ok(const int64_t o[2]) { return o[0] >= -AT_FAR && o[0] <= AT_FAR && o[1] >= -AT_FAR && o[1] <= AT_FAR; }

// follow mode: the extent goes to `to`; the cells that entered it become UNKNOWN -- a strip of columns over every row, then a strip
// of rows over the remaining columns; a move of A or more on an axis is the first strip alone, A wide
int move_extent(gvom_handle *h, const int64_t to[2])
{
    const int A = h->atlas.A;
    const int64_t m = A - 1, dx = to[0] - h->atlas.E[0], dy = to[1] - h->atlas.E[1];
    const int64_t ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
    const int wx = (ax >= A || ay >= A) ? A : (int)ax, wy = wx == A ? 0 : (int)ay;
    const int64_t sx = (dx > 0 && wx < A) ? to[0] + A - wx : to[0];                  // the strip of columns: [sx, sx + wx)
    const int64_t ox = (dx > 0 || wx == A) ? to[0] : to[0] + wx;                     // the other columns: [ox, ox + A - wx)
    const int64_t sy = dy > 0 ? to[1] + A - wy : to[1];                              // the strip of rows: [sy, sy + wy)
    HIPCHK(h, gvom_launch_atlas_move(h->stream, h->atlas.mem, A, (int)(sx & m), (int)(to[1] & m), wx, A, h->atlas.cnt));
    HIPCHK(h, gvom_launch_atlas_move(h->stream, h->atlas.mem, A, (int)(ox & m), (int)(sy & m), A - wx, wy, h->atlas.cnt));
    h->atlas.E[0] = to[0]; h->atlas.E[1] = to[1];
    return GVOM_OK;
}

int need_atlas(gvom_handle *h, const char *fn)
{
    if (h->sharded) return refuse(h, fn, "sharded handles are not supported");
    return h->atlas.A ? GVOM_OK : refuse(h, fn, "no atlas is configured (gvom_atlas_configure)");
}
}  // namespace

extern "C" {
VIS int gvom_atlas_configure(gvom_t *h, int32_t cells, int mode, const int64_t fixed_origin[2])
{
    if (!h) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->sharded) return refuse(h, "gvom_atlas_configure", "sharded handles are not supported");
    if (cells != 0) {
        if (cells < GVOM_ATLAS_MIN_CELLS || cells > GVOM_ATLAS_MAX_CELLS || (cells & (cells - 1))) { h->err = "gvom_atlas_configure: the side must be a power of two in 64 .. 4096"; return GVOM_ERR_INVALID; }
        if (cells < h->prm.xy_size) { h->err = "gvom_atlas_configure: the atlas must be at least as large as the window (xy_size)"; return GVOM_ERR_INVALID; }
        if (mode != GVOM_ATLAS_FOLLOW && mode != GVOM_ATLAS_FIXED) { h->err = "gvom_atlas_configure: unknown mode"; return GVOM_ERR_INVALID; }
        if (fixed_origin && !origin_ok(fixed_origin)) { h->err = "gvom_atlas_configure: an origin beyond 2^40 cells"; return GVOM_ERR_INVALID; }
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (cells != h->atlas.A) {                                              // another size, or none: the kernels that use the old one first
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (h->atlas.mem) HIPCHK(h, hipFree(h->atlas.mem.p));
        h->atlas.mem.p = nullptr; h->atlas.A = 0;
        if (cells == 0) return GVOM_OK;
        HIPCHK(h, hipMalloc((void **)&h->atlas.mem.p, gvom_atlas_bytes(cells)));
        ++h->atlas.allocs;
    }
    if (cells == 0) return GVOM_OK;
    if (!h->atlas.cnt) { HIPCHK(h, hipMalloc((void **)&h->atlas.cnt.p, 256)); ++h->atlas.allocs; }
    if (!h->atlas.pin) HIPCHK(h, hipHostMalloc((void **)&h->atlas.pin.p, 256, hipHostMallocDefault));
    h->atlas.A = cells; h->atlas.follow = mode == GVOM_ATLAS_FOLLOW ? 1 : 0;
    h->atlas.E[0] = fixed_origin ? fixed_origin[0] : 0; h->atlas.E[1] = fixed_origin ? fixed_origin[1] : 0;
    h->atlas.seq = 0;
    for (int k = 0; k < 3; ++k) h->atlas.last[k] = 0;
    HIPCHK(h, join_second_stream(h));
    HIPCHK(h, hipMemsetAsync(h->atlas.cnt, 0, 256, h->stream));
    HIPCHK(h, gvom_launch_atlas_fill(h->stream, h->atlas.mem, cells, 0, (size_t)cells * cells));
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
    HIPCHK(h, hipMemsetAsync(h->atlas.cnt, 0, 256, h->stream));
    HIPCHK(h, gvom_launch_atlas_fill(h->stream, h->atlas.mem, h->atlas.A, 0, (size_t)h->atlas.A * h->atlas.A));
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
    int64_t O[3] = {0, 0, h->atlas.last[2]};
    AtlasMaps in;
    if (map_set_id >= 0) {
        DevSet *m = nullptr;
        if ((rc = map_set_of(h, map_set_id, &m))) return rc;
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
        if ((rc = stage_buf(h, h->atlas, n2 * 60))) return rc;
        char *st = (char *)h->atlas.stage.p;
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
    HIPCHK(h, hipMemsetAsync(h->atlas.cnt, 0, 24, h->stream));              // the six counters of the last integrate
    if (h->atlas.follow) {
        const int64_t to[2] = {O[0] + xy / 2 - h->atlas.A / 2, O[1] + xy / 2 - h->atlas.A / 2};
        if ((rc = move_extent(h, to))) return rc;
    }
    const Window w = window_of(h, O);
    ++h->atlas.seq;
    for (int k = 0; k < 3; ++k) h->atlas.last[k] = O[k];
    HIPCHK(h, gvom_launch_atlas_merge(h->stream, h->atlas.mem, h->atlas.A, in, xy, w.rx, w.ry, w.px, w.py, h->atlas.seq, h->atlas.cnt));
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
    const int64_t R[2] = {origin_cells ? origin_cells[0] : h->atlas.last[0], origin_cells ? origin_cells[1] : h->atlas.last[1]};
    const int xy = h->prm.xy_size;
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *set = nullptr, *pset = nullptr;
    if ((rc = map_set_acquire(h, "gvom_atlas_recall", &set))) return rc;
    const size_t bytes = set_bytes(GVOM_PRODUCT_ATLAS_RECALL, xy, 0, 0);
    if ((rc = product_acquire(h, GVOM_PRODUCT_ATLAS_RECALL, bytes, bytes, "gvom_atlas_recall", &h->atlas, &pset))) return rc;
    HIPCHK(h, join_second_stream(h));
    if ((rc = set_wait_releases(h, set)) || (rc = set_wait_releases(h, pset))) return rc;
    AtlasMaps out = maps_of_set(set);
    out.stamp = part_ptr<int32_t>(pset, 0);
    int32_t *const counts = part_ptr<int32_t>(pset, 1);
    HIPCHK(h, hipMemsetAsync(counts, 0, 16, h->stream));
    const Window w = window_of(h, R);
    HIPCHK(h, gvom_launch_atlas_recall(h->stream, h->atlas.mem, h->atlas.A, out, xy, w.rx, w.ry, w.px, w.py, h->atlas.seq, counts));
    HIPCHK(h, hipEventRecord(set->ready, h->stream));
    if ((rc = product_publish(h, pset, product_id))) return rc;
    set->origin[0] = R[0]; set->origin[1] = R[1]; set->origin[2] = h->atlas.last[2];
    set->id = ++h->dset_seq;
    *set_id = set->id;
    if (origin_world) {
        origin_world[0] = (double)R[0] * h->prm.xy_resolution; origin_world[1] = (double)R[1] * h->prm.xy_resolution;
        origin_world[2] = (double)h->atlas.last[2] * h->prm.z_resolution;
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
    const int A = h->atlas.A;
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *pset = nullptr;
    const size_t bytes = set_bytes(GVOM_PRODUCT_ATLAS_EXTENT, 0, 0, A);
    if ((rc = product_acquire(h, GVOM_PRODUCT_ATLAS_EXTENT, bytes, bytes, "gvom_atlas_extent", &h->atlas, &pset))) return rc;
    pset->cap = A;
    HIPCHK(h, join_second_stream(h));
    if ((rc = set_wait_releases(h, pset))) return rc;
    AtlasMaps out;
    memset(&out, 0, sizeof out);
    for (int k = 0; k < 3; ++k) out.i[k] = part_ptr<int32_t>(pset, k);
    for (int k = 0; k < 2; ++k) out.f[k] = part_ptr<unsigned long long>(pset, 3 + k);
    out.stamp = part_ptr<int32_t>(pset, 5);
    const Window w = window_of(h, h->atlas.E);
    HIPCHK(h, gvom_launch_atlas_recall(h->stream, h->atlas.mem, A, out, A, 0, 0, w.px, w.py, h->atlas.seq, nullptr));
    if (extent_origin) { extent_origin[0] = h->atlas.E[0]; extent_origin[1] = h->atlas.E[1]; }
    return product_publish(h, pset, product_id);
}

VIS int gvom_atlas_counts(gvom_t *h, int64_t out[8])
{
    if (!h || !out) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    const int rc = need_atlas(h, "gvom_atlas_counts");
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(h->atlas.pin, h->atlas.cnt, 32, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int k = 0; k < 7; ++k) out[k] = h->atlas.pin[k];
    out[7] = h->atlas.seq;
    return GVOM_OK;
}

// ---- atlas fields (include/gvom_hip.h "atlas fields") -----------------------------------------------------------------------------------
// gvom_cost_to_go's solve at the atlas's side: the front ends of gvom_atlas_field.hip read the toroidal planes in place and write the
// unwrapped obstacle distances and cost map, k_clearance_cols and the solver (ctg_solve, gvom_product_calls.hip) run on those as on any
// [y][x] map of A x A cells.  The buffers are the handle's own at side A (atlas_field.solve.work, atlas_field.clr): gvom_cost_to_go's stay as they are.
VIS int gvom_atlas_cost_to_go(gvom_t *h, const gvom_ctg_params *params, const int64_t *goals, int64_t n_goals, int32_t max_cost,
                              int32_t max_rounds, int flags, int64_t *product_id, int64_t info[4], int64_t extent_origin[2])
{
    if (!h || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *product_id = -1;
    for (int k = 0; info && k < 4; ++k) info[k] = 0;
    const char *const fn = "gvom_atlas_cost_to_go";
    int rc = need_atlas(h, fn);
    if (rc) return rc;
    if (flags & ~(GVOM_CTG_NO_NEGATIVE | GVOM_CTG_UNKNOWN_BLOCKS)) { h->err = "gvom_atlas_cost_to_go: unknown flag bits"; return GVOM_ERR_INVALID; }
    if (!params) { h->err = "gvom_atlas_cost_to_go: the cost parameters must not be NULL"; return GVOM_ERR_INVALID; }
    if ((rc = check_goals(h, fn, goals, n_goals, max_cost, max_rounds))) return rc;
    CtgCostParams C;
    if ((rc = ctg_cost_params(h, fn, params, flags, &C))) return rc;
    const int A = h->atlas.A;
    const int64_t E[2] = {h->atlas.E[0], h->atlas.E[1]};
    std::vector<int32_t> rel((size_t)2 * n_goals);                          // the goals as the solver takes them: extent cells
    for (int64_t k = 0; k < 2 * n_goals; ++k) {
        const int64_t g = goals[k], e = E[k & 1];
        if (g < e || g >= e + A) {
            h->err = "gvom_atlas_cost_to_go: a goal lies outside the extent: cell (" + std::to_string(goals[k & ~(int64_t)1]) + ", " +
                     std::to_string(goals[k | 1]) + "), extent [" + std::to_string(E[0]) + ", " + std::to_string(E[0] + A) + ") x [" +
                     std::to_string(E[1]) + ", " + std::to_string(E[1] + A) + ")";
            return GVOM_ERR_INVALID;
        }
        rel[k] = (int32_t)(g - e);
    }
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *set = nullptr;
    const size_t a2 = (size_t)A * A, bytes = set_bytes(GVOM_PRODUCT_ATLAS_FIELD, 0, 0, A);
    if ((rc = product_acquire(h, GVOM_PRODUCT_ATLAS_FIELD, bytes, bytes, fn, &h->atlas_field, &set))) return rc;
    set->cap = A;
    const int nt = gvom_ctg_tiles(A);
    const GoalWork lay = goal_work(nt * nt, 8, 0);
    if ((rc = solve_work_reserve(h, h->atlas_field, lay.end))) return rc;
    const size_t clr_g = align256(a2 * 2), clr_map = align256(a2 * 4);
    if (C.inflation_cells2 > 0 && (rc = stage_buf(h, h->atlas_field, h->atlas_field.clr, clr_g + 2 * clr_map))) return rc;
    const GoalWorkPtrs G = goal_work_ptrs(h->atlas_field.solve, lay);
    HIPCHK(h, join_second_stream(h));
    if ((rc = goal_work_start(h, G, rel.data(), (size_t)n_goals * 8)) || (rc = set_wait_releases(h, set))) return rc;
    int32_t *D = part_ptr<int32_t>(set, 0);
    uint8_t *dir = part_ptr<uint8_t>(set, 1);
    uint16_t *c16 = part_ptr<uint16_t>(set, 2);
    const Window w = window_of(h, E);                                       // (its storage phase is the extent's)
    const int32_t *cd2 = nullptr;
    if (C.inflation_cells2 > 0) {
        char *q = (char *)h->atlas_field.clr.p;
        HIPCHK(h, gvom_launch_atlas_clearance_rows(h->stream, h->atlas.mem, A, w.px, w.py, C.use_negative != 0, C.density_threshold, (uint16_t *)q));
        HIPCHK(h, gvom_launch_clearance_cols(h->stream, A, h->prm.xy_resolution, C.inflation_cells2, (const uint16_t *)q, (float *)(q + clr_g),
                                             (int32_t *)(q + clr_g + clr_map)));
        cd2 = (const int32_t *)(q + clr_g + clr_map);
    }
    HIPCHK(h, gvom_launch_atlas_travcost(h->stream, h->atlas.mem, A, w.px, w.py, cd2, C, c16));
    SolveRounds S;
    if ((rc = ctg_solve(h, h->atlas_field.solve, G, A, nullptr, c16, D, dir, (int)n_goals, max_cost, max_rounds, &S))) return rc;
    set->origin[0] = E[0]; set->origin[1] = E[1]; set->origin[2] = 0;
    if ((rc = goal_solve_finish(h, fn, h->atlas_field.solve, set, product_id, S, max_rounds, info))) return rc;
    if (extent_origin) { extent_origin[0] = E[0]; extent_origin[1] = E[1]; }
    return GVOM_OK;
}

VIS int gvom_atlas_field_window(gvom_t *h, int64_t field_id, int64_t map_set_id, const int64_t origin_cells[2], int64_t *product_id)
{
    if (!h || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *product_id = -1;
    const char *const fn = "gvom_atlas_field_window";
    if (h->sharded) return refuse(h, fn, "sharded handles are not supported");
    DevSet *f = nullptr;
    int rc;
    if ((rc = atlas_field_of(h, fn, field_id, &f)) || (rc = check_one_source(h, fn, map_set_id >= 0, origin_cells, !origin_cells, "a map set id", "origin_cells", "origin_cells"))) return rc;
    int64_t R[2];
    if (map_set_id >= 0) {
        DevSet *m = nullptr;
        if ((rc = map_set_of(h, map_set_id, &m))) return rc;
        R[0] = m->origin[0]; R[1] = m->origin[1];
    } else {
        if (!origin_ok(origin_cells)) { h->err = "gvom_atlas_field_window: an origin beyond 2^40 cells"; return GVOM_ERR_INVALID; }
        R[0] = origin_cells[0]; R[1] = origin_cells[1];
    }
    const int xy = h->prm.xy_size, A = (int)f->cap;
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *set = nullptr;
    const size_t bytes = set_bytes(GVOM_PRODUCT_COSTFIELD, xy, 0, 0);
    if ((rc = product_acquire(h, GVOM_PRODUCT_COSTFIELD, bytes, bytes, fn, &h->atlas_field, &set))) return rc;
    HIPCHK(h, join_second_stream(h));
    if ((rc = set_wait_releases(h, set))) return rc;
    const int rx = (int)std::max(-AT_REL, std::min(AT_REL, R[0] - f->origin[0])), ry = (int)std::max(-AT_REL, std::min(AT_REL, R[1] - f->origin[1]));
    HIPCHK(h, gvom_launch_atlas_field_window(h->stream, A, part_ptr<const int32_t>(f, 0), part_ptr<const uint8_t>(f, 1), part_ptr<const uint16_t>(f, 2), xy, rx, ry,
                                             part_ptr<int32_t>(set, 0), part_ptr<uint8_t>(set, 1), part_ptr<uint16_t>(set, 2)));
    return product_publish(h, set, product_id);
}

// ---- atlas frontiers (include/gvom_hip.h "atlas frontiers") ------------------------------------------------------------------------------
// gvom_frontiers at the side of an atlas field: k_atlas_frontier_mark (gvom_atlas_frontier.hip) reads c and D from the field and the
// visibility in place from the atlas as it is now, everything behind it is frontier_solve (gvom_product_calls.hip) on a work buffer of
// the handle's own at that side (atlas_frontiers.solve.work): gvom_frontiers' window-sized one stays as it is.
VIS int gvom_atlas_frontiers(gvom_t *h, int64_t field_id, int32_t min_cells, int32_t max_clusters, int64_t *product_id, int64_t info[4],
                             int64_t extent_origin[2])
{
    if (!h || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *product_id = -1;
    for (int k = 0; info && k < 4; ++k) info[k] = 0;
    const char *const fn = "gvom_atlas_frontiers";
    int rc = need_atlas(h, fn);
    if (rc) return rc;
    DevSet *f = nullptr;
    if ((rc = atlas_field_of(h, fn, field_id, &f)) || (rc = check_clusters(h, fn, min_cells, max_clusters))) return rc;
    const int Af = (int)f->cap;
    const int64_t F[2] = {f->origin[0], f->origin[1]};
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *set = nullptr;
    const size_t bytes = set_bytes(GVOM_PRODUCT_ATLAS_FRONTIERS, 0, 0, max_clusters, Af);
    if ((rc = product_acquire(h, GVOM_PRODUCT_ATLAS_FRONTIERS, bytes, bytes, fn, &h->atlas_frontiers, &set))) return rc;
    set->cap = max_clusters; set->cols = Af;
    FrWork W;
    if ((rc = frontier_work(h, h->atlas_frontiers, Af, &W))) return rc;
    HIPCHK(h, join_second_stream(h));
    HIPCHK(h, hipMemsetAsync(W.cnt, 0, W.clear_bytes, h->stream));          // the counters and both halves of the flags
    if ((rc = set_wait_releases(h, set))) return rc;
    const int32_t *D = part_ptr<const int32_t>(f, 0);
    const uint16_t *c16 = part_ptr<const uint16_t>(f, 2);
    const Window w = window_of(h, F);                                       // the field's corner relative to the extent as it is now
    const Window e = window_of(h, h->atlas.E);                              // (its storage phase is the extent's)
    HIPCHK(h, gvom_launch_atlas_frontier_mark(h->stream, Af, c16, D, h->atlas.mem, h->atlas.A, w.rx, w.ry, e.px, e.py, W.L, W.count, W.fl,
                                              W.cnt + FR_CNT_CELLS));
    if ((rc = frontier_solve(h, fn, h->atlas_frontiers.solve, Af, D, W, min_cells, max_clusters, set, product_id, info))) return rc;
    set->origin[0] = F[0]; set->origin[1] = F[1]; set->origin[2] = 0;
    if (extent_origin) { extent_origin[0] = F[0]; extent_origin[1] = F[1]; }
    return GVOM_OK;
}
}  // extern "C"
