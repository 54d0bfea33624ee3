// gvom_debug.hip -- reads of the handle's state for tests, tools and the reference's debug attributes: every one of them waits
// for the GPU and copies through a temporary; none is on the per-step path.
#include "gvom_host.h"

extern "C" {
static void *map_ptr(gvom_handle *h, int which, size_t *esz, int *stride)
{
    *esz = 8; *stride = h->prm.xy_size;
    switch (which) {
    case GVOM_MAP_HEIGHT: *stride = h->hs; return h->height;
    case GVOM_MAP_INFERRED_HEIGHT: *stride = h->hs; return h->inferred;
    case GVOM_MAP_SLOPE_X: return h->slope_x;
    case GVOM_MAP_SLOPE_Y: return h->slope_y;
    case GVOM_MAP_ROUGHNESS: return h->rough;
    case GVOM_MAP_GUESSED_DELTA: return h->guessed;
    default: return nullptr;
    }
}

VIS int gvom_device_buffer(gvom_t *h, int which, void **ptr, int64_t *bytes, int64_t *row_stride_bytes)
{
    if (!h || !ptr) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    int64_t b = 0, rs = 0;
    switch (which) {
    case GVOM_BUF_HEIGHT_MAPS: *ptr = h->hmaps; rs = (int64_t)h->hs * 8; b = rs * h->prm.xy_size; break;
    case GVOM_BUF_FUSED_CELLS: *ptr = h->counters + 10; b = 8; rs = 8; break;
    default: return GVOM_ERR_INVALID;
    }
    if (bytes) *bytes = b;
    if (row_stride_bytes) *row_stride_bytes = rs;
    return GVOM_OK;
}

VIS int gvom_get_state(gvom_t *h, gvom_state *out)
{
    if (!h || !out) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    { const int rc0 = settle_count(h); if (rc0) return rc0; }
    memset(out, 0, sizeof *out);
    out->buffer_index = h->buffer_index;
    out->last_buffer_index = h->last_buffer_index;
    out->has_combined = h->has_combined ? 1 : 0;
    out->combined_cell_count = h->combined_cell_count;
    if (h->has_combined)
        for (int k = 0; k < 3; ++k) out->combined_origin[k] = (double)h->fused[h->cur].origin[k];
    for (int k = 0; k < 3; ++k) out->ego_position[k] = h->ego[k];
    return GVOM_OK;
}

VIS int gvom_slot_filled(gvom_t *h, int slot)
{
    if (!h || slot < 0 || slot >= h->prm.buffer_size) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    return h->slots[h->ring[slot]].filled ? 1 : 0;
}

VIS int gvom_read_dense(gvom_t *h, int which, int32_t *state, int32_t *hit, int32_t *total,
                        float *min_h, double origin[3], int64_t *cell_count)
{
    if (!h) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    const int32_t *st; const uint4 *cr; const uint32_t *tg; uint32_t ep; const int64_t *org; int64_t cnt;
    { const int rc0 = settle_count(h); if (rc0) return rc0; }
    if (which == GVOM_WHICH_FUSED) {
        if (!h->has_combined) return GVOM_NO_DATA;
        const Fused &F = h->fused[h->cur];
        st = F.state; cr = (const uint4 *)F.rows.p; org = F.origin; cnt = F.count; tg = F.tags; ep = F.epoch;
    } else {
        if (which < 0 || which >= h->prm.buffer_size) return GVOM_ERR_INVALID;
        const Slot &s = h->slots[h->ring[which]];
        if (!s.filled) return GVOM_NO_DATA;
        st = s.state; cr = (const uint4 *)s.crows.p; org = s.origin; cnt = s.count; tg = s.tags; ep = s.epoch;
    }
    const size_t V = h->V;
    int32_t *tmp = nullptr;
    HIPCHK(h, hipMalloc((void **)&tmp, V * 16));
    int om[3];
    window_phase(h, org, om);
    hipError_t e = join_second_stream(h);
    if (e == hipSuccess) e = gvom_launch_read_dense(h->stream, h->prm.xy_size, h->prm.z_size, om, h->sy_lo, h->sy_hi,
                                          tg, ep, st, cr,
                                          tmp, tmp + V, tmp + 2 * V, (float *)(tmp + 3 * V), nullptr);
    if (e == hipSuccess) e = sync_streams(h);
    if (e == hipSuccess && state) e = hipMemcpy(state, tmp, V * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && hit) e = hipMemcpy(hit, tmp + V, V * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && total) e = hipMemcpy(total, tmp + 2 * V, V * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && min_h) e = hipMemcpy(min_h, tmp + 3 * V, V * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && cell_count && cnt < 0) {       // a scan's occupied voxels are counted on demand
        std::vector<int32_t> stv(V);
        e = hipMemcpy(stv.data(), tmp, V * 4, hipMemcpyDeviceToHost);
        cnt = 0;
        for (size_t i = 0; i < V; ++i) cnt += stv[i] >= 0;
    }
    hipFree(tmp);
    HIPCHK(h, e);
    if (origin) for (int k = 0; k < 3; ++k) origin[k] = (double)org[k];
    if (cell_count) *cell_count = cnt;
    return GVOM_OK;
}

// Test hook / reference attributes metrics_buffer, combined_metrics (gvom.py:54-83,234,281; statistics
// handles only): rows_dense[V] = compact row of every occupied voxel of slot / fused map `which` in the
// reference's voxel order, -1 elsewhere.
VIS int gvom_read_rows(gvom_t *h, int which, int32_t *rows_dense)
{
    if (!h || !rows_dense) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    const int32_t *st; const uint32_t *tg; uint32_t ep; const int64_t *org;
    if (which == GVOM_WHICH_FUSED) {
        if (!h->has_combined) return GVOM_NO_DATA;
        const Fused &F = h->fused[h->cur];
        st = F.state; org = F.origin; tg = F.tags; ep = F.epoch;
    } else {
        if (which < 0 || which >= h->prm.buffer_size) return GVOM_ERR_INVALID;
        const Slot &sl = h->slots[h->ring[which]];
        if (!sl.filled) return GVOM_NO_DATA;
        st = sl.state; org = sl.origin; tg = sl.tags; ep = sl.epoch;
    }
    const size_t V = h->V;
    int32_t *tmp = nullptr;
    HIPCHK(h, hipMalloc((void **)&tmp, V * 4));
    int om[3];
    window_phase(h, org, om);
    hipError_t e = join_second_stream(h);
    if (e == hipSuccess) e = gvom_launch_read_dense(h->stream, h->prm.xy_size, h->prm.z_size, om, h->sy_lo, h->sy_hi, tg, ep, st,
                                          nullptr, nullptr, nullptr, nullptr, nullptr, tmp);
    if (e == hipSuccess) e = sync_streams(h);
    if (e == hipSuccess) e = hipMemcpy(rows_dense, tmp, V * 4, hipMemcpyDeviceToHost);
    hipFree(tmp);
    HIPCHK(h, e);
    return GVOM_OK;
}

// out[j][0..9] = the statistics of compact row rows[j] of slot `which` (float64: {mean xyz, covariance
// xx xy xz yy yz zz, count}) or of the fused map (float32).  GVOM_NO_DATA without GVOM_FLAG_VOXEL_STATISTICS.
VIS int gvom_gather_metrics(gvom_t *h, int which, const int32_t *rows, int64_t n, void *out)
{
    if (!h || !rows || !out || n < 0) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    stats_demand(h);
    HIPCHK(h, hipSetDevice(h->device));
    const void *src; int f64;
    if (which == GVOM_WHICH_FUSED) {
        if (!h->has_combined || !h->fused[h->cur].has_metrics) return GVOM_NO_DATA;
        src = h->fused[h->cur].metrics.p; f64 = 0;
    } else {
        if (which < 0 || which >= h->prm.buffer_size) return GVOM_ERR_INVALID;
        const Slot &sl = h->slots[h->ring[which]];
        if (!sl.filled || !sl.has_metrics) return GVOM_NO_DATA;
        src = sl.metrics.p; f64 = 1;
    }
    if (n == 0) return GVOM_OK;
    const size_t esz = f64 ? 8 : 4;
    char *tmp = nullptr;
    HIPCHK(h, hipMalloc((void **)&tmp, (size_t)n * 4 + (size_t)n * 10 * esz));
    hipError_t e = join_second_stream(h);
    if (e == hipSuccess) e = hipMemcpy(tmp + (size_t)n * 10 * esz, rows, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = gvom_launch_gather_rows10(h->stream, f64, src, (const int32_t *)(tmp + (size_t)n * 10 * esz), n, tmp);
    if (e == hipSuccess) e = sync_streams(h);
    if (e == hipSuccess) e = hipMemcpy(out, tmp, (size_t)n * 10 * esz, hipMemcpyDeviceToHost);
    hipFree(tmp);
    HIPCHK(h, e);
    return GVOM_OK;
}

VIS int gvom_read_map2d(gvom_t *h, int which2d, double *out)
{
    if (!h || !out) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->has_combined || !h->maps_valid) return GVOM_NO_DATA;
    HIPCHK(h, hipSetDevice(h->device));
    size_t esz; int stride; const double *src = (const double *)map_ptr(h, which2d, &esz, &stride);
    if (!src) return GVOM_ERR_INVALID;
    const Fused &F = h->fused[h->cur];
    double *tmp = nullptr;
    HIPCHK(h, hipMalloc((void **)&tmp, h->cells2d * 8));
    int om[3];
    window_phase(h, F.origin, om);
    hipError_t e = join_second_stream(h);
    if (e == hipSuccess) e = gvom_launch_unwrap_f64(h->stream, h->prm.xy_size, om[0], om[1], src, stride, tmp);
    if (e == hipSuccess) e = sync_streams(h);
    if (e == hipSuccess) e = hipMemcpy(out, tmp, h->cells2d * 8, hipMemcpyDeviceToHost);
    hipFree(tmp);
    HIPCHK(h, e);
    return GVOM_OK;
}

// reference: lookup.reshape((xy, xy, z), order='F') >= 0  -> out[x][y][z] (gvom.py:356-361): k_occupancy, then one copy of V bytes
VIS int gvom_get_occupancy(gvom_t *h, uint8_t *out_xyz)
{
    if (!h || !out_xyz) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->has_combined) return GVOM_NO_DATA;
    HIPCHK(h, hipSetDevice(h->device));
    const Fused &F = h->fused[h->cur];
    OccParams P;
    occ_params(h, F, P);
    uint8_t *tmp = nullptr;
    HIPCHK(h, hipMalloc((void **)&tmp, h->V));
    hipError_t e = join_second_stream(h);
    if (e == hipSuccess) e = gvom_launch_occupancy(h->stream, P, F.state, F.tags, tmp, h->tune_occ_clear != 0);
    if (e == hipSuccess) e = sync_streams(h);
    if (e == hipSuccess) e = hipMemcpy(out_xyz, tmp, h->V, hipMemcpyDeviceToHost);
    hipFree(tmp);
    HIPCHK(h, e);
    return GVOM_OK;
}

static int debug_maps(gvom_t *h, float *out7, float *out3)
{
    if (!h) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->has_combined || !h->maps_valid) return GVOM_NO_DATA;      // gvom.py:381-383
    HIPCHK(h, hipSetDevice(h->device));
    const Fused &F = h->fused[h->cur];
    const size_t n2 = h->cells2d;
    float *tmp = nullptr;
    HIPCHK(h, hipMalloc((void **)&tmp, n2 * 7 * 4));
    hipError_t e = join_second_stream(h);
    if (e == hipSuccess) e = launch_height_cloud(h, F, out7 ? tmp : nullptr, out3 ? tmp : nullptr);
    if (e == hipSuccess) e = sync_streams(h);
    if (e == hipSuccess) e = hipMemcpy(out7 ? out7 : out3, tmp, n2 * (out7 ? 7 : 3) * 4, hipMemcpyDeviceToHost);
    hipFree(tmp);
    HIPCHK(h, e);
    return GVOM_OK;
}

// Gvom.make_debug_voxel_map (gvom.py:363-378, kernels :1333-1378, :454-473)
VIS int gvom_debug_voxel_map(gvom_t *h, float *out, int64_t max_rows, int64_t *rows)
{
    return gvom_debug_voxel_eigen(h, out, nullptr, max_rows, rows);
}

// the same, also returning the three eigenvalues of every row (reference attribute voxels_eigenvalues,
// gvom.py:1333-1378), row for row with `out`
VIS int gvom_debug_voxel_eigen(gvom_t *h, float *out, float *eigen, int64_t max_rows, int64_t *rows)
{
    if (!h || !out || max_rows < 0) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    stats_demand(h);
    if (!h->has_combined || !h->fused[h->cur].has_metrics) return GVOM_NO_DATA;
    HIPCHK(h, hipSetDevice(h->device));
    const Fused &F = h->fused[h->cur];
    Map2dParams P;
    cloud_params(h, F, P);
    float *tmp = nullptr;
    const size_t mr = (size_t)(max_rows > 0 ? max_rows : 1);
    HIPCHK(h, hipMalloc((void **)&tmp, mr * 44));         // 8 + 3 floats per row
    float *tmp_e = eigen ? tmp + mr * 8 : nullptr;
    hipError_t e = join_second_stream(h);
    if (e == hipSuccess) e = hipMemsetAsync(h->counters + 12, 0, 8, h->stream);
    if (e == hipSuccess)
        e = gvom_launch_voxel_cloud(h->stream, P, (double)F.origin[0], (double)F.origin[1], (double)F.origin[2],
                                    F.state, F.tags, (const uint4 *)F.rows.p,
                                    (const float *)F.metrics.p, tmp, tmp_e, max_rows,
                                    (unsigned long long *)(h->counters + 12));
    unsigned long long cnt = 0;
    if (e == hipSuccess) e = sync_streams(h);
    if (e == hipSuccess) e = hipMemcpy(&cnt, h->counters + 12, 8, hipMemcpyDeviceToHost);
    const int64_t nrows = (int64_t)cnt < max_rows ? (int64_t)cnt : max_rows;
    if (e == hipSuccess && nrows > 0) e = hipMemcpy(out, tmp, (size_t)nrows * 32, hipMemcpyDeviceToHost);
    if (e == hipSuccess && nrows > 0 && eigen) e = hipMemcpy(eigen, tmp_e, (size_t)nrows * 12, hipMemcpyDeviceToHost);
    hipFree(tmp);
    HIPCHK(h, e);
    if (rows) *rows = (int64_t)cnt;
    return GVOM_OK;
}

VIS int gvom_debug_height_map(gvom_t *h, float *out) { return out ? debug_maps(h, out, nullptr) : GVOM_ERR_INVALID; }
VIS int gvom_debug_inferred_height_map(gvom_t *h, float *out) { return out ? debug_maps(h, nullptr, out) : GVOM_ERR_INVALID; }

VIS int gvom_get_scan_stats(gvom_t *h, gvom_scan_stats *out)
{
    if (!h || !out) return GVOM_ERR_INVALID;
    int slot;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        slot = h->last_buffer_index;
        if (!h->slots[h->ring[slot]].filled) return GVOM_NO_DATA;
    }
    const size_t V = h->V;
    std::vector<int32_t> hit(V), total(V);
    int64_t cells = 0;
    int rc = gvom_read_dense(h, slot, nullptr, hit.data(), nullptr, nullptr, nullptr, &cells);
    if (rc) return rc;
    // total of free voxels lives in the state code; read it densely
    std::vector<int32_t> state(V);
    rc = gvom_read_dense(h, slot, state.data(), nullptr, total.data(), nullptr, nullptr, nullptr);
    if (rc) return rc;
    int64_t sh = 0, st = 0;
    for (size_t i = 0; i < V; ++i) {
        sh += hit[i];
        st += state[i] >= 0 ? (int64_t)total[i] : (int64_t)(-(int64_t)state[i] - 1);
    }
    std::lock_guard<std::mutex> lk(h->mu);
    out->points = h->slots[h->ring[slot]].stats.points;
    out->cells = cells; out->sum_hit = sh; out->sum_total = st;
    return GVOM_OK;
}

#ifdef GVOM_DIAG
// diagnostic library only (not part of include/gvom_hip.h): k_trace's per-wave timeline of the last scan,
// 4 uint64 per wave {start, set-up done (0: the wave left before it walked), end, HW_ID | XCC_ID << 32} in
// dispatch order [row][workgroup][wave]; grid[0] workgroups per row, grid[1] rows (tools/trace_timeline.py)
VIS int gvom_diag_timeline(gvom_t *h, unsigned long long *out, int64_t max_words, int grid[2])
{
    if (!h || !out || !grid) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, sync_streams(h));
    grid[0] = h->tl_grid[0]; grid[1] = h->tl_grid[1];
    const int64_t words = (int64_t)grid[0] * grid[1] * 8 * 4 + 8 +     // + 8 summary words (steps by lookup mode)
                          ((int64_t)grid[0] * grid[1] * 8 / 64 + 1) * 128;   // + the step profiles of every 64th wave
    if (!h->tl.p || words <= 8) return GVOM_NO_DATA;
    HIPCHK(h, hipMemcpy(out, h->tl.p, (size_t)(words < max_words ? words : max_words) * 8, hipMemcpyDeviceToHost));
    return GVOM_OK;
}
#endif
}  // extern "C"
