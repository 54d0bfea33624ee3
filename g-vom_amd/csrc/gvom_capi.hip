// gvom_capi.hip -- the scan unit of the C ABI's host side (the file keeps the name of the former single host unit; the other host
// units are gvom_handle, gvom_combine, gvom_sets, gvom_product_calls and gvom_debug .hip, and gvom_host.h is what they share): parameter setup, the pipeline (upload, layout probe, directional sort, trace, encode or eager
// fusion, statistics), the commit into the ring, and the split calls of a sharded map.
#include "gvom_host.h"

namespace gvom_host {
static void fill_scan_params(const gvom_handle *h, const int64_t origin[3], const double *tf, ScanParams &P, int64_t n_points = 0, int mo_maxsteps = 0)
{
    const gvom_params &p = h->prm;
    P.xy_res = p.xy_resolution; P.z_res = p.z_resolution;
    P.min_d2 = p.min_distance * p.min_distance;
    for (int k = 0; k < 3; ++k) P.origin[k] = (double)origin[k];
    P.has_tf = tf ? 1 : 0;
    for (int k = 0; k < 12; ++k) P.tf[k] = tf ? tf[k] : 0.0;
    P.pt0[0] = (float)(h->ego[0] / p.xy_resolution);
    P.pt0[1] = (float)(h->ego[1] / p.xy_resolution);
    P.pt0[2] = (float)(h->ego[2] / p.z_resolution);
    P.rinv[0] = (float)(1.0 / p.xy_resolution); P.rinv[1] = (float)(1.0 / p.z_resolution);
    P.drcp[0] = 1.0 / p.xy_resolution; P.drcp[1] = 1.0 / p.z_resolution;
    P.fastdiv = h->tune_fastdiv == 0 ? 0 : h->fastdiv_ok;
    for (int k = 0; k < 3; ++k) {
        const int64_t size = k < 2 ? p.xy_size : p.z_size;
        const bool small = origin[k] > -(1ll << 18) && origin[k] < (1ll << 18) && size >= 5;
        P.win_lo[k] = small ? (float)(origin[k] + 2) : 1.0f;      // (integers below 2^24: exact)
        P.win_hi[k] = small ? (float)(origin[k] + size - 2) : 0.0f;
    }
    P.xy = p.xy_size; P.zs = p.z_size;
    window_phase(h, origin, P.om);
    P.sy_lo = h->sy_lo; P.sy_hi = h->sy_hi;
    P.off[0] = h->in_off[0]; P.off[1] = h->in_off[1]; P.off[2] = h->in_off[2];
    P.in_f32 = h->in_f32 ? 1 : 0;
    P.nseg = h->nseg;
    {
        auto lg = [](int v) { int k = 0; while ((1 << k) < v) ++k; return (1 << k) == v ? k : -1; };
        P.lg_nseg = lg(h->nseg); P.lg_zs = lg(p.z_size);
        if (P.lg_nseg < 0 || P.lg_zs < 0) P.lg_nseg = P.lg_zs = -1;
    }
    P.sxq = h->sxq;
    P.shard_world = h->world; P.shard_rank = h->rank; P.shard_rows = h->world > 1 ? p.xy_size / h->world : p.xy_size;
    P.stat_e = p.xy_eigen_dist;
    // DDA step segments: the ego sits at the window centre, so a ray takes at most size/2 + 2 steps.
    // Segments exist to fill the chip with waves when a scan has few returns (a 131 k-point scan is 2
    // waves per SIMD); every segment wave repeats the ray set-up and replays the earlier steps, so
    // clouds with plenty of returns use fewer segments.  The last two segments are shortened: their
    // workgroups are dispatched last and only the longest rays reach them.  (Measured, 256^3 / 131 k
    // points: 5 segments 43.6 us, 6: 44.1, 7: 43.8, 4: 46.4; flush period 16: -0.4 us against 12.)
    {
        // (multi-origin scans: the ray origins are wherever the caller says -- mo_maxsteps, from the origins at hand, see mo_table)
        const int maxsteps = mo_maxsteps > 0 ? mo_maxsteps : (p.xy_size > p.z_size ? p.xy_size : p.z_size) / 2 + 2;
        // "plenty of returns": more 64-ray bundles than three quarters of the device's resident wave slots
        // (MI355X: 256 CUs x 32 waves -> 393,216 returns)
        const bool many = n_points / 64 > 3 * (int64_t)h->resident_blocks;
        int nsegs = many ? 3 : 5;
        if (h->tune_segs > 0) nsegs = h->tune_segs;
        if (nsegs > 9) nsegs = 9;
        if (nsegs > maxsteps / 8) nsegs = maxsteps / 8 > 0 ? maxsteps / 8 : 1;
        P.nsegs = nsegs;
        // flush period (final step body; c4: 8 / 12 / 16 / 24 / 32 -> 552 / 537 / 545 / 608 / 638 us, c5 12 / 16: 2438 / 2460,
        // m256 and c3: 12 = 16)
        P.lc_period = h->tune_period > 0 ? h->tune_period : (many ? 12 : 16);
        if (P.lc_period > 32) P.lc_period = 32;          // the line cache is direct-mapped with 64 entries
        // endpoint blocks first: their atomics retire under the walk; clouds with plenty of returns (several dispatch rounds
        // anyway) do the endpoint work inside segment 0's waves instead (-1): one wave and one load of the returns less per
        // bundle (r5, ep_row 0 / -1: c4 615.6 / 605.6 us per step, c5 2297 / 2052; c3 145.9 / 148.0 and m256 98.2 / 98.1 keep the row)
        P.ep_row = h->tune_ep_row >= -1 ? h->tune_ep_row : (many ? -1 : 0);
        if (P.ep_row > P.nsegs) P.ep_row = P.nsegs;
        // issue priority by remaining work (k_trace, prio_by_remaining): steps per priority level.  Measured, off / 4 / 8 / 16:
        // m256 40.1 / 40.1 / 39.0 / 40.4 us, c2 39.2 / - / 36.7 / -, c3 70.6 / - / 68.2 / -, c4 unchanged
        P.prio_div = h->tune_prio >= 0 ? h->tune_prio : 8;
        P.f32_sqrt = h->f32_sqrt ? 1 : 0;
        P.ilv_lg = 0; P.ilv_len = n_points;
        {
            // automatic: what the layout probe found in the previous cloud of as many returns, at most 4 sub-clouds side by
            // side (c5, 16 sensors: interleave 4 / 8 / 16 -> k_trace 1450 / 1653 / 1745 us: a wave should keep >= 16 azimuths)
            // (multi-origin scans: no interleave, no directional order, no layout probe -- all three judge directions seen from
            // ONE sensor position; a forced knob is ignored there)
            int K = h->tune_ilv > 1 && mo_maxsteps <= 0 ? h->tune_ilv : 1;
            if (h->tune_ilv == 0 && h->counters_host && mo_maxsteps <= 0) {
                // the layout probe's last answer {n << 8 | log2 K} (host-mapped; written by a kernel of an EARLIER scan)
                const unsigned long long w = *(volatile unsigned long long *)(h->counters_host + 8);
                if ((int64_t)(w >> 8) == n_points) K = 1 << (int)(w & 7ull);
            }
            if (K > 64 || (K & (K - 1)) != 0 || n_points <= 0 || n_points % K != 0) K = 1;
            while ((1 << P.ilv_lg) < K) ++P.ilv_lg;
            P.ilv_len = n_points / K;
            // interleaved sub-clouds keep a wave's 64 rays inside a few accumulator lines per step: the line cache holds a
            // longer run (c4, interleave 4: period 12 / 16 / 24 / 32 -> 390 / 379 / 370 / 372 us)
            if (K > 1 && h->tune_period <= 0) P.lc_period = 24;
        }
        P.dbg = gvom_diag_env("GVOM_TRACE_DEBUG");
        const double w_last = nsegs <= 3 ? 0.35 : 0.6;
        const double unit = nsegs >= 3 ? (double)maxsteps / ((nsegs - 2) + 0.85 + w_last) : (double)maxsteps / nsegs;
        double acc = 0.0;
        for (int k = 0; k < 10; ++k) {
            P.seg_start[k] = (int)(acc + 0.5);
            acc += (nsegs < 3 || k < nsegs - 2) ? unit : (k == nsegs - 2 ? 0.85 * unit : (k == nsegs - 1 ? w_last * unit : unit));
        }
    }
    P.epoch = 0;
}

// div_by_res() (gvom_trace.hip) replaces (double)x / d, x a float32, by two fused multiply-adds around r = RN(1 / d).  It is
// used for a divisor only after this check: every float32 significand (2^23 of them: the rounding of the quotient depends on
// nothing else, see there) through the same three operations, against the divide.  ~30 ms per divisor, once per process.
__attribute__((target("fma"))) static bool verify_fastdiv_all(double d, double r)
{
    for (uint32_t m = 0; m < (1u << 23); ++m) {
        const uint32_t bits = 0x3f800000u | m;
        float xf;
        memcpy(&xf, &bits, 4);
        const double x = (double)xf;
        const double q = x * r;
        const double e = __builtin_fma(-q, d, x);
        const double q2 = __builtin_fma(e, r, q);
        if (q2 != x / d) return false;
    }
    return true;
}
bool verify_fastdiv(double d)
{
    static std::mutex mu;
    static std::vector<std::pair<double, bool>> known;
    if (!(d > 0x1p-64 && d < 0x1p64)) return false;        // (also NaN: no float32 coordinate over or underflows anything for such a d)
    if (!__builtin_cpu_supports("fma")) return false;      // (no hardware fma on this host to check with: the divide stays)
    std::lock_guard<std::mutex> lk(mu);
    for (const auto &k : known) if (k.first == d) return k.second;
    const bool ok = verify_fastdiv_all(d, 1.0 / d);
    known.emplace_back(d, ok);
    return ok;
}

// A failed scan must not leak into the next one: k_trace may already have added to the dense
// accumulators and raised the in-grid flag.  Clears them (stream-ordered, best effort).
static void scan_abort(gvom_handle *h)
{
    (void)hipMemsetAsync(h->hit, 0, h->acc_elems * 4, h->stream);
    (void)hipMemsetAsync(h->total, 0, h->acc_elems * 4, h->stream);
    (void)hipMemsetAsync(h->mh, 0, h->acc_elems * 4, h->stream);
    (void)hipMemsetAsync(h->counters, 0, GVOM_CNT_WORDS * 4, h->stream);
    if (h->stream_s) (void)hipStreamSynchronize(h->stream_s);
    h->s_pending = h->fs_pending = false;
    h->before_valid[0] = h->before_valid[1] = false;
    (void)hipStreamSynchronize(h->stream);
    (void)hipGetLastError();
    h->pending = false;
    h->scan_inflight = false;
}

// Optional per-voxel statistics of the scan just encoded, on the statistics stream beside whatever
// follows.  nrows: candidate compact rows; extra / n_extra: returns received from other ranks (sharded map).
static int enqueue_scan_stats(gvom_handle *h, const ScanParams &P, int dtype, Slot &st, int64_t n, int64_t nrows, const void *extra, int64_t n_extra)
{
    const uint32_t par = h->stats_scan & 1u;
    HIPCHK(h, hipEventRecord(h->ev_before[par], h->stream_s));   // the statistics stream's work up to here
    h->before_valid[par] = true;
    ++h->stats_scan;
    HIPCHK(h, hipEventRecord(h->ev_enc_s, h->stream));
    HIPCHK(h, hipStreamWaitEvent(h->stream_s, h->ev_enc_s, 0));
    HIPCHK(h, gvom_launch_stats(h->stream_s, P, dtype, h->world_pts[par].p, n, st.state, st.tags,
                                h->prm.xy_eigen_dist, h->prm.z_eigen_dist, (double *)st.base.p, (double *)st.metrics.p,
                                (const uint32_t *)st.rowvox.p, nrows, extra, n_extra));
    HIPCHK(h, hipEventRecord(h->ev_sdone, h->stream_s));
    h->s_pending = true;
    return GVOM_OK;
}

// k_encfuse behind k_trace (eager fusion, see gvom_handle::hmaps2): the staging slot encoded and fused with the previous
// map into the SPARE fused / height / count buffers.  Nothing the handle's readers look at changes before fuse_impl adopts it.
static int eager_launch(gvom_handle *h, const ScanParams &P, Slot &st, const int64_t origin[3], uint32_t seq)
{
    const gvom_params &p = h->prm;
    const int nxt = h->has_combined ? 1 - h->cur : 0;
    Fused &F = h->fused[nxt];
    const Fused *prev = (h->has_combined && h->fused[h->cur].valid) ? &h->fused[h->cur] : nullptr;
    FuseParams FP;
    fill_fuse_frame(h, origin, FP);
    FP.nslots = 1; FP.has_prev = prev ? 1 : 0;
    FP.nz = h->tune_encfuse & 15; FP.cpw = (h->tune_encfuse >> 4) & 3;      // A/B knob (waves per column block; bit 0 blocks in dispatch order, bit 1 the 16-sx form)
    MapDesc pd;
    memset(&pd, 0, sizeof pd);
    if (prev) {
        pd.state = prev->state; pd.rows = (const uint4 *)prev->rows.p;
        pd.d[0] = clamp_delta(origin[0] - prev->origin[0], p.xy_size);
        pd.d[1] = clamp_delta(origin[1] - prev->origin[1], p.xy_size);
        pd.d[2] = clamp_delta(origin[2] - prev->origin[2], p.z_size);
        pd.epoch = prev->epoch; pd.tags = prev->tags;
    }
    int bw, nw, nblocks; size_t row_cap;
    gvom_encfuse_shape(p.xy_size, p.z_size, FP.nz | (FP.cpw << 4), &bw, &nw, &nblocks, &row_cap);
    h->last_encfuse[0] = bw; h->last_encfuse[1] = nw;
    if (row_cap >= 2147483648ull) { h->err = "fused row space exceeds 31 bits"; return GVOM_ERR_CAPACITY; }
    int rc;
    if ((rc = ensure(h, F.rows, row_cap * 16))) return rc;
    F.valid = false;                                       // (the spare buffer: nobody reads it as a map)
    FP.epoch = ++h->epoch;
    // a pending k_fuse_stats that reads THIS buffer's states / tile tags -- the merge of a fusion through k_fuse1 / k_fuse4 (its
    // "previous map"), or of a dropped speculation (its target) -- must be done before this kernel rewrites them (the wait sits
    // between k_trace and this kernel).  The merge of an ADOPTED speculation does not: it reads its previous map through a link table.
    if (h->fs_pending && h->fs_reads[nxt]) HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_fsdone, 0));
    h->spec_has_metrics = false;
    int32_t *flink = nullptr;
    if (h->stats) {
        if ((rc = ensure(h, h->flink[nxt], row_cap * 4))) return rc;
        flink = (int32_t *)h->flink[nxt].p;
        // the statistics half of this speculative fusion (enqueued by scan_launch behind the scan's own statistics): sources = the
        // staging slot (same frame: no shift) and the previous map if it carries statistics of its own
        if ((rc = ensure(h, F.metrics, row_cap * 40))) return rc;
        h->spec_FP = FP;
        memset(&h->spec_KD, 0, sizeof h->spec_KD);
        MapDesc &sd = h->spec_KD.d[0];
        sd.state = st.state; sd.rows = (const uint4 *)st.crows.p; sd.epoch = st.epoch; sd.tags = st.tags; sd.metrics = st.metrics.p;
        if (prev) { h->spec_KD.d[1] = pd; h->spec_KD.d[1].metrics = prev->has_metrics ? prev->metrics.p : nullptr; h->spec_KD.d[1].link = flink; }
        h->spec_has_metrics = true;
    }
    HIPCHK(h, gvom_launch_encfuse(h->stream, P, FP, pd, flink, h->hit, h->total, h->mh, st.state, (uint4 *)st.crows.p, st.tags,
                                  F.state, (uint4 *)F.rows.p, F.tags, h->blockcounts2, h->hmaps2, h->hmaps2 + p.xy_size,
                                  h->counters, (unsigned long long *)h->counters_host_dev, seq));
    h->spec_valid = true; h->spec_nxt = nxt; h->spec_slot = h->staging; h->spec_blocks = nblocks; h->spec_epoch = FP.epoch;
    h->spec_origin[0] = origin[0]; h->spec_origin[1] = origin[1]; h->spec_origin[2] = origin[2];
    h->last_scan_spec = true;
    return GVOM_OK;
}

// where a scan's window starts, in voxels: centred on the ego (gvom.py:124).  Whole numbers, kept as doubles
static void scan_window_origin(const gvom_handle *h, double origin[3])
{
    origin[0] = floor((h->ego[0] / h->prm.xy_resolution) - h->prm.xy_size / 2.0);
    origin[1] = floor((h->ego[1] / h->prm.xy_resolution) - h->prm.xy_size / 2.0);
    origin[2] = floor((h->ego[2] / h->prm.z_resolution) - h->prm.z_size / 2.0);
}

// Scan kernels up to (not including) the commit.  `dev_pts` is device memory.
static int scan_launch(gvom_handle *h, std::unique_lock<std::mutex> &lk, const void *dev_pts, int64_t n, int64_t stride_elems,
                int dtype, const double *tf, bool shard_local = false, const RayOrigins *mo = nullptr, int mo_maxsteps = 0)
{
    const gvom_params &p = h->prm;
    double wo[3];
    scan_window_origin(h, wo);
    const int64_t origin[3] = {(int64_t)wo[0], (int64_t)wo[1], (int64_t)wo[2]};
    int rc;
    if (h->epoch >= 0xFFFFFF00u && (rc = renumber_epochs(h))) return rc;
    ScanParams P;
    fill_scan_params(h, origin, tf, P, n, mo ? mo_maxsteps : 0);
    h->last_multi_origin = mo ? 1 : 0;
    // (a combine in flight -- combine_maps_async, or a second thread inside combine_maps -- has k_map2d's PCIe stores running
    // beside this trace: raised trace waves would take its issue slots (pipelined m256 91.7 us per step against 89.6, c3 122.0 / 115.5))
    if (h->pending_combine && h->tune_prio < 0) P.prio_div = 0;
    h->last_knobs[0] = P.nsegs; h->last_knobs[1] = P.lc_period; h->last_knobs[2] = P.ep_row; h->last_knobs[3] = P.prio_div;
    h->last_knobs[4] = 1 << P.ilv_lg;
    Slot &st = h->slots[h->staging];
    auto now_pending = [&]() {                             // both exits: the scan sits in the staging slot, uncommitted
        st.count = -1;                                     // occupied voxels: counted on demand (test hooks)
        st.origin[0] = origin[0]; st.origin[1] = origin[1]; st.origin[2] = origin[2];
        st.stats_valid = false;
        st.stats.points = n;
        h->pending = true;
        h->pending_n = n;
        return GVOM_OK;
    };
    // the staging slot may still be a SOURCE of a fusion running on the second stream (asynchronous combine: the
    // second scan after gvom_combine_begin writes the slot the ring has just evicted)
    if (h->fuse_b_unjoined && ((h->fuse_b_slots >> h->staging) & 1ull)) HIPCHK(h, join_fuse_stream(h));
    st.epoch = ++h->epoch;                                 // tiles stamped by this scan
    P.epoch = st.epoch;
    st.has_metrics = h->stats;
    h->scan_inflight = true;
    const size_t esz = dtype == GVOM_DTYPE_F32 ? 4 : 8;
    // compact rows are indexed by return (the row of an occupied voxel = the index of one of its returns)
    const size_t cap = std::max<size_t>(1, (size_t)n);
    if ((rc = ensure(h, st.crows, cap * 16))) return rc;
    Buf &wpts = h->world_pts[h->stats_scan & 1u];
    // (a sharded map's received endpoints get rows behind the rank's own returns: room for as many again; gvom_shard_scan_merge
    // grows the arrays, keeping their contents, if more arrive)
    const size_t scap = h->sharded ? 2 * cap : cap;
    if (h->stats && ((rc = ensure(h, wpts, (size_t)(n > 0 ? n : 1) * 3 * esz)) || (rc = ensure(h, st.metrics, scap * 80)) ||
                     (rc = ensure(h, st.base, scap * 8 * GVOM_BASE_PITCH)) || (rc = ensure(h, st.rowvox, scap * 4)))) return rc;
    double t0 = now_ns();
    const uint32_t seq = ++h->scan_seq;
    if (h->profiling) HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
    // voxels are looked up with 32-bit integer arithmetic: exact while |origin| < 2^30 (2e8 m at
    // 0.2 m voxels); beyond that the kernels take the reference's literal f64 form
    bool big = false;
    for (int k = 0; k < 3; ++k)
        if (origin[k] >= (1ll << 30) || origin[k] <= -(1ll << 30)) big = true;
    if (h->stats) {
        // what the statistics stream may still be reading of the things this scan rewrites (see ev_before): the
        // previous scan's own statistics are NOT among them and keep running beside this scan's trace
        const uint32_t prev_par = (h->stats_scan + 1u) & 1u;
        if (!h->stats_prev_committed && h->s_pending) HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_sdone, 0));
        else if (h->before_valid[prev_par]) {
            // (normally long complete: then no wait packet goes in front of the trace)
            if (hipEventQuery(h->ev_before[prev_par]) == hipSuccess) h->before_valid[prev_par] = false;
            else { (void)hipGetLastError(); HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_before[prev_par], 0)); }
        }
        HIPCHK(h, hipMemsetAsync(st.rowvox.p, 0xFF, st.rowvox.bytes, h->stream));   // no row claimed yet
    }
    ShardExchange X;
    X.ep_send = nullptr; X.ep_cnt = nullptr; X.ep_cap = 0; X.sp_send = nullptr; X.sp_cnt = nullptr;
    if (h->sharded) {
#ifdef GVOM_HOOKS
        if (h->tune_churn > 0 && h->x_send_eps.p) {            // test hook (gvom_set_tuning "churn"): a fresh allocation every scan
            h->retired.push_back(h->x_send_eps);                 // (as a region that grows: retired, not freed)
            h->x_send_eps.p = nullptr; h->x_send_eps.bytes = 0;
        }
#endif
        if ((rc = ensure(h, h->x_send_eps, (size_t)h->world * (size_t)(n > 0 ? n : 1) * 8))) return rc;
        h->x_ep_cap = n > 0 ? n : 1;
        X.ep_send = (uint2 *)h->x_send_eps.p; X.ep_cnt = h->x_ecnt; X.ep_cap = (long)h->x_ep_cap;
        if (h->stats && h->world > 1) {
            if ((rc = ensure(h, h->x_send_sp, (size_t)h->world * (size_t)h->x_ep_cap * 3 * esz))) return rc;
            X.sp_send = h->x_send_sp.p; X.sp_cnt = h->x_spcnt;
        }
    }
    P.tl = nullptr; P.tl_words = 0;
#ifdef GVOM_DIAG
    if (gvom_diag_env("GVOM_TRACE_TIMELINE") && n > 0) {
        h->tl_grid[0] = (int)((n + 511) / 512); h->tl_grid[1] = P.nsegs + (P.ep_row >= 0 ? 1 : 0);
        P.prof_on = gvom_diag_env("GVOM_TRACE_STEPPROF");
        // (+ step profiles: 128 words for every 64th wave)
        const size_t bytes = (size_t)h->tl_grid[0] * h->tl_grid[1] * 8 * 32 + 64 + ((size_t)h->tl_grid[0] * h->tl_grid[1] * 8 / 64 + 1) * 1024;
        P.tl_words = (long)h->tl_grid[0] * h->tl_grid[1] * 8 * 4;
        if ((rc = ensure(h, h->tl, bytes))) return rc;
        HIPCHK(h, hipMemsetAsync(h->tl.p, 0, bytes, h->stream));
        P.tl = (unsigned long long *)h->tl.p;
    }
#endif
    hipError_t le = hipSuccess;
    // the layout probe's LAST answer, read before this scan's probe is launched: every kernel of the earlier scans has completed
    // (their process_pointcloud returned behind k_trace), so which scan starts to sort is deterministic (read behind
    // the launch, scan k or k + 1 saw the new verdict depending on how fast the probe ran)
    const unsigned long long probe_word = h->counters_host ? *(volatile unsigned long long *)(h->counters_host + 8) : 0ull;
    if (h->tune_ilv == 0 && n >= 8192 && !mo) {
        // layout probe: only for clouds whose length is STABLE (the same as the previous scan's: a node that drops invalid
        // returns hands over a different length every scan -- its sub-clouds do not start at multiples of n / K, nothing to find,
        // nothing to pay), on the second cloud of a length and every 32nd scan after it; in front of k_trace (the caller may
        // free the cloud as soon as this call has returned, i.e. once k_trace is done); its answer serves LATER scans
        // A stream whose length CHANGES from scan to scan (invalid returns dropped) is looked at every 8th scan all the same -- for the
        // "is this order any good for the trace" half of the answer only, which does not depend on the exact length
        const bool stable = n == h->last_n && (n != h->probe_n || ++h->probe_age >= 32);
        const bool varying = n != h->last_n && ++h->probe_var_age >= 8;
        if (stable || varying) {
            if (stable) { h->probe_n = n; h->probe_age = 0; }
            h->probe_var_age = 0;
            le = gvom_launch_layout_probe(h->stream, P, dtype, dev_pts, stride_elems, n, 2, (unsigned long long *)(h->counters_host_dev + 8));
            if (le != hipSuccess) { scan_abort(h); HIPCHK(h, le); }
        }
        h->last_n = n;
    }
    P.perm = nullptr;
    {   // directional order: forced, or the probe's verdict on the previous cloud of this length ("scattered", bit 3 of its answer)
        int sort = h->tune_dirsort == 1 || h->tune_dirsort == 2 ? h->tune_dirsort : 0;   // 1: cube cells, 2: elevation rows
        if (mo) sort = 0;                                  // (bins are directions seen from ONE sensor position)
        if (h->tune_dirsort == 0 && !mo && h->tune_ilv == 0 && h->counters_host) {
            const unsigned long long w = probe_word;
            const int64_t np_ = (int64_t)(w >> 8);
            // (the verdict on a cloud of about this length -- within a quarter -- holds for this one)
            if (np_ > 0 && (np_ == n || (n > np_ - np_ / 4 && n < np_ + np_ / 4))) sort = (int)((w >> 3) & 3ull);
        }
        h->last_dirsort = 0;
        if (sort && n >= 256 && n < (1ll << 31)) {
            if ((rc = ensure(h, h->dir_keys, (size_t)n * 2)) || (rc = ensure(h, h->dir_perm, (size_t)n * 4))) return rc;
            uint32_t *hist = h->dir_hist + (h->dir_flip & 1u) * GVOM_DIRBINS, *next = h->dir_hist + ((h->dir_flip + 1u) & 1u) * GVOM_DIRBINS;
            ++h->dir_flip;
            le = gvom_launch_dirbin(h->stream, P, sort == 2 ? 2 : 1, dtype, dev_pts, stride_elems, n, (uint16_t *)h->dir_keys.p, hist, next,
                                    h->dir_hist + 2 * GVOM_DIRBINS, (uint32_t *)h->dir_perm.p);
            if (le != hipSuccess) { scan_abort(h); HIPCHK(h, le); }
            P.perm = (const uint32_t *)h->dir_perm.p;
            P.ilv_lg = 0; P.ilv_len = n;
            h->last_dirsort = sort == 2 ? 2 : 1;
            h->last_knobs[4] = 1;
        }
    }
    le = gvom_launch_trace(h->stream, P, X, dtype, big, dev_pts, stride_elems, n,
                                      h->stats ? wpts.p : nullptr, h->hit, h->total, h->mh, st.state,
                                      st.tags, h->counters, h->stats ? (double *)st.metrics.p : nullptr,
                                      h->stats ? (double *)st.base.p : nullptr,
                                      h->stats ? (uint32_t *)st.rowvox.p : nullptr, mo);
    if (le != hipSuccess) { scan_abort(h); HIPCHK(h, le); }
    if (h->profiling) HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    // (a sharded map of ONE rank has no other ranks' rows: nothing to pack, no counts to publish and to wait for -- the scan
    // is encoded right behind the trace, as on an unsharded handle, and gvom_shard_scan_merge only commits it)
    const bool solo = shard_local && h->world == 1;
    h->solo_encoded = solo;
    if (shard_local && !solo) {
        // sharded map: the ray passes in other ranks' rows are packed for their owners; the counts go
        // to host-mapped memory (the caller sizes the exchange with them); k_encode follows in
        // scan_merge, once the other ranks' contributions have been added
        le = gvom_launch_pack(h->stream, P, h->total, st.tags, h->x_send_ids, h->x_send_pay, h->x_qcnt, h->x_ecnt, h->x_spcnt,
                              h->counters, h->x_host_dev, seq);
        if (le != hipSuccess) { scan_abort(h); HIPCHK(h, le); }
        volatile unsigned long long *flag = (volatile unsigned long long *)(h->x_host + 2 * h->world + 1);
        if (!wait_published(h, lk, flag, seq, false, &h->last_wait_ns[0])) {
            hipError_t se = hipStreamSynchronize(h->stream);
            if (se != hipSuccess || (uint32_t)*flag != seq) {
                scan_abort(h);
                h->err = "sharded scan: pack counts were never published";
                return GVOM_ERR_HIP;
            }
        }
        h->pending_any = h->x_host[2 * h->world] != 0;
        h->pending_P = P;
        h->pending_dtype = dtype;
        return now_pending();
    }
    // one-slot rings: encode + fuse in one pass, speculating that combine_maps comes next (see gvom_handle::hmaps2)
    const bool eager = h->hmaps2 && h->tune_eager != 0 && (h->tune_eager == 1 || h->eager_waste < 3) && !gvom_diag_env("GVOM_TRACE_DEBUG");
    h->last_scan_spec = false;
    if (eager) {
        if ((rc = eager_launch(h, P, st, origin, seq))) { scan_abort(h); return rc; }
        st.has_code16 = false;
    } else {
        // the 16-bit codes are read by k_fuse4 only: a one-slot ring fuses through k_fuse1 (unless the A/B knob says otherwise)
        const bool codes = st.code16 && (p.buffer_size > 1 || h->tune_fuse1 == 1 || h->sharded);
        le = gvom_launch_encode(h->stream, P, h->hit, h->total, h->mh, st.state, codes ? st.code16 : nullptr, (uint4 *)st.crows.p,
                                st.tags, h->counters,
                                (unsigned long long *)h->counters_host_dev, seq, h->resident_blocks);
        if (le != hipSuccess) { scan_abort(h); HIPCHK(h, le); }
        st.has_code16 = codes;
    }
    if (h->profiling) { HIPCHK(h, hipEventRecord(h->ev[2], h->stream)); h->ev_scan = true; }
    if (h->stats && (rc = enqueue_scan_stats(h, P, dtype, st, n, n, nullptr, 0))) return rc;
    if (eager && h->spec_has_metrics) {
        // behind k_stats / k_stats_gather on the statistics stream (which waited for k_encfuse): the merge of the speculative fusion
        Fused &F = h->fused[h->spec_nxt];
        HIPCHK(h, gvom_launch_fuse_stats(h->stream_s, h->spec_FP, h->spec_KD, nullptr, F.state, F.tags, (float *)F.metrics.p));
        HIPCHK(h, hipEventRecord(h->ev_fsdone, h->stream_s));
        HIPCHK(h, hipEventRecord(h->ev_sdone, h->stream_s));
        h->s_pending = h->fs_pending = true;
        h->fs_reads[h->spec_nxt] = true; h->fs_reads[1 - h->spec_nxt] = false;      // (its previous map through the link table)
    }
    HT(h, 0, t0);                                        // scan: launches
    // Wait only for k_trace: k_encode's first thread publishes {seq, any-in-grid} to host-mapped
    // memory.  The caller gets control back while k_encode still runs; everything it can do next
    // with this handle is stream-ordered behind it.
    {
        volatile unsigned long long *flag = (volatile unsigned long long *)h->counters_host;
        if (!wait_published(h, lk, flag, seq, true, &h->last_wait_ns[0])) {
            hipError_t se = hipStreamSynchronize(h->stream);
            if (se != hipSuccess || (uint32_t)(*flag >> 32) != seq) {
                scan_abort(h);
                h->err = se != hipSuccess ? std::string("scan failed: ") + hipGetErrorString(se)
                                          : "scan completion was never published";
                return GVOM_ERR_HIP;
            }
        }
    }
    HT(h, 1, t0);                                        // scan: wait
    if (h->host_timing) h->host_calls++;
    {
        const unsigned long long fl = *(volatile unsigned long long *)h->counters_host;
        h->pending_any = (fl & 0x80000000ull) != 0;        // some return landed in the grid
    }
    return now_pending();
}

static void scan_commit(gvom_handle *h, bool accept)
{
    h->scan_inflight = false;
    if (!h->pending) return;
    h->pending = false;
    h->stats_prev_committed = accept;
    if (!accept) { h->spec_valid = false; h->last_scan_spec = false; return; }   // gvom.py:148-150: ring untouched (a speculative fusion of it is dropped)
    const int b = h->buffer_index;                         // gvom.py:163-175
    const int old = h->ring[b];
    h->ring[b] = h->staging;
    h->staging = old;
    h->slots[h->ring[b]].filled = true;
    h->fresh_scan = true;
    h->slots[old].filled = false;
    h->last_buffer_index = b;
    h->buffer_index = (b + 1 >= h->prm.buffer_size) ? 0 : b + 1;
}

// ---- the three parts of a scan call, shared by the cloud routes (process_impl) and the range-image route (range_image_impl);
// all of them under scan_mu and mu ----
// 1. what the call does to the handle before any data moves.  != 0: the call returns that (GVOM_EMPTY_CLOUD included)
static int scan_begin(gvom_handle *h, const double ego[3], const int64_t *off_bytes, size_t esz, bool widen_f32, bool defer, int64_t n)
{
    HIPCHK(h, hipSetDevice(h->device));
    for (int k = 0; k < 3; ++k) h->in_off[k] = off_bytes ? (int)(off_bytes[k] / (int64_t)esz) : k;
    h->in_f32 = widen_f32;
    h->ego[0] = ego[0]; h->ego[1] = ego[1]; h->ego[2] = ego[2];       // gvom.py:102-104
    // a sharded scan whose second half never came (the exchange failed between gvom_shard_scan_local and
    // gvom_shard_scan_merge): k_trace's additions to this rank's rows were never encoded or zeroed
    if (h->pending && h->sharded) scan_abort(h);
    h->pending = false;
    if (h->spec_valid) {                                   // a scan behind a scan: the speculative fusion of the first is dropped
        h->spec_valid = false;
        if (h->eager_waste < 4) ++h->eager_waste;
        ++h->eager_stat[1];
    }
    if (h->sharded && !defer) { h->err = "a sharded handle scans through gvom_shard_scan_local / gvom_shard_scan_merge"; return GVOM_ERR_INVALID; }
    if (n == 0 && !defer) return GVOM_EMPTY_CLOUD;                     // gvom.py:107-109 (a rank's share of a sharded scan may be empty)
    return GVOM_OK;
}

// 2. host data into the handle's staging buffers (which are free: their readers sit in front of the previous scan's k_trace, and
// that had completed when its call returned)
struct Upload { void *dst; const void *src; size_t bytes; };
static int scan_upload(gvom_handle *h, std::unique_lock<std::mutex> &lk, const Upload *up, int count)
{
    if (hipStreamQuery(h->stream) == hipErrorNotReady) {
        // the main stream still has work queued (a combine from another thread, the previous k_encode): upload beside it
        lk.unlock();                                  // a pageable source is staged by the calling thread: not under the handle mutex
        hipError_t ue = hipSuccess;
        for (int k = 0; k < count && ue == hipSuccess; ++k)
            ue = hipMemcpyAsync(up[k].dst, up[k].src, up[k].bytes, hipMemcpyHostToDevice, h->stream_up);
        lk.lock();
        HIPCHK(h, ue);
        HIPCHK(h, hipEventRecord(h->ev_up, h->stream_up));
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_up, 0));
    } else {
        (void)hipGetLastError();
        for (int k = 0; k < count; ++k)
            HIPCHK(h, hipMemcpyAsync(up[k].dst, up[k].src, up[k].bytes, hipMemcpyHostToDevice, h->stream));
    }
    return GVOM_OK;
}

// 3. the cloud is now at `dev` (or will be, in stream order): scan it, commit it
static int scan_finish(gvom_handle *h, std::unique_lock<std::mutex> &lk, const void *dev, int64_t n, int64_t stride_elems, int dtype,
                const double *tf, bool defer, const RayOrigins *mo = nullptr, int mo_maxsteps = 0)
{
    int rc = scan_launch(h, lk, dev, n, stride_elems, dtype, tf, defer, mo, mo_maxsteps);
    if (rc) return rc;
    if (defer) return GVOM_OK;
    const bool accept = h->pending_any;                   // == (global occupied-voxel count > 0), gvom.py:147-150
    scan_commit(h, accept);
    return accept ? GVOM_OK : GVOM_NO_OVERLAP;
}

// a pinned staging buffer of at least `bytes` (grown by half as much again; contents not kept)
static int ensure_pinned(gvom_handle *h, PinPtr<void> &b, size_t bytes)
{
    if (b.bytes >= bytes) return GVOM_OK;
    if (b.p) HIPCHK(h, hipHostFree(b.p));
    b.p = nullptr; b.bytes = 0;
    HIPCHK(h, hipHostMalloc(&b.p, bytes + bytes / 2, hipHostMallocDefault));
    b.bytes = bytes + bytes / 2;
    return GVOM_OK;
}

// ---- multi-origin scans: the host half ----
struct OriginArgs { const double *origins; int32_t K; const uint16_t *index; };   // (index: in the memory the cloud is in, or nullptr)
inline size_t mo_index_offset(int32_t K) { return ((size_t)K * 12 + 255) & ~(size_t)255; }
static bool mo_origins_valid(const double *origins, int32_t K)
{
    if (!origins || K < 1 || K > 65536) return false;
    for (int64_t k = 0; k < (int64_t)K * 3; ++k)
        if (!std::isfinite(origins[k])) return false;
    return true;
}
// Room for the table (and `idx_n` index entries) in the pinned staging copy and in device memory; the table itself, as the host
// computes ScanParams::pt0 from the ego (fill_scan_params): one float64 division, one rounding to float32.  Returns through
// *maxsteps the step bound the segment table is sized with: a dominant-axis DDA moves one voxel per step along its dominant axis,
// so a ray that starts `e` voxels from the farthest face of the window has left it after e + 2 steps; an origin more than a voxel
// outside the window takes no step at all (its first one lies outside) and does not count.
static int mo_table(gvom_handle *h, const double *origins, int32_t K, int64_t idx_n, int *maxsteps)
{
    const gvom_params &p = h->prm;
    const size_t bytes = mo_index_offset(K) + (size_t)idx_n * 2;
    int rc = ensure(h, h->multi_origin.dev, bytes);
    if (rc) return rc;
    if ((rc = ensure_pinned(h, h->multi_origin.pin, bytes))) return rc;
    double lo[3], size[3];
    scan_window_origin(h, lo);
    size[0] = size[1] = p.xy_size; size[2] = p.z_size;
    const double longest = (double)(p.xy_size > p.z_size ? p.xy_size : p.z_size);
    float *tab = (float *)h->multi_origin.pin.p;
    double far_ = 0.0;
    for (int32_t k = 0; k < K; ++k) {
        double e = 0.0;
        for (int a = 0; a < 3; ++a) {
            const float v = (float)(origins[3 * k + a] / (a < 2 ? p.xy_resolution : p.z_resolution));
            tab[3 * k + a] = v;
            const double d0 = (double)v - lo[a], d1 = lo[a] + size[a] - (double)v;
            e = std::max(e, std::max(d0, d1));
        }
        if (e <= longest + 1.0) far_ = std::max(far_, e);
    }
    *maxsteps = far_ > 0.0 ? (int)far_ + 3 : (int)longest / 2 + 2;
    return GVOM_OK;
}

static int process_impl(gvom_handle *h, const void *xyz, bool on_device, int64_t n, int64_t row_stride_bytes,
                 int dtype, const double ego[3], const double *tf, bool defer, const int64_t *off_bytes = nullptr,
                 bool widen_f32 = false, const OriginArgs *mo = nullptr)
{
    if (!h || !ego || n < 0 || (dtype != GVOM_DTYPE_F32 && dtype != GVOM_DTYPE_F64))
        return GVOM_ERR_INVALID;
    // widen_f32: float32 records (esz = 4 for addressing) scanned by the float64 kernels
    const size_t esz = (dtype == GVOM_DTYPE_F32 || widen_f32) ? 4 : 8;
    if (widen_f32 && dtype != GVOM_DTYPE_F64) return GVOM_ERR_INVALID;
    if (n > 0 && (!xyz || row_stride_bytes < (int64_t)(3 * esz) || row_stride_bytes % esz != 0))
        return GVOM_ERR_INVALID;
    if (n >= 2147483647LL) return GVOM_ERR_CAPACITY;
    if (mo) {                                             // (before anything is enqueued or the handle changes)
        if (!mo_origins_valid(mo->origins, mo->K)) return GVOM_ERR_INVALID;
        if (mo->index && !on_device)
            for (int64_t i = 0; i < n; ++i)
                if ((int32_t)mo->index[i] >= mo->K) return GVOM_ERR_INVALID;
    }
    int64_t last_field = 2 * (int64_t)esz;                               // byte offset of the last field read
    if (off_bytes) {
        last_field = 0;
        for (int k = 0; k < 3; ++k) {
            if (off_bytes[k] < 0 || off_bytes[k] % (int64_t)esz != 0 || off_bytes[k] + (int64_t)esz > row_stride_bytes)
                return GVOM_ERR_INVALID;
            if (off_bytes[k] > last_field) last_field = off_bytes[k];
        }
    }
    std::lock_guard<std::mutex> scan_lk(h->scan_mu);      // scans of one handle are serialised (one staging slot, one set of accumulators)
    std::unique_lock<std::mutex> lk(h->mu);
    if (mo && h->sharded) { h->err = "multi-origin scans are not supported on a sharded handle"; return GVOM_ERR_INVALID; }
    int rc = scan_begin(h, ego, off_bytes, esz, widen_f32, defer, n);
    if (rc) return rc;
    const void *dev = xyz;
    Upload up[2];
    int ups = 0;
    RayOrigins RO = {nullptr, nullptr, 0u};
    int mo_maxsteps = 0;
    if (mo && n > 0) {                                     // (first: from pinned memory, in flight while the cloud's own upload runs)
        const bool host_idx = mo->index && !on_device;
        if ((rc = mo_table(h, mo->origins, mo->K, host_idx ? n : 0, &mo_maxsteps))) return rc;
        const size_t ioff = mo_index_offset(mo->K);
        if (host_idx) memcpy((char *)h->multi_origin.pin.p + ioff, mo->index, (size_t)n * 2);
        up[ups++] = {h->multi_origin.dev.p, h->multi_origin.pin, host_idx ? ioff + (size_t)n * 2 : (size_t)mo->K * 12};
        RO.tab = (const float *)h->multi_origin.dev.p; RO.K = (uint32_t)mo->K;
        RO.idx = host_idx ? (const uint16_t *)((const char *)h->multi_origin.dev.p + ioff) : mo->index;
    }
    if (!on_device && n > 0) {
        if ((rc = ensure(h, h->in_pts, (size_t)n * row_stride_bytes))) return rc;
        up[ups++] = {h->in_pts.p, xyz, (size_t)(n - 1) * row_stride_bytes + (size_t)last_field + esz};
        dev = h->in_pts.p;
    }
    if (ups && (rc = scan_upload(h, lk, up, ups))) return rc;
    return scan_finish(h, lk, dev, n, row_stride_bytes / (int64_t)esz, dtype, tf, defer, RO.tab ? &RO : nullptr, mo_maxsteps);
}

// A range image (gvom_process_range_image): raw -> (host images: staging buffer ->) k_unproject -> in_pts, then the scan of in_pts
// as process_impl runs it on an uploaded host cloud of H * W returns
static int range_image_impl(gvom_handle *h, const void *raw, bool on_device, int range_dtype, int64_t row_stride_bytes,
                     const double *col_poses, int cloud_dtype, const double ego[3], const double *tf, bool from_columns = false)
{
    if (from_columns && !col_poses) return GVOM_ERR_INVALID;
    if (!h || !ego || !raw || (cloud_dtype != GVOM_DTYPE_F32 && cloud_dtype != GVOM_DTYPE_F64)) return GVOM_ERR_INVALID;
    if (range_dtype != GVOM_RANGE_U16 && range_dtype != GVOM_RANGE_U32 && range_dtype != GVOM_RANGE_F32) return GVOM_ERR_INVALID;
    const int64_t rsz = range_dtype == GVOM_RANGE_U16 ? 2 : 4;
    std::lock_guard<std::mutex> scan_lk(h->scan_mu);
    std::unique_lock<std::mutex> lk(h->mu);
    if (h->sharded) { h->err = "range images are not supported on a sharded handle"; return GVOM_ERR_INVALID; }
    if (h->range_image.H <= 0) { h->err = "gvom_process_range_image: no sensor model (gvom_sensor_model_set)"; return GVOM_ERR_INVALID; }
    const int64_t H = h->range_image.H, W = h->range_image.W, n = H * W;
    if (row_stride_bytes < W * rsz || row_stride_bytes % rsz != 0) { h->err = "gvom_process_range_image: bad row stride"; return GVOM_ERR_INVALID; }
    // every pixel traced from its column's sensor position: O[w] = the translation of C[w] through the cloud's transform, in the
    // transform's own order of operations (load_return)
    std::vector<double> col_org;
    if (from_columns) {
        if (W > 65536) { h->err = "gvom_process_range_image_origins: more than 65536 columns"; return GVOM_ERR_INVALID; }
        col_org.resize((size_t)W * 3);
        for (int64_t w = 0; w < W; ++w) {
            const double t0 = col_poses[w * 12 + 3], t1 = col_poses[w * 12 + 7], t2 = col_poses[w * 12 + 11];
            for (int k = 0; k < 3; ++k)
                col_org[w * 3 + k] = tf ? ((t0 * tf[4 * k] + t1 * tf[4 * k + 1]) + t2 * tf[4 * k + 2]) + tf[4 * k + 3] : (k == 0 ? t0 : (k == 1 ? t1 : t2));
        }
        if (!mo_origins_valid(col_org.data(), (int32_t)W)) { h->err = "gvom_process_range_image_origins: non-finite column position"; return GVOM_ERR_INVALID; }
    }
    int rc = scan_begin(h, ego, nullptr, 0, false, false, n);
    if (rc) return rc;
    const size_t tsz = cloud_dtype == GVOM_DTYPE_F32 ? 4 : 8;
    if ((rc = ensure(h, h->in_pts, (size_t)n * 3 * tsz))) return rc;
    Upload up[3];
    int ups = 0;
    RayOrigins RO = {nullptr, nullptr, 0u};
    int mo_maxsteps = 0;
    if (from_columns) {
        if ((rc = mo_table(h, col_org.data(), (int32_t)W, 0, &mo_maxsteps))) return rc;
        up[ups++] = {h->multi_origin.dev.p, h->multi_origin.pin, (size_t)W * 12};
        RO.tab = (const float *)h->multi_origin.dev.p; RO.K = (uint32_t)W;   // index[i] = i % W: the pixel's column
    }
    if (col_poses) {                                       // (first: see RangeImageState::poses_pin)
        const size_t bytes = (size_t)W * 96;
        if ((rc = ensure(h, h->range_image.poses, bytes))) return rc;
        if ((rc = ensure_pinned(h, h->range_image.poses_pin, bytes))) return rc;
        memcpy(h->range_image.poses_pin, col_poses, bytes);
        up[ups++] = {h->range_image.poses.p, h->range_image.poses_pin, bytes};
    }
    if (!on_device) {
        const size_t bytes = (size_t)(H - 1) * row_stride_bytes + (size_t)(W * rsz);
        if ((rc = ensure(h, h->range_image.raw, bytes))) return rc;
        up[ups++] = {h->range_image.raw.p, raw, bytes};
    }
    if (ups && (rc = scan_upload(h, lk, up, ups))) return rc;
    UnprojectParams U;
    U.raw = on_device ? raw : h->range_image.raw.p; U.row_stride = row_stride_bytes;
    U.dir = (const double *)h->range_image.model.p; U.off = U.dir + (size_t)n * 3;
    U.poses = col_poses ? (const double *)h->range_image.poses.p : nullptr;
    U.out = h->in_pts.p;
    U.scale = h->range_image.scale; U.min_range = h->range_image.min; U.max_range = h->range_image.max;
    U.W = (uint32_t)W; U.n = (uint32_t)n;
    HIPCHK(h, gvom_launch_unproject(h->stream, U, range_dtype, cloud_dtype));
    return scan_finish(h, lk, h->in_pts.p, n, 3, cloud_dtype, tf, false, from_columns ? &RO : nullptr, mo_maxsteps);
}
}  // namespace gvom_host

extern "C" {
VIS int gvom_process_pointcloud(gvom_t *h, const void *xyz, int64_t n, int64_t row_stride_bytes,
                                int dtype, const double ego[3], const double *transform_4x4)
{
    return process_impl(h, xyz, false, n, row_stride_bytes, dtype, ego, transform_4x4, false);
}

VIS int gvom_process_pointcloud_device(gvom_t *h, const void *xyz_dev, int64_t n,
                                       int64_t row_stride_bytes, int dtype, const double ego[3],
                                       const double *transform_4x4)
{
    return process_impl(h, xyz_dev, true, n, row_stride_bytes, dtype, ego, transform_4x4, false);
}

// Ingest side of the ROS node (gvom_ros.py:93-109): the packed bytes of a
// sensor_msgs/PointCloud2 (`data`, width*height records of point_step bytes, little-endian FLOAT32
// or FLOAT64 fields x, y, z at the given byte offsets) are scanned directly; the host-side
// ros_numpy expansion to an xyz array disappears.  ros_numpy drops records with a non-finite
// coordinate; here such records take part and have no effect (no in-grid endpoint, no ray step).
VIS int gvom_process_pointcloud2(gvom_t *h, const void *data, int64_t n_points, int64_t point_step,
                                 int64_t off_x, int64_t off_y, int64_t off_z, int dtype,
                                 const double ego[3], const double *transform_4x4)
{
    const int64_t off[3] = {off_x, off_y, off_z};
    // ros_numpy returns a float64 array whatever the field type (get_xyz_points, dtype=np.float), so
    // the reference computes a FLOAT32 cloud in f64 as well: widen on load, run the f64 kernels
    return process_impl(h, data, false, n_points, point_step, GVOM_DTYPE_F64, ego, transform_4x4, false, off,
                        dtype == GVOM_DTYPE_F32);
}

// ---- range images (include/gvom_hip.h "range images") -------------------------------------------
// The model lives in device memory; a scan holds scan_mu until its k_trace -- which sits behind its k_unproject on the stream --
// has completed, so whoever gets scan_mu here finds no reader of the old model in flight (the stream is drained all the same:
// a scan that failed half-way may have left one).  The second wait makes the caller's arrays free on return.
VIS int gvom_sensor_model_set(gvom_t *h, int32_t H, int32_t W, const double *dir, const double *off,
                              double range_scale, double min_range, double max_range)
{
    if (!h || H < 1 || W < 1 || (int64_t)H * W >= (1ll << 31) || !dir) return GVOM_ERR_INVALID;
    if (!(range_scale > 0.0) || !std::isfinite(range_scale) || std::isnan(min_range) || std::isnan(max_range)) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> scan_lk(h->scan_mu);
    std::unique_lock<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const size_t half = (size_t)H * W * 24;
    h->range_image.H = h->range_image.W = 0;
    int rc = ensure(h, h->range_image.model, 2 * half);
    if (rc) return rc;
    char *m = (char *)h->range_image.model.p;
    HIPCHK(h, hipMemcpyAsync(m, dir, half, hipMemcpyHostToDevice, h->stream));
    if (off) HIPCHK(h, hipMemcpyAsync(m + half, off, half, hipMemcpyHostToDevice, h->stream));
    else HIPCHK(h, hipMemsetAsync(m + half, 0, half, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->range_image.H = H; h->range_image.W = W;
    ++h->range_image.gen;                                                   // (what the voxel atlas keeps of the model is stale from here on)
    h->range_image.scale = range_scale; h->range_image.min = min_range; h->range_image.max = max_range;
    return GVOM_OK;
}

VIS int gvom_process_range_image(gvom_t *h, const void *raw, int on_device, int range_dtype, int64_t row_stride_bytes,
                                 const double *col_poses, int cloud_dtype, const double ego[3], const double *transform_4x4)
{
    return range_image_impl(h, raw, on_device != 0, range_dtype, row_stride_bytes, col_poses, cloud_dtype, ego, transform_4x4);
}

// ---- multi-origin scans (include/gvom_hip.h "multi-origin scans") ---------------------------------
VIS int gvom_process_pointcloud_origins(gvom_t *h, const void *xyz, int on_device, int64_t n, int64_t row_stride_bytes, int dtype,
                                        const double *origins, int32_t K, const uint16_t *index, const double ego[3],
                                        const double *transform_4x4)
{
    const OriginArgs mo = {origins, K, index};
    return process_impl(h, xyz, on_device != 0, n, row_stride_bytes, dtype, ego, transform_4x4, false, nullptr, false, &mo);
}

VIS int gvom_process_range_image_origins(gvom_t *h, const void *raw, int on_device, int range_dtype, int64_t row_stride_bytes,
                                         const double *col_poses, int cloud_dtype, const double ego[3], const double *transform_4x4)
{
    return range_image_impl(h, raw, on_device != 0, range_dtype, row_stride_bytes, col_poses, cloud_dtype, ego, transform_4x4, true);
}

// ---- scan of a sharded map (one rank per GPU; DESIGN.md "Multi-GPU") ---------------------------
// gvom_shard_scan_local: this rank's share of the scan (possibly empty): traces ITS rays over the whole
//   window, leaves what fell into its own rows in its accumulators and packs the rest for the owners.
//   send_quads[d] / send_eps[d] = dirty quads (1 KiB each + a 4-byte id) / endpoints (8 bytes each) for
//   rank d; *any_ingrid = some return of this rank landed in the grid.
// gvom_shard_buffer: the send / receive regions, by peer rank, for the transport (RCCL: gvom_comm_*).
// gvom_shard_recv_reserve: sizes the endpoint receive regions once the counts are known.
// gvom_shard_scan_merge: adds what the other ranks sent, encodes this rank's rows and commits the scan
//   iff `accept` (the reference's "no overlap" test, gvom.py:147-150, is on the whole scan).
VIS int gvom_shard_scan_local(gvom_t *h, const void *xyz, int on_device, int64_t n, int64_t row_stride_bytes,
                              int dtype, const double ego[3], const double *transform_4x4,
                              int64_t *send_quads, int64_t *send_eps, int *any_ingrid)
{
    if (!h || !h->sharded) return GVOM_ERR_INVALID;
    int rc = process_impl(h, xyz, on_device != 0, n, row_stride_bytes, dtype, ego, transform_4x4, true);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    for (int d = 0; d < h->world; ++d) {
        if (send_quads) send_quads[d] = h->solo_encoded ? 0 : (int64_t)h->x_host[d];
        if (send_eps) send_eps[d] = h->solo_encoded ? 0 : (int64_t)h->x_host[h->world + d];
    }
    if (any_ingrid) *any_ingrid = h->pending_any ? 1 : 0;
    return GVOM_OK;
}

VIS int gvom_shard_recv_reserve(gvom_t *h, const int64_t *recv_eps)
{
    if (!h || !h->sharded || !recv_eps) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    int64_t tot = 0;
    for (int sidx = 0; sidx < h->world; ++sidx) {
        h->x_recv_ep_off[sidx] = tot;
        if (recv_eps[sidx] < 0) return GVOM_ERR_INVALID;
        tot += sidx == h->rank ? 0 : recv_eps[sidx];
    }
    h->x_recv_ep_off[h->world] = tot;
    return ensure(h, h->x_recv_eps, (size_t)(tot > 0 ? tot : 1) * 8);
}

// Per-voxel statistics on a sharded map (handles created with GVOM_FLAG_VOXEL_STATISTICS): after gvom_shard_scan_local,
// send_returns[d] = returns (3 values of the cloud's type each) this rank has for rank d -- every return whose
// (2 xy_eigen_dist + 1)-row neighbourhood reaches into d's rows; the transport moves GVOM_XBUF_SEND_RETURNS to the peers'
// GVOM_XBUF_RECV_RETURNS (sized by gvom_shard_stats_reserve from the exchanged counts) before gvom_shard_scan_merge.
VIS int gvom_shard_stats_counts(gvom_t *h, int64_t *send_returns)
{
    if (!h || !h->sharded || !send_returns) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    for (int d = 0; d < h->world; ++d) send_returns[d] = (h->stats && h->pending && !h->solo_encoded) ? (int64_t)h->x_host[2 * h->world + 2 + d] : 0;
    return GVOM_OK;
}

VIS int gvom_shard_stats_reserve(gvom_t *h, const int64_t *recv_returns, int dtype)
{
    if (!h || !h->sharded || !recv_returns || (dtype != GVOM_DTYPE_F32 && dtype != GVOM_DTYPE_F64)) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    if (h->pending_n > 0 && dtype != h->pending_dtype) { h->err = "the ranks' clouds differ in type"; return GVOM_ERR_INVALID; }
    h->pending_dtype = dtype;                             // (a rank with an empty share takes the others' type)
    int64_t tot = 0;
    for (int sidx = 0; sidx < h->world; ++sidx) {
        h->x_recv_sp_off[sidx] = tot;
        if (recv_returns[sidx] < 0) return GVOM_ERR_INVALID;
        tot += sidx == h->rank ? 0 : recv_returns[sidx];
    }
    h->x_recv_sp_off[h->world] = tot;
    const size_t esz3 = (h->pending_dtype == GVOM_DTYPE_F32 ? 4 : 8) * 3;
    return ensure(h, h->x_recv_sp, (size_t)(tot > 0 ? tot : 1) * esz3);
}

VIS int gvom_shard_buffer(gvom_t *h, int which, int peer, void **ptr, int64_t *capacity_bytes)
{
    if (!h || !h->sharded || !ptr || peer < 0 || peer >= h->world) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    const size_t myQ = h->x_myQ;
    int64_t cap = 0;
    switch (which) {
    case GVOM_XBUF_SEND_IDS: *ptr = h->x_send_ids + (size_t)peer * myQ; cap = (int64_t)myQ * 4; break;
    case GVOM_XBUF_SEND_QUADS: *ptr = (char *)h->x_send_pay + (size_t)peer * myQ * 1024; cap = (int64_t)myQ * 1024; break;
    case GVOM_XBUF_SEND_EPS: *ptr = (char *)h->x_send_eps.p + (size_t)peer * (size_t)h->x_ep_cap * 8; cap = h->x_ep_cap * 8; break;
    case GVOM_XBUF_RECV_IDS: *ptr = h->x_recv_ids + (size_t)peer * myQ; cap = (int64_t)myQ * 4; break;
    case GVOM_XBUF_RECV_QUADS: *ptr = (char *)h->x_recv_pay + (size_t)peer * myQ * 1024; cap = (int64_t)myQ * 1024; break;
    case GVOM_XBUF_RECV_EPS:
        *ptr = (char *)h->x_recv_eps.p + (size_t)h->x_recv_ep_off[peer] * 8;
        cap = (h->x_recv_ep_off[peer + 1] - h->x_recv_ep_off[peer]) * 8; break;
    case GVOM_XBUF_SEND_RETURNS: {
        const size_t esz3 = (h->pending_dtype == GVOM_DTYPE_F32 ? 4 : 8) * 3;
        if (!h->x_send_sp.p) return GVOM_NO_DATA;
        *ptr = (char *)h->x_send_sp.p + (size_t)peer * (size_t)h->x_ep_cap * esz3; cap = h->x_ep_cap * (int64_t)esz3; break;
    }
    case GVOM_XBUF_RECV_RETURNS: {
        const size_t esz3 = (h->pending_dtype == GVOM_DTYPE_F32 ? 4 : 8) * 3;
        if (!h->x_recv_sp.p) return GVOM_NO_DATA;
        *ptr = (char *)h->x_recv_sp.p + (size_t)h->x_recv_sp_off[peer] * esz3;
        cap = (h->x_recv_sp_off[peer + 1] - h->x_recv_sp_off[peer]) * (int64_t)esz3; break;
    }
    default: return GVOM_ERR_INVALID;
    }
    if (capacity_bytes) *capacity_bytes = cap;
    return GVOM_OK;
}

VIS int gvom_shard_scan_merge(gvom_t *h, const int64_t *recv_quads, const int64_t *recv_eps, int accept)
{
    if (!h || !h->sharded || !recv_quads || !recv_eps) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->pending) return GVOM_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    if (h->solo_encoded) {                                 // one rank: gvom_shard_scan_local has encoded the scan already
        h->solo_encoded = false;
        scan_commit(h, accept != 0);
        return GVOM_OK;
    }
    Slot &st = h->slots[h->staging];
    const ScanParams &P = h->pending_P;
    int64_t tot_eps = 0;
    for (int sidx = 0; sidx < h->world; ++sidx) {
        if (sidx == h->rank) continue;
        if (recv_quads[sidx] < 0 || recv_quads[sidx] > (int64_t)h->x_myQ || recv_eps[sidx] < 0 ||
            recv_eps[sidx] != h->x_recv_ep_off[sidx + 1] - h->x_recv_ep_off[sidx]) {
            h->err = "gvom_shard_scan_merge: receive counts do not match gvom_shard_recv_reserve / the slab size";
            return GVOM_ERR_INVALID;
        }
        tot_eps += recv_eps[sidx];
    }
    // compact rows: this rank's returns first, the received endpoints behind them
    // (at least one row: k_fuse redirects the loads of unoccupied voxels to row 0 of every source)
    const size_t cap = std::max<size_t>(1, (size_t)h->pending_n + (size_t)tot_eps);
    int rc;
    if ((rc = ensure(h, st.crows, cap * 16))) return rc;
    if (h->stats) {                                       // rows of the received endpoints: behind the rank's own (contents kept)
        const size_t old_rows = st.rowvox.bytes / 4;
        if ((rc = ensure_keep(h, st.metrics, cap * 80)) || (rc = ensure_keep(h, st.base, cap * 8 * GVOM_BASE_PITCH)) ||
            (rc = ensure_keep(h, st.rowvox, cap * 4))) return rc;
        if (st.rowvox.bytes / 4 > old_rows)
            HIPCHK(h, hipMemsetAsync((uint32_t *)st.rowvox.p + old_rows, 0xFF, st.rowvox.bytes - old_rows * 4, h->stream));
    }
    double t0 = now_ns();
    {   // everything received, whatever the source, in one launch each (quads, endpoints)
        ShardUnpack X;
        uint32_t acc = 0;
        for (int sidx = 0; sidx <= GVOM_MAX_SLOTS; ++sidx) {
            X.q_off[sidx] = acc;
            if (sidx < h->world && sidx != h->rank) acc += (uint32_t)recv_quads[sidx];
        }
        hipError_t le = gvom_launch_unpack(h->stream, P, X, h->x_recv_ids, h->x_recv_pay, (uint32_t)h->x_myQ, (uint32_t)tot_eps,
                                           h->x_recv_eps.p, (long)h->pending_n, h->hit, h->total, h->mh, st.state, st.tags,
                                           h->stats ? (double *)st.metrics.p : nullptr, h->stats ? (double *)st.base.p : nullptr,
                                           h->stats ? (uint32_t *)st.rowvox.p : nullptr);
        if (le != hipSuccess) { scan_abort(h); HIPCHK(h, le); }
    }
    const uint32_t seq = ++h->scan_seq;
    hipError_t le = gvom_launch_encode(h->stream, P, h->hit, h->total, h->mh, st.state, st.code16, (uint4 *)st.crows.p,
                                       st.tags, h->counters,
                                       (unsigned long long *)h->counters_host_dev, seq, h->resident_blocks);
    if (le != hipSuccess) { scan_abort(h); HIPCHK(h, le); }
    st.has_code16 = st.code16 != nullptr;
    if (h->profiling) { HIPCHK(h, hipEventRecord(h->ev[2], h->stream)); h->ev_scan = true; }
    if (h->stats) {
        // this rank's own returns (all of them: a return outside its rows can still reach into them) and the ones the
        // other ranks sent, in the direct form over this rank's rows
        const int64_t tot_sp = h->world > 1 ? h->x_recv_sp_off[h->world] : 0;
        if ((rc = enqueue_scan_stats(h, P, h->pending_dtype, st, h->pending_n, (int64_t)cap, h->x_recv_sp.p, tot_sp))) return rc;
    }
    HT(h, 0, t0);
    // (no host wait: everything the caller can do next with this handle is stream-ordered behind k_encode)
    scan_commit(h, accept != 0);
    return GVOM_OK;
}
}  // extern "C"
