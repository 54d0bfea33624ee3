// gvom_combine.hip -- host side of a combine: the temporal fusion and the 2-D stage, their completion, the output buffers and every
// combine entry point that ends in host memory (the device one: gvom_sets.hip).
#include "gvom_host.h"

namespace gvom_host {
// what a fusion into the frame `origin` needs besides its sources (fuse_impl, eager_launch)
void fill_fuse_frame(const gvom_handle *h, const int64_t origin[3], FuseParams &P)
{
    const gvom_params &p = h->prm;
    memset(&P, 0, sizeof P);
    P.xy = p.xy_size; P.zs = p.z_size;
    window_phase(h, origin, P.om);
    P.sy_lo = h->sy_lo; P.sy_hi = h->sy_hi;
    P.nseg = h->nseg;
    P.hs = h->hs;
    for (int k = 0; k < 3; ++k) { P.origin[k] = (double)origin[k]; P.ego[k] = h->ego[k]; }
    P.xy_res = p.xy_resolution; P.z_res = p.z_resolution;
    P.radius2 = p.robot_radius * p.robot_radius;
    P.ground_to_lidar_height = p.ground_to_lidar_height;
}

// z decomposition of k_fuse: chunks of zc levels (16 whenever z_size <= 256), cpw chunks per wave,
// nz waves per workgroup.  Small workgroups (<= 4 waves when possible) keep several of them
// resident per CU, so one workgroup's end-of-column barrier never idles the CU.
static int choose_nz(int zs, int *zc, int *cpw)
{
    int nchunks = (zs + 15) / 16;
    if (nchunks < 1) nchunks = 1;
    if (nchunks > 16) nchunks = 16;
    *zc = (zs + nchunks - 1) / nchunks;
    nchunks = (zs + *zc - 1) / *zc;
    int want_waves = 4;
    *cpw = (nchunks + want_waves - 1) / want_waves;
    if (*cpw < 1) *cpw = 1;
    if (*cpw > 4) *cpw = 4;                               // a wave's tiles (16 per chunk) fit one 64-bit mask
    return (nchunks + *cpw - 1) / *cpw;
}

// fusion + column reductions (k_fuse) into fused[1 - cur]; `on`: the stream (nullptr: the main one; the second
// stream for an asynchronous combine, where it is ordered behind the previous k_map2d by itself)
int fuse_impl(gvom_handle *h, hipStream_t on)
{
    const hipStream_t fs = on ? on : h->stream;
    const gvom_params &p = h->prm;
    const Slot &last = h->slots[h->ring[h->last_buffer_index]];
    if (!last.filled) return GVOM_EMPTY_BUFFER;                        // gvom.py:179-181
    // before any map descriptor below copies an epoch
    if (h->epoch >= 0xFFFFFF00u) { int rc0 = renumber_epochs(h); if (rc0) return rc0; }
    // statistics on demand: the fourth combine in a row that nobody read the statistics before -> it merges none, the scans stop computing them
    if (h->stats_auto && h->stats && ++h->stats_idle > 3) { h->stats = false; h->stats_release = true; }
    if (h->spec_valid && !on && h->spec_slot == h->ring[h->last_buffer_index] && h->spec_nxt == (h->has_combined ? 1 - h->cur : 0)) {
        // eager fusion: k_encfuse has (or will have, in stream order) written exactly what this call would compute -- the one
        // slot, the previous map and the ego are what they were when the scan launched it.  Adopt: swap the spares in.
        Fused &S = h->fused[h->spec_nxt];
        S.origin[0] = h->spec_origin[0]; S.origin[1] = h->spec_origin[1]; S.origin[2] = h->spec_origin[2];
        S.epoch = h->spec_epoch;
        S.valid = true;
        S.has_metrics = h->spec_has_metrics;               // (its k_fuse_stats runs, or has run, on the statistics stream: readers join it)
        std::swap(h->hmaps, h->hmaps2);
        h->height = h->hmaps; h->inferred = h->hmaps + h->prm.xy_size;
        std::swap(h->blockcounts, h->blockcounts2);
        h->cnt_blocks = h->spec_blocks;
        h->cur = h->spec_nxt;
        h->has_combined = true;
        h->maps_valid = false;
        h->spec_valid = false;
        h->eager_waste = 0;
        ++h->eager_stat[0];
        h->last_fuse = GVOM_ROUTE_ENCFUSE;
        h->last_scan_spec = false; h->fresh_scan = false;
        h->stage_ms[3] = 0.0f;                             // (the fusion's time is inside the scan's second kernel)
        if (h->stats_release && !h->scan_inflight) release_statistics_buffers(h);
        return GVOM_OK;
    }
    if (h->spec_valid) { h->spec_valid = false; ++h->eager_stat[1]; }
    else if (h->fresh_scan && !h->last_scan_spec && h->eager_waste > 0) --h->eager_waste;   // a combine right behind a plainly encoded scan: the pattern is coming back
    h->last_scan_spec = false;
    h->fresh_scan = false;
    h->cnt_blocks = h->fuse_blocks;
    if (!on) HIPCHK(h, join_map_stream(h));
    const int nxt = h->has_combined ? 1 - h->cur : 0;
    Fused &F = h->fused[nxt];
    const Fused *prev = (h->has_combined && h->fused[h->cur].valid) ? &h->fused[h->cur] : nullptr;
    F.origin[0] = last.origin[0]; F.origin[1] = last.origin[1]; F.origin[2] = last.origin[2];
    FuseParams P;
    fill_fuse_frame(h, F.origin, P);
    int ns = 0;
    bool all_codes = true;
    // this fusion merges the statistics iff every slot of the ring carries its own; a previous map WITHOUT them (the
    // statistics were switched on again after a pause) contributes none (k_fuse_stats skips a source without metrics): the
    // statistics restart from the ring
    bool fstats = h->stats;
    for (int i = 0; i < p.buffer_size && fstats; ++i) { const Slot &s = h->slots[h->ring[i]]; if (s.filled && !s.has_metrics) fstats = false; }
    for (int i = 0; i < p.buffer_size; ++i) {                          // slot order, gvom.py:198
        const Slot &s = h->slots[h->ring[i]];
        if (!s.filled) continue;
        MapDesc &d = h->descs_host[ns++];
        d.state = s.state; d.rows = (const uint4 *)s.crows.p;
        d.d[0] = clamp_delta(F.origin[0] - s.origin[0], p.xy_size);
        d.d[1] = clamp_delta(F.origin[1] - s.origin[1], p.xy_size);
        d.d[2] = clamp_delta(F.origin[2] - s.origin[2], p.z_size);
        d.epoch = s.epoch; d.tags = s.tags; d.metrics = fstats ? s.metrics.p : nullptr;
        d.code16 = s.code16;
        all_codes = all_codes && s.has_code16;
    }
    P.nslots = ns;
    P.has_prev = prev ? 1 : 0;
    if (prev) {
        MapDesc &d = h->descs_host[ns];
        d.state = prev->state; d.rows = (const uint4 *)prev->rows.p;
        d.d[0] = clamp_delta(F.origin[0] - prev->origin[0], p.xy_size);
        d.d[1] = clamp_delta(F.origin[1] - prev->origin[1], p.xy_size);
        d.d[2] = clamp_delta(F.origin[2] - prev->origin[2], p.z_size);
        d.epoch = prev->epoch; d.tags = prev->tags; d.metrics = (fstats && prev->has_metrics) ? prev->metrics.p : nullptr;
        d.code16 = nullptr;
    }
    P.nz = choose_nz(p.z_size, &P.zc, &P.cpw);
    P.dbg = gvom_diag_env("GVOM_FUSE_DEBUG");
    // one slot in the ring (buffer_size 1, or a ring that has only just begun): k_fuse1 -- up to 8 waves per column block, 2
    // chunks per wave where the grid is high enough (a shorter chain of dependent round trips per wave)
    if (ns == 1 && P.zc == 16 && p.xy_size % 4 == 0 && (h->tune_fuse1 != 1 || !all_codes) && !(P.dbg & 8)) {
        const int nchunks = (p.z_size + 15) / 16;
        int nz = nchunks < 8 ? nchunks : 8;
        int cpw = (nchunks + nz - 1) / nz;
        if (cpw <= 4) { P.one_slot = 1; P.nz = nz; P.cpw = cpw; }
    }
    F.epoch = ++h->epoch;
    P.epoch = F.epoch;
    // every wave of k_fuse owns a static range of 64*zc compact rows (no global reservation)
    const size_t row_cap = (size_t)h->fuse_blocks * P.nz * 64 * P.zc * P.cpw;
    if (row_cap >= 2147483648ull) { h->err = "fused row space exceeds 31 bits"; return GVOM_ERR_CAPACITY; }
    int rc;
    if ((rc = ensure(h, F.rows, row_cap * 16))) return rc;
    if (fstats && (rc = ensure(h, F.metrics, row_cap * 40))) return rc;
    F.has_metrics = fstats;
    const int nsrc = ns + (prev ? 1 : 0);
    // the previous k_fuse_stats reads (as its "previous map") the fused buffer this fusion writes, and the descriptor
    // table this call refills
    if (h->fs_pending) HIPCHK(h, hipStreamWaitEvent(fs, h->ev_fsdone, 0));
    FuseDescs KD;
    const MapDesc *descs_mem = nullptr;
    if (nsrc <= GVOM_KARG_DESCS) {
        memcpy(KD.d, h->descs_host, sizeof(MapDesc) * nsrc);
    } else {
        HIPCHK(h, hipMemcpyAsync(h->descs_dev, h->descs_host, sizeof(MapDesc) * nsrc,
                                 hipMemcpyHostToDevice, fs));
        descs_mem = h->descs_dev;
    }
    if (h->profiling) HIPCHK(h, hipEventRecord(h->ev[4], fs));
    h->last_fuse = 0;
    HIPCHK(h, gvom_launch_fuse(fs, P, KD, descs_mem, F.state, (uint4 *)F.rows.p,
                               F.tags, h->blockcounts,
                               h->height, h->inferred, &h->last_fuse));
    if (h->profiling) { HIPCHK(h, hipEventRecord(h->ev[5], fs)); h->ev_fuse = true; }
    if (fstats) {                                        // beside k_map2d, behind this fusion and the scans' statistics
        HIPCHK(h, hipEventRecord(h->ev_fz_s, fs));
        HIPCHK(h, hipStreamWaitEvent(h->stream_s, h->ev_fz_s, 0));
        HIPCHK(h, gvom_launch_fuse_stats(h->stream_s, P, KD, descs_mem, F.state, F.tags, (float *)F.metrics.p));
        h->fs_reads[0] = h->fs_reads[1] = true;          // (its target's states and, as "previous map", the other buffer's)
        HIPCHK(h, hipEventRecord(h->ev_fsdone, h->stream_s));
        HIPCHK(h, hipEventRecord(h->ev_sdone, h->stream_s));
        h->s_pending = h->fs_pending = true;
    }
    F.valid = true;
    h->cur = nxt;
    h->has_combined = true;
    h->maps_valid = false;
    if (h->stats_release && !h->scan_inflight) release_statistics_buffers(h);   // (this fusion merged no statistics: fstats was false)
    return GVOM_OK;
}

// 2-D maps (k_map2d) from height/inferred of the whole window (all rows must be present).
// gathered: sharded run -- every row of the interleaved height buffer (heights + owner-computed
// positive densities) has been all-gathered and this rank computes ALL rows of the outputs.
// host_out: the host address of a caller's output buffer (out_dev is its device view).  The four maps in [y][x] order into a
// buffer from gvom_output_buffer_alloc go through the buffer's content record (k_map2d's DELTA form: runs that are default now and
// were default the last time are not stored); every other write into a caller's buffer DROPS its record -- the occupancy grids,
// the sharded form, "delta_out" 0 -- so that a record never describes bytes somebody else has written since.
int map2d_impl(gvom_handle *h, bool gathered, bool publish, char *out_dev, bool yx, const double *occ, hipStream_t on,
               uint32_t done_seq, bool dev_set, void *host_out)
{
    const hipStream_t ms = on ? on : h->stream;
    const gvom_params &p = h->prm;
    const Fused &F = h->fused[h->cur];
    Map2dParams P;
    memset(&P, 0, sizeof P);
    P.dbg = gvom_diag_env("GVOM_MAP2D_DEBUG");
    P.xy = p.xy_size; P.zs = p.z_size;
    window_phase(h, F.origin, P.om);
    P.y_lo = gathered ? 0 : h->sy_lo; P.y_hi = gathered ? p.xy_size : h->sy_hi;
    P.origin_z = (double)F.origin[2];
    P.xy_res = p.xy_resolution; P.z_res = p.z_resolution;
    P.pos_thr = p.positive_obstacle_threshold; P.neg_thr = p.negative_obstacle_threshold;
    P.slope_thr = p.slope_obstacle_threshold; P.robot_height = p.robot_height;
    P.out_yx = yx ? 1 : 0;
    if (occ) { P.occ = 1; P.occ_density_thr = occ[0]; P.occ_min_rough = occ[1]; P.occ_max_rough = occ[2]; }
    P.gathered_pos = gathered ? 1 : 0;
    P.nseg = h->nseg;
    P.hs = h->hs;
    P.epoch = F.epoch;
    if (done_seq && !h->tune_flag_kernel) {       // the synchronous combine's completion flag (finish_combine): stored by k_map2d's last workgroup
        P.done_flag = (unsigned long long *)(h->counters_host_dev + 4);
        P.done_count = h->counters + GVOM_CNT_MAPDONE;
        P.done_seq = done_seq;
    }
    const size_t n2 = h->cells2d;
    int32_t *o_pos = (int32_t *)out_dev, *o_neg = o_pos + n2, *o_vis = o_neg + n2;
    double *o_rgh = (double *)(o_vis + n2);
    if (dev_set) {                                // a device map set (DevSet): f64 maps 3-8, then i32 maps 0-2
        const size_t S = dev_map_stride(p.xy_size);
        P.out_dev = 1;
        o_rgh = (double *)out_dev;
        o_pos = (int32_t *)(o_rgh + 6 * S); o_neg = o_pos + S; o_vis = o_neg + S;
    }
    uint8_t *bits = nullptr;
    if (host_out && !dev_set) {
        const bool recorded = h->tune_delta_out != 0 && yx && !occ && !gathered && !h->sharded && !(P.dbg & 1) &&
                              std::find(h->out_bufs.begin(), h->out_bufs.end(), host_out) != h->out_bufs.end();
        if (!recorded) h->out_rec.forget(host_out);
        else {
            const size_t slot_bytes = align256(gvom_outrec_bytes(p.xy_size));
            if (!h->out_rec_bits) HIPCHK(h, hipMalloc((void **)&h->out_rec_bits, slot_bytes * GVOM_OUTREC_MAX));
            bool fresh = false;
            const int slot = h->out_rec.use(host_out, p.xy_size, &fresh);
            bits = h->out_rec_bits + (size_t)slot * slot_bytes;
            // (on the kernel's stream: every k_map2d of this handle is ordered behind the one before it, whichever stream it ran on)
            if (fresh) {
                const hipError_t e = hipMemsetAsync(bits, 0xFF, slot_bytes, ms);
                if (e != hipSuccess) { h->out_rec.forget(host_out); HIPCHK(h, e); }
            }
        }
    }
    if (h->profiling) HIPCHK(h, hipEventRecord(h->ev[6], ms));
    {
        const hipError_t e = gvom_launch_map2d(ms, P, F.state, F.tags, (const uint4 *)F.rows.p,
                                               h->height, h->inferred, h->slope_x,
                                               h->slope_y, h->rough, h->guessed, o_pos, o_neg, o_rgh, o_vis,
                                               h->blockcounts, h->cnt_blocks,
                                               publish ? (unsigned long long *)(h->counters_host_dev + 2) : nullptr, bits);
        if (e != hipSuccess && bits) h->out_rec.forget(host_out);      // (a launch that failed: what the buffer holds is anybody's guess)
        HIPCHK(h, e);
    }
    if (h->profiling) { HIPCHK(h, hipEventRecord(h->ev[7], ms)); h->ev_map = true; }
    h->maps_valid = true;
    return GVOM_OK;
}

// sharded runs: positive-obstacle densities of this rank's rows into the height buffer
static int posdens_impl(gvom_handle *h)
{
    const gvom_params &p = h->prm;
    const Fused &F = h->fused[h->cur];
    Map2dParams P;
    memset(&P, 0, sizeof P);
    P.xy = p.xy_size; P.zs = p.z_size;
    window_phase(h, F.origin, P.om);                      // (k_posdens reads om[2] only)
    P.y_lo = h->sy_lo; P.y_hi = h->sy_hi;
    P.origin_z = (double)F.origin[2];
    P.z_res = p.z_resolution;
    P.pos_thr = p.positive_obstacle_threshold; P.robot_height = p.robot_height;
    P.nseg = h->nseg; P.hs = h->hs; P.epoch = F.epoch;
    // its first workgroup also publishes the fused cell count (k_fuse has completed by then)
    HIPCHK(h, gvom_launch_posdens(h->stream, P, F.state, F.tags, (const uint4 *)F.rows.p,
                                  h->hmaps, h->blockcounts, h->fuse_blocks,
                                  (unsigned long long *)(h->counters_host_dev + 2),
                                  (unsigned long long *)(h->counters + 10)));
    return GVOM_OK;
}

// the fused cell count as the GPU published it in the host-mapped counter; every caller has waited for that in its own way
static void adopt_fused_count(gvom_handle *h)
{
    unsigned long long c;
    memcpy(&c, h->counters_host + 2, 8);
    h->fused[h->cur].count = (int64_t)c;
    h->combined_cell_count = (int64_t)c;
    h->count_pending = false;
}

// Waits for the combine's kernels with the handle mutex RELEASED (a second thread -- the ROS node's
// cloud callback -- can hand the next scan over meanwhile: its kernels queue up behind k_map2d and the
// GPU does not idle between the steps); other combine calls are held off by combine_mu / pending_combine.
static int finish_combine(gvom_handle *h, std::unique_lock<std::mutex> &lk, uint32_t seq)
{
    // completion: k_map2d's last workgroup stores the sequence number into host-mapped memory (map2d_impl) and the host
    // spins on it (an event wait notices the end of the stream several microseconds later; round 3's one-thread kernel
    // behind k_map2d cost 4 us of every step)
    if (h->tune_flag_kernel) HIPCHK(h, gvom_launch_publish_seq(h->stream, (unsigned long long *)(h->counters_host_dev + 4), seq));
    HIPCHK(h, hipEventRecord(h->ev_done, h->stream));
    h->pending_combine = true;
    hipError_t e = hipSuccess;
    if (!wait_published(h, lk, (volatile unsigned long long *)(h->counters_host + 4), seq, false, &h->last_wait_ns[1])) {
        lk.unlock();
        e = hipEventSynchronize(h->ev_done);
        lk.lock();
    }
    h->pending_combine = false;
    HIPCHK(h, e);
    adopt_fused_count(h);
    collect_stage_ms(h);
    return GVOM_OK;
}

// the fused cell count of a device combine: read from the host-mapped counter once its k_map2d has completed (handle mutex held)
int settle_count(gvom_handle *h)
{
    if (!h->count_pending) return GVOM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipEventSynchronize(h->ev_dcount));
    adopt_fused_count(h);
    return GVOM_OK;
}
}  // namespace gvom_host

extern "C" {
// A caller's own output buffer must be COHERENT pinned memory (see gvom_hip.h, gvom_combine_maps_into): the completion flag is only
// ordered behind the maps for write-through stores.  Buffers from gvom_output_buffer_alloc are; others are asked once.
static int check_out_buffer(gvom_handle *h, void *pinned_out)
{
    if (std::find(h->out_bufs.begin(), h->out_bufs.end(), pinned_out) != h->out_bufs.end() || pinned_out == h->last_checked_out) return GVOM_OK;
    unsigned int flags = 0;
    if (hipHostGetFlags(&flags, pinned_out) != hipSuccess) { (void)hipGetLastError(); h->err = "output buffer is not pinned host memory (hipHostMalloc)"; return GVOM_ERR_INVALID; }
    if (!(flags & hipHostMallocCoherent) || !(flags & hipHostMallocMapped)) {
        h->err = "output buffer must be coherent, device-mapped pinned memory (hipHostMallocMapped | hipHostMallocCoherent; gvom_output_buffer_alloc returns such)";
        return GVOM_ERR_INVALID;
    }
    h->last_checked_out = pinned_out;
    return GVOM_OK;
}

// One body for the synchronous combines: fusion, k_map2d, the wait for its completion flag, the origin.  With a caller's buffer
// k_map2d writes there ([y][x] order; `occ`: the occupancy grids); without one, into the handle's own pinned staging buffer ([x][y]
// order), from where the four maps are copied to `copy_to` -- still under both locks: the next combine overwrites the staging buffer.
struct HostMaps { int32_t *positive, *negative; double *roughness; int32_t *visibility; };
static int combine_sync(gvom_handle *h, double origin_world[3], void *pinned_out, const double *occ, const HostMaps *copy_to)
{
    std::lock_guard<std::mutex> ck(h->combine_mu);
    std::unique_lock<std::mutex> lk(h->mu);
    if (h->pending_combine) { h->err = "a combine begun with gvom_combine_begin has not been ended"; return GVOM_ERR_INVALID; }
    HIPCHK(h, hipSetDevice(h->device));
    if (pinned_out) { const int rc0 = check_out_buffer(h, pinned_out); if (rc0) return rc0; }
    double t0 = now_ns();
    int rc = fuse_impl(h);
    if (rc) return rc;
    char *dev = h->out_host_dev;
    if (pinned_out) HIPCHK(h, hipHostGetDevicePointer((void **)&dev, pinned_out, 0));
    const uint32_t done_seq = ++h->combine_seq;
    if ((rc = map2d_impl(h, false, true, dev, pinned_out != nullptr, occ, nullptr, done_seq, false, pinned_out))) return rc;
    HT(h, 2, t0);                                        // combine: launches
    if ((rc = finish_combine(h, lk, done_seq))) { if (pinned_out) h->out_rec.forget(pinned_out); return rc; }
    HT(h, 3, t0);                                        // combine: wait
    if (copy_to) {
        const size_t n2 = h->cells2d;
        const char *stage = (const char *)h->out_host;
        if (copy_to->positive) memcpy(copy_to->positive, stage, n2 * 4);
        if (copy_to->negative) memcpy(copy_to->negative, stage + n2 * 4, n2 * 4);
        if (copy_to->visibility) memcpy(copy_to->visibility, stage + n2 * 8, n2 * 4);
        if (copy_to->roughness) memcpy(copy_to->roughness, stage + n2 * 12, n2 * 8);
        HT(h, 4, t0);                                    // combine: pinned -> caller copies
    }
    world_origin(h, h->fused[h->cur], origin_world);
    return GVOM_OK;
}

VIS int gvom_combine_maps(gvom_t *h, double origin_world[3], int32_t *positive, int32_t *negative,
                          double *roughness, int32_t *visibility)
{
    if (!h || h->sharded) return GVOM_ERR_INVALID;
    const HostMaps out = {positive, negative, roughness, visibility};
    return combine_sync(h, origin_world, nullptr, nullptr, &out);
}

// ---- zero-copy outputs ---------------------------------------------------------------------
// gvom_output_buffer_alloc returns a pinned, device-mapped host buffer of 20*xy*xy bytes laid out
// [positive i32 | negative i32 | visibility i32 | roughness f64] (each xy*xy, COLUMN-major:
// cell (x, y) at m[y*xy + x]).
// gvom_combine_maps_into makes k_map2d write the four maps straight into such a buffer: no D2H
// copy command and no pinned->caller memcpy.  The caller owns the buffer until it frees it
// (g-vom_amd/gvom.py recycles them through a pool when the returned numpy arrays are collected).
VIS int gvom_output_buffer_alloc(gvom_t *h, void **host_ptr)
{
    if (!h || !host_ptr) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    // GVOM_OUT_COHERENT=1: fine-grained (coherent) pinned memory -- stores leave the GPU as they are
    // issued instead of being written back from L2 at the end of the kernel
    HIPCHK(h, hipHostMalloc(host_ptr, h->cells2d * 20, hipHostMallocMapped | hipHostMallocCoherent));
    h->out_bufs.push_back(*host_ptr);
    return GVOM_OK;
}

VIS int gvom_output_buffer_free(gvom_t *h, void *host_ptr)
{
    if (!h || !host_ptr) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, sync_streams(h));
    for (size_t k = 0; k < h->out_bufs.size(); ++k)
        if (h->out_bufs[k] == host_ptr) { h->out_bufs[k] = h->out_bufs.back(); h->out_bufs.pop_back(); break; }
    if (h->last_checked_out == host_ptr) h->last_checked_out = nullptr;
    h->out_rec.forget(host_ptr);                         // (the allocator may hand the address out again)
    HIPCHK(h, hipHostFree(host_ptr));
    return GVOM_OK;
}

// The CONTENT RECORD of an output buffer (k_map2d stores only the runs that changed: include/gvom_hip.h) is dropped: the next
// combine into `host_ptr` stores every run again.  For a caller that has written into the buffer itself.  Unknown pointers are fine.
VIS int gvom_output_forget(gvom_t *h, void *host_ptr)
{
    if (!h || !host_ptr) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    h->out_rec.forget(host_ptr);
    return GVOM_OK;
}

// Read-back of a buffer's record (measurements, tests): waits for the handle's streams and copies the record's bytes -- one per
// (32 x 8 tile, wave), gvom_outrec.h -- to `bits` (`cap` bytes available); *n: bytes the record has.  GVOM_NO_DATA: no record.
VIS int gvom_output_record(gvom_t *h, void *host_ptr, uint8_t *bits, size_t cap, size_t *n, uint64_t *generation)
{
    if (!h || !host_ptr || !n) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    const int slot = h->out_rec.find(host_ptr);
    if (slot < 0 || !h->out_rec_bits) return GVOM_NO_DATA;
    *n = gvom_outrec_bytes(h->prm.xy_size);
    if (generation) *generation = h->out_rec.e[slot].gen;
    if (!bits) return GVOM_OK;
    if (cap < *n) return GVOM_ERR_CAPACITY;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, sync_streams(h));
    HIPCHK(h, hipMemcpy(bits, h->out_rec_bits + (size_t)slot * align256(*n), *n, hipMemcpyDeviceToHost));
    return GVOM_OK;
}

VIS int gvom_combine_maps_into(gvom_t *h, double origin_world[3], void *pinned_out)
{
    if (!h || !pinned_out || h->sharded) return GVOM_ERR_INVALID;
    return combine_sync(h, origin_world, pinned_out, nullptr, nullptr);
}

// combine_maps + the ROS node's post-processing (gvom_ros.py:141-165) in one call: the fusion
// advances exactly as in gvom_combine_maps, but k_map2d writes the five int8
// nav_msgs/OccupancyGrid.data arrays [hard | soft | certainty | negative | roughness] (each xy*xy
// bytes, x fastest = the node's reshape(order='F')) into the pinned buffer: 5 bytes per cell cross
// PCIe instead of 20.
VIS int gvom_combine_occupancy_into(gvom_t *h, double origin_world[3], void *pinned_out,
                                    double density_threshold, double min_roughness, double max_roughness)
{
    if (!h || !pinned_out || h->sharded) return GVOM_ERR_INVALID;
    const double occ[3] = {density_threshold, min_roughness, max_roughness};
    return combine_sync(h, origin_world, pinned_out, occ, nullptr);
}

// ---- asynchronous combine --------------------------------------------------------------------
// gvom_combine_begin = gvom_combine_maps_into / gvom_combine_occupancy_into (occ != NULL: its three
// thresholds) without the wait: the fusion is enqueued on the handle's stream, k_map2d on a second
// stream behind it.  The caller may hand the next scan to gvom_process_pointcloud* right away: its
// k_trace / k_encode run WHILE k_map2d stores the maps over PCIe (the next fusion waits for it on the
// device).  gvom_combine_end waits for the maps (handle mutex released while it waits) and completes
// the call; `pinned_out` must not be read before it returns.  One combine may be pending at a time.
VIS int gvom_combine_begin(gvom_t *h, void *pinned_out, const double *occ)
{
    if (!h || !pinned_out || h->sharded) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->pending_combine) { h->err = "a combine begun with gvom_combine_begin has not been ended"; return GVOM_ERR_INVALID; }
    HIPCHK(h, hipSetDevice(h->device));
    { const int rc0 = check_out_buffer(h, pinned_out); if (rc0) return rc0; }
    { const int rc0 = settle_count(h); if (rc0) return rc0; }   // (a device combine's count, before the fusion moves on)
    double t0 = now_ns();
    // k_map2d goes to the second stream, and with a ring of three or more filled slots the fusion too (behind
    // the scan's k_encode on the main stream): the next scan's k_trace / k_encode overlap them -- they touch the
    // accumulators and the spare slot only.  (Measured, pipelined use, fusion on the main / the second stream:
    // m256 86.5 / 88.8 us per step, c4 680 / 692, but c3 137 / 115, m256b8 119 / 102: a long fusion is worth it.)
    int filled = 0;
    for (int i = 0; i < h->prm.buffer_size; ++i) filled += h->slots[h->ring[i]].filled ? 1 : 0;
    const bool fuse_on_b = filled >= 3;
    int rc;
    if (fuse_on_b) {
        HIPCHK(h, hipEventRecord(h->ev_fused, h->stream));
        HIPCHK(h, hipStreamWaitEvent(h->stream_b, h->ev_fused, 0));
        if ((rc = fuse_impl(h, h->stream_b))) return rc;
        HIPCHK(h, hipEventRecord(h->ev_fuse_b, h->stream_b));
        h->fuse_b_unjoined = true;
        h->fuse_b_slots = 0;
        for (int i = 0; i < h->prm.buffer_size; ++i)
            if (h->slots[h->ring[i]].filled) h->fuse_b_slots |= 1ull << h->ring[i];
    } else {
        if ((rc = fuse_impl(h))) return rc;
        HIPCHK(h, hipEventRecord(h->ev_fused, h->stream));
        HIPCHK(h, hipStreamWaitEvent(h->stream_b, h->ev_fused, 0));
    }
    char *dev = nullptr;
    HIPCHK(h, hipHostGetDevicePointer((void **)&dev, pinned_out, 0));
    if ((rc = map2d_impl(h, false, true, dev, true, occ, h->stream_b, 0, false, pinned_out))) return rc;
    HIPCHK(h, hipEventRecord(h->ev_mapped, h->stream_b));
    h->mapped_unjoined = true;
    h->pending_combine = true;
    HT(h, 2, t0);
    return GVOM_OK;
}

VIS int gvom_combine_end(gvom_t *h, double origin_world[3])
{
    if (!h) return GVOM_ERR_INVALID;
    std::unique_lock<std::mutex> lk(h->mu);
    if (!h->pending_combine) { h->err = "gvom_combine_end without gvom_combine_begin"; return GVOM_ERR_INVALID; }
    HIPCHK(h, hipSetDevice(h->device));
    double t0 = now_ns();
    // (an event wait: in the pipelined use the maps are usually there already, and a completion-flag kernel on
    // the second stream would cost more than it saves -- measured 91.0 against 86.5 us per step)
    lk.unlock();                                           // process_pointcloud may run meanwhile
    const hipError_t e = hipEventSynchronize(h->ev_mapped);
    lk.lock();
    h->pending_combine = false;                            // (also on failure: the handle must not stay blocked)
    h->fuse_b_unjoined = false;                            // k_map2d has completed, and the fusion in front of it
    if (e != hipSuccess) h->out_rec.clear();               // (what the buffer holds is anybody's guess)
    HIPCHK(h, e);
    adopt_fused_count(h);
    HT(h, 3, t0);
    world_origin(h, h->fused[h->cur], origin_world);
    return GVOM_OK;
}

// ---- split combine for the sharded layer (g-vom_amd/gvom_sharded.py) ---------------------
// 1. gvom_combine_fuse: local slab fusion; height/inferred rows of this rank are valid.
// 2. gvom_rows_export / gvom_rows_import: device<->device copies of 2-D map rows in storage
//    order ([sy][sx], row range of a rank is contiguous) to/from caller-owned device buffers
//    (the collectives run on those, e.g. torch.distributed all_gather over RCCL).
// 3. gvom_combine_map2d: local rows of the four outputs, in storage order.
// 4. gvom_finalize_outputs: storage order -> the reference's [x][y] window order (rank 0).
VIS int gvom_combine_fuse(gvom_t *h, int64_t *local_cells)
{
    if (!h) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    int rc = fuse_impl(h);
    if (rc) return rc;
    // third row of the height buffer + the cell count -- unless this rank holds every row (a sharded map of ONE rank): nothing
    // is gathered then, and k_map2d computes the densities of its own cells and publishes the count, as on an unsharded handle
    if (!(h->sharded && h->world == 1) && (rc = posdens_impl(h))) return rc;
    if (h->sharded) {                                     // no host wait: the count stays on the device (GVOM_BUF_FUSED_CELLS)
        if (local_cells) *local_cells = -1;
        return GVOM_OK;
    }
    HIPCHK(h, sync_streams(h));                           // (a split combine call: plain wait under the handle mutex)
    adopt_fused_count(h);
    collect_stage_ms(h);
    if (local_cells) *local_cells = h->fused[h->cur].count;
    return GVOM_OK;
}

VIS int gvom_set_combined_cell_count(gvom_t *h, int64_t global_cells)
{
    if (!h) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    h->combined_cell_count = global_cells;
    return GVOM_OK;
}

// sharded runs, after the in-place all_gather of GVOM_BUF_HEIGHT_MAPS: all rows of the four
// outputs, written by the GPU straight into a pinned buffer from gvom_output_buffer_alloc
// (same layout as gvom_combine_maps_into).  Synchronises.
VIS int gvom_combine_map2d_into(gvom_t *h, double origin_world[3], void *pinned_out)
{
    if (!h || !pinned_out) return GVOM_ERR_INVALID;
    std::unique_lock<std::mutex> lk(h->mu);              // (ONE lock object: finish_combine releases it while the host spins)
    if (!h->has_combined) return GVOM_NO_DATA;
    HIPCHK(h, hipSetDevice(h->device));
    { const int rc0 = check_out_buffer(h, pinned_out); if (rc0) return rc0; }   // (the completion flag is only sound for coherent pinned memory)
    char *dev = nullptr;
    HIPCHK(h, hipHostGetDevicePointer((void **)&dev, pinned_out, 0));
    // completion as in the unsharded combine: k_map2d's last workgroup stores a flag the host spins on (a stream
    // synchronisation notices the end of the stream several microseconds later); the count was published by k_posdens
    const uint32_t done_seq = ++h->combine_seq;
    const bool solo = h->sharded && h->world == 1;       // (every row is this rank's: no gathered densities, see gvom_combine_fuse)
    int rc = map2d_impl(h, !solo, solo, dev, true, nullptr, nullptr, done_seq, false, pinned_out);
    if (rc == GVOM_OK) rc = finish_combine(h, lk, done_seq);
    if (rc) return rc;
    world_origin(h, h->fused[h->cur], origin_world);
    return GVOM_OK;
}
}  // extern "C"
