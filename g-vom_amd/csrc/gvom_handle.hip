// gvom_handle.hip -- the handle of the C ABI declared in include/gvom_hip.h: creation and destruction, the device arena and the
// process-wide export pool, stream joins and host waits, tuning / profiling / info calls, region generations.
//
// Replaces the host bodies of the reference's Gvom.__init__ / process_pointcloud /
// combine_maps (/root/reference/scripts/gvom.py:29-354, "gvom.py:NNN").  Differences in
// mechanism, not in results:
//   * all device memory is a grow-only arena owned by the handle (the reference allocates
//     ~17 arrays per call);
//   * 3 launches per scan and 2 per combine on one private HIP stream (reference: ~20 and
//     ~35+3B), one 16-byte D2H per scan, one D2H of the four maps per combine;
//   * ring slots are swapped with a spare staging slot on commit, so a rejected scan
//     (gvom.py:148-150) leaves the ring untouched.
#include "gvom_host.h"

namespace gvom_host {
// (process-wide: a value names one state of one handle's allocations -- gvom_alloc_generation)
static std::atomic<uint64_t> g_alloc_generation{0};

// Regions another process has had mapped are never given back to the allocator while this process lives (a later allocation
// tends to get their address, and importers that open "it" have been seen reading the OLD memory: profiles/r3_peer_churn.txt).
// They wait in a process-wide POOL instead, with their real sizes and their generation (= the name the communicators know
// the allocation by: a region that becomes current again is neither exported nor opened a second time), and the next
// handle that needs an exportable region of that size takes one from there.  The pool is accounted exactly; past
// GVOM_POOL_WARN_BYTES it says so on stderr, once -- it never falls back to freeing.
#define GVOM_POOL_WARN_BYTES ((size_t)16 << 30)
struct ExportPool {
    std::mutex m;
    std::vector<Buf> v;
    size_t bytes = 0;
    bool warned = false;
};
static ExportPool g_pool;
static void pool_put(void *p, size_t bytes, uint64_t gen)
{
    if (!p) return;
    std::lock_guard<std::mutex> lk(g_pool.m);
    Buf b; b.p = p; b.bytes = bytes; b.gen = gen;
    g_pool.v.push_back(b);
    g_pool.bytes += bytes;
    if (g_pool.bytes > GVOM_POOL_WARN_BYTES && !g_pool.warned) {
        g_pool.warned = true;
        fprintf(stderr, "libgvom_hip: %zu MiB of device memory that other processes may have mapped are parked (never freed while "
                        "the process lives; re-used by later sharded handles of the same sizes): create fewer exported handles per process\n",
                g_pool.bytes >> 20);
    }
}
// an exportable allocation of exactly `bytes` (a multiple of 2 MiB): a parked one, or a fresh one
// (*reused: the region came out of the pool, i.e. some peer may STILL have it mapped: its next owner must park it again
// whether or not it exports anything itself -- ADVICE r4)
static hipError_t pool_get(size_t bytes, void **p, uint64_t *gen, bool *reused = nullptr)
{
    {
        std::lock_guard<std::mutex> lk(g_pool.m);
        for (size_t k = 0; k < g_pool.v.size(); ++k)
            if (g_pool.v[k].bytes == bytes) {
                *p = g_pool.v[k].p; *gen = g_pool.v[k].gen;
                if (reused) *reused = true;
                g_pool.bytes -= bytes;
                g_pool.v.erase(g_pool.v.begin() + (long)k);
                return hipSuccess;
            }
    }
    *gen = ++g_alloc_generation;
    return hipMalloc(p, bytes);
}

int ensure(gvom_handle *h, Buf &b, size_t bytes)
{
    if (b.bytes >= bytes) return GVOM_OK;
    size_t want = bytes + bytes / 2 + 256;
    const bool exported = &b == &h->x_send_eps || &b == &h->x_send_sp;
    if (exported) want = exportable_size(want);
    // (a region another process may have mapped is never freed while the handle lives: freed and re-allocated, the new region
    // tends to get the old one's address, and importers that re-open "it" were seen reading the OLD memory -- a silently
    // different map after ~50 scans of the churn test.  Growth is geometric: the retired regions add up to less than the last.)
    if (b.p && exported) { h->retired.push_back(b); b.p = nullptr; }
    if (b.p) HIPCHK(h, hipFree(b.p));
    b.p = nullptr; b.bytes = 0;
    if (exported) HIPCHK(h, pool_get(want, &b.p, &b.gen, &h->holds_pooled));
    else { HIPCHK(h, hipMalloc(&b.p, want)); b.gen = ++g_alloc_generation; }
    b.bytes = want;
    if (&b == &h->x_send_eps || &b == &h->x_send_sp) h->alloc_gen = b.gen;   // (see gvom_alloc_generation)
    return GVOM_OK;
}

// grows a device buffer KEEPING its contents (stream-ordered copy, then a wait: rare)
int ensure_keep(gvom_handle *h, Buf &b, size_t bytes)
{
    if (b.bytes >= bytes) return GVOM_OK;
    const size_t want = bytes + bytes / 2 + 256;
    void *np = nullptr;
    HIPCHK(h, hipMalloc(&np, want));
    if (b.p) {
        HIPCHK(h, hipMemcpyAsync(np, b.p, b.bytes, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipFree(b.p));
    }
    b.p = np; b.bytes = want;
    return GVOM_OK;
}

static int create_impl(const gvom_params *params, int device_id, int rank, int world, bool sharded, gvom_t **out)
{
    if (!params || !out) return GVOM_ERR_INVALID;
    *out = nullptr;
    if (params->xy_size <= 0 || params->z_size <= 0 || params->buffer_size <= 0 ||
        !(params->xy_resolution > 0) || !(params->z_resolution > 0) || world <= 0 || rank < 0 ||
        rank >= world)
        return GVOM_ERR_INVALID;
    if (params->buffer_size >= GVOM_MAX_SLOTS || params->z_size > 1024 || world > GVOM_MAX_SLOTS) return GVOM_ERR_CAPACITY;
    // a sharded map: every rank owns xy/world storage rows, a multiple of 4 (accumulator patches are
    // 4 rows high); per-voxel statistics need every return on the owner and are not exchanged
    if (sharded && params->xy_size % (4 * world) != 0) return GVOM_ERR_INVALID;
    const double Vd = (double)params->xy_size * params->xy_size * params->z_size;
    if (Vd >= 2147483648.0) return GVOM_ERR_CAPACITY;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev)
        return GVOM_ERR_NO_DEVICE;
    gvom_handle *h = new gvom_handle();
    h->alloc_gen = h->handle_gen = ++g_alloc_generation;
    h->prm = *params;
    h->device = device_id;
    h->rank = rank; h->world = world; h->sharded = sharded;
    h->stats = (params->reserved0 & GVOM_FLAG_VOXEL_STATISTICS) != 0;
    h->stats_auto = !h->stats && !sharded && (params->reserved0 & GVOM_FLAG_STATISTICS_ON_DEMAND) != 0;
    if (h->stats_auto) h->stats = true;
    h->f32_sqrt = (params->reserved0 & GVOM_FLAG_CUDA_F32_SQRT) != 0;
    h->fastdiv_ok = (verify_fastdiv(params->xy_resolution) ? 1 : 0) | (verify_fastdiv(params->z_resolution) ? 2 : 0);
    if (const char *v = getenv("GVOM_VOXEL_STATISTICS")) { h->stats = atoi(v) != 0; h->stats_auto = false; }
    // sharded statistics send a return to the ranks that own the first and the last row of its neighbourhood: the
    // neighbourhood (2 xy_eigen_dist + 1 rows) must not reach over a whole slab
    if (sharded && h->stats && world > 1 && 2 * params->xy_eigen_dist + 1 > params->xy_size / world) { delete h; return GVOM_ERR_INVALID; }
    if (const char *v = getenv("GVOM_HOST_TIMING")) h->host_timing = atoi(v) != 0;
    const int xy = params->xy_size, zs = params->z_size;
    h->sy_lo = (int)((int64_t)xy * rank / world);
    h->sy_hi = (int)((int64_t)xy * (rank + 1) / world);
    h->V = (size_t)xy * xy * zs;
    h->slabV = (size_t)(h->sy_hi - h->sy_lo) * xy * zs;
    h->cells2d = (size_t)xy * xy;
    h->nseg = (xy + 63) / 64;
    h->ntiles = (size_t)xy * zs * h->nseg;
#define CK(call)                                                                                \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            fprintf(stderr, "gvom_create: %s failed: %s\n", #call, hipGetErrorString(e_));      \
            gvom_destroy(h);                                                                    \
            return GVOM_ERR_HIP;                                                                \
        }                                                                                       \
    } while (0)
    CK(hipSetDevice(device_id));
    CK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->own_stream = h->stream;
    {   // the second stream's kernels (fusion, k_map2d: latency- and PCIe-bound, few waves) go ahead of the
        // instruction-bound k_trace they overlap with in an asynchronous combine
        int lo = 0, hi = 0;
        CK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        CK(hipStreamCreateWithPriority(&h->stream_b, hipStreamNonBlocking, hi));
    }
    CK(hipEventCreateWithFlags(&h->ev_fused, hipEventDisableTiming));
    CK(hipEventCreateWithFlags(&h->ev_mapped, hipEventDisableTiming));
    CK(hipEventCreateWithFlags(&h->ev_done, hipEventDisableTiming));
    CK(hipEventCreateWithFlags(&h->ev_fuse_b, hipEventDisableTiming));
    CK(hipStreamCreateWithFlags(&h->stream_up, hipStreamNonBlocking));
    CK(hipStreamCreateWithFlags(&h->stream_s, hipStreamNonBlocking));
    for (hipEvent_t *e : {&h->ev_enc_s, &h->ev_fz_s, &h->ev_sdone, &h->ev_fsdone, &h->ev_before[0], &h->ev_before[1]})
        CK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    CK(hipEventCreateWithFlags(&h->ev_up, hipEventDisableTiming));
    // accumulators are micro-tiled in 4x4 (x,y) patches (gvom_internal.h "ACCUMULATOR LAYOUT")
    // row pitch of the patch rows, padded (GVOM_ACC_PAD lines of 64 B) so that the z levels of one
    // (x, y) patch -- xy*16 bytes apart, a multiple of 4 KiB for xy = 256 -- do not all map to the
    // same memory channel
    h->sxq = (xy + 3) / 4 + h->acc_pad;
    const size_t acc_elems = (size_t)h->sxq * ((xy + 3) / 4) * zs * 16 + 256;
    h->acc_elems = acc_elems;
    CK(hipMalloc((void **)&h->hit, acc_elems * 4));
    CK(hipMalloc((void **)&h->total, acc_elems * 4));
    CK(hipMalloc((void **)&h->mh, acc_elems * 4));
    CK(hipMemsetAsync(h->hit, 0, acc_elems * 4, h->stream));
    CK(hipMemsetAsync(h->total, 0, acc_elems * 4, h->stream));
    CK(hipMemsetAsync(h->mh, 0, acc_elems * 4, h->stream));
    {   // 256-thread workgroups the device keeps resident (8 per CU at <= 64 VGPRs / <= 80 SGPRs)
        hipDeviceProp_t pr;
        CK(hipGetDeviceProperties(&pr, device_id));
        h->resident_blocks = (unsigned)pr.multiProcessorCount * 8u;
    }
    h->slots.resize(params->buffer_size + 1);
    for (auto &s : h->slots) {
        CK(hipMalloc((void **)&s.state, h->V * 4));
        if ((params->xy_size & 3) == 0) CK(hipMalloc((void **)&s.code16, h->V * 2));
        CK(hipMalloc((void **)&s.tags, h->ntiles * 4));
        CK(hipMemsetAsync(s.tags, 0, h->ntiles * 4, h->stream));
    }
    h->ring.resize(params->buffer_size);
    for (int i = 0; i < params->buffer_size; ++i) h->ring[i] = i;
    h->staging = params->buffer_size;
    for (int k = 0; k < 2; ++k) {
        CK(hipMalloc((void **)&h->fused[k].state, h->V * 4));
        CK(hipMalloc((void **)&h->fused[k].tags, h->ntiles * 4));
        CK(hipMemsetAsync(h->fused[k].tags, 0, h->ntiles * 4, h->stream));
    }
    CK(hipMalloc((void **)&h->dir_hist.p, 3 * GVOM_DIRBINS * 4));
    CK(hipMemsetAsync(h->dir_hist, 0, 3 * GVOM_DIRBINS * 4, h->stream));
    CK(hipMalloc((void **)&h->counters, GVOM_CNT_WORDS * 4));
    CK(hipHostMalloc((void **)&h->counters_host, 64, hipHostMallocMapped | hipHostMallocCoherent));
    CK(hipHostGetDevicePointer((void **)&h->counters_host_dev, h->counters_host, 0));
    memset(h->counters_host, 0, 64);
    CK(hipMemsetAsync(h->counters, 0, GVOM_CNT_WORDS * 4, h->stream));
    CK(hipMalloc((void **)&h->descs_dev, sizeof(MapDesc) * (GVOM_MAX_SLOTS + 1)));
    CK(hipHostMalloc((void **)&h->descs_host, sizeof(MapDesc) * (GVOM_MAX_SLOTS + 1)));
    h->fuse_blocks = ((xy + 63) / 64) * (h->sy_hi - h->sy_lo);
    CK(hipMalloc((void **)&h->blockcounts, (size_t)(h->fuse_blocks > 0 ? h->fuse_blocks : 1) * 4));
    CK(hipMemsetAsync(h->blockcounts, 0, (size_t)(h->fuse_blocks > 0 ? h->fuse_blocks : 1) * 4, h->stream));
    h->cnt_blocks = h->fuse_blocks;
    if (!sharded && params->buffer_size == 1 && xy % 16 == 0 && zs >= 4) {       // eager fusion possible (with or without statistics)
        CK(hipMalloc((void **)&h->blockcounts2, (size_t)(h->fuse_blocks > 0 ? h->fuse_blocks : 1) * 4));
        CK(hipMemsetAsync(h->blockcounts2, 0, (size_t)(h->fuse_blocks > 0 ? h->fuse_blocks : 1) * 4, h->stream));
        CK(hipMalloc((void **)&h->hmaps2, h->cells2d * 24));
    }
    h->hs = 3 * xy;
    if (sharded) CK(pool_get(exportable_size(h->cells2d * 24), (void **)&h->hmaps, &h->fixed_gen[2], &h->holds_pooled));
    else CK(hipMalloc((void **)&h->hmaps, h->cells2d * 24));
    h->height = h->hmaps; h->inferred = h->hmaps + xy;
    double **maps[4] = {&h->slope_x, &h->slope_y, &h->rough, &h->guessed};
    for (auto m : maps) CK(hipMalloc((void **)m, h->cells2d * 8));

    // coherent: gvom_combine_maps learns of completion from a flag a later kernel stores (finish_combine), not from a
    // stream synchronisation; k_map2d's stores to non-coherent host memory would only be guaranteed visible after one
    CK(hipHostMalloc(&h->out_host, h->cells2d * 20, hipHostMallocMapped | hipHostMallocCoherent));
    CK(hipHostGetDevicePointer((void **)&h->out_host_dev, h->out_host, 0));
    if (sharded) {
        // rank exchange regions (DESIGN.md "Multi-GPU"): a quad = 4 storage rows x 64 sx at one sz
        h->x_Q = (size_t)(xy / 4) * zs * h->nseg;
        h->x_myQ = h->x_Q / world;
        CK(pool_get(exportable_size(h->x_Q * 4), (void **)&h->x_send_ids, &h->fixed_gen[0], &h->holds_pooled));
        CK(pool_get(exportable_size(h->x_Q * 1024), &h->x_send_pay, &h->fixed_gen[1], &h->holds_pooled));
        CK(hipMalloc((void **)&h->x_recv_ids, h->x_Q * 4));
        CK(hipMalloc(&h->x_recv_pay, h->x_Q * 1024));
        CK(hipMalloc((void **)&h->x_qcnt, (size_t)world * 64));
        CK(hipMalloc((void **)&h->x_ecnt, (size_t)world * 64));
        CK(hipMalloc((void **)&h->x_spcnt, (size_t)world * 64));
        CK(hipMemsetAsync(h->x_qcnt, 0, (size_t)world * 64, h->stream));
        CK(hipMemsetAsync(h->x_ecnt, 0, (size_t)world * 64, h->stream));
        CK(hipMemsetAsync(h->x_spcnt, 0, (size_t)world * 64, h->stream));
        CK(hipHostMalloc((void **)&h->x_host, (size_t)(3 * world + 2) * 8, hipHostMallocMapped | hipHostMallocCoherent));
        CK(hipHostGetDevicePointer((void **)&h->x_host_dev, h->x_host, 0));
        memset(h->x_host, 0, (size_t)(3 * world + 2) * 8);
        h->x_recv_ep_off.assign(world + 1, 0);
        h->x_recv_sp_off.assign(world + 1, 0);
    }
    for (auto &e : h->ev) CK(hipEventCreate(&e));
    CK(hipStreamSynchronize(h->stream));
#undef CK
    *out = h;
    return GVOM_OK;
}

// Somebody reads the per-voxel statistics: a handle that computes them ON DEMAND keeps doing so, or starts again (the caller of
// this read finds no data; the scans that follow carry statistics, and the fused map does once every ring slot does).
void stats_demand(gvom_handle *h)
{
    h->stats_idle = 0;
    if (h->stats_auto && !h->stats) { h->stats = true; h->stats_release = false; }
}

// Statistics on demand, switched off: their buffers (the slots' metrics / own-voxel moments / row tables, the fused maps' metrics,
// the kept clouds -- 40 bytes per voxel and fused map alone: 2.7 GB on the 512^2 x 128 grid) go back to the allocator; a later
// demand allocates them again.  Everything that can still read or write them runs on the statistics stream: waited for first
// (a scan of another thread whose trace is still in flight writes its slot's tables: the release then waits for a later combine).
void release_statistics_buffers(gvom_handle *h)
{
    h->stats_release = false;
    (void)hipStreamSynchronize(h->stream_s);
    h->s_pending = h->fs_pending = false;
    h->before_valid[0] = h->before_valid[1] = false;
    auto fb = [](Buf &b) { if (b.p) (void)hipFree(b.p); b.p = nullptr; b.bytes = 0; };
    for (auto &sl : h->slots) { fb(sl.metrics); fb(sl.base); fb(sl.rowvox); sl.has_metrics = false; }
    for (int k = 0; k < 2; ++k) { fb(h->fused[k].metrics); h->fused[k].has_metrics = false; }
    fb(h->world_pts[0]); fb(h->world_pts[1]); fb(h->flink[0]); fb(h->flink[1]);
    h->spec_has_metrics = false;
}

// Tile epochs are 32-bit and only grow (two per step).  Before the counter can wrap, every live map
// is re-tagged with a small epoch and every other tag is zeroed, so a stale tile can never collide
// with a future epoch.  (2^32 epochs = ~3 days at 7.7 kHz.)
int renumber_epochs(gvom_handle *h)
{
    HIPCHK(h, sync_streams(h));
    h->spec_valid = false;                                 // (its fused tiles carry an epoch of the old numbering)
    uint32_t next = 0;
    for (size_t k = 0; k < h->slots.size(); ++k) {
        Slot &sl = h->slots[k];
        // the staging slot's tiles are dead -- unless a scan is in flight in it (a combine thread can get here while
        // the scan's thread waits for k_trace with the handle mutex released, or between the two halves of a sharded
        // scan): its kernels have completed (sync above), its tiles keep a live epoch and the commit finds it intact
        const bool inflight = (int)k == h->staging && (h->scan_inflight || h->pending);
        const uint32_t fresh = (sl.filled || inflight) ? ++next : 0u;
        HIPCHK(h, gvom_launch_retag(h->stream, sl.tags, h->ntiles, sl.epoch, fresh));
        sl.epoch = fresh;
        if (inflight) h->pending_P.epoch = fresh;         // gvom_shard_scan_merge's kernels stamp / test this epoch
    }
    for (int k = 0; k < 2; ++k) {
        Fused &f = h->fused[k];
        const uint32_t fresh = f.valid ? ++next : 0u;
        HIPCHK(h, gvom_launch_retag(h->stream, f.tags, h->ntiles, f.epoch, fresh));
        f.epoch = fresh;
    }
    h->epoch = next;
    HIPCHK(h, sync_streams(h));
    return GVOM_OK;
}

// host waits for everything the handle has enqueued (both streams)
hipError_t sync_streams(gvom_handle *h)
{
    if (h->mapped_unjoined || h->fuse_b_unjoined) {
        hipError_t e = hipStreamSynchronize(h->stream_b);
        if (e != hipSuccess) return e;
        h->mapped_unjoined = false;
        h->fuse_b_unjoined = false;
    }
    if (h->s_pending || h->fs_pending) {
        hipError_t e = hipStreamSynchronize(h->stream_s);
        if (e != hipSuccess) return e;
        h->s_pending = h->fs_pending = false;
        h->before_valid[0] = h->before_valid[1] = false;
    }
    return hipStreamSynchronize(h->stream);
}
// main stream waits (on the device) for a fusion still running on the second stream: before it overwrites a
// ring slot that fusion reads, or reads the fused map it writes
hipError_t join_fuse_stream(gvom_handle *h)
{
    if (!h->fuse_b_unjoined) return hipSuccess;
    h->fuse_b_unjoined = false;
    return hipStreamWaitEvent(h->stream, h->ev_fuse_b, 0);
}
// main stream waits (on the device) for a k_map2d still running on the second stream: it reads what
// the next fusion writes (fused double buffer, height maps, block counts)
hipError_t join_map_stream(gvom_handle *h)
{
    if (!h->mapped_unjoined) return hipSuccess;
    h->mapped_unjoined = false;
    h->fuse_b_unjoined = false;                            // (k_map2d runs behind that fusion on the same stream)
    return hipStreamWaitEvent(h->stream, h->ev_mapped, 0);
}

// the read hooks launch on the main stream and read what an asynchronous combine's kernels write on the second
hipError_t join_second_stream(gvom_handle *h)
{
    hipError_t e = join_map_stream(h);
    if (e == hipSuccess) e = join_fuse_stream(h);
    if (e == hipSuccess && h->s_pending) e = hipStreamWaitEvent(h->stream, h->ev_sdone, 0);   // the statistics stream's work
    return e;
}

// Waits until the GPU has published sequence number `seq` in the 64-bit host-mapped word `flag` (high
// half, or the whole word).  `lk` (the handle mutex) is RELEASED while waiting, so combine_maps from
// another thread is not locked out for the length of a trace.  A wait that took long the last time (c5:
// milliseconds) first SLEEPS most of that time away (all but a fifth, at least 250 us) and spins over the rest: the core is free meanwhile
// and the wake-up still comes within microseconds (a sleep has a granularity of ~60 us; spinning with short
// sleeps in between overshot a 250 us wait by 30 us).  `last_ns`: this wait's duration the previous time.
bool wait_published(gvom_handle *h, std::unique_lock<std::mutex> &lk, volatile unsigned long long *flag, uint32_t seq,
                    bool high_half, double *last_ns)
{
    auto done = [&]() { return (uint32_t)(high_half ? (*flag >> 32) : *flag) == seq; };
    lk.unlock();
    const double start = now_ns();
    bool slept = false;
    if (last_ns && *last_ns > 6.0e5 && !done()) {
        // all but the last fifth, at least 250 us (a sleep may run 100 us over and more)
        const double margin = *last_ns * 0.2 > 2.5e5 ? *last_ns * 0.2 : 2.5e5;
        usleep((useconds_t)((*last_ns - margin) * 1e-3));
        slept = true;
    }
    // the estimate follows only what has been OBSERVED: completion seen while spinning gives the true duration;
    // a flag already set after the sleep means the sleep was too long -- halve it (an outlier, e.g. a first
    // call that allocated, cannot keep every later wait long); never more than 20 ms
    const bool overslept = slept && done();
    unsigned spins = 0;
    bool ok = true;
    while (!done()) {
        _mm_pause();
        if ((++spins & 0x3ff) == 0) {
            const double waited = now_ns() - start;
            if (waited > 2.0e9) { ok = false; break; }                // device trouble: the caller falls back
            if (waited > 2.0e7) usleep(50);                           // far beyond anything expected: stop burning the core
        }
    }
    if (last_ns) {
        const double est = overslept ? *last_ns * 0.5 : now_ns() - start;
        *last_ns = est < 2.0e7 ? est : 2.0e7;
    }
    lk.lock();
    return ok;
}

// stage times of every profiling event pair recorded since the last collection (stream is idle)
void collect_stage_ms(gvom_handle *h)
{
    if (h->ev_scan) {
        hipEventElapsedTime(&h->stage_ms[0], h->ev[0], h->ev[1]);
        hipEventElapsedTime(&h->stage_ms[1], h->ev[1], h->ev[2]);
        h->stage_ms[2] = 0.0f;             // min-height runs inside the k_encode launch
    }
    if (h->ev_fuse) hipEventElapsedTime(&h->stage_ms[3], h->ev[4], h->ev[5]);
    // (the combine's completion flag goes out before k_map2d's launch has formally ended: wait for its event)
    if (h->ev_map && hipEventSynchronize(h->ev[7]) == hipSuccess) hipEventElapsedTime(&h->stage_ms[4], h->ev[6], h->ev[7]);
    h->ev_scan = h->ev_fuse = h->ev_map = false;
    (void)hipGetLastError();               // never leave a sticky error behind for the launchers
}
}  // namespace gvom_host

extern "C" {
VIS int gvom_create(const gvom_params *params, int device_id, gvom_t **out)
{
    return create_impl(params, device_id, 0, 1, false, out);
}

VIS int gvom_create_sharded(const gvom_params *params, int device_id, int rank, int world, gvom_t **out)
{
    return create_impl(params, device_id, rank, world, true, out);
}

VIS void gvom_destroy(gvom_t *h)
{
    if (!h) return;
    hipSetDevice(h->device);
    if (h->stream_b) hipStreamSynchronize(h->stream_b);
    if (h->stream) hipStreamSynchronize(h->stream);
    auto fb = [](Buf &b) { if (b.p) hipFree(b.p); b.p = nullptr; b.bytes = 0; };
    hipFree(h->hit); hipFree(h->total); hipFree(h->mh);
    // Regions another process has had mapped (the peer transport exported them: "exported" is set through gvom_set_tuning) go
    // to the process-wide pool (see pool_put), the others back to the allocator
    auto park = [&](void *ptr, size_t bytes, uint64_t gen) {
        if (!ptr) return;
        if (h->exported || h->holds_pooled) pool_put(ptr, bytes, gen); else hipFree(ptr);
    };
    for (Buf &r : h->retired) park(r.p, r.bytes, r.gen);
    if (h->sharded) {
        park(h->x_send_ids, exportable_size(h->x_Q * 4), h->fixed_gen[0]); park(h->x_send_pay, exportable_size(h->x_Q * 1024), h->fixed_gen[1]);
        park(h->x_send_eps.p, h->x_send_eps.bytes, h->x_send_eps.gen); park(h->x_send_sp.p, h->x_send_sp.bytes, h->x_send_sp.gen);
        park(h->hmaps, exportable_size(h->cells2d * 24), h->fixed_gen[2]); h->hmaps = nullptr;
    }
    h->x_send_eps.p = nullptr; h->x_send_sp.p = nullptr;
    hipFree(h->x_recv_ids); hipFree(h->x_recv_pay);
    hipFree(h->x_qcnt); hipFree(h->x_ecnt); hipFree(h->x_spcnt); fb(h->x_recv_eps); fb(h->x_recv_sp);
    if (h->x_host) hipHostFree(h->x_host);
    for (auto &s : h->slots) { hipFree(s.state); hipFree(s.code16); hipFree(s.tags); fb(s.crows); fb(s.metrics); fb(s.base); fb(s.rowvox); }
    for (auto &f : h->fused) { hipFree(f.state); hipFree(f.tags); fb(f.rows); fb(f.metrics); }
    // (the scan path's grow-only buffers and everything the calls keep -- the records of gvom_host.h -- own their memory: `delete h` below)
    hipFree(h->counters); if (h->counters_host) hipHostFree(h->counters_host);
    hipFree(h->descs_dev); if (h->descs_host) hipHostFree(h->descs_host);
    hipFree(h->blockcounts); hipFree(h->blockcounts2); hipFree(h->hmaps2);
    hipFree(h->hmaps); hipFree(h->slope_x); hipFree(h->slope_y);
    hipFree(h->rough); hipFree(h->guessed);
    if (h->out_host) hipHostFree(h->out_host);
    h->out_rec.clear(); hipFree(h->out_rec_bits);
    {   // device map sets: exported ones outlive the handle and go at their last release
        std::vector<DevSet *> idle;
        {
            std::lock_guard<std::mutex> g(g_set_mu);
            for (std::vector<DevSet *> *v : {&h->dsets, &h->psets})
                for (DevSet *s : *v) { if (s->exports > 0) s->orphan = true; else idle.push_back(s); }
        }
        for (DevSet *s : idle) set_free(s);
        h->dsets.clear(); h->psets.clear();
        if (h->ev_dcount) hipEventDestroy(h->ev_dcount);
    }
    for (auto &e : h->ev) if (e) hipEventDestroy(e);
    if (h->ev_fused) hipEventDestroy(h->ev_fused);
    if (h->ev_mapped) hipEventDestroy(h->ev_mapped);
    if (h->ev_done) hipEventDestroy(h->ev_done);
    if (h->ev_fuse_b) hipEventDestroy(h->ev_fuse_b);
    if (h->ev_up) hipEventDestroy(h->ev_up);
    if (h->stream_up) { hipStreamSynchronize(h->stream_up); hipStreamDestroy(h->stream_up); }
    if (h->stream_s) { hipStreamSynchronize(h->stream_s); hipStreamDestroy(h->stream_s); }
    for (hipEvent_t e : {h->ev_enc_s, h->ev_fz_s, h->ev_sdone, h->ev_fsdone, h->ev_before[0], h->ev_before[1]}) if (e) hipEventDestroy(e);
    if (h->stream_b) hipStreamDestroy(h->stream_b);
    if (h->own_stream) hipStreamDestroy(h->own_stream);
    delete h;
}

// ---- plumbing for the sharded layer: the library's own device buffers take part in the collectives
// directly (a rank's rows are one contiguous block of each buffer), on the library's stream, without
// host synchronisation in between.
VIS int gvom_sync(gvom_t *h)
{
    if (!h) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, sync_streams(h));
    collect_stage_ms(h);
    return GVOM_OK;
}

VIS int gvom_last_stage_ms(gvom_t *h, float ms[GVOM_N_STAGES])
{
    if (!h || !ms) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->ev_scan || h->ev_fuse || h->ev_map) {
        HIPCHK(h, hipSetDevice(h->device));
        HIPCHK(h, sync_streams(h));
        collect_stage_ms(h);
    }
    for (int k = 0; k < GVOM_N_STAGES; ++k) ms[k] = h->stage_ms[k];
    return GVOM_OK;
}

// host-side phase times in microseconds per call, averaged since creation (GVOM_HOST_TIMING=1):
// [0] scan launches [1] scan wait [2] combine launches [3] combine wait [4] output copies
VIS int gvom_host_timing(gvom_t *h, double us[8])
{
    if (!h || !us) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    for (int k = 0; k < 8; ++k) us[k] = h->host_calls ? h->host_ns[k] / h->host_calls / 1e3 : 0.0;
    return GVOM_OK;
}

// the clamps of gvom_set_tuning's product knobs: rounds per look at the counters ("<call>_batch"; 0: the default), sweeps a tile makes at
// most per round ("<call>_inner"; 0: the default), and megabytes a call may use (< 0: its default)
static int clamp_rounds(int v) { return v < 0 ? 0 : std::min(v, GVOM_CTG_MAX_BATCH); }
static int clamp_sweeps(int v) { return v < 0 ? 0 : v; }
static int clamp_mb(int v, int dflt, int cap) { return v < 0 ? dflt : std::min(v, cap); }
// name == call + suffix
static bool names(const char *name, const char *call, const char *suffix)
{
    const size_t n = strlen(call);
    return !strncmp(name, call, n) && !strcmp(name + n, suffix);
}
// the calls that wait, by the word their tuning names begin with: "<call>_inner" / "<call>_batch" are set and read for the window's
// three (the atlas forms run under those), "<call>_tiles" is read for all, "<call>_rounds" for those marked
struct SolverNames { const char *call; SolveWork *w; bool tuned, rounds; };
static const int N_SOLVERS = 5;
static void solver_names(gvom_handle *h, SolverNames s[N_SOLVERS])
{
    s[0] = {"cost_to_go", &h->cost_to_go.solve, true, false};      // (inner 0: 256, batch 0: 8)
    s[1] = {"frontier", &h->frontiers.solve, true, true};          // (inner 0: 256, batch 0: 8)
    s[2] = {"pose_field", &h->pose_field.solve, true, true};       // (inner 0: 64, batch 0: 8)
    s[3] = {"atlas_field", &h->atlas_field.solve, false, false};
    s[4] = {"atlas_frontier", &h->atlas_frontiers.solve, false, true};
}

// Performance knobs that never change a result: "segs" = step segments per ray in k_trace, "period" =
// committing steps between two flushes of a wave's line cache, "ep_row" = dispatch row of the endpoint
// blocks, "prio" = steps of remaining walk per issue-priority level of a trace wave (0 / 0 / -2 / -1: automatic).
VIS int gvom_set_tuning(gvom_t *h, const char *name, int value)
{
    if (!h || !name) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    SolverNames solvers[N_SOLVERS];
    solver_names(h, solvers);
    for (const SolverNames &s : solvers) {
        if (s.tuned && names(name, s.call, "_inner")) { s.w->tune_inner = clamp_sweeps(value); return GVOM_OK; }
        if (s.tuned && names(name, s.call, "_batch")) { s.w->tune_batch = clamp_rounds(value); return GVOM_OK; }
    }
    if (!strcmp(name, "segs")) h->tune_segs = value;
    else if (!strcmp(name, "ep_row")) h->tune_ep_row = value;
    else if (!strcmp(name, "period")) h->tune_period = value;
    else if (!strcmp(name, "prio")) h->tune_prio = value;
    else if (!strcmp(name, "interleave")) h->tune_ilv = value;
    else if (!strcmp(name, "flag_kernel")) h->tune_flag_kernel = value;
    else if (!strcmp(name, "fuse1")) h->tune_fuse1 = value;
    else if (!strcmp(name, "encfuse")) h->tune_encfuse = value;
    else if (!strcmp(name, "dirsort")) h->tune_dirsort = value;
    else if (!strcmp(name, "fastdiv")) h->tune_fastdiv = value;
    else if (!strcmp(name, "eager")) { h->tune_eager = value; h->eager_waste = 0; }
    else if (!strcmp(name, "delta_out")) { if (value >= 0) h->tune_delta_out = value != 0; if (value <= 0) h->out_rec.clear(); }   // (-1: drop every record, keep the setting)   // 0: every run of the returned maps is stored, no record kept
    else if (!strcmp(name, "viewpoint_bitmap_mb")) h->viewpoints.mb = clamp_mb(value, GVOM_VIEWPOINT_DEFAULT_MB, GVOM_VIEWPOINT_MAX_MB);   // megabytes of bitmaps per launch (0: one viewpoint per launch; < 0: the default, 256)
    else if (!strcmp(name, "voxel_distance_mb")) h->voxel_atlas.mb = clamp_mb(value, GVOM_VDIST_DEFAULT_MB, GVOM_VDIST_MAX_MB);   // megabytes of halo-grown intermediates a distance field may use (< 0: the default, 256)
    else if (!strcmp(name, "occupancy_clear")) h->tune_occ_clear = value;   // k_occupancy: 1 = clear the grid first, write live tile columns only
    else if (!strcmp(name, "exported")) h->exported = value != 0;       // (set by the peer transport, gvom_comm.hip)
#ifdef GVOM_HOOKS
    // test hooks (include/gvom_hip_test.h; lib/libgvom_hip_test.so only)
    else if (!strcmp(name, "churn")) h->tune_churn = value;             // a fresh endpoint send region every scan
    else if (!strcmp(name, "epoch_bias")) h->epoch += (uint32_t)value;   // advances the tile-epoch counter (towards its wrap)
#endif
    else return GVOM_ERR_INVALID;
    return GVOM_OK;
}

VIS int gvom_get_tuning(gvom_t *h, const char *name, int *value)
{
    if (!h || !name || !value) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    static const char *const knobs[5] = {"segs", "period", "ep_row", "prio", "interleave"};
    for (int k = 0; k < 5; ++k)
        if (!strcmp(name, knobs[k])) { *value = h->last_knobs[k]; return GVOM_OK; }     // (the last scan's, not the settings)
    // read-only, "<call>_allocations": the device allocations the call's entry points have made on this handle (its record's count)
    const struct { const char *call; const CallState &c; } calls[] = {
        {"clearance", h->clearance}, {"raycast", h->raycast}, {"cost_to_go", h->cost_to_go}, {"rollout", h->rollouts}, {"attitude", h->attitude},
        {"body", h->body}, {"alignment", h->alignment}, {"frontier", h->frontiers}, {"viewpoint", h->viewpoints}, {"pose_field", h->pose_field},
        {"atlas", h->atlas}, {"atlas_field", h->atlas_field}, {"atlas_frontier", h->atlas_frontiers}, {"voxel_atlas", h->voxel_atlas},
        {"attitude_volume", h->attitude_volume}, {"body_volume", h->body_volume}};
    for (const auto &c : calls)
        if (names(name, c.call, "_allocations")) { *value = c.c.allocs; return GVOM_OK; }
    // the calls that wait: read-only "<call>_tiles" / "<call>_rounds" = tile relaxations / rounds of the last call, and the two knobs
    SolverNames solvers[N_SOLVERS];
    solver_names(h, solvers);
    for (const SolverNames &s : solvers) {
        if (names(name, s.call, "_tiles")) { *value = s.w->last_tiles; return GVOM_OK; }
        if (s.rounds && names(name, s.call, "_rounds")) { *value = s.w->last_rounds; return GVOM_OK; }
        if (s.tuned && names(name, s.call, "_inner")) { *value = s.w->tune_inner; return GVOM_OK; }
        if (s.tuned && names(name, s.call, "_batch")) { *value = s.w->tune_batch; return GVOM_OK; }
    }
    if (!strcmp(name, "dirsort")) { *value = h->last_dirsort; return GVOM_OK; }
    if (!strcmp(name, "eager_adopted")) { *value = h->eager_stat[0]; return GVOM_OK; }
    if (!strcmp(name, "eager_dropped")) { *value = h->eager_stat[1]; return GVOM_OK; }
    if (!strcmp(name, "fuse_kernel")) { *value = h->last_fuse; return GVOM_OK; }                         // read-only, GVOM_ROUTE_*
    if (!strcmp(name, "encfuse_width")) { *value = h->last_encfuse[0]; return GVOM_OK; }                // read-only: sx per column block of the last k_encfuse (32 / 16; 0: none yet)
    if (!strcmp(name, "encfuse_waves")) { *value = h->last_encfuse[1]; return GVOM_OK; }                // read-only: its waves per column block
    if (!strcmp(name, "device_map_sets")) { *value = (int)h->dsets.size(); return GVOM_OK; }             // read-only: allocated device map sets
    static const char *const cl_names[4] = {"clearance_lgw", "clearance_rows_per_tile", "clearance_lds_bytes", "clearance_chunks"};
    for (int k = 0; k < 4; ++k)                                                                          // read-only: the launch shape of the last gvom_clearance
        if (!strcmp(name, cl_names[k])) { *value = h->clearance.shape[k]; return GVOM_OK; }
    if (!strcmp(name, "raycast")) { *value = 1; return GVOM_OK; }                                       // read-only: the library has gvom_raycast
    if (!strcmp(name, "cost_to_go")) { *value = 1; return GVOM_OK; }                                    // read-only: the library has gvom_cost_to_go
    if (!strcmp(name, "rollouts")) { *value = 1; return GVOM_OK; }                                      // read-only: the library has gvom_score_rollouts
    if (!strcmp(name, "footprint")) { *value = h->footprint.H > 0 ? 1 : 0; return GVOM_OK; }            // read-only: a footprint table is set
    if (!strcmp(name, "alignments")) { *value = 1; return GVOM_OK; }                                    // read-only: the library has gvom_score_alignments
    if (!strcmp(name, "attitude")) { *value = 1; return GVOM_OK; }                                      // read-only: the library has gvom_score_attitude
    if (!strcmp(name, "chassis")) { *value = h->chassis.H > 0 ? 1 : 0; return GVOM_OK; }                // read-only: a chassis is set
    if (!strcmp(name, "body")) { *value = 1; return GVOM_OK; }                                          // read-only: the library has gvom_body_set and gvom_score_body
    if (!strcmp(name, "body_spheres")) { *value = h->body.S; return GVOM_OK; }                          // read-only: the spheres of the body table (0: none set)
    if (!strcmp(name, "frontiers")) { *value = 1; return GVOM_OK; }                                     // read-only: the library has gvom_frontiers
    if (!strcmp(name, "viewpoints")) { *value = 1; return GVOM_OK; }                                    // read-only: the library has gvom_score_viewpoints
    if (!strcmp(name, "viewpoint_batch")) { *value = h->viewpoints.last_batch; return GVOM_OK; }        // read-only: viewpoints per launch of the last gvom_score_viewpoints
    if (!strcmp(name, "viewpoint_bitmap_mb")) { *value = h->viewpoints.mb; return GVOM_OK; }
    if (!strcmp(name, "pose_field")) { *value = 1; return GVOM_OK; }                                    // read-only: the library has gvom_pose_field
    if (!strcmp(name, "primitives")) { *value = h->pose_field.H > 0 ? 1 : 0; return GVOM_OK; }          // read-only: a primitive table is set
    if (!strcmp(name, "atlas")) { *value = h->atlas.A; return GVOM_OK; }                                 // read-only: the side of the configured atlas in cells, 0 without one
    if (!strcmp(name, "atlas_cost_to_go")) { *value = 1; return GVOM_OK; }                              // read-only: the library has gvom_atlas_cost_to_go and gvom_atlas_field_window
    if (!strcmp(name, "atlas_frontiers")) { *value = 1; return GVOM_OK; }                               // read-only: the library has gvom_atlas_frontiers
    if (!strcmp(name, "attitude_volume")) { *value = 1; return GVOM_OK; }                               // read-only: the library has gvom_attitude_volume and gvom_pose_field_attitude
    if (!strcmp(name, "body_volume")) { *value = 1; return GVOM_OK; }                                   // read-only: the library has gvom_body_volume and gvom_pose_field_volumes
    if (!strcmp(name, "voxel_atlas")) { *value = h->voxel_atlas.A; return GVOM_OK; }                     // read-only: the side A of the configured voxel atlas, 0 without one
    if (!strcmp(name, "voxel_atlas_alignments")) { *value = 1; return GVOM_OK; }                         // read-only: the library has gvom_voxel_atlas_score_alignments
    if (!strcmp(name, "voxel_atlas_levels")) { *value = h->voxel_atlas.A ? h->voxel_atlas.Z : 0; return GVOM_OK; }   // read-only: its levels Z
    if (!strcmp(name, "voxel_atlas_viewpoint_batch")) { *value = h->voxel_atlas.last_batch; return GVOM_OK; }   // read-only: poses per launch of the last gvom_voxel_atlas_score_viewpoints
    if (!strcmp(name, "voxel_changes")) { *value = 1; return GVOM_OK; }                                  // read-only: the library has gvom_voxel_atlas_changes
    if (!strcmp(name, "voxel_distance_field")) { *value = 1; return GVOM_OK; }                          // read-only: the library has gvom_voxel_atlas_distance_field and gvom_voxel_distance_sample
    if (!strcmp(name, "voxel_distance_mb")) { *value = h->voxel_atlas.mb; return GVOM_OK; }
    if (!strcmp(name, "voxel_distance_halo_xy")) { *value = h->voxel_atlas.halo[0]; return GVOM_OK; }    // read-only: Hxy of the last gvom_voxel_atlas_distance_field
    if (!strcmp(name, "voxel_distance_halo_z")) { *value = h->voxel_atlas.halo[1]; return GVOM_OK; }     // read-only: its Hz
    if (!strcmp(name, "alignment_grid_bytes")) { *value = (int)(h->alignment.grid.bytes > 0x7fffffffu ? 0x7fffffffu : h->alignment.grid.bytes); return GVOM_OK; }   // read-only: the class grid's allocation
    if (!strcmp(name, "alignment_points_per_block")) { *value = GVOM_ALIGN_PTS_BLOCK; return GVOM_OK; }  // read-only: returns per k_align_score workgroup
    if (!strcmp(name, "alignment_candidate_group")) { *value = GVOM_ALIGN_CAND_GROUP; return GVOM_OK; }  // read-only: candidates per k_align_score workgroup
    if (!strcmp(name, "device_product_sets")) { *value = (int)h->psets.size(); return GVOM_OK; }        // read-only: allocated device product sets (every kind)
    if (!strcmp(name, "occupancy_clear")) { *value = h->tune_occ_clear; return GVOM_OK; }
    if (!strcmp(name, "delta_out")) { *value = h->tune_delta_out; return GVOM_OK; }
    if (!strcmp(name, "output_records")) { *value = h->out_rec.size(); return GVOM_OK; }                // read-only: output buffers with a content record
    if (!strcmp(name, "multi_origin")) { *value = 1; return GVOM_OK; }                                  // read-only: the library has the multi-origin entry points
    if (!strcmp(name, "multi_origin_ran")) { *value = h->last_multi_origin; return GVOM_OK; }           // read-only: the last scan ran the per-lane-origin trace
    if (!strcmp(name, "range_image")) { *value = h->range_image.H > 0 ? 1 : 0; return GVOM_OK; }        // read-only: a sensor model is set
    if (!strcmp(name, "fastdiv")) { *value = h->tune_fastdiv == 0 ? 0 : h->fastdiv_ok; return GVOM_OK; }   // bit 0 / 1: xy / z resolution divided by reciprocal
    return GVOM_ERR_INVALID;
}

VIS int gvom_set_profiling(gvom_t *h, int on)
{
    if (!h) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    h->profiling = on != 0;
    return GVOM_OK;
}

VIS void *gvom_stream(gvom_t *h) { return h ? (void *)h->stream : nullptr; }
// A value that differs between any two handles of the process and changes whenever one of the handle's SEND regions
// (gvom_shard_buffer GVOM_XBUF_SEND_*; the only grow-only buffers another rank ever reads) has been re-allocated:
// whoever caches something derived from their addresses (the peer transport's exported allocations) knows when to
// look again.  (GVOM_BUF_HEIGHT_MAPS and the quad regions are allocated once, with the handle.)
VIS uint64_t gvom_alloc_generation(gvom_t *h) { return h ? h->alloc_gen : 0; }
// The same for ONE region (which = GVOM_XBUF_SEND_* or -1 for GVOM_BUF_HEIGHT_MAPS): a value that names the allocation the
// region lies in -- it changes exactly when that allocation is replaced (and differs between handles).
// The region `which` (GVOM_XBUF_SEND_IDS / _QUADS / _EPS / _RETURNS, or -1: GVOM_BUF_HEIGHT_MAPS) moves into a FRESH allocation of the
// same size, contents included; the old one is parked (a peer may have it mapped).  For the transport: an allocation the HSA
// runtime refuses to export, or that a peer cannot open, is replaced by one that has no history.
VIS int gvom_shard_renew_region(gvom_t *h, int which)
{
    if (!h || !h->sharded) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    void **pp = nullptr;
    size_t bytes = 0;
    uint64_t *gen = nullptr;
    switch (which) {
    case GVOM_XBUF_SEND_IDS: pp = (void **)&h->x_send_ids; bytes = exportable_size(h->x_Q * 4); gen = &h->fixed_gen[0]; break;
    case GVOM_XBUF_SEND_QUADS: pp = &h->x_send_pay; bytes = exportable_size(h->x_Q * 1024); gen = &h->fixed_gen[1]; break;
    case GVOM_XBUF_SEND_EPS: pp = &h->x_send_eps.p; bytes = h->x_send_eps.bytes; gen = &h->x_send_eps.gen; break;
    case GVOM_XBUF_SEND_RETURNS: pp = &h->x_send_sp.p; bytes = h->x_send_sp.bytes; gen = &h->x_send_sp.gen; break;
    case -1: pp = (void **)&h->hmaps; bytes = exportable_size(h->cells2d * 24); gen = &h->fixed_gen[2]; break;
    default: return GVOM_ERR_INVALID;
    }
    if (!*pp || !bytes) return GVOM_NO_DATA;
    void *np = nullptr;
    HIPCHK(h, hipMalloc(&np, bytes));                      // (fresh: never from the pool)
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(np, *pp, bytes, hipMemcpyDeviceToDevice));
    HIPCHK(h, hipDeviceSynchronize());
    Buf old; old.p = *pp; old.bytes = bytes; old.gen = *gen;
    h->retired.push_back(old);
    *pp = np;
    *gen = ++g_alloc_generation;
    if (which == -1) { h->height = h->hmaps; h->inferred = h->hmaps + h->prm.xy_size; }
    if (which == GVOM_XBUF_SEND_EPS || which == GVOM_XBUF_SEND_RETURNS) h->alloc_gen = *gen;
    return GVOM_OK;
}

VIS uint64_t gvom_region_generation(gvom_t *h, int which)
{
    if (!h) return 0;
    if (which == GVOM_XBUF_SEND_EPS) return h->x_send_eps.gen ? h->x_send_eps.gen : h->handle_gen;
    if (which == GVOM_XBUF_SEND_RETURNS) return h->x_send_sp.gen ? h->x_send_sp.gen : h->handle_gen;
    if (which == GVOM_XBUF_SEND_IDS && h->fixed_gen[0]) return h->fixed_gen[0];
    if (which == GVOM_XBUF_SEND_QUADS && h->fixed_gen[1]) return h->fixed_gen[1];
    if (which == -1 && h->fixed_gen[2]) return h->fixed_gen[2];
    return h->handle_gen;
}

VIS const char *gvom_last_error(gvom_t *h) { return h ? h->err.c_str() : "null handle"; }

VIS int gvom_backend_info(char *buf, size_t len)
{
    if (!buf || len == 0) return GVOM_ERR_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        snprintf(buf, len, "libgvom_hip abi %d (gfx950 code object); no HIP device visible", GVOM_ABI_VERSION);
        return GVOM_ERR_NO_DEVICE;
    }
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, 0) != hipSuccess) return GVOM_ERR_HIP;
    snprintf(buf, len, "libgvom_hip abi %d; device0=%s arch=%s CUs=%d; %d device(s)", GVOM_ABI_VERSION,
             pr.name, pr.gcnArchName, pr.multiProcessorCount, ndev);
    return GVOM_OK;
}

VIS int gvom_abi_version(void) { return GVOM_ABI_VERSION; }
}  // extern "C"
