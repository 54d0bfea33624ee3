// gvom_export.hip -- device-resident results: map sets and product sets (DevSet) with their exports, releases and DLPack capsules,
// gvom_combine_maps_device, the 3-D products, the clearance map, ray queries and cost-to-go fields.
#include "gvom_host.h"

namespace gvom_host {
std::mutex g_set_mu;

void set_free(DevSet *s)                                   // (no export left and unreachable: not under g_set_mu)
{
    int dev = 0;
    hipGetDevice(&dev);
    hipSetDevice(s->device);
    for (hipEvent_t e : s->rel) { hipEventSynchronize(e); hipEventDestroy(e); }   // consumers' reads are done before the memory goes
    for (hipEvent_t e : s->rel_spare) hipEventDestroy(e);
    if (s->ready) { hipEventSynchronize(s->ready); hipEventDestroy(s->ready); }
    if (s->mem) hipFree(s->mem);
    hipSetDevice(dev);
    (void)hipGetLastError();
    delete s;
}

void occ_params(const gvom_handle *h, const Fused &F, OccParams &P)
{
    memset(&P, 0, sizeof P);
    P.xy = h->prm.xy_size; P.zs = h->prm.z_size;
    window_phase(h, F.origin, P.om);
    P.y_lo = h->sy_lo; P.y_hi = h->sy_hi;
    P.nseg = h->nseg; P.epoch = F.epoch;
}

void cloud_params(const gvom_handle *h, const Fused &F, Map2dParams &P)
{
    const gvom_params &p = h->prm;
    memset(&P, 0, sizeof P);
    P.xy = p.xy_size; P.zs = p.z_size;
    window_phase(h, F.origin, P.om);
    P.y_lo = h->sy_lo; P.y_hi = h->sy_hi;
    P.xy_res = p.xy_resolution; P.z_res = p.z_resolution;
    P.nseg = h->nseg; P.epoch = F.epoch;
}

// the frame of the fused map F as k_raycast reads it (gvom_launch_raycast names the fields), and what of a query depends on it
void raycast_params(const gvom_handle *h, const Fused &F, ScanParams &P, RayQuery &Q)
{
    const gvom_params &p = h->prm;
    memset(&P, 0, sizeof P);
    P.xy_res = p.xy_resolution; P.z_res = p.z_resolution;
    P.drcp[0] = 1.0 / p.xy_resolution; P.drcp[1] = 1.0 / p.z_resolution;
    P.fastdiv = h->tune_fastdiv == 0 ? 0 : h->fastdiv_ok;
    P.xy = p.xy_size; P.zs = p.z_size;
    P.sy_lo = h->sy_lo; P.sy_hi = h->sy_hi;
    P.nseg = h->nseg; P.epoch = F.epoch;
    P.f32_sqrt = h->f32_sqrt ? 1 : 0;
    window_phase(h, F.origin, P.om);
    bool far = false;
    for (int k = 0; k < 3; ++k) {
        P.origin[k] = (double)F.origin[k];
        far = far || F.origin[k] <= -((int64_t)1 << 24) || F.origin[k] >= ((int64_t)1 << 24);
    }
    Q.lit = (far || p.z_size > p.xy_size) ? 1 : 0;        // (the integer window test assumes z_size <= xy_size and a near origin)
    Q.cap = (uint32_t)p.xy_size + (uint32_t)p.z_size;
}

hipError_t launch_height_cloud(gvom_handle *h, const Fused &F, float *out7, float *out3)
{
    const double org[3] = {(double)F.origin[0], (double)F.origin[1], (double)F.origin[2]};
    int om[3];
    window_phase(h, F.origin, om);
    return gvom_launch_debug_height(h->stream, h->prm.xy_size, om[0], om[1], org, h->prm.xy_resolution, h->prm.z_resolution,
                                    h->height, h->hs, h->rough, h->slope_x, h->slope_y, out7, h->guessed, out3);
}
}  // namespace gvom_host

// DLPack v0.8 (legacy) and v1.0 (versioned) layouts (as the DLPack specification defines them; no header of another project is included)
namespace {
struct DLDevice { int32_t device_type; int32_t device_id; };
struct DLDataType { uint8_t code; uint8_t bits; uint16_t lanes; };
struct DLTensor { void *data; DLDevice device; int32_t ndim; DLDataType dtype; int64_t *shape; int64_t *strides; uint64_t byte_offset; };
struct DLManagedTensor { DLTensor dl_tensor; void *manager_ctx; void (*deleter)(DLManagedTensor *); };
struct DLPackVersion { uint32_t major; uint32_t minor; };
struct DLManagedTensorVersioned { DLPackVersion version; void *manager_ctx; void (*deleter)(DLManagedTensorVersioned *); uint64_t flags; DLTensor dl_tensor; };
enum { kDLInt = 0, kDLUInt = 1, kDLFloat = 2, kDLROCM = 10 };
}  // namespace

extern "C" {
// ---- device-resident maps (gvom_combine_maps_device) -----------------------------------------
// The fusion advances exactly as in gvom_combine_maps; k_map2d's DEV form writes the nine maps into a DevSet in device memory
// and the call returns once the work is enqueued.  Consumers take a set through exports (their stream waits on the set's
// ready event) and give it back through releases (an event on their stream): no host wait on either side.

// one release: an event on the consumer's stream (none for GVOM_STREAM_NOSYNC), the export count goes down; an orphaned set
// goes with its last release.  Needs neither the handle nor the Python GIL.
static hipError_t set_release(DevSet *s, void *consumer_stream)
{
    hipError_t e = hipSuccess;
    bool free_it = false;
    {
        std::lock_guard<std::mutex> g(g_set_mu);
        if (consumer_stream != GVOM_STREAM_NOSYNC) {
            int dev = 0;
            hipGetDevice(&dev);
            if (dev != s->device) hipSetDevice(s->device);
            const hipStream_t st = (hipStream_t)consumer_stream;
            size_t k = 0;
            while (k < s->rel_streams.size() && s->rel_streams[k] != st) ++k;
            if (k == s->rel_streams.size()) {                // (a stream seen before: its newer event covers the older reads too)
                hipEvent_t ev = nullptr;
                if (!s->rel_spare.empty()) { ev = s->rel_spare.back(); s->rel_spare.pop_back(); }
                else e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
                if (e == hipSuccess) { s->rel_streams.push_back(st); s->rel.push_back(ev); }
            }
            if (e == hipSuccess) e = hipEventRecord(s->rel[k], st);
            if (dev != s->device) hipSetDevice(dev);
        }
        if (s->exports > 0) --s->exports;
        free_it = s->orphan && s->exports == 0;
    }
    if (free_it) set_free(s);
    return e;
}

static DevSet *find_set(const std::vector<DevSet *> &sets, int64_t set_id)
{
    if (set_id < 0) return nullptr;
    for (DevSet *s : sets) if (s->id == set_id) return s;
    return nullptr;
}

// ---- what a set holds: the only place that knows the layouts --------------------------------------------------------------
struct SetPart { void *ptr; int ndim; int64_t shape[3], strides[3]; uint8_t code, bits; size_t bytes; };
static size_t set_bytes(int kind, int xy, int zs, int64_t cap)
{
    const size_t n2 = (size_t)xy * xy;
    switch (kind) {
    case 0: return dev_map_stride(xy) * 60;
    case GVOM_PRODUCT_OCCUPANCY: return n2 * zs;
    case GVOM_PRODUCT_VOXEL_CLOUD: return 256 + align256((size_t)cap * 32) + align256((size_t)cap * 12);
    case GVOM_PRODUCT_HEIGHT_CLOUD: return n2 * 28;
    case GVOM_PRODUCT_INFERRED_HEIGHT_CLOUD: return n2 * 12;
    case GVOM_PRODUCT_CLEARANCE: return align256(n2 * 4) + n2 * 4;
    case GVOM_PRODUCT_RAYCAST: return align256((size_t)cap * 16) + (size_t)cap * 12;
    case GVOM_PRODUCT_COSTFIELD: return align256(n2 * 4) + align256(n2) + n2 * 2;
    }
    return 0;
}
static bool set_part(const DevSet *s, int part, SetPart *d)
{
    const int64_t xy = s->xy, n2 = xy * xy;
    memset(d, 0, sizeof *d);
    d->ndim = 2; d->code = kDLFloat; d->bits = 32;
    d->shape[2] = d->strides[2] = 1;
    auto rows = [&](void *ptr, int64_t n, int64_t cols) { d->ptr = ptr; d->shape[0] = n; d->shape[1] = cols; d->strides[0] = cols; d->strides[1] = 1; };
    switch (s->kind) {
    case 0: {                                              // map `part` of a map set: [x, y] indexing, column-major
        if (part < 0 || part > 8) return false;
        const size_t S = dev_map_stride(s->xy);
        d->ptr = part >= 3 ? (void *)((double *)s->mem + (size_t)(part - 3) * S) : (void *)((int32_t *)((double *)s->mem + 6 * S) + (size_t)part * S);
        d->shape[0] = d->shape[1] = xy; d->strides[0] = 1; d->strides[1] = xy;
        d->code = part >= 3 ? kDLFloat : kDLInt; d->bits = part >= 3 ? 64 : 32;
        break;
    }
    case GVOM_PRODUCT_OCCUPANCY:
        if (part != 0) return false;
        d->ptr = s->mem; d->ndim = 3; d->code = kDLUInt; d->bits = 8;
        d->shape[0] = d->shape[1] = xy; d->shape[2] = s->zs;
        d->strides[0] = xy * s->zs; d->strides[1] = s->zs; d->strides[2] = 1;
        break;
    case GVOM_PRODUCT_VOXEL_CLOUD:
        if (part == 0) rows(s->mem + 256, s->cap, 8);
        else if (part == 1) rows(s->mem + 256 + align256((size_t)s->cap * 32), s->cap, 3);
        else if (part == 2) { d->ptr = s->mem; d->ndim = 1; d->shape[0] = 1; d->strides[0] = 1; d->shape[1] = d->strides[1] = 1; d->code = kDLInt; d->bits = 64; }
        else return false;
        break;
    case GVOM_PRODUCT_HEIGHT_CLOUD: if (part != 0) return false; rows(s->mem, n2, 7); break;
    case GVOM_PRODUCT_INFERRED_HEIGHT_CLOUD: if (part != 0) return false; rows(s->mem, n2, 3); break;
    case GVOM_PRODUCT_CLEARANCE:                           // [x, y] indexing, column-major, like a device map
        if (part < 0 || part > 1) return false;
        d->ptr = s->mem + (part ? align256((size_t)n2 * 4) : 0);
        d->shape[0] = d->shape[1] = xy; d->strides[0] = 1; d->strides[1] = xy;
        if (part) d->code = kDLInt;
        break;
    case GVOM_PRODUCT_RAYCAST:
        if (part == 0) { rows(s->mem, s->cap, 4); d->code = kDLInt; }
        else if (part == 1) rows(s->mem + align256((size_t)s->cap * 16), s->cap, 3);
        else return false;
        break;
    case GVOM_PRODUCT_COSTFIELD:                           // [x, y] indexing, column-major, like a device map
        if (part < 0 || part > 2) return false;
        d->ptr = s->mem + (part ? align256((size_t)n2 * 4) : 0) + (part == 2 ? align256((size_t)n2) : 0);
        d->shape[0] = d->shape[1] = xy; d->strides[0] = 1; d->strides[1] = xy;
        d->code = part ? kDLUInt : kDLInt; d->bits = part == 0 ? 32 : (part == 1 ? 8 : 16);
        break;
    default: return false;
    }
    d->bytes = (size_t)(d->shape[0] * d->shape[1] * d->shape[2]) * (d->bits / 8);
    return true;
}

// ---- pool: a free set of the kind (and size), or a new one ------------------------------------------------------------------
// sets of `kind` nobody holds an export of go back to the pool (their ids are stale from here on); returns one that holds
// `bytes`, or nullptr.  Free sets of the kind that are too small are given up.
static DevSet *set_recycle(std::vector<DevSet *> &sets, int kind, size_t bytes)
{
    DevSet *set = nullptr;
    std::vector<DevSet *> small;
    {
        std::lock_guard<std::mutex> g(g_set_mu);
        for (size_t k = 0; k < sets.size();) {
            DevSet *s = sets[k];
            if (s->kind == kind && s->exports == 0) {
                s->id = -1;
                if (s->bytes < bytes) { small.push_back(s); sets.erase(sets.begin() + (long)k); continue; }
                if (!set) set = s;
            }
            ++k;
        }
    }
    for (DevSet *s : small) set_free(s);
    return set;
}
static int set_new(gvom_handle *h, std::vector<DevSet *> &sets, int kind, size_t bytes, DevSet **out)
{
    DevSet *s = new DevSet;
    s->device = h->device; s->xy = h->prm.xy_size; s->zs = h->prm.z_size; s->kind = kind;
    s->bytes = bytes;
    hipError_t e = hipMalloc((void **)&s->mem, s->bytes);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ready, hipEventDisableTiming);
    if (e != hipSuccess) { set_free(s); HIPCHK(h, e); }
    sets.push_back(s);
    *out = s;
    return GVOM_OK;
}
// a reused set: its consumers' reads come first (the handle's stream waits on every release event)
static int set_wait_releases(gvom_handle *h, DevSet *set)
{
    std::lock_guard<std::mutex> g(g_set_mu);
    for (hipEvent_t e : set->rel) HIPCHK(h, hipStreamWaitEvent(h->stream, e, 0));
    set->rel_spare.insert(set->rel_spare.end(), set->rel.begin(), set->rel.end());
    set->rel.clear(); set->rel_streams.clear();
    return GVOM_OK;
}

// ---- exports, releases, DLPack, host copies: the same for every kind (`maps`: which of the handle's two id spaces) -------------
static int set_export(gvom_handle *h, bool maps, int64_t set_id, int part, void *consumer_stream, DevSet **out_set, SetPart *d)
{
    DevSet *s = find_set(maps ? h->dsets : h->psets, set_id);
    if (maps && (part < 0 || part > 8)) { h->err = "map index outside 0..8"; return GVOM_ERR_INVALID; }
    if (!s) { h->err = maps ? "unknown or stale device map set id" : "unknown or stale device product id"; return GVOM_ERR_INVALID; }
    if (!set_part(s, part, d)) { h->err = "part index outside the parts of this device product"; return GVOM_ERR_INVALID; }
    HIPCHK(h, hipSetDevice(h->device));
    if (consumer_stream != GVOM_STREAM_NOSYNC) HIPCHK(h, hipStreamWaitEvent((hipStream_t)consumer_stream, s->ready, 0));
    {
        std::lock_guard<std::mutex> g(g_set_mu);
        ++s->exports;
    }
    *out_set = s;
    return GVOM_OK;
}

static int set_release_id(gvom_handle *h, bool maps, int64_t set_id, void *consumer_stream)
{
    DevSet *s = find_set(maps ? h->dsets : h->psets, set_id);
    if (!s) { h->err = maps ? "unknown or stale device map set id" : "unknown or stale device product id"; return GVOM_ERR_INVALID; }
    {
        std::lock_guard<std::mutex> g(g_set_mu);
        if (s->exports == 0) { h->err = maps ? "gvom_device_map_release: the set has no live export" : "gvom_device_product_release: the product has no live export"; return GVOM_ERR_INVALID; }
    }
    HIPCHK(h, set_release(s, consumer_stream));
    return GVOM_OK;
}

// the manager context of one DLPack export: the set, the consumer stream its release is recorded on, shape and strides
struct DlpackCtx {
    DevSet *set;
    void *stream;
    int64_t shape[3], strides[3];
    DLManagedTensor legacy;
    DLManagedTensorVersioned versioned;
};
static void dlpack_delete_legacy(DLManagedTensor *m)
{
    DlpackCtx *c = (DlpackCtx *)m->manager_ctx;
    set_release(c->set, c->stream);
    delete c;
}
static void dlpack_delete_versioned(DLManagedTensorVersioned *m)
{
    DlpackCtx *c = (DlpackCtx *)m->manager_ctx;
    set_release(c->set, c->stream);
    delete c;
}

static int set_dlpack(gvom_handle *h, bool maps, int64_t set_id, int part, void *consumer_stream, int versioned, void **managed)
{
    DevSet *s = nullptr;
    SetPart d;
    const int rc = set_export(h, maps, set_id, part, consumer_stream, &s, &d);
    if (rc) return rc;
    DlpackCtx *c = new DlpackCtx();
    c->set = s; c->stream = consumer_stream;
    for (int k = 0; k < 3; ++k) { c->shape[k] = d.shape[k]; c->strides[k] = d.strides[k]; }
    DLTensor t;
    t.data = d.ptr;
    t.device.device_type = kDLROCM; t.device.device_id = h->device;
    t.ndim = d.ndim;
    t.dtype.code = d.code; t.dtype.bits = d.bits; t.dtype.lanes = 1;
    t.shape = c->shape; t.strides = c->strides;
    t.byte_offset = 0;
    if (versioned) {
        c->versioned.version.major = 1; c->versioned.version.minor = 0;
        c->versioned.manager_ctx = c;
        c->versioned.deleter = dlpack_delete_versioned;
        c->versioned.flags = 0;
        c->versioned.dl_tensor = t;
        *managed = &c->versioned;
    } else {
        c->legacy.dl_tensor = t;
        c->legacy.manager_ctx = c;
        c->legacy.deleter = dlpack_delete_legacy;
        *managed = &c->legacy;
    }
    return GVOM_OK;
}

static int set_copy(gvom_handle *h, bool maps, int64_t set_id, int part, void *host_out)
{
    DevSet *s = nullptr;
    SetPart d;
    int rc = set_export(h, maps, set_id, part, GVOM_STREAM_NOSYNC, &s, &d);
    if (rc) return rc;
    hipError_t e = hipEventSynchronize(s->ready);
    const size_t bytes = maps ? h->cells2d * (d.bits / 8) : d.bytes;      // (a map: xy*xy elements, without the set's padding)
    if (e == hipSuccess && bytes) e = hipMemcpy(host_out, d.ptr, bytes, hipMemcpyDeviceToHost);
    set_release(s, GVOM_STREAM_NOSYNC);
    HIPCHK(h, e);
    return GVOM_OK;
}

VIS int gvom_combine_maps_device(gvom_t *h, double origin_world[3], int64_t *set_id)
{
    if (!h || !set_id) return GVOM_ERR_INVALID;
    if (h->sharded) { h->err = "gvom_combine_maps_device: sharded handles are not supported"; return GVOM_ERR_INVALID; }
    std::lock_guard<std::mutex> ck(h->combine_mu);
    std::unique_lock<std::mutex> lk(h->mu);
    if (h->pending_combine) { h->err = "a combine begun with gvom_combine_begin has not been ended"; return GVOM_ERR_INVALID; }
    HIPCHK(h, hipSetDevice(h->device));
    double t0 = now_ns();
    *set_id = -1;
    // unused sets go back to the pool; then a free one, or a new one (at most GVOM_MAX_DEVICE_SETS)
    DevSet *set = set_recycle(h->dsets, 0, 0);
    if (!set && !h->slots[h->ring[h->last_buffer_index]].filled) return GVOM_EMPTY_BUFFER;
    if (!set) {
        if ((int)h->dsets.size() >= GVOM_MAX_DEVICE_SETS) {
            h->err = "gvom_combine_maps_device: all 8 device map sets are exported; release some (gvom_device_map_release, or drop the tensors)";
            return GVOM_ERR_CAPACITY;
        }
        const int rc0 = set_new(h, h->dsets, 0, set_bytes(0, h->prm.xy_size, 0, 0), &set);
        if (rc0) return rc0;
    }
    if (!h->ev_dcount) HIPCHK(h, hipEventCreateWithFlags(&h->ev_dcount, hipEventDisableTiming));
    int rc = fuse_impl(h);
    if (rc) return rc;
    if ((rc = set_wait_releases(h, set))) return rc;
    if ((rc = map2d_impl(h, false, true, set->mem, true, nullptr, nullptr, 0, true))) return rc;
    HIPCHK(h, hipEventRecord(set->ready, h->stream));
    HIPCHK(h, hipEventRecord(h->ev_dcount, h->stream));
    h->count_pending = true;
    set->id = ++h->dset_seq;
    *set_id = set->id;
    HT(h, 2, t0);
    world_origin(h, h->fused[h->cur], origin_world);
    return GVOM_OK;
}

VIS int gvom_device_map_export(gvom_t *h, int64_t set_id, int which, void *consumer_stream, void **ptr, int64_t strides[2])
{
    if (!h || !ptr || !strides) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    DevSet *s = nullptr;
    SetPart d;
    const int rc = set_export(h, true, set_id, which, consumer_stream, &s, &d);
    if (rc) return rc;
    *ptr = d.ptr;
    strides[0] = d.strides[0]; strides[1] = d.strides[1];
    return GVOM_OK;
}

VIS int gvom_device_map_release(gvom_t *h, int64_t set_id, void *consumer_stream)
{
    if (!h) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    return set_release_id(h, true, set_id, consumer_stream);
}

VIS int gvom_device_map_dlpack(gvom_t *h, int64_t set_id, int which, void *consumer_stream, int versioned, void **managed)
{
    if (!h || !managed) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    return set_dlpack(h, true, set_id, which, consumer_stream, versioned, managed);
}

VIS int gvom_device_map_copy(gvom_t *h, int64_t set_id, int which, void *host_out)
{
    if (!h || !host_out) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    return set_copy(h, true, set_id, which, host_out);
}

// ---- device-resident 3-D products (gvom_device_product) ----------------------------------------------------------------------
// A snapshot of the current fused map (occupancy grid, voxel cloud) or of the last combine's 2-D maps (the two height clouds),
// written into a product set on the handle's stream behind whatever produced its inputs; the call enqueues and returns.  Later
// scans and combines never touch a product: it is a copy, reused only once nobody holds an export of it and behind its
// consumers' release events.

VIS int gvom_device_product(gvom_t *h, int kind, int64_t max_rows, int64_t *product_id)
{
    if (!h || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *product_id = -1;
    if (kind == GVOM_PRODUCT_CLEARANCE) { h->err = "gvom_device_product: a clearance product is made by gvom_clearance"; return GVOM_ERR_INVALID; }
    if (kind == GVOM_PRODUCT_RAYCAST) { h->err = "gvom_device_product: a raycast product is made by gvom_raycast"; return GVOM_ERR_INVALID; }
    if (kind == GVOM_PRODUCT_COSTFIELD) { h->err = "gvom_device_product: a cost field is made by gvom_cost_to_go"; return GVOM_ERR_INVALID; }
    if (kind < 1 || kind > GVOM_N_PRODUCT_KINDS) { h->err = "gvom_device_product: unknown product kind"; return GVOM_ERR_INVALID; }
    if (h->sharded) { h->err = "gvom_device_product: sharded handles are not supported"; return GVOM_ERR_INVALID; }
    if (kind == GVOM_PRODUCT_VOXEL_CLOUD) stats_demand(h);                  // a read of the statistics, like gvom_debug_voxel_map
    if (!h->has_combined) return GVOM_NO_DATA;
    if ((kind == GVOM_PRODUCT_HEIGHT_CLOUD || kind == GVOM_PRODUCT_INFERRED_HEIGHT_CLOUD) && !h->maps_valid) return GVOM_NO_DATA;
    if (kind == GVOM_PRODUCT_VOXEL_CLOUD && !h->fused[h->cur].has_metrics) return GVOM_NO_DATA;
    HIPCHK(h, hipSetDevice(h->device));
    int64_t cap = 0;
    if (kind == GVOM_PRODUCT_VOXEL_CLOUD) {
        cap = max_rows;
        if (cap <= 0) {                                                      // the fused cell count (settles a device combine's pending count)
            const int rc0 = settle_count(h);
            if (rc0) return rc0;
            cap = h->combined_cell_count;
        }
        if (cap < 1) cap = 1;
    }
    const int xy = h->prm.xy_size, zs = h->prm.z_size;
    DevSet *set = set_recycle(h->psets, kind, set_bytes(kind, xy, zs, cap));
    if (!set) {
        int n = 0;
        for (DevSet *s : h->psets) n += s->kind == kind;
        if (n >= GVOM_MAX_PRODUCT_SETS) {
            h->err = "gvom_device_product: all 4 device product sets of this kind are exported; release some (gvom_device_product_release, or drop the tensors)";
            return GVOM_ERR_CAPACITY;
        }
        const int rc0 = set_new(h, h->psets, kind, set_bytes(kind, xy, zs, cap + cap / 2), &set);   // (a cloud grows with the map: headroom)
        if (rc0) return rc0;
    }
    set->cap = cap;
    const Fused &F = h->fused[h->cur];
    HIPCHK(h, join_second_stream(h));
    int rc = set_wait_releases(h, set);
    if (rc) return rc;
    SetPart d;
    switch (kind) {
    case GVOM_PRODUCT_OCCUPANCY: {
        OccParams P;
        occ_params(h, F, P);
        HIPCHK(h, gvom_launch_occupancy(h->stream, P, F.state, F.tags, (uint8_t *)set->mem, h->tune_occ_clear != 0));
        break;
    }
    case GVOM_PRODUCT_VOXEL_CLOUD: {
        Map2dParams P;
        cloud_params(h, F, P);
        SetPart e;
        set_part(set, 0, &d); set_part(set, 1, &e);
        HIPCHK(h, hipMemsetAsync(set->mem, 0, 8, h->stream));
        HIPCHK(h, gvom_launch_voxel_cloud(h->stream, P, (double)F.origin[0], (double)F.origin[1], (double)F.origin[2], F.state, F.tags,
                                          (const uint4 *)F.rows.p, (const float *)F.metrics.p, (float *)d.ptr, (float *)e.ptr, cap,
                                          (unsigned long long *)set->mem));
        break;
    }
    case GVOM_PRODUCT_HEIGHT_CLOUD: HIPCHK(h, launch_height_cloud(h, F, (float *)set->mem, nullptr)); break;
    default: HIPCHK(h, launch_height_cloud(h, F, nullptr, (float *)set->mem)); break;
    }
    HIPCHK(h, hipEventRecord(set->ready, h->stream));
    set->id = ++h->pset_seq;
    *product_id = set->id;
    return GVOM_OK;
}

VIS int gvom_device_product_export(gvom_t *h, int64_t product_id, int part, void *consumer_stream, void **ptr, int32_t *ndim,
                                   int64_t shape[3], int64_t strides[3])
{
    if (!h || !ptr || !ndim || !shape || !strides) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    DevSet *s = nullptr;
    SetPart d;
    const int rc = set_export(h, false, product_id, part, consumer_stream, &s, &d);
    if (rc) return rc;
    *ptr = d.ptr; *ndim = d.ndim;
    for (int k = 0; k < 3; ++k) { shape[k] = d.shape[k]; strides[k] = d.strides[k]; }
    return GVOM_OK;
}

VIS int gvom_device_product_release(gvom_t *h, int64_t product_id, void *consumer_stream)
{
    if (!h) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    return set_release_id(h, false, product_id, consumer_stream);
}

VIS int gvom_device_product_dlpack(gvom_t *h, int64_t product_id, int part, void *consumer_stream, int versioned, void **managed)
{
    if (!h || !managed) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    return set_dlpack(h, false, product_id, part, consumer_stream, versioned, managed);
}

VIS int gvom_device_product_copy(gvom_t *h, int64_t product_id, int part, void *host_out)
{
    if (!h || !host_out) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    return set_copy(h, false, product_id, part, host_out);
}

// ---- obstacle clearance (gvom_clearance) ---------------------------------------------------------------------------------------
// The distance from every cell to the nearest hard obstacle of a positive / negative map pair, as a product of kind
// GVOM_PRODUCT_CLEARANCE: two kernels (gvom_clearance.hip) on the handle's stream, behind the k_map2d that wrote the map set
// they read -- and in front of whatever recycles that set later, which runs on the same stream.  Enqueues and returns.
VIS int gvom_clearance(gvom_t *h, int64_t map_set_id, const int32_t *positive, const int32_t *negative, int on_device,
                       double density_threshold, int32_t max_cells2, int flags, int64_t *product_id)
{
    if (!h || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *product_id = -1;
    if (h->sharded) { h->err = "gvom_clearance: sharded handles are not supported"; return GVOM_ERR_INVALID; }
    if (flags & ~GVOM_CLEARANCE_NO_NEGATIVE) { h->err = "gvom_clearance: unknown flag bits"; return GVOM_ERR_INVALID; }
    if (density_threshold != density_threshold) { h->err = "gvom_clearance: the density threshold is not a number"; return GVOM_ERR_INVALID; }
    if (map_set_id >= 0 && (positive || negative)) { h->err = "gvom_clearance: give a map set id or map pointers, not both"; return GVOM_ERR_INVALID; }
    if (map_set_id < 0 && !positive) { h->err = "gvom_clearance: give a map set id or a positive map"; return GVOM_ERR_INVALID; }
    const int xy = h->prm.xy_size;
    if (xy > GVOM_CLEARANCE_MAX_XY) { h->err = "gvom_clearance: maps of more than 4096 cells a side are not supported"; return GVOM_ERR_CAPACITY; }
    const size_t n2 = (size_t)xy * xy;
    const int32_t *pos = positive, *neg = negative;
    if (map_set_id >= 0) {
        DevSet *m = find_set(h->dsets, map_set_id);
        if (!m) { h->err = "unknown or stale device map set id"; return GVOM_ERR_INVALID; }
        SetPart d;
        set_part(m, 0, &d); pos = (const int32_t *)d.ptr;
        set_part(m, 1, &d); neg = (const int32_t *)d.ptr;
    }
    HIPCHK(h, hipSetDevice(h->device));
    const int kind = GVOM_PRODUCT_CLEARANCE;
    DevSet *set = set_recycle(h->psets, kind, set_bytes(kind, xy, 0, 0));
    if (!set) {
        int n = 0;
        for (DevSet *s : h->psets) n += s->kind == kind;
        if (n >= GVOM_MAX_PRODUCT_SETS) {
            h->err = "gvom_clearance: all 4 device product sets of this kind are exported; release some (gvom_device_product_release, or drop the tensors)";
            return GVOM_ERR_CAPACITY;
        }
        const int rc0 = set_new(h, h->psets, kind, set_bytes(kind, xy, 0, 0), &set);
        if (rc0) return rc0;
        ++h->cl_allocs;
    }
    int rc;
    if (!h->cl_g.p) {
        if ((rc = ensure(h, h->cl_g, gvom_clearance_scratch_bytes(xy)))) return rc;
        ++h->cl_allocs;
    }
    HIPCHK(h, join_second_stream(h));
    if (map_set_id < 0 && !on_device) {                                     // host maps: staged, and up before the call returns
        if (!h->cl_stage.p) {
            if ((rc = ensure(h, h->cl_stage, 2 * n2 * 4))) return rc;
            ++h->cl_allocs;
        }
        int32_t *st = (int32_t *)h->cl_stage.p;
        HIPCHK(h, hipMemcpyAsync(st, positive, n2 * 4, hipMemcpyHostToDevice, h->stream));
        if (negative) HIPCHK(h, hipMemcpyAsync(st + n2, negative, n2 * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        pos = st; neg = negative ? st + n2 : nullptr;
    }
    if (flags & GVOM_CLEARANCE_NO_NEGATIVE) neg = nullptr;
    if ((rc = set_wait_releases(h, set))) return rc;
    SetPart d0, d1;
    set_part(set, 0, &d0); set_part(set, 1, &d1);
    HIPCHK(h, gvom_launch_clearance(h->stream, xy, h->prm.xy_resolution, pos, neg, density_threshold, max_cells2,
                                    (uint16_t *)h->cl_g.p, (float *)d0.ptr, (int32_t *)d1.ptr, h->cl_shape));
    HIPCHK(h, hipEventRecord(set->ready, h->stream));
    set->id = ++h->pset_seq;
    *product_id = set->id;
    return GVOM_OK;
}

// ---- ray queries (gvom_raycast) --------------------------------------------------------------------------------------------------
// n segments walked through the CURRENT fused map by k_raycast (gvom_query.hip), read-only, on the handle's stream behind
// whatever produced that map; the result is a product of kind GVOM_PRODUCT_RAYCAST sized by n.  Enqueues and returns; later
// scans and combines run behind the kernel on the same stream and never touch the product.
VIS int gvom_raycast(gvom_t *h, const float *from, int64_t K, const float *to, int64_t n, int on_device, int flags,
                     double origin_voxels[3], int64_t *product_id)
{
    if (!h || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *product_id = -1;
    if (h->sharded) { h->err = "gvom_raycast: sharded handles are not supported"; return GVOM_ERR_INVALID; }
    if (!from || !to) { h->err = "gvom_raycast: from and to must not be NULL"; return GVOM_ERR_INVALID; }
    if (n < 1) { h->err = "gvom_raycast: n must be at least 1"; return GVOM_ERR_INVALID; }
    if (K != 1 && K != n) { h->err = "gvom_raycast: K must be 1 or n"; return GVOM_ERR_INVALID; }
    if (flags & ~(GVOM_RAY_UNKNOWN_BLOCKS | GVOM_RAY_CHECK_TARGET)) { h->err = "gvom_raycast: unknown flag bits"; return GVOM_ERR_INVALID; }
    if (n > GVOM_RAYCAST_MAX_RAYS) { h->err = "gvom_raycast: more than 2^26 rays in one call"; return GVOM_ERR_CAPACITY; }
    if (!h->has_combined) return GVOM_NO_DATA;
    HIPCHK(h, hipSetDevice(h->device));
    const int kind = GVOM_PRODUCT_RAYCAST;
    const size_t bytes = set_bytes(kind, 0, 0, n);
    DevSet *set = set_recycle(h->psets, kind, bytes);
    if (!set) {
        int held = 0;
        for (DevSet *s : h->psets) held += s->kind == kind;
        if (held >= GVOM_MAX_PRODUCT_SETS) {
            h->err = "gvom_raycast: all 4 device product sets of this kind are exported; release some (gvom_device_product_release, or drop the tensors)";
            return GVOM_ERR_CAPACITY;
        }
        const int rc0 = set_new(h, h->psets, kind, bytes, &set);
        if (rc0) return rc0;
        ++h->rq_allocs;
    }
    set->cap = n;
    int rc;
    const Fused &F = h->fused[h->cur];
    ScanParams P;
    RayQuery Q;
    memset(&Q, 0, sizeof Q);
    raycast_params(h, F, P, Q);
    Q.from = from; Q.to = to; Q.n = (long)n;
    Q.one_origin = K == 1 ? 1 : 0;
    Q.unknown_blocks = (flags & GVOM_RAY_UNKNOWN_BLOCKS) ? 1 : 0;
    Q.check_target = (flags & GVOM_RAY_CHECK_TARGET) ? 1 : 0;
    HIPCHK(h, join_second_stream(h));
    if (!on_device) {                                                       // host segments: staged, and up before the call returns
        const size_t kb = (size_t)K * 12, nb = (size_t)n * 12;
        if (h->rq_stage.bytes < align256(kb) + nb) {
            if ((rc = ensure(h, h->rq_stage, align256(kb) + nb))) return rc;
            ++h->rq_allocs;
        }
        char *st = (char *)h->rq_stage.p;
        HIPCHK(h, hipMemcpyAsync(st, from, kb, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(st + align256(kb), to, nb, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        Q.from = (const float *)st; Q.to = (const float *)(st + align256(kb));
    }
    if ((rc = set_wait_releases(h, set))) return rc;
    SetPart d0, d1;
    set_part(set, 0, &d0); set_part(set, 1, &d1);
    HIPCHK(h, gvom_launch_raycast(h->stream, P, Q, F.state, F.tags, (int32_t *)d0.ptr, (float *)d1.ptr));
    HIPCHK(h, hipEventRecord(set->ready, h->stream));
    set->id = ++h->pset_seq;
    *product_id = set->id;
    for (int k = 0; origin_voxels && k < 3; ++k) origin_voxels[k] = (double)F.origin[k];
    return GVOM_OK;
}
// ---- cost-to-go fields (gvom_cost_to_go) ------------------------------------------------------------------------------------------
// The navigation function of a cost map -- a caller's, or the one k_travcost builds from a device map set -- as a product of kind
// GVOM_PRODUCT_COSTFIELD.  The kernels (gvom_costfield.hip) run on the handle's stream behind the combine that wrote the set, and
// whatever recycles the set later runs behind them.  Unlike the other product calls this one WAITS: rounds of k_ctg_relax are
// enqueued a batch at a time, the batch's per-round counters come back through pinned memory, and the first round that flagged no
// tile ends the solve (the rounds enqueued behind it found nothing to do).
VIS int gvom_cost_to_go(gvom_t *h, int64_t map_set_id, const gvom_ctg_params *params, const int32_t *cost, int on_device,
                        const int32_t *goals, int64_t n_goals, int32_t max_cost, int32_t max_rounds, int flags,
                        int64_t *product_id, int64_t info[4])
{
    if (!h || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *product_id = -1;
    for (int k = 0; info && k < 4; ++k) info[k] = 0;
    if (h->sharded) { h->err = "gvom_cost_to_go: sharded handles are not supported"; return GVOM_ERR_INVALID; }
    if (flags & ~(GVOM_CTG_NO_NEGATIVE | GVOM_CTG_UNKNOWN_BLOCKS)) { h->err = "gvom_cost_to_go: unknown flag bits"; return GVOM_ERR_INVALID; }
    if (map_set_id >= 0 && cost) { h->err = "gvom_cost_to_go: give a map set id or a cost map, not both"; return GVOM_ERR_INVALID; }
    if (map_set_id < 0 && !cost) { h->err = "gvom_cost_to_go: give a map set id or a cost map"; return GVOM_ERR_INVALID; }
    if (map_set_id >= 0 && !params) { h->err = "gvom_cost_to_go: a map set needs the cost parameters"; return GVOM_ERR_INVALID; }
    if (!goals || n_goals < 1 || n_goals > GVOM_CTG_MAX_GOALS) { h->err = "gvom_cost_to_go: between 1 and 65536 goals"; return GVOM_ERR_INVALID; }
    if (max_cost < 0 || max_cost > GVOM_CTG_MAX_COST) { h->err = "gvom_cost_to_go: max_cost outside 0 .. 2^30"; return GVOM_ERR_INVALID; }
    if (max_rounds < 0) { h->err = "gvom_cost_to_go: max_rounds must not be negative"; return GVOM_ERR_INVALID; }
    const int xy = h->prm.xy_size;
    if (xy > GVOM_CLEARANCE_MAX_XY) { h->err = "gvom_cost_to_go: maps of more than 4096 cells a side are not supported"; return GVOM_ERR_CAPACITY; }
    const size_t n2 = (size_t)xy * xy;
    for (int64_t k = 0; k < 2 * n_goals; ++k)
        if (goals[k] < 0 || goals[k] >= xy) { h->err = "gvom_cost_to_go: a goal lies outside the window"; return GVOM_ERR_INVALID; }
    CtgCostParams C;
    memset(&C, 0, sizeof C);
    DevSet *m = nullptr;
    if (map_set_id >= 0) {
        const gvom_ctg_params &p = *params;
        const bool ok = p.density_threshold == p.density_threshold && p.inflation_cells2 >= 0 && p.base >= 1 &&
                        p.soft_weight >= 0 && p.soft_weight <= 65535 && p.unknown_cost >= 0 && p.unknown_cost <= 65535 &&
                        p.rough_weight >= 0 && p.rough_weight <= 65535 &&
                        (p.rough_weight == 0 || (isfinite(p.min_roughness) && isfinite(p.max_roughness) && p.max_roughness > p.min_roughness));
        if (!ok) { h->err = "gvom_cost_to_go: bad cost parameters (NaN threshold, base < 1, a weight outside 0 .. 65535, a negative inflation, or an empty / non-finite roughness range)"; return GVOM_ERR_INVALID; }
        m = find_set(h->dsets, map_set_id);
        if (!m) { h->err = "unknown or stale device map set id"; return GVOM_ERR_INVALID; }
        C.density_threshold = p.density_threshold; C.min_roughness = p.min_roughness; C.max_roughness = p.max_roughness;
        C.inflation_cells2 = p.inflation_cells2; C.base = p.base; C.soft_weight = p.soft_weight; C.unknown_cost = p.unknown_cost;
        C.rough_weight = p.rough_weight;
        C.use_negative = (flags & GVOM_CTG_NO_NEGATIVE) ? 0 : 1; C.unknown_blocks = (flags & GVOM_CTG_UNKNOWN_BLOCKS) ? 1 : 0;
    } else if (!on_device) {
        for (size_t k = 0; k < n2; ++k)
            if (cost[k] < 0 || cost[k] > 65535) { h->err = "gvom_cost_to_go: a host cost map holds a value outside 0 .. 65535"; return GVOM_ERR_INVALID; }
    }
    HIPCHK(h, hipSetDevice(h->device));
    const int kind = GVOM_PRODUCT_COSTFIELD;
    DevSet *set = set_recycle(h->psets, kind, set_bytes(kind, xy, 0, 0));
    if (!set) {
        int n = 0;
        for (DevSet *s : h->psets) n += s->kind == kind;
        if (n >= GVOM_MAX_PRODUCT_SETS) {
            h->err = "gvom_cost_to_go: all 4 device product sets of this kind are exported; release some (gvom_device_product_release, or drop the tensors)";
            return GVOM_ERR_CAPACITY;
        }
        const int rc0 = set_new(h, h->psets, kind, set_bytes(kind, xy, 0, 0), &set);
        if (rc0) return rc0;
        ++h->ctg_allocs;
    }
    int rc;
    const int nt = gvom_ctg_tiles(xy), ntiles = nt * nt;
    const size_t flags_off = 256, goals_off = flags_off + align256((size_t)2 * ntiles * 4);
    if (!h->ctg_work.p) {
        if ((rc = ensure(h, h->ctg_work, goals_off + (size_t)GVOM_CTG_MAX_GOALS * 8))) return rc;
        ++h->ctg_allocs;
    }
    if (!h->ctg_pin) HIPCHK(h, hipHostMalloc((void **)&h->ctg_pin, 256, hipHostMallocDefault));
    uint32_t *cnt = (uint32_t *)h->ctg_work.p;
    uint32_t *fl = (uint32_t *)((char *)h->ctg_work.p + flags_off);
    int32_t *gdev = (int32_t *)((char *)h->ctg_work.p + goals_off);
    HIPCHK(h, join_second_stream(h));
    const int32_t *cost32 = nullptr;
    if (map_set_id < 0 && !on_device) {                                     // a host cost map: staged
        if (!h->ctg_stage.p) {
            if ((rc = ensure(h, h->ctg_stage, n2 * 4))) return rc;
            ++h->ctg_allocs;
        }
        HIPCHK(h, hipMemcpyAsync(h->ctg_stage.p, cost, n2 * 4, hipMemcpyHostToDevice, h->stream));
        cost32 = (const int32_t *)h->ctg_stage.p;
    } else if (map_set_id < 0) cost32 = cost;
    const size_t clr_g = align256(gvom_clearance_scratch_bytes(xy)), clr_map = align256(n2 * 4);
    if (m && C.inflation_cells2 > 0 && !h->ctg_clr.p) {
        if ((rc = ensure(h, h->ctg_clr, clr_g + 2 * clr_map))) return rc;
        ++h->ctg_allocs;
    }
    HIPCHK(h, hipMemcpyAsync(gdev, goals, (size_t)n_goals * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(cnt, 0, 256, h->stream));
    if ((rc = set_wait_releases(h, set))) return rc;
    SetPart d0, d1, d2;
    set_part(set, 0, &d0); set_part(set, 1, &d1); set_part(set, 2, &d2);
    int32_t *D = (int32_t *)d0.ptr;
    uint16_t *c16 = (uint16_t *)d2.ptr;
    if (m) {
        SetPart mp, mn, mv, mr;
        set_part(m, 0, &mp); set_part(m, 1, &mn); set_part(m, 2, &mv); set_part(m, 3, &mr);
        const int32_t *cd2 = nullptr;
        if (C.inflation_cells2 > 0) {
            char *q = (char *)h->ctg_clr.p;
            HIPCHK(h, gvom_launch_clearance(h->stream, xy, h->prm.xy_resolution, (const int32_t *)mp.ptr,
                                            C.use_negative ? (const int32_t *)mn.ptr : nullptr, C.density_threshold, C.inflation_cells2,
                                            (uint16_t *)q, (float *)(q + clr_g), (int32_t *)(q + clr_g + clr_map)));
            cd2 = (const int32_t *)(q + clr_g + clr_map);
        }
        HIPCHK(h, gvom_launch_travcost(h->stream, xy, (const int32_t *)mp.ptr, (const int32_t *)mn.ptr, (const int32_t *)mv.ptr,
                                       (const double *)mr.ptr, cd2, C, c16));
    }
    HIPCHK(h, gvom_launch_ctg_seed(h->stream, xy, cost32, c16, D, fl, gdev, (int)n_goals, cnt + CTG_CNT_SEEDED));
    const int32_t cap = max_cost == 0 ? GVOM_CTG_MAX_COST : max_cost;
    const int inner = h->tune_ctg_inner > 0 ? h->tune_ctg_inner : 256;
    const int batch = h->tune_ctg_batch > 0 ? h->tune_ctg_batch : 8;
    // by induction over the tile crossings of a shortest path the solve ends after at most (crossings + 1) rounds of tiles that
    // reach their fixed point; the limit below is beyond anything xy <= 4096 can need and only keeps this loop finite
    const int64_t limit = max_rounds > 0 ? (int64_t)max_rounds : (int64_t)1 << 22;
    int64_t rounds = 0, tiles = 0;
    bool converged = false;
    while (!converged && rounds < limit) {
        const int nb = (int)std::min<int64_t>(batch, limit - rounds);
        if (rounds) HIPCHK(h, hipMemsetAsync(cnt, 0, 2 * GVOM_CTG_MAX_BATCH * 4, h->stream));
        for (int r = 0; r < nb; ++r) {
            const int64_t k = rounds + r;
            HIPCHK(h, gvom_launch_ctg_relax(h->stream, xy, c16, D, fl + (k & 1) * ntiles, fl + ((k + 1) & 1) * ntiles, cnt + r,
                                            cnt + CTG_CNT_RELAXED + r, cap, inner));
        }
        HIPCHK(h, hipMemcpyAsync(h->ctg_pin, cnt, 2 * GVOM_CTG_MAX_BATCH * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        int ran = nb;
        for (int r = 0; r < nb; ++r) {
            tiles += h->ctg_pin[CTG_CNT_RELAXED + r];
            if (h->ctg_pin[r] == 0) { converged = true; ran = r + 1; break; }
        }
        rounds += ran;
    }
    HIPCHK(h, gvom_launch_ctg_dirs(h->stream, xy, c16, D, (uint8_t *)d1.ptr, cnt + CTG_CNT_REACHED));
    HIPCHK(h, hipEventRecord(set->ready, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->ctg_pin, cnt, 256, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (!converged && max_rounds == 0) { h->err = "gvom_cost_to_go: the field did not settle"; return GVOM_ERR_HIP; }
    h->ctg_last_tiles = (int)std::min<int64_t>(tiles, INT32_MAX);
    if (info) { info[0] = converged ? 1 : 0; info[1] = rounds; info[2] = h->ctg_pin[CTG_CNT_REACHED]; info[3] = h->ctg_pin[CTG_CNT_SEEDED]; }
    set->id = ++h->pset_seq;
    *product_id = set->id;
    return GVOM_OK;
}
}  // extern "C"
