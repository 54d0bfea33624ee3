// gvom_sets.hip -- device-resident results as sets (DevSet): the pool of map sets and product sets, their exports, releases,
// DLPack capsules and host copies, and gvom_combine_maps_device.  What a set holds is gvom_setlayout.h's to say; the calls that
// make a product (gvom_product_calls.hip) take a set through product_acquire and hand it out through product_publish.
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

DevSet *find_set(const std::vector<DevSet *> &sets, int64_t set_id)
{
    if (set_id < 0) return nullptr;
    for (DevSet *s : sets) if (s->id == set_id) return s;
    return nullptr;
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
enum { kDLROCM = 10 };
}  // namespace

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

// a new map set (at most GVOM_MAX_DEVICE_SETS; GVOM_ERR_CAPACITY, in fn's name, beyond)
static int map_set_new(gvom_handle *h, const char *fn, DevSet **set)
{
    if ((int)h->dsets.size() >= GVOM_MAX_DEVICE_SETS) {
        h->err = std::string(fn) + ": all 8 device map sets are exported; release some (gvom_device_map_release, or drop the tensors)";
        return GVOM_ERR_CAPACITY;
    }
    const int rc = set_new(h, h->dsets, 0, set_bytes(0, h->prm.xy_size, 0, (int64_t)dev_map_stride(h->prm.xy_size)), set);
    if (rc) return rc;
    (*set)->cap = (int64_t)dev_map_stride(h->prm.xy_size);                  // (a map set: the elements from one map to the next)
    return GVOM_OK;
}

namespace gvom_host {
// the pool path of a call that writes a map set (gvom_atlas_recall; gvom_combine_maps_device has the same two steps around its empty-ring
// answer): unused sets go back to the pool, then a free one, or a new one
int map_set_acquire(gvom_handle *h, const char *fn, DevSet **set)
{
    if ((*set = set_recycle(h->dsets, 0, 0))) return GVOM_OK;
    return map_set_new(h, fn, set);
}

// a reused set: its consumers' reads come first (the handle's stream waits on every release event)
int set_wait_releases(gvom_handle *h, DevSet *set)
{
    std::lock_guard<std::mutex> g(g_set_mu);
    for (hipEvent_t e : set->rel) HIPCHK(h, hipStreamWaitEvent(h->stream, e, 0));
    set->rel_spare.insert(set->rel_spare.end(), set->rel.begin(), set->rel.end());
    set->rel.clear(); set->rel_streams.clear();
    return GVOM_OK;
}

// the pool path of every product call: a free set of `kind` that holds need_bytes (free sets of the kind that are too small are given
// up), or a new one of new_bytes counted in the call's record (null: not counted); GVOM_ERR_CAPACITY, in fn's name, with GVOM_MAX_PRODUCT_SETS held
// (GVOM_MAX_DEVICE_SETS of the stamps of recalled map sets)
int product_acquire(gvom_handle *h, int kind, size_t need_bytes, size_t new_bytes, const char *fn, CallState *call, DevSet **set)
{
    if ((*set = set_recycle(h->psets, kind, need_bytes))) return GVOM_OK;
    int n = 0;
    for (DevSet *s : h->psets) n += s->kind == kind;
    const int most = kind == GVOM_PRODUCT_ATLAS_RECALL ? GVOM_MAX_DEVICE_SETS : GVOM_MAX_PRODUCT_SETS;   // (a recall's stamps go with its map set: as many)
    if (n >= most) {
        h->err = std::string(fn) + ": all " + std::to_string(most) + " device product sets of this kind are exported; release some (gvom_device_product_release, or drop the tensors)";
        return GVOM_ERR_CAPACITY;
    }
    const int rc = set_new(h, h->psets, kind, new_bytes, set);
    if (!rc && call) ++call->allocs;
    return rc;
}

// the set is written (as far as the handle's stream is concerned): exports wait on `ready`, and the set gets the id they ask for
int product_publish(gvom_handle *h, DevSet *set, int64_t *product_id)
{
    HIPCHK(h, hipEventRecord(set->ready, h->stream));
    set->id = ++h->pset_seq;
    *product_id = set->id;
    return GVOM_OK;
}
}  // namespace gvom_host

extern "C" {
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
static void dlpack_delete(DlpackCtx *c)
{
    set_release(c->set, c->stream);
    delete c;
}
static void dlpack_delete_legacy(DLManagedTensor *m) { dlpack_delete((DlpackCtx *)m->manager_ctx); }
static void dlpack_delete_versioned(DLManagedTensorVersioned *m) { dlpack_delete((DlpackCtx *)m->manager_ctx); }

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

// ---- device-resident maps (gvom_combine_maps_device) -----------------------------------------
// The fusion advances exactly as in gvom_combine_maps; k_map2d's DEV form writes the nine maps into a DevSet in device memory
// and the call returns once the work is enqueued.  Consumers take a set through exports (their stream waits on the set's
// ready event) and give it back through releases (an event on their stream): no host wait on either side.
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
        const int rc0 = map_set_new(h, "gvom_combine_maps_device", &set);
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
    for (int k = 0; k < 3; ++k) set->origin[k] = h->fused[h->cur].origin[k];
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

VIS int gvom_device_map_origin(gvom_t *h, int64_t set_id, int64_t origin_cells[3])
{
    if (!h || !origin_cells) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    DevSet *s = find_set(h->dsets, set_id);
    if (!s) { h->err = "unknown or stale device map set id"; return GVOM_ERR_INVALID; }
    for (int k = 0; k < 3; ++k) origin_cells[k] = s->origin[k];
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
}  // extern "C"
