// gvom_host.h -- private to the host units of libgvom_hip.so (gvom_handle / gvom_capi (scans) / gvom_combine / gvom_sets / gvom_product_calls /
// gvom_atlas_calls / gvom_voxel_atlas_calls / gvom_debug .hip): the handle and what it is made of, and the functions that cross those units' boundaries (namespace
// gvom_host; -fvisibility=hidden keeps them out of the dynamic symbol table) -- among them what the product calls and the atlas calls
// share: the round driver of the calls that wait, their epilogue, the argument checks, the staging of host inputs (at the end of this
// file).  Not part of the public interface (include/gvom_hip.h is); no kernel unit includes it.
#pragma once
#include "gvom_internal.h"
#include "gvom_ingest.h"
#include "gvom_outrec.h"
#include "gvom_setlayout.h"
#include "gvom_solvework.h"
#include "../../include/gvom_hip.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>
#include <immintrin.h>
#include <algorithm>
#include <atomic>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#define VIS __attribute__((visibility("default")))

namespace gvom_host {
struct Buf {                                   // grow-only device buffer
    void *p = nullptr;
    size_t bytes = 0;
    uint64_t gen = 0;                          // changes with every (re-)allocation (process-wide unique: gvom_region_generation)
};

// WHAT OWNS ITS MEMORY.  OwnedBuf is a Buf whose end frees it: ensure, ensure_keep and stage_buf take it as the Buf it is, and a
// member of this type needs no line in gvom_destroy -- `delete h` gives it back.  Owned<T, Free> is the same for a typed pointer that
// is allocated once where it is used (hipMalloc / hipHostMalloc into .p): DevPtr frees with hipFree, PinPtr -- pinned host memory --
// with hipHostFree; `bytes` is for the owner that grows one (ensure_pinned).  All move-only.  Who frees by hand all the same (a
// reconfigured atlas, the statistics' buffers) frees .p and sets it to null, as before.  NOT owning, on purpose: Slot and Fused (in
// vectors, freed selectively), the exported send regions (parked, not freed) and DevSet (may outlive the handle).
struct OwnedBuf : Buf {
    OwnedBuf() = default;
    OwnedBuf(OwnedBuf &&o) noexcept : Buf(o) { o.p = nullptr; o.bytes = 0; }
    OwnedBuf &operator=(OwnedBuf &&o) noexcept { std::swap<Buf>(*this, o); return *this; }
    OwnedBuf(const OwnedBuf &) = delete;
    OwnedBuf &operator=(const OwnedBuf &) = delete;
    ~OwnedBuf() { if (p) (void)hipFree(p); }
};
template <class T, hipError_t (*Free)(void *)> struct Owned {
    T *p = nullptr;
    size_t bytes = 0;
    Owned() = default;
    Owned(Owned &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    Owned &operator=(Owned &&o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); return *this; }
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { if (p) (void)Free((void *)p); }
    operator T *() const { return p; }
};
template <class T> using DevPtr = Owned<T, hipFree>;
template <class T> using PinPtr = Owned<T, hipHostFree>;

struct Slot {                                  // one scan in sparse form
    int32_t *state = nullptr;                  // [V] storage order
    uint16_t *code16 = nullptr;                // [V] 16-bit codes of the same voxels (xy % 4 == 0 grids), read by k_fuse4
    uint32_t *tags = nullptr;                  // [ntiles] tile epochs (live iff == epoch)
    uint32_t epoch = 0;
    Buf crows;                                 // compact rows, uint4 each: {hit, total, min-height bits, 0}
    Buf metrics, base, rowvox;                 // optional statistics: double[rows][10] x2 (metrics; own-voxel moments), row -> voxel
    int64_t origin[3] = {0, 0, 0};
    int64_t count = 0;
    bool filled = false;
    bool has_code16 = false;                   // the last encode wrote the 16-bit codes (k_fuse4 may read this slot)
    bool has_metrics = false;                  // the scan computed its per-voxel statistics (metrics / base / rowvox are this scan's)
    bool stats_valid = false;
    gvom_scan_stats stats = {0, 0, 0, 0};
};

struct Fused {
    int32_t *state = nullptr;
    uint32_t *tags = nullptr;
    uint32_t epoch = 0;
    Buf rows;                                  // compact rows, uint4 each (as a slot's)
    Buf metrics;                               // optional statistics: float[rows][10]
    int64_t origin[3] = {0, 0, 0};
    int64_t count = 0;                         // rows on THIS rank
    bool valid = false;
    bool has_metrics = false;                  // k_fuse_stats merged the statistics of this map (every source had its own)
};

// DEVICE MAP SETS (gvom_combine_maps_device): one device allocation per set holding the nine maps of one combine.  A set is handed
// out by EXPORTS (the consumer stream waits on `ready`) and taken back by RELEASES (an event recorded on the consumer stream); the
// combine that reuses the set first makes the handle's stream wait on every release event.  A set with live exports outlives the
// handle (orphan) and is freed at its last release.  PRODUCT SETS (gvom_device_product and the other product calls) are the same
// thing with another KIND of contents: one allocation with a kind and a shape, the same ready event, export count, release events
// and orphaning.  What a set of each kind holds, and where: gvom_setlayout.h, the only place that knows the layouts.
struct DevSet : SetShape {                     // (mem, xy, kind, zs, cap: gvom_setlayout.h)
    size_t bytes = 0;
    int device = 0;
    hipEvent_t ready = nullptr;                // recorded on the handle's stream behind the set's k_map2d
    int64_t id = -1;                           // sequence number of the combine that wrote it; -1: free
    int exports = 0;                           // live exports
    std::vector<hipStream_t> rel_streams;      // release events since the set was written, one per consumer stream
    std::vector<hipEvent_t> rel, rel_spare;
    bool orphan = false;                       // the handle is gone
    int64_t origin[3] = {0, 0, 0};             // a map set: the integer voxel origin of its window (the combine's, or the recall's x and y)
};
#define GVOM_MAX_DEVICE_SETS 8
#define GVOM_N_PRODUCT_KINDS 4                  // the kinds gvom_device_product makes (clearance products, raycast products and cost fields have entry points of their own)
#define GVOM_RAYCAST_MAX_RAYS ((int64_t)1 << 26)
// a goal solver's counters (uint32) behind the rounds' (gvom_solvework.h): [32] reached cells, [33] goals seeded
#define CTG_CNT_REACHED 32
#define CTG_CNT_SEEDED 33
#define GVOM_FRONTIER_MAX_CLUSTERS (1 << 20)
#define GVOM_VIEWPOINT_MAX_POSES 65536
#define GVOM_VIEWPOINT_MAX_BEAMS ((int64_t)1 << 22)
#define GVOM_VIEWPOINT_DEFAULT_MB 256
#define GVOM_VIEWPOINT_MAX_MB 4096
#define GVOM_VDIST_DEFAULT_MB 256
#define GVOM_VDIST_MAX_MB 4096
#define GVOM_VDIST_MAX_POINTS ((int64_t)1 << 26)
// the frontier labelling's counters (uint32) behind the rounds': [32] frontier cells, [33] kept clusters, [34] clusters dropped by
// min_cells, [35] frontier cells in kept clusters
#define FR_CNT_CELLS 32
#define FR_CNT_KEPT 33
// DevSet::exports / rel* / orphan: a DLPack deleter runs on whatever thread frees the consumer's tensor, without the handle
extern std::mutex g_set_mu;                               // (gvom_sets.hip)

// what a call that WAITS keeps on the handle: the work buffer its rounds run on (gvom_solvework.h has the layouts), the pinned copy of
// the counters the host loop reads, its tuning (gvom_set_tuning "<call>_inner" / "<call>_batch"; 0: the defaults) and the rounds and
// tile relaxations of the last call (gvom_get_tuning "<call>_rounds" / "<call>_tiles").  The atlas forms run under the tuning of the
// window's calls: their own is never set
struct SolveWork {
    OwnedBuf work;
    PinPtr<uint32_t> pin;
    int tune_inner = 0, tune_batch = 0;
    int last_rounds = 0, last_tiles = 0;
};

// WHAT A CALL KEEPS ON THE HANDLE, one record per call (struct gvom_handle has them by the calls' names).  The shared core is
// CallState: the staging copy of the caller's host inputs, and the count of every device allocation the call's entry points have
// made on this handle -- its buffers here and its product sets (gvom_get_tuning "<call>_allocations").  stage_buf, stage_host,
// product_acquire and the fills of the walk queries take the record; a second buffer of the same record is passed beside it.  A
// record adds only what its call really has: GroundCall the ground map of the map-set route (ground_reserve), SolveCall the work of a
// call that waits (solve_work_reserve, frontier_work).  Every buffer is grow-only, allocated by the first call that needs it, and
// owned: nothing here is freed by name.
struct CallState {
    OwnedBuf stage;
    int allocs = 0;
};
struct GroundCall : CallState { OwnedBuf ground; };
struct SolveCall : CallState { SolveWork solve; };

// RANGE IMAGES (gvom_sensor_model_set / gvom_process_range_image): the sensor model in device memory -- [n][3] directions, then
// [n][3] offsets, n = H * W -- and the staging buffers of host images and column poses.  k_unproject (gvom_ingest.hip)
// turns an image into the cloud in in_pts, which the scan then reads like an uploaded host cloud
struct RangeImageState {
    OwnedBuf model, raw, poses;
    // column poses go through a pinned staging copy: a second PAGEABLE upload per scan is a second staged, blocking copy of the
    // runtime (m256, 196 KB of poses: +27 us per step); copied here by the calling thread and sent from pinned memory, the
    // transfer is in flight while the image's own upload runs.  Free again once the scan's k_trace has completed, as in_pts is
    PinPtr<void> poses_pin;
    int32_t H = 0, W = 0;                               // 0: no model set
    double scale = 0.0, min = 0.0, max = 0.0;
    uint64_t gen = 0;                                   // counts the gvom_sensor_model_set calls (VoxelAtlasState::model_gen)
};
// MULTI-ORIGIN scans (gvom_process_pointcloud_origins / gvom_process_range_image_origins): the K x 3 float32 table of ray
// origins in voxels, followed (host index) by the uint16 index of every return: ONE region in device memory, one pinned
// staging copy the calling thread fills (as RangeImageState::poses_pin), one upload per scan, re-used across scans
struct MultiOriginState {
    OwnedBuf dev;
    PinPtr<void> pin;
};
// CLEARANCE (gvom_clearance): g = the row pass's uint16 distances, stage = the staging copy of a caller's host maps, each allocated
// by the first call that needs it; allocs counts every device allocation the entry point has made on this handle
// (these two and its product sets: gvom_get_tuning "clearance_allocations")
struct ClearanceCall : CallState {
    OwnedBuf g;
    int shape[4] = {0, 0, 0, 0};                        // the launch shape of the last gvom_clearance (gvom_get_tuning "clearance_lgw" ...), from gvom_launch_clearance
};
// RAY QUERIES (gvom_raycast): stage = the staging copy of a caller's host segments ([K][3] origins, then [n][3] end points), grown by
// the first call that needs more; allocs counts every device allocation the entry point has made on this handle (this
// buffer and its product sets: gvom_get_tuning "raycast_allocations")
struct RaycastCall : CallState {};
// COST-TO-GO FIELDS (gvom_cost_to_go): solve.work = goal_work() with goals of 2 int32; stage = the staging copy of a caller's
// host cost map; clr = what gvom_launch_clearance needs for the inflation of the map-set route (its row scratch, a distance
// map nobody reads, d2).  Each is allocated by the first call that needs it; allocs counts those and the entry point's product
// sets (gvom_get_tuning "cost_to_go_allocations")
struct CostToGoCall : SolveCall { OwnedBuf clr; };
// ROLLOUT SCORING (gvom_footprint_set / gvom_score_rollouts): FootprintTable::tab = the footprint table in device memory -- start[H + 1]
// int32, then at offs_at bytes (a multiple of 256) the offsets, 4 bytes each (dx low, dy high) --, total = its offsets and gen the
// gvom_footprint_set calls so far; RolloutCall::stage = the staging
// copy of a caller's host maps and poses; its allocs counts the device allocations gvom_score_rollouts has made on this handle
// (stage and its product sets: gvom_get_tuning "rollout_allocations"; the table is in nobody's count)
struct FootprintTable {
    OwnedBuf tab;
    size_t offs_at = 0;
    int H = 0;                                          // 0: no footprint set
    int total = 0;
    uint64_t gen = 0;
};
struct RolloutCall : CallState {};
// TERRAIN ATTITUDE SCORING (gvom_chassis_set / gvom_score_attitude): ChassisTable::tab = the chassis table in device memory -- the wheel
// offsets [H][4][2] float64, then at cs_at bytes (a multiple of 256) cos_sin [H][2] float64 --, c the chassis itself and gen the
// gvom_chassis_set calls so far; AttitudeCall::ground = the ground map
// k_attitude_ground writes on the map-set route, stage = the staging copy of a caller's host ground map and poses; allocs
// counts the device allocations gvom_score_attitude has made on this handle (ground, stage and its product sets:
// gvom_get_tuning "attitude_allocations"; the table is in nobody's count)
struct ChassisTable {
    OwnedBuf tab;
    size_t cs_at = 0;
    int H = 0;                                          // 0: no chassis set
    gvom_chassis_t c = {};
    uint64_t gen = 0;
};
struct AttitudeCall : GroundCall {};
// BODY CLEARANCE SCORING (gvom_body_set / gvom_score_body): tab = the sphere table in device memory, [256][4] float32 of which S
// are set (0: no body), ground = the ground map k_attitude_ground writes on the map-set route, stage = the staging copy of a
// caller's host field, ground map and poses; allocs counts the device allocations the two entry points have made on this handle
// (the three and the product sets: gvom_get_tuning "body_allocations")
struct BodyCall : GroundCall {
    OwnedBuf tab;
    int S = 0;
};
// SCAN ALIGNMENT SCORING (gvom_score_alignments): grid = the class grid k_align_field rebuilds in every call (2 bits per voxel,
// gvom_align_grid_bytes: gvom_get_tuning "alignment_grid_bytes" reads what is allocated), stage = the staging copy of a caller's
// host cloud and transforms; allocs counts the device allocations the entry point has made on this handle (the two and its product sets)
struct AlignmentCall : CallState { OwnedBuf grid; };
// FRONTIER EXTRACTION (gvom_frontiers): solve.work = fr_offsets() at the window's side; stage = the staging copy of a caller's host
// maps.  Each is allocated by the first call that needs it; allocs counts those and the entry point's product sets
// (gvom_get_tuning "frontier_allocations")
struct FrontierCall : SolveCall {};
// VIEWPOINT SCORING (gvom_score_viewpoints): bitmaps = one bitmap of the window's voxels per viewpoint of a batch, cleared on the
// stream before every batch; at most mb megabytes ("viewpoint_bitmap_mb"; a bitmap that alone is larger makes batches of
// one).  stage = the staging copy of a caller's host poses.  Each is allocated by the first call that needs it; allocs counts
// those and the entry point's product sets (gvom_get_tuning "viewpoint_allocations"); last_batch: viewpoints per launch of the
// last call ("viewpoint_batch", read-only)
struct ViewpointCall : CallState {
    OwnedBuf bitmaps;
    int mb = GVOM_VIEWPOINT_DEFAULT_MB;
    int last_batch = 0;
};
// POSE FIELDS (gvom_primitives_set / gvom_pose_field): tab = the primitive table in device memory -- start[H + 1] int32, then at
// prims_at bytes (a multiple of 256) the primitives, 8 bytes each (int16 dx, dy, h_to, w) --, H its headings (0: none set) and
// R its largest |dx|, |dy|: the halo of a tile.  solve.work = goal_work() with goals of 3 int32 and, as its tail,
// the uint16 cost map converted from a caller's int32 one; stage = the staging copy of a caller's host cost map.  Each is allocated
// by the first call that needs it; allocs counts those and the entry point's product sets (gvom_get_tuning "pose_field_allocations")
struct PoseFieldCall : SolveCall {
    OwnedBuf tab;
    size_t prims_at = 0;
    int H = 0, R = 0;
};
// MAP ATLAS (gvom_atlas_*): mem = the ten planes of A x A cells (gvom_internal.h "map atlas"; A == 0: none
// configured), cnt = 256 bytes of int32 counters in device memory and pin their pinned copy for gvom_atlas_counts,
// stage = the staging copy of a caller's nine host maps.  E = the extent's origin in world cells, seq = integrates so far,
// last = the origin of the last integrated set (the default of a recall; z is what a recall reports).  allocs counts the
// device allocations the entry points have made on this handle (gvom_get_tuning "atlas_allocations")
struct AtlasState : CallState {
    DevPtr<char> mem;
    DevPtr<int32_t> cnt;
    PinPtr<int32_t> pin;
    int A = 0, follow = 1;
    int64_t E[2] = {0, 0}, last[3] = {0, 0, 0};
    int32_t seq = 0;
};
// ATLAS FIELDS (gvom_atlas_cost_to_go / gvom_atlas_field_window): the solver's buffers at the atlas's side A, apart from the
// window-sized ones of gvom_cost_to_go -- solve.work = goal_work() at that side (the goals relative to the extent); clr = the
// inflation's row distances (A*A uint16), a distance map nobody reads and d2 (A*A x 4 bytes each), allocated by the first call that
// inflates.  allocs counts those and the two entry points' product sets (gvom_get_tuning "atlas_field_allocations").  No host
// inputs: stage stays empty
struct AtlasFieldCall : SolveCall { OwnedBuf clr; };
// ATLAS FRONTIERS (gvom_atlas_frontiers): solve.work = gvom_frontiers' work buffer (fr_offsets) at the side of the FIELD the call was
// given, 8 bytes per cell plus flags and counters -- apart from the window-sized one of FrontierCall, which an atlas call never touches.
// allocs counts it and the entry point's product sets (gvom_get_tuning "atlas_frontier_allocations").  No host inputs: stage stays empty
struct AtlasFrontierCall : SolveCall {};
// VOXEL ATLAS (gvom_voxel_atlas_*): mem = the pairs of A x A x Z voxels (gvom_voxel_atlas.hip has the layout; A == 0: none
// configured), cnt = 256 bytes of uint64 counters in device memory (gvom_internal.h VA_CNT_*) and pin their pinned copy for
// gvom_voxel_atlas_counts; E = the extent's origin in world voxels, seq = integrates so far, last = the window origin of the last
// integrate (the default of a box), outside / moved = counts [5] and [6] of the last integrate, which the host computes.  stage =
// the staging copy of a caller's host segments or poses, with the viewpoints' boxes behind them; bitmaps = the viewpoints' bitmaps
// under "viewpoint_bitmap_mb".  dmax / omax = the sensor model's largest finite |direction| and |offset| per axis, read back by the
// first viewpoint call after a gvom_sensor_model_set (RangeImageState::gen counts those; model_gen says which model the two were made of).
// allocs counts the device allocations the entry points have made on this handle (gvom_get_tuning "voxel_atlas_allocations"): ONE
// counter and one stage buffer for the three walk queries, the distance field and the change query
struct VoxelAtlasState : SolveCall {
    DevPtr<unsigned long long> mem, cnt;
    PinPtr<unsigned long long> pin;
    OwnedBuf bitmaps;
    int A = 0, Z = 0, follow = 1;
    int64_t E[3] = {0, 0, 0}, last[3] = {0, 0, 0};
    int64_t seq = 0, outside = 0, moved = 0;
    double dmax[3] = {0, 0, 0}, omax[3] = {0, 0, 0};
    uint64_t model_gen = 0;
    int last_batch = 0;                                 // poses per launch of the last gvom_voxel_atlas_score_viewpoints ("voxel_atlas_viewpoint_batch", read-only)
    // VOXEL DISTANCE FIELDS (gvom_voxel_atlas_distance_field): dist = the halo-grown intermediates of the x and y passes (gvom_internal.h
    // VDistFrame), grow-only, counted in allocs, at most mb megabytes ("voxel_distance_mb"); halo = {Hxy, Hz} of the last
    // call ("voxel_distance_halo_xy" / "_z", read-only)
    OwnedBuf dist;
    int mb = GVOM_VDIST_DEFAULT_MB;
    int halo[2] = {0, 0};
    // VOXEL ATLAS CHANGES (gvom_voxel_atlas_changes): solve.work = gvom_frontiers' work buffer (fr_offsets) at the window's side; chg = 256
    // bytes of uint64 counters {appeared, vanished, outside}, then the bit planes (gvom_vchange_planes_bytes), the columns' level pairs
    // and the distance plane, each 256-byte aligned; both grow-only and counted in allocs
    OwnedBuf chg;
};
// ATTITUDE VOLUMES (gvom_attitude_volume): tab = what k_volume_attitude_table makes of the footprint table and the chassis --
// (u - am, v) float64 pairs of every footprint cell, then at wcell_at bytes (a multiple of 256) per heading the wheels' cell offsets and the
// footprint's box, [H][12] int32 --, rebuilt by the first call after a gvom_footprint_set / gvom_chassis_set (FootprintTable::gen / ChassisTable::gen count those; fp_gen
// / at_gen say which pair the table was made of; FootprintTable::total = the offsets of the footprint table).  ground = the ground map of
// the map-set route, stage = the staging copy of a caller's host ground map.  allocs counts the device allocations the entry
// point has made on this handle (the three and its product sets: gvom_get_tuning "attitude_volume_allocations")
struct AttitudeVolumeCall : GroundCall {
    OwnedBuf tab;
    size_t wcell_at = 0;
    uint64_t fp_gen = 0, at_gen = 0;
};
// BODY VOLUMES (gvom_body_volume): the wheel offsets come from AttitudeVolumeCall::tab (rebuilt by the same rule, allocated once for both entry
// points and counted in ITS allocs); ground = the ground map of the map-set route, stage = the staging copy of a caller's host
// field and ground map.  allocs counts the device allocations the entry point has made on this handle (the two and its product
// sets: gvom_get_tuning "body_volume_allocations")
struct BodyVolumeCall : GroundCall {};
}  // namespace gvom_host

using namespace gvom_host;

struct gvom_handle {
    gvom_params prm;
    int device = 0;
    int rank = 0, world = 1;
    bool sharded = false;                               // created by gvom_create_sharded: scans / combines go through the split entry points
    int sy_lo = 0, sy_hi = 0;
    size_t V = 0, slabV = 0, cells2d = 0, ntiles = 0;
    int nseg = 1;
    uint32_t epoch = 0;                                 // last tile epoch handed out
    hipStream_t stream = nullptr;
    std::mutex mu;                                      // handle state
    std::mutex scan_mu;                                 // one scan at a time (held across the wait for k_trace, during which `mu` is free)
    std::string err;

    uint32_t *hit = nullptr, *total = nullptr, *mh = nullptr;   // dense accumulators (hit, ray passes, min-height), zero between scans
    size_t acc_elems = 0;
    int tune_segs = 0, tune_ep_row = -2, tune_period = 0; // gvom_set_tuning (0 / -2: automatic)
    int tune_prio = -1;                                 // gvom_set_tuning "prio" (-1: automatic)
    int tune_ilv = 0;                                   // gvom_set_tuning "interleave": sub-clouds per cloud (0: automatic, 1: off)
    int last_knobs[5] = {0, 0, 0, 0, 1};                // gvom_get_tuning: segs, period, ep_row, prio, interleave of the last scan
    int64_t last_n = -1;                                // returns of the previous scan
    uint32_t probe_var_age = 0;                         // scans of changing length since the probe last ran
    int64_t probe_n = -1; uint32_t probe_age = 0;       // layout probe (k_layout_probe): the length it last looked at, scans since
    int tune_fuse1 = 0;                                 // gvom_set_tuning "fuse1": 1 = the one-slot fusion through k_fuse4 as well (A/B)
    int tune_flag_kernel = 0;                           // gvom_set_tuning "flag_kernel": 1 = the combine's completion flag from a kernel of its own (round 3's form)
    int tune_churn = 0;                                 // test hook: re-allocate the endpoint send region every scan
    uint64_t alloc_gen = 0;                             // changes whenever a send region of this handle is re-allocated
    uint64_t handle_gen = 0;                            // this handle's own number (its fixed allocations)
    bool exported = false;                              // a transport has exported this handle's send regions to other processes
    bool holds_pooled = false;                          // some region of this handle came out of the process-wide pool (a peer may still have it mapped)
    std::vector<Buf> retired;                           // outgrown / replaced exported regions (possibly still mapped by peers), with their sizes
    uint64_t fixed_gen[3] = {0, 0, 0};                  // generations of the fixed exported allocations: send ids, send quads, height-map rows
    // rank exchange of a sharded map (world > 1): send / receive regions, indexed by peer rank
    uint32_t *x_send_ids = nullptr, *x_recv_ids = nullptr;     // quad ids: [Q] by owner / [world][myQ] by source
    void *x_send_pay = nullptr, *x_recv_pay = nullptr;         // 1 KiB per quad, same indexing
    Buf x_send_eps, x_recv_eps;                                 // endpoints {L, min-height}: [world][ep_cap] / concatenated by source
    int64_t x_ep_cap = 0;
    std::vector<int64_t> x_recv_ep_off;                         // receive offsets (endpoints) by source, [world + 1]
    uint32_t *x_qcnt = nullptr, *x_ecnt = nullptr, *x_spcnt = nullptr;   // device counters, [world * 16] each
    unsigned long long *x_host = nullptr, *x_host_dev = nullptr;   // pinned, mapped: [3*world + 2]
    Buf x_send_sp, x_recv_sp;                                   // sharded statistics: returns (3 values each) for / from other ranks
    std::vector<int64_t> x_recv_sp_off;                         // receive offsets (returns) by source, [world + 1]
    int pending_dtype = 0;                                      // cloud type of the scan between scan_local and scan_merge
    size_t x_Q = 0, x_myQ = 0;
    ScanParams pending_P;                                       // scan parameters between scan_local and scan_merge
    unsigned resident_blocks = 2048;                    // 256-thread workgroups resident on the device (queried)
    bool f32_sqrt = false;                              // GVOM_FLAG_CUDA_F32_SQRT
    std::vector<Slot> slots;                            // buffer_size + 1 (one is staging)
    std::vector<int> ring;                              // ring position -> slots index
    int staging = 0;
    int buffer_index = 0, last_buffer_index = 0;
    OwnedBuf in_pts, world_pts[2];                      // world_pts: the returns as k_trace stored them for k_stats, alternating per scan
    uint32_t *counters = nullptr;                       // device: [0] scan rows, [2..3] fuse rows (u64)
    uint32_t *counters_host = nullptr;                  // pinned, device-mapped: kernels publish counts here
    uint32_t *counters_host_dev = nullptr;              // device view of counters_host

    // pending (uncommitted) scan
    bool pending = false;
    bool pending_any = false;
    int64_t pending_origin[3] = {0, 0, 0};
    int64_t pending_n = 0;

    Fused fused[2];
    int cur = 0;                                        // fused[cur] is the latest if valid
    bool has_combined = false;
    int64_t combined_cell_count = 0;                    // global count if set by the sharded layer
    MapDesc *descs_dev = nullptr, *descs_host = nullptr;
    uint32_t *blockcounts = nullptr;                    // per-workgroup occupied counts of k_fuse
    int fuse_blocks = 0;
    int cnt_blocks = 0;                                 // entries of blockcounts the last fusion wrote (k_map2d sums them)
    // EAGER FUSION (one-slot rings: buffer_size 1, unsharded, no statistics, xy % 16 == 0).  The scan launches k_encfuse
    // behind k_trace instead of k_encode: the slot is encoded AND fused with the previous map in one pass over the
    // accumulators, into the spare fused buffer, a spare height buffer and a spare count array -- speculating that the
    // next call is combine_maps (the reference node's pattern: one combine per scan).  fuse_impl adopts the result (swaps
    // the spares in) iff nothing has changed since; otherwise it is dropped and the combine runs k_fuse1 over the encoded
    // slot as before.  Same results either way (tests: eager on / off / mixed call orders).
    double *hmaps2 = nullptr;                           // spare [sy][3][sx] buffer (k_encfuse's column tails)
    uint32_t *blockcounts2 = nullptr;
    bool spec_valid = false;                            // a speculative fusion is waiting to be adopted
    int spec_nxt = 0, spec_slot = 0, spec_blocks = 0;
    uint32_t spec_epoch = 0;
    int64_t spec_origin[3] = {0, 0, 0};
    // ... with per-voxel statistics: the speculative fusion's statistics half (k_fuse_stats on the statistics stream, behind the
    // scan's own k_stats / k_stats_gather) is enqueued with the scan too; what it needs of eager_launch's frame is kept here
    bool spec_has_metrics = false;                      // the speculative fused map will carry merged statistics
    OwnedBuf flink[2];                                  // per fused buffer: link[fused row] = row in the previous map (k_encfuse -> k_fuse_stats)
    bool fs_reads[2] = {false, false};                  // the pending k_fuse_stats reads fused[i]'s states / tile tags
    FuseParams spec_FP;
    FuseDescs spec_KD;
    // DIRECTIONAL ORDER of unordered clouds (k_dirbin_*, ScanParams::perm): "dirsort" 1 always, -1 never, 0 automatic -- when the
    // layout probe found no spatial order in the previous cloud of this length (BASELINE c1's 50,000 random points: k_trace 65 -> 16 us)
    int tune_dirsort = 0;
    OwnedBuf dir_keys, dir_perm;                        // uint16 key / uint32 position -> return, per return
    DevPtr<uint32_t> dir_hist;                          // [3][GVOM_DIRBINS]: two histograms (alternating, zero between uses) + the bins' cursors
    uint32_t dir_flip = 0;
    int last_dirsort = 0;                               // gvom_get_tuning "dirsort": the last scan ran in directional order
    int tune_encfuse = 0;                               // gvom_set_tuning "encfuse": A/B of k_encfuse's shape (low 4 bits: waves per block, bit 4: blocks in dispatch order, bit 5: the 16-sx form)
    int last_encfuse[2] = {0, 0};                       // gvom_get_tuning "encfuse_width" / "encfuse_waves": the shape of the last k_encfuse launched
    int tune_fastdiv = -1;                              // gvom_set_tuning "fastdiv": 0 = IEEE divides by the resolutions in k_trace, else the verified reciprocal form
    int fastdiv_ok = 0;                                 // bit 0 / 1: div_by_res() verified for xy_resolution / z_resolution (verify_fastdiv)
    int tune_eager = -1;                                // gvom_set_tuning "eager": 0 off, 1 always, -1 automatic (off after 3 wasted in a row)
    int eager_waste = 0;                                // speculations dropped in a row (saturates at 4)
    int eager_stat[2] = {0, 0};                         // adopted / dropped since creation (gvom_get_tuning "eager_adopted" / "eager_dropped")
    int last_fuse = 0;                                  // the last fusion's kernel, GVOM_ROUTE_* (gvom_get_tuning "fuse_kernel"; 0: none yet)
    bool last_scan_spec = false;                        // the last accepted scan went through k_encfuse
    bool solo_encoded = false;                          // a sharded handle of ONE rank: gvom_shard_scan_local has already encoded the scan (nothing to wait for)
    bool fresh_scan = false;                            // a scan has been committed and no combine has looked at it yet

    double *hmaps = nullptr;                            // [sy][3][sx]: height | inferred height | positive density
    double *height = nullptr, *inferred = nullptr;      // = hmaps, hmaps + xy  (row stride hs = 3*xy)
    int hs = 0;
    double *slope_x = nullptr, *slope_y = nullptr, *rough = nullptr, *guessed = nullptr;   // [sy][sx]
    hipStream_t own_stream = nullptr;                   // created by the library
    // asynchronous combine (gvom_combine_begin / _end): k_map2d runs on a second stream, so the next
    // scan's k_trace / k_encode (instruction-bound) overlap its PCIe-bound stores
    hipStream_t stream_b = nullptr;
    // host clouds go up on a stream of their own when the main stream is busy (the ROS node's two threads: the cloud
    // callback hands scan k + 1 over while the timer thread's combine k is still running): the copy engine moves the
    // cloud while k_fuse / k_map2d run, and k_trace waits for it on the device
    hipStream_t stream_up = nullptr;
    hipEvent_t ev_up = nullptr;
    // per-voxel statistics (opt-in) run on a stream of their own: k_stats / k_stats_gather beside the combine's fusion,
    // k_fuse_stats beside k_map2d's PCIe-bound stores.  ev_enc_s / ev_fz_s: main (or fusion) stream -> statistics
    // stream; ev_sdone: everything enqueued on the statistics stream so far (the next k_trace rewrites what it reads);
    // ev_fsdone: the last k_fuse_stats (the next fusion rewrites the fused buffer it reads as "previous")
    hipStream_t stream_s = nullptr;
    hipEvent_t ev_enc_s = nullptr, ev_fz_s = nullptr, ev_sdone = nullptr, ev_fsdone = nullptr;
    // ev_before[k & 1]: the statistics stream's work enqueued BEFORE scan k's own -- all that can still read what scan
    // k + 1 rewrites (the slot it stages into left the ring at commit k; its buffer of stored returns was scan k - 1's):
    // scan k + 1 waits for that, not for scan k's statistics, which run beside it
    hipEvent_t ev_before[2] = {nullptr, nullptr};
    bool before_valid[2] = {false, false};
    uint32_t stats_scan = 0;                             // scans with statistics so far (parity selects the buffers above)
    bool stats_prev_committed = true;                    // a rejected scan leaves its slot as the staging slot: the next scan rewrites it
    bool s_pending = false, fs_pending = false;          // recorded and not known to have completed
    hipEvent_t ev_fused = nullptr, ev_mapped = nullptr, ev_done = nullptr;
    std::mutex combine_mu;                              // one combine call at a time (taken before `mu`)
    bool pending_combine = false;                       // begun, not ended
    uint32_t combine_seq = 0;                           // completion flag of the synchronous combine (counters_host + 4)
    double last_wait_ns[2] = {0.0, 0.0};                // how long the scan / the combine waited last time (wait_published)
    bool mapped_unjoined = false;                       // ev_mapped recorded; the main stream has not waited on it
    // a fusion enqueued on the second stream (asynchronous combine, rings of >= 3 filled slots) READS the ring slots
    // it was given; the main stream must not overwrite one of them (the second scan after the begin does: the
    // oldest slot becomes the staging slot) nor read the fused map it writes before it has finished
    hipEvent_t ev_fuse_b = nullptr;
    bool fuse_b_unjoined = false;                       // ev_fuse_b recorded; the main stream has not waited on it
    uint64_t fuse_b_slots = 0;                          // bit k: slots[k] is a source of that fusion
    bool scan_inflight = false;                         // a scan's kernels are enqueued and it is not committed yet (scan_mu held)
    std::vector<void *> out_bufs;                        // buffers handed out by gvom_output_buffer_alloc (coherent by construction)
    void *last_checked_out = nullptr;                    // a caller's own output buffer whose flags have been checked
    // CONTENT RECORD of the output buffers (gvom_outrec.h; k_map2d's DELTA form): which of out_bufs has which slot of out_rec_bits
    // (GVOM_OUTREC_MAX slots of gvom_outrec_bytes(xy) bytes, rounded up to 256; allocated by the first combine that needs it).
    // Only buffers from gvom_output_buffer_alloc are recorded: their lifetime is the library's to see.
    OutRecTable out_rec;
    uint8_t *out_rec_bits = nullptr;
    int tune_delta_out = 1;                             // gvom_set_tuning "delta_out": 0 = every combine stores every run (and keeps no record)
    void *out_host = nullptr;                           // pinned, device-mapped staging for the 4 outputs
    char *out_host_dev = nullptr;                       // device view of out_host (zero-copy target)
    uint32_t scan_seq = 0;                              // sequence number of the {seq,count} flag
    bool ev_scan = false, ev_fuse = false, ev_map = false;   // which profiling events are recorded
    bool maps_valid = false;

    double ego[3] = {0, 0, 0};
    int in_off[3] = {0, 1, 2};                          // element offsets of x, y, z in the cloud being scanned
    bool in_f32 = false;                                // float32 records widened to a float64 computation (PointCloud2 ingest)

    OwnedBuf tl;                                        // diagnostic build: k_trace's timeline of the last scan (GVOM_TRACE_TIMELINE)
    int tl_grid[2] = {0, 0};
    double host_ns[8] = {0, 0, 0, 0, 0, 0, 0, 0};       // host-side phase timing (GVOM_HOST_TIMING)
    long host_calls = 0;
    bool host_timing = false;
    bool stats = false;                                 // per-voxel statistics computed by the NEXT scan / merged by the next fusion
    // ON DEMAND (GVOM_FLAG_STATISTICS_ON_DEMAND): the statistics start ON -- the reference computes them in every scan and
    // combine (gvom.py:159, 276-284) and its node reads them every tick (gvom_ros.py:171) -- and go OFF at the fourth combine
    // in a row that nobody read them before (fuse_impl: ++stats_idle > 3; a read is stats_demand(): gvom_gather_metrics,
    // gvom_debug_voxel_map / _eigen and the voxel-cloud device product -- NOT gvom_read_rows); a later read finds no data and
    // switches them ON again for the scans that follow
    bool stats_auto = false;
    int stats_idle = 0;                                 // combines since the statistics were last read
    bool stats_release = false;                         // they have just been switched off: their buffers go at the end of this combine
    int acc_pad = 7, sxq = 0;                           // accumulator row pitch (lines) = ceil(xy/4) + acc_pad
    bool profiling = false;
    hipEvent_t ev[8] = {nullptr};
    float stage_ms[GVOM_N_STAGES] = {0, 0, 0, 0, 0};
    // device map sets (gvom_combine_maps_device)
    std::vector<DevSet *> dsets;
    int64_t dset_seq = 0;
    std::vector<DevSet *> psets;                        // product sets (gvom_device_product), every kind; ids from pset_seq
    int64_t pset_seq = 0;
    int tune_occ_clear = 0;                             // gvom_set_tuning "occupancy_clear": 1 = clear the grid, write live tile columns only (A/B)
    bool count_pending = false;                         // the last combine was a device combine: its fused cell count is read
    hipEvent_t ev_dcount = nullptr;                     //   from the host-mapped counter once this event (behind its k_map2d) has completed
    // WHAT THE CALLS KEEP, one record each (declared above, each with what it holds): the two ingest routes, then the product calls
    RangeImageState range_image;
    MultiOriginState multi_origin;
    int last_multi_origin = 0;                          // the last scan ran the per-lane-origin trace (gvom_get_tuning "multi_origin_ran")
    ClearanceCall clearance;
    RaycastCall raycast;
    CostToGoCall cost_to_go;
    FootprintTable footprint;
    RolloutCall rollouts;
    ChassisTable chassis;
    AttitudeCall attitude;
    BodyCall body;
    AlignmentCall alignment;
    FrontierCall frontiers;
    ViewpointCall viewpoints;
    PoseFieldCall pose_field;
    AtlasState atlas;
    AtlasFieldCall atlas_field;
    AtlasFrontierCall atlas_frontiers;
    VoxelAtlasState voxel_atlas;
    AttitudeVolumeCall attitude_volume;
    BodyVolumeCall body_volume;
};

namespace gvom_host {
inline double now_ns() { timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e9 + t.tv_nsec; }
#define HT(h, slot, t0) do { if ((h)->host_timing) { double n_ = now_ns(); (h)->host_ns[slot] += n_ - (t0); (t0) = n_; } } while (0)

#define HIPCHK(h, call)                                                                         \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            char b_[512];                                                                       \
            snprintf(b_, sizeof b_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),      \
                     __FILE__, __LINE__);                                                       \
            (h)->err = b_;                                                                      \
            return GVOM_ERR_HIP;                                                                \
        }                                                                                       \
    } while (0)

// Allocations another process may map (the peer transport exports the send regions and the height-map rows) are whole
// multiples of 2 MiB: the HSA runtime carves smaller ones out of shared 2 MiB blocks, and a block cannot be exported
// twice -- a second small region landing in an exported block is what hipIpcGetMemHandle refused ("invalid argument").
inline size_t exportable_size(size_t bytes) { const size_t g = (size_t)2 << 20; return ((bytes ? bytes : 1) + g - 1) / g * g; }

inline int64_t floor_mod(int64_t a, int64_t n) { int64_t r = a % n; return r < 0 ? r + n : r; }

inline int clamp_delta(int64_t d, int size)
{   // any |d| >= size puts the whole source window outside; keep ints small
    if (d > size) return size;
    if (d < -size) return -size;
    return (int)d;
}

// the ring-window phase of a map whose window starts at world voxel `origin`: om = origin mod size (gvom_internal.h "STORAGE LAYOUT")
inline void window_phase(const gvom_handle *h, const int64_t origin[3], int om[3])
{
    for (int k = 0; k < 3; ++k) om[k] = (int)floor_mod(origin[k], k < 2 ? h->prm.xy_size : h->prm.z_size);
}

// the world position of a fused map's window corner, for the combine calls (gvom.py:185-188); `out` may be null
inline void world_origin(const gvom_handle *h, const Fused &F, double out[3])
{
    for (int k = 0; out && k < 3; ++k) out[k] = (double)F.origin[k] * (k < 2 ? h->prm.xy_resolution : h->prm.z_resolution);
}

// ---- functions that cross unit boundaries, by the unit that defines them ----
// gvom_handle.hip
int ensure(gvom_handle *h, Buf &b, size_t bytes);
int ensure_keep(gvom_handle *h, Buf &b, size_t bytes);
void stats_demand(gvom_handle *h);
void release_statistics_buffers(gvom_handle *h);
int renumber_epochs(gvom_handle *h);
hipError_t sync_streams(gvom_handle *h);
hipError_t join_fuse_stream(gvom_handle *h);
hipError_t join_map_stream(gvom_handle *h);
hipError_t join_second_stream(gvom_handle *h);
bool wait_published(gvom_handle *h, std::unique_lock<std::mutex> &lk, volatile unsigned long long *flag, uint32_t seq,
                    bool high_half, double *last_ns);
void collect_stage_ms(gvom_handle *h);
// gvom_capi.hip (scans)
bool verify_fastdiv(double d);
// gvom_combine.hip
void fill_fuse_frame(const gvom_handle *h, const int64_t origin[3], FuseParams &P);
int fuse_impl(gvom_handle *h, hipStream_t on = nullptr);
int map2d_impl(gvom_handle *h, bool gathered, bool publish, char *out_dev, bool yx, const double *occ = nullptr,
               hipStream_t on = nullptr, uint32_t done_seq = 0, bool dev_set = false, void *host_out = nullptr);
int settle_count(gvom_handle *h);
// gvom_sets.hip
void set_free(DevSet *s);
DevSet *find_set(const std::vector<DevSet *> &sets, int64_t set_id);
int set_wait_releases(gvom_handle *h, DevSet *set);
int product_acquire(gvom_handle *h, int kind, size_t need_bytes, size_t new_bytes, const char *fn, CallState *call, DevSet **set);   // (call: whose allocs a new set counts in; null: nobody's)
int product_publish(gvom_handle *h, DevSet *set, int64_t *product_id);
int map_set_acquire(gvom_handle *h, const char *fn, DevSet **set);
// gvom_product_calls.hip
void occ_params(const gvom_handle *h, const Fused &F, OccParams &P);
void cloud_params(const gvom_handle *h, const Fused &F, Map2dParams &P);
hipError_t launch_height_cloud(gvom_handle *h, const Fused &F, float *out7, float *out3);
// ---- what the product calls and the atlas calls (gvom_atlas_calls.hip) share; defined in gvom_product_calls.hip unless inline ----
// part `part` of a set as a launcher takes it.  The part numbers are literals at the call sites: one the set's kind does not have is
// a mistake in the calling unit, and stops the process instead of handing a kernel a null pointer
template <class T> inline T *part_ptr(const DevSet *s, int part)
{
    SetPart d;
    if (!set_part(s, part, &d)) { fprintf(stderr, "gvom: a device set of kind %d has no part %d\n", s->kind, part); abort(); }
    return (T *)d.ptr;
}

// the metric frame of the fused map F for the kernels that turn world coordinates into voxels (ScanParams, AlignParams): the
// resolutions, their reciprocals, whether the verified reciprocal form may be used, the window's corner
template <class P> inline void metric_frame(const gvom_handle *h, const Fused &F, P &p)
{
    p.xy_res = h->prm.xy_resolution; p.z_res = h->prm.z_resolution;
    p.drcp[0] = 1.0 / h->prm.xy_resolution; p.drcp[1] = 1.0 / h->prm.z_resolution;
    p.fastdiv = h->tune_fastdiv == 0 ? 0 : h->fastdiv_ok;
    for (int k = 0; k < 3; ++k) p.origin[k] = (double)F.origin[k];
}

// grows buffer `b` of the call's record to at least `bytes`; an allocation counts in the record.  Without `b`: the record's stage buffer
inline int stage_buf(gvom_handle *h, CallState &call, Buf &b, size_t bytes)
{
    if (b.bytes >= bytes) return GVOM_OK;
    const int rc = ensure(h, b, bytes);
    call.allocs += rc ? 0 : 1;
    return rc;
}
inline int stage_buf(gvom_handle *h, CallState &call, size_t bytes) { return stage_buf(h, call, call.stage, bytes); }

// HOST INPUTS: the present ones of `n` parts (src null: absent) copied into the call's stage buffer, grown as stage_buf does, each but the last listed
// padded to 256 bytes; dev[i] = where part i went (null: absent).  sync: the call returns with the copies done (the caller's arrays
// are free again); otherwise they are in flight on the handle's stream, as a call that waits anyway leaves them
struct HostPart { const void *src; size_t bytes; };
int stage_host(gvom_handle *h, CallState &call, const HostPart *parts, int n, bool sync, const void **dev);

// THE ARGUMENT CHECKS.  refuse: h->err = fn + ": " + what, and the code.  The others are what more than one entry point checks: each
// refuses in fn's name and returns the code, or GVOM_OK.  A caller keeps the order its checks always had: these fold only runs of
// checks that stand together in every caller
int refuse(gvom_handle *h, const char *fn, const std::string &what, int code = GVOM_ERR_INVALID);
int check_one_source(gvom_handle *h, const char *fn, bool id, bool also, bool missing, const char *by_id, const char *both, const char *other);   // "give <by_id> or <both>, not both" / "give <by_id> or <other>"
int check_goals(gvom_handle *h, const char *fn, const void *goals, int64_t n_goals, int32_t max_cost, int32_t max_rounds);
int check_rollout_shape(gvom_handle *h, const char *fn, int64_t K, int64_t T, const int64_t origin_cells[2]);
int check_side(gvom_handle *h, const char *fn);                            // windows of more than 4096 cells a side
int check_clusters(gvom_handle *h, const char *fn, int32_t min_cells, int32_t max_clusters);
int check_host_cost(gvom_handle *h, const char *fn, const int32_t *cost, size_t n2);
int cost_field_of(gvom_handle *h, const char *fn, int64_t id, DevSet **f);
int atlas_field_of(gvom_handle *h, const char *fn, int64_t id, DevSet **f);
int map_set_of(gvom_handle *h, int64_t id, DevSet **m);                    // (its text names no function)
// ctg_cost_params: the caller's cost parameters and flags checked and turned into what the launchers take
int ctg_cost_params(gvom_handle *h, const char *fn, const gvom_ctg_params *params, int flags, CtgCostParams *C);

// THE CALLS THAT WAIT.  solve_rounds is the one loop: batches of at most `batch` relaxation rounds up to `limit` rounds in all, round
// k enqueued by enqueue(k, flags in, flags out, &any[r], &ran[r]) -- a hipError_t -- on the two halves of fl, the batch's counters
// back through pin, and the first round that flagged no tile ends it (solve_look).  No allocation, nothing but the handle's stream.
struct SolveRounds { bool converged = false; int64_t rounds = 0, tiles = 0; };
template <class Enqueue> int solve_rounds(gvom_handle *h, uint32_t *cnt, uint32_t *fl, uint32_t *pin, int ntiles, int batch, int64_t limit,
                                          Enqueue enqueue, SolveRounds *out);
int solve_work_reserve(gvom_handle *h, SolveCall &call, size_t bytes);     // a work buffer of at least `bytes` in call.solve, and the pinned counters
// the goal solvers (gvom_cost_to_go, gvom_atlas_cost_to_go, gvom_pose_field): the parts of their work buffer, the goals sent up and
// the counters cleared on the stream, and -- behind the solve -- the epilogue: the set published, the counters fetched, a solve that
// did not settle under max_rounds == 0 retracted in fn's name, info and w.last_* filled
struct GoalWorkPtrs { uint32_t *cnt, *fl; int32_t *goals; char *tail; };
inline GoalWorkPtrs goal_work_ptrs(const SolveWork &w, const GoalWork &o)
{
    char *p = (char *)w.work.p;
    return GoalWorkPtrs{(uint32_t *)p, (uint32_t *)(p + o.flags), (int32_t *)(p + o.goals), p + o.tail};
}
int goal_work_start(gvom_handle *h, const GoalWorkPtrs &G, const void *goals, size_t bytes);
int goal_solve_finish(gvom_handle *h, const char *fn, SolveWork &w, DevSet *set, int64_t *product_id, const SolveRounds &S, int32_t max_rounds,
                      int64_t info[4]);
// ctg_solve: seed, the rounds and the directions on a map of n x n cells whose uint16 costs are in c16 (or come from cost32), on a
// work buffer laid out for n; the rounds run under gvom_cost_to_go's tuning.  It waits; the caller finishes with goal_solve_finish
int ctg_solve(gvom_handle *h, SolveWork &w, const GoalWorkPtrs &G, int n, const int32_t *cost32, uint16_t *c16, int32_t *D, uint8_t *dir,
              int n_goals, int32_t max_cost, int32_t max_rounds, SolveRounds *out);
// the part of gvom_frontiers that gvom_atlas_frontiers shares: everything around the marking kernel.  frontier_work: the work buffer
// for n x n cells (fr_offsets) reserved in call.solve, and its parts; the caller clears the first clear_bytes -- counters and flags -- on the
// stream, waits for its set's releases and marks.  frontier_solve: the rows' initialisation, the rounds under gvom_frontiers' tuning,
// the finish, the set's publication, info and w.last_*; errors are in fn's name.  It waits.  `more` (gvom_voxel_atlas_changes' part 4;
// empty for the frontier calls) is enqueued behind the finish and in front of the publication: what it writes is part of the product.
struct FrWork { uint32_t *cnt, *fl, *bc, *L, *count; size_t clear_bytes; };
int frontier_work(gvom_handle *h, SolveCall &call, int n, FrWork *W);
int frontier_solve(gvom_handle *h, const char *fn, SolveWork &w, int n, const int32_t *D, const FrWork &W, int32_t min_cells,
                   int32_t max_clusters, DevSet *set, int64_t *product_id, int64_t info[4], const std::function<hipError_t()> &more = {});

// THE WALK QUERIES -- rays, viewpoints, alignments -- against the fused window (gvom_product_calls.hip) and against the voxel atlas
// (gvom_voxel_atlas_calls.hip): what the two members of a pair do alike.  A caller keeps its own product kind, record (stage buffer
// and alloc counter), frame (raycast_params / walk_frame), launches and the one limit only it has, in the order they always had.
//   rays         check_rays; rays_fill: everything of Q but lit and cap, which the frame gave, the join of the second stream, and host
//                segments staged, up before it returns, with Q pointed at them
//   viewpoints   check_views: the checks up to the beam limits, with the beam counts as it leaves them; `span` = side + levels of what
//                is walked, `spans` its words in the refusal ("xy_size + z_size" / "cells + levels").  views_batch: bitmaps of `bits`
//                bits in whole 256-byte lines, as many as "viewpoint_bitmap_mb" holds, at most K and the grid's limit.  views_fill:
//                everything of Q but poses.  views_run: the rows cleared, per batch the bitmaps cleared and batch(nk) launched with
//                Q.k0 set, then best() behind the last batch
//   alignments   check_align: the checks and the class grid's size (*grid_bytes); align_fill: everything of P but its frame, the join
//                of the second stream, and host transforms and cloud staged, up before it returns (*cdev, *tdev: where the kernels read)
int check_rays(gvom_handle *h, const char *fn, const float *from, int64_t K, const float *to, int64_t n, int flags);
int rays_fill(gvom_handle *h, CallState &call, const float *from, int64_t K, const float *to, int64_t n, int on_device, int flags, RayQuery &Q);
struct ViewBeams { int64_t nh, nw, nb; };
int check_views(gvom_handle *h, const char *fn, const double *poses, int64_t K, double max_range, int32_t stride_h, int32_t stride_w, int flags,
                int64_t span, const char *spans, ViewBeams *B);
int64_t views_batch(const gvom_handle *h, int64_t bits, int64_t K, size_t *bm_words);
void views_fill(const gvom_handle *h, const RayQuery &R, const ViewBeams &B, int64_t K, double max_range, int32_t stride_h, int32_t stride_w, int flags,
                size_t bm_words, ViewQuery &Q);
int views_run(gvom_handle *h, Buf &bitmaps, ViewQuery &Q, int64_t batch, int32_t *rows, const std::function<hipError_t(int)> &launch_batch,
              const std::function<hipError_t()> &launch_best);
int check_align(gvom_handle *h, const char *fn, const float *cloud, int64_t n, const double *transforms, int64_t K, int dilate, const int32_t weights[5],
                size_t *grid_bytes);
int align_fill(gvom_handle *h, CallState &call, const float *cloud, int64_t n, const double *transforms, int64_t K, int on_device, int dilate,
               const int32_t weights[5], AlignParams &P, const float **cdev, const double **tdev);
}  // namespace gvom_host
