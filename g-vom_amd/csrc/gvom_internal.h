// gvom_internal.h -- shared between the kernels (gvom_trace / gvom_fuse / gvom_map2d / gvom_stats / gvom_query .hip) and the C-ABI host
// layer (the host units around gvom_host.h).  Not part of the public interface (include/gvom_hip.h is).
//
// STORAGE LAYOUT (DESIGN.md "Data layout in HBM")
//   Voxels are stored WORLD-ANCHORED (toroidal): the voxel with world index (xw, yw, zw)
//   lives at storage coordinates (sx, sy, sz) = (xw mod xy, yw mod xy, zw mod zs) and linear
//   index L = (sy * zs + sz) * xy + sx   -- x fastest (coalesced 64-lane rows), then z (a
//   whole column of one y-row is a contiguous xy*zs*4-byte block), y slowest (multi-GPU
//   slabs are contiguous).  Every per-voxel array of every scan and of the fused map uses
//   the same L for the same world voxel, so temporal fusion is element-wise and rows
//   never migrate between GPUs when the robot-centred window moves.
//   A map with integer origin o (window voxel (0,0,0) == world voxel o) converts window
//   coordinates with om = o mod size:  s = w + om (minus size if >= size).
//   2-D maps are stored in the same anchoring: [sy][sx] (x fastest); a rank's rows are one
//   contiguous block, so the height-map all-gather of a sharded run is a plain all_gather.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GVOM_MAX_SLOTS 64

// Timing experiments (parts of a kernel switched off; results are WRONG when set) exist only in the
// diagnostic build (make diag -> lib/libgvom_hip_diag.so, -DGVOM_DIAG): there the GVOM_*_DEBUG
// environment variables are read per call.  The production library compiles every such test away and
// reads no environment variable that can change a result.
#include <stdlib.h>
#include <string.h>
// TEST HOOKS (include/gvom_hip_test.h: the "epoch_bias" and "churn" knobs, the GVOM_TEST_IPC_REFUSE fault injector) exist only
// in lib/libgvom_hip_test.so (make test-lib, -DGVOM_TEST_HOOKS: the production kernels + the hooks) and in the diagnostic
// build; the production library does not contain them.
#if defined(GVOM_DIAG) || defined(GVOM_TEST_HOOKS)
#define GVOM_HOOKS 1
#endif
#ifdef GVOM_DIAG
#define GVOM_DBG(P, bits) ((P).dbg & (bits))
static inline int gvom_diag_env(const char *name) { const char *v = getenv(name); return v ? atoi(v) : 0; }
#else
#define GVOM_DBG(P, bits) 0
static inline int gvom_diag_env(const char *) { return 0; }
#endif

// TILES: 64 consecutive sx of one (sy, sz) row = 256 bytes of every per-voxel array.  Tile index
// T = (sy*zs + sz)*nseg + (sx >> 6), nseg = ceil(xy/64).  Every scan / fused map carries one
// uint32 tag per tile; a tile holds valid data iff tag == the map's epoch, otherwise all its
// voxels read as "never observed" (-1) and their stored bytes are stale and never read.  Epochs
// only grow, so tag arrays are never cleared.
// ACCUMULATOR LAYOUT (hit[], total[] only -- private to k_trace / k_encode): micro-tiled so that one
// 64-byte line holds a 4 (x) x 4 (y) patch of voxels at one z:
//   A(sx, sy, sz) = ((((sy >> 2) * zs + sz) * sxq + (sx >> 2)) << 4) + ((sy & 3) << 2) + (sx & 3)
// The hardware merges the lanes of one atomic instruction that fall into the same 64-B line into
// one memory-side request, and k_trace runs at that request rate; with rows of 16 consecutive x
// per line an x-dominant ray bundle (all lanes at the same x, spread over y) needed one request
// per distinct y.  Patches make x- and y-dominant bundles equally cheap (about half the requests).
// device counter block (uint32 words; 512 bytes).  The two counters k_trace adds to live on separate
// cache lines: same-line atomics are serialised by the memory system.
#define GVOM_CNT_INGRID 64     // != 0: some return of the scan in flight landed in the grid
#define GVOM_CNT_MAPDONE 32    // k_map2d: workgroups that have finished (the last one stores the combine's completion flag)
#define GVOM_CNT_WORDS 192

struct ScanParams {
    double xy_res, z_res;
    double min_d2;        // min_distance * min_distance (f64 product, gvom.py:1067)
    double origin[3];     // window origin in voxels, integer valued (gvom.py:123-126)
    double tf[12];        // rows 0..2 of the 4x4 (gvom.py:1044-1052)
    float  pt0[3];        // (float)(ego / res)  (gvom.py:1097-1099)
    float  rinv[2];       // (float)(1 / xy_res), (float)(1 / z_res): k_trace's conservative early-exit estimate only
    double drcp[2];       // RN(1 / xy_res), RN(1 / z_res) for div_by_res(): the EXACT quotient of a float32 coordinate without a divide
    int    fastdiv;       // bit 0 / 1: the host has verified drcp[0] / drcp[1] over all 2^23 float32 significands (gvom_create)
    float  win_lo[3], win_hi[3];   // k_trace: the window shrunk by 2 voxels, in voxel coordinates (origin + 2 .. origin + size - 2): a run
                          //   of steps between two positions inside it needs no window test.  lo > hi (never true) when |origin| >= 2^18
    int    has_tf;
    int    xy, zs;
    int    om[3];         // origin mod size (storage offset)
    int    sy_lo, sy_hi;  // storage rows ENCODED by this handle: [sy_lo, sy_hi) (a rank's slab; all rows otherwise)
    int    nseg;          // tiles per (sy, sz) row
    int    lg_nseg, lg_zs;  // log2 of nseg and zs when BOTH are powers of two, else -1 (k_encode decomposes quad numbers by shifts then)
    int    nsegs;         // k_trace: step segments s = (seg_start[s], seg_start[s+1]], the last one open-ended
    int    seg_start[10];
    int    ep_row;        // k_trace: blockIdx.y of the endpoint blocks (the other rows are the segments)
    int    prio_div;      // k_trace: issue priority of a wave = min(3, steps it still has to walk / prio_div); 0: hardware default
    int    lc_period;     // k_trace: flush the wave's line cache every lc_period committing steps
    int    ilv_lg;        // k_trace: log2 K of the sub-cloud interleave (0: lane l of bundle b takes return 64 b + l).  A cloud that is
                          //   K equally long sub-clouds behind one another (K sensors, K sweeps) whose returns of equal position
                          //   are neighbours in space: position p = 64 b + l takes return (p mod K) * ilv_len + p / K, so the K
                          //   neighbours sit in neighbouring lanes of ONE wave (merged steps, shared accumulator lines).  A
                          //   permutation of who traces which return: it cannot change a result.
    long   ilv_len;       // returns per sub-cloud (n / K; n % K == 0 or ilv_lg = 0)
    const uint32_t *perm; // k_trace: nullptr, or the DIRECTIONAL ORDER of an unordered cloud (k_dirbin_*): position p takes return perm[p].
                          //   A wave's 64 rays then point the same way (one of 1536 direction bins) and share accumulator lines; as with
                          //   the interleave, only WHO traces which return changes
    int    f32_sqrt;      // GVOM_FLAG_CUDA_F32_SQRT: ray_length = sqrtf(f32 sum) (real Numba-CUDA typing, gvom.py:1109)
    int    sxq;           // accumulator layout: 4x4 (x,y) patches per row of patches = ceil(xy/4) + padding
    uint32_t epoch;       // this scan's tile epoch
    int    off[3];        // element offsets of x, y, z inside a point record (0, 1, 2 unless PointCloud2 ingest)
    int    in_f32;        // 1: the records hold float32 fields that are widened to the (float64) compute type,
                          //    as ros_numpy hands the reference a float64 array (stride and offsets in 4-byte units)
    int    stat_e;        // xy_eigen_dist (sharded statistics: which ranks a return's neighbourhood reaches)
    int    shard_world, shard_rank, shard_rows;   // ranks of a sharded map (1, 0, xy when unsharded): rank r owns storage rows [r*shard_rows, (r+1)*shard_rows)
    int    dbg;           // diagnostic build only
    int    prof_on;       // diagnostic build only (GVOM_TRACE_STEPPROF): sampled waves record s_memtime stamps of their first 32 steps
    long   tl_words;      // diagnostic build only: words of per-wave records in tl; 8 summary words follow
    unsigned long long *tl;   // diagnostic build only (GVOM_TRACE_TIMELINE): 4 words per wave {start, set-up done, end, hardware id}
};

// rank exchange, k_trace side: endpoints in another rank's rows are appended to that rank's send list
struct ShardExchange {
    uint2    *ep_send;    // [world][ep_cap] {voxel L, min-height sample}
    uint32_t *ep_cnt;     // [world * 16] (one counter per 64-B line)
    long      ep_cap;
    // per-voxel statistics on a sharded map: a return goes (x, y, z in the cloud's type) to every OTHER rank that owns a
    // storage row of its (2 xy_eigen_dist + 1)-row neighbourhood -- at most two ranks (slabs are at least that high)
    void     *sp_send;    // [world][ep_cap] x 3 values; nullptr: statistics off
    uint32_t *sp_cnt;     // [world * 16]
};

// multi-origin scans (gvom_process_pointcloud_origins): return i is traced from row index[i] of a table of K ray origins
struct RayOrigins {
    const float    *tab;  // device, [K][3]: (float)(origin / resolution), the per-return ScanParams::pt0 (gvom.py:1097-1099)
    const uint16_t *idx;  // device, [n], or nullptr: index[i] = i % K
    uint32_t        K;
};

// ray queries (gvom_raycast, k_raycast in gvom_query.hip): n segments from[K == 1 ? 0 : i] -> to[i] in world metres, walked through
// the fused map whose frame (resolutions, window origin, storage phase, tile epoch, sqrt typing) a ScanParams carries
struct RayQuery {
    const float *from, *to;   // device, [K][3] / [n][3]
    long     n;
    int      one_origin;      // K == 1: every ray starts at from[0]
    int      unknown_blocks;  // GVOM_RAY_UNKNOWN_BLOCKS: the first never-observed voxel stops the ray
    int      check_target;    // GVOM_RAY_CHECK_TARGET: the end point's own voxel is examined behind the last step
    int      lit;             // 1: the literal float64 window lookup in every step (z_size > xy_size, or |origin| >= 2^24)
    uint32_t cap;             // xy_size + z_size: no ray takes more steps inside the window (ray_steps' cap)
};

// viewpoint scoring (gvom_score_viewpoints, gvom_viewpoint.hip): K sensor poses, the selected beams h = 0, stride_h, .. < H and
// w = 0, stride_w, .. < W of the handle's sensor model, walked like RayQuery's segments through the fused map of a ScanParams
struct ViewQuery {
    const double *poses;      // device, [K][12]: rows 0..2 of the sensor-to-world matrices
    const double *dir, *off;  // device, [H*W][3] each: the sensor model
    double   max_range;
    int      W;               // columns of the model
    int      stride_h, stride_w;
    int      nh, nw;          // selected rows and columns
    int      nwc;             // waves per selected row: ceil(nw / 64)
    int      nb;              // nh * nw
    int      K;
    int      k0;              // first viewpoint of the launch (its blockIdx.y = 0)
    int      unknown_blocks;  // GVOM_RAY_UNKNOWN_BLOCKS
    int      lit;             // as RayQuery::lit
    uint32_t cap;             // as RayQuery::cap
    uint32_t bm_words;        // 32-bit words from one viewpoint's bitmap to the next (>= ceil(xy*xy*zs / 32))
};
#define GVOM_VIEWPOINT_MAX_BATCH 32768   // viewpoints per launch (the grid's y extent)

#define GVOM_PACK_CHUNK 64     // quads per k_pack workgroup
#define GVOM_BASE_PITCH 16     // doubles per row of a scan's own-voxel moments (10 used): one 128-byte block per row
// rank exchange, owner side: received quads of all source ranks are unpacked by one launch
struct ShardUnpack { uint32_t q_off[GVOM_MAX_SLOTS + 1]; };    // q_off[s] = first quad (wave) of source s, q_off[world] = total

struct MapDesc {          // one source map of the fusion (ring slot or previous fused map)
    const int32_t  *state;
    const uint4 *rows;      // compact rows, 16 bytes each: {hit, total, min-height (float bits), 0} -- one line access per row
    int d[3];               // fused origin - this map's origin (window shift), clamped
    uint32_t epoch;         // tile (T) of this map is live iff tags[T] == epoch
    const uint32_t *tags;
    const void *metrics;    // optional per-row statistics: double[rows][10] (ring slot) or float[rows][10] (fused)
    union {
        const uint16_t *code16; // ring slots of xy % 4 == 0 grids: 16-bit codes (see k_encode); nullptr for the previous map
        const int32_t *link;    // k_fuse_stats, the PREVIOUS map of an eager fusion: link[fused row] = that voxel's row in the previous
                                //   map (< 0: it contributes nothing), written by k_encfuse -- the merge then reads neither the
                                //   previous map's states nor its tile tags (which the NEXT scan's k_encfuse overwrites)
    };
};

#define GVOM_KARG_DESCS 17   // ring slots + previous map passed by kernel argument when they fit
struct FuseDescs { MapDesc d[GVOM_KARG_DESCS]; };

struct FuseParams {
    int xy, zs;
    int om[3];              // fused origin mod size
    int nslots;             // number of non-empty ring slots (descs[0..nslots))
    int has_prev;           // descs[nslots] is the previous fused map
    int sy_lo, sy_hi;
    int nseg;               // tiles per (sy, sz) row
    int hs;                 // row stride (elements) of the height / inferred-height maps
    uint32_t epoch;         // epoch of the fused map being written
    int nz;                 // z-chunks per workgroup (block = 64 * nz threads)
    int zc;                 // window-z cells per chunk (<= 64)
    int cpw;                // chunks per wave (a wave walks them in ascending z)
    int one_slot;           // 1: k_fuse1 (one ring slot + the previous map; nz <= 8 waves of cpw <= 4 chunks)
    int dbg;                // diagnostic build only (GVOM_FUSE_DEBUG): 1 no code stores, 2 no emit, 4 all tiles dead
    double origin[3];       // fused origin (voxels)
    double ego[3];          // latest ego (gvom.py:294-295)
    double xy_res, z_res;
    double radius2;         // robot_radius^2 (gvom.py:533)
    double ground_to_lidar_height;
};

struct Map2dParams {
    int xy, zs;
    int om[3];
    int y_lo, y_hi;         // STORAGE rows [sy] computed by this rank
    int nseg;
    int hs;                 // row stride (elements) of the height / inferred-height maps
    int gathered_pos;       // 1: positive-obstacle densities come from the gathered height buffer (sharded)
    uint32_t epoch;         // epoch of the fused map (tile liveness of fstate)
    int dbg;                // diagnostic build only (GVOM_MAP2D_DEBUG)
    int out_yx;             // 1: returned maps in [y][x] memory order (column-major [x, y]); 0: row-major [x][y]
    double origin_z;        // fused origin z (voxels)
    double xy_res, z_res;
    double pos_thr, neg_thr, slope_thr, robot_height;
    int occ;                // 1: write the five int8 occupancy grids of gvom_ros.py:141-165 instead of the four maps
    double occ_density_thr, occ_min_rough, occ_max_rough;
    // completion flag of the synchronous combine, stored by the LAST workgroup to finish (no kernel behind k_map2d): every
    // wave waits for its own stores to be acknowledged, one lane per workgroup then counts itself in (device-scope atomic);
    // whoever sees the count complete stores done_seq into host-mapped memory and re-arms the counter
    unsigned long long *done_flag;   // nullptr: no flag
    uint32_t *done_count;
    uint32_t done_seq;
    int out_dev;            // 1: the output is a device MAP SET (k_map2d's DEV form, gvom_combine_maps_device): nine [y][x] maps,
                            //    out_rough = map 3 and the start of the f64 block (maps 4-8 follow at dev_map_stride(xy) elements)
                            //    (last member: it sits in what was the struct's tail padding, the other forms' kernel arguments keep their offsets)
};
// elements between two maps of a device map set: xy*xy rounded up to 32 (every map starts 256-byte aligned)
__host__ __device__ __forceinline__ size_t dev_map_stride(int xy) { return ((size_t)xy * xy + 31) & ~(size_t)31; }

// k_occupancy (gvom_products.hip): the fused map as the dense uint8 grid out[x][y][z] of gvom.py:356-361
#define GVOM_OCC_ZC 128         // window z levels per workgroup (a 128-byte run of every output row)
struct OccParams {
    int xy, zs;
    int om[3];              // fused origin mod size
    int y_lo, y_hi;         // STORAGE rows this handle holds (the others read as empty)
    int nseg;
    uint32_t epoch;         // epoch of the fused map (tile liveness)
};

// ---- launchers (gvom_trace / _fuse / _map2d / _stats / _products .hip) ---------------------------------------------
hipError_t gvom_launch_trace(hipStream_t s, const ScanParams &P, const ShardExchange &X, int dtype, bool big_origin, const void *pts,
                             int64_t stride_elems, int64_t n, void *world, uint32_t *hit,
                             uint32_t *total, uint32_t *mh, int32_t *state, uint32_t *tags,
                             uint32_t *counters, double *stat_sums, double *stat_base,
                             uint32_t *stat_rowvox, const RayOrigins *origins = nullptr);
hipError_t gvom_launch_pack(hipStream_t s, const ScanParams &P, uint32_t *total, const uint32_t *tags, uint32_t *send_ids,
                            void *send_pay, uint32_t *qcnt, uint32_t *ecnt, uint32_t *spcnt, uint32_t *counters,
                            unsigned long long *host_out, uint32_t seq);
hipError_t gvom_launch_unpack(hipStream_t s, const ScanParams &P, const ShardUnpack &X, const uint32_t *ids_all,
                              const void *pay_all, uint32_t my_quads, uint32_t ne, const void *eps, long row_base,
                              uint32_t *hit, uint32_t *total, uint32_t *mh, int32_t *state, uint32_t *tags,
                              double *stat_sums, double *stat_base, uint32_t *stat_rowvox);
hipError_t gvom_launch_encode(hipStream_t s, const ScanParams &P, uint32_t *hit, uint32_t *total, uint32_t *mh,
                              int32_t *state, uint16_t *code16, uint4 *crows, const uint32_t *tags,
                              uint32_t *counters, unsigned long long *host_flag, uint32_t seq, unsigned resident_blocks);
hipError_t gvom_launch_layout_probe(hipStream_t s, const ScanParams &P, int dtype, const void *pts, int64_t stride_elems, int64_t n,
                                    int max_lg, unsigned long long *host_word);
hipError_t gvom_launch_publish_seq(hipStream_t s, unsigned long long *host_flag, uint32_t seq);
// directional order of an unordered cloud: keys[n] (scratch), hist / cursor: GVOM_DIRBINS counters each (hist zero on entry, zeroed
// again for the next use on exit: the caller alternates two), perm[n] out
#define GVOM_DIRBINS 8192      // mode 1: 6 cube faces x 16 x 16 (1536 used); mode 2: 256 sin(elevation) rows x 32 azimuth sectors
hipError_t gvom_launch_dirbin(hipStream_t s, const ScanParams &P, int mode, int dtype, const void *pts, int64_t stride_elems, int64_t n,
                              uint16_t *keys, uint32_t *hist, uint32_t *hist_next, uint32_t *cursor, uint32_t *perm);
// *route: the kernel launched (gvom_get_tuning "fuse_kernel"); GVOM_ROUTE_ENCFUSE is an adopted eager fusion
enum { GVOM_ROUTE_FUSE1 = 1, GVOM_ROUTE_FUSE4_2 = 2, GVOM_ROUTE_FUSE4_4 = 3, GVOM_ROUTE_FUSE_SHORT = 4, GVOM_ROUTE_FUSE_TALL = 5,
       GVOM_ROUTE_ENCFUSE = 6, GVOM_ROUTE_DESCS_MEM = 16 };
hipError_t gvom_launch_fuse(hipStream_t s, const FuseParams &P, const FuseDescs &KD,
                            const MapDesc *descs_dev, int32_t *fstate, uint4 *frows,
                            uint32_t *ftags, uint32_t *blockcounts, double *height, double *inferred, int *route);
void gvom_encfuse_shape(int xy, int zs, int tune, int *bw, int *nw, int *nblocks, size_t *row_cap);
// flink (or nullptr): per fused row, the voxel's row in the previous map -- what the statistics merge of this speculative fusion needs
hipError_t gvom_launch_encfuse(hipStream_t s, const ScanParams &P, const FuseParams &F, const MapDesc &prev, int32_t *flink, uint32_t *hit,
                               uint32_t *total, uint32_t *mh, int32_t *state, uint4 *crows, const uint32_t *stags,
                               int32_t *fstate, uint4 *frows, uint32_t *ftags, uint32_t *blockcounts, double *height,
                               double *inferred, uint32_t *counters, unsigned long long *host_flag, uint32_t seq);
hipError_t gvom_launch_map2d(hipStream_t s, const Map2dParams &P, const int32_t *fstate, const uint32_t *ftags,
                             const uint4 *frows, const double *height,
                             const double *inferred, double *slope_x, double *slope_y,
                             double *rough, double *guessed, int32_t *out_pos, int32_t *out_neg,
                             double *out_rough, int32_t *out_vis, const uint32_t *blockcounts,
                             int nblocks, unsigned long long *host_counter, uint8_t *out_bits = nullptr);
// ---- optional per-voxel statistics (gvom.py:1172-1299, 858-909, 1333-1378, 454-473)
// nrows: candidate compact rows (the scan's returns, + received endpoints on a sharded map); extra / n_extra: returns
// received from other ranks (sharded statistics), accumulated like the rank's own
hipError_t gvom_launch_stats(hipStream_t s, const ScanParams &P, int dtype, const void *world, int64_t n,
                             const int32_t *state, const uint32_t *tags, int xy_e, int z_e, double *base,
                             double *sums, const uint32_t *rowvox, int64_t nrows, const void *extra, int64_t n_extra);
hipError_t gvom_launch_fuse_stats(hipStream_t s, const FuseParams &P, const FuseDescs &KD, const MapDesc *descs_dev,
                                  const int32_t *fstate, const uint32_t *ftags, float *fmetrics);
hipError_t gvom_launch_voxel_cloud(hipStream_t s, const Map2dParams &P, double o0, double o1, double o2,
                                   const int32_t *fstate, const uint32_t *ftags, const uint4 *frows,
                                   const float *fmetrics, float *out, float *eig, int64_t max_rows,
                                   unsigned long long *row_counter);
hipError_t gvom_launch_gather_rows10(hipStream_t s, int is_f64, const void *src, const int32_t *rows, int64_t n, void *out);
hipError_t gvom_launch_retag(hipStream_t s, uint32_t *tags, size_t n, uint32_t old_epoch, uint32_t new_epoch);
// test hooks / debug accessors
hipError_t gvom_launch_read_dense(hipStream_t s, int xy, int zs, const int om[3], int sy_lo, int sy_hi,
                                  const uint32_t *tags, uint32_t epoch, const int32_t *state, const uint4 *crows,
                                  int32_t *o_state,
                                  int32_t *o_hit, int32_t *o_total, float *o_minh, int32_t *o_row);
// out[x][y][z] (window order, C-contiguous, V bytes) = 1 where the fused voxel is occupied.  clear_first: the grid is cleared
// with hipMemsetAsync and only tile columns with a live tile are written (otherwise the kernel writes every byte itself)
hipError_t gvom_launch_occupancy(hipStream_t s, const OccParams &P, const int32_t *fstate, const uint32_t *ftags, uint8_t *out,
                                 bool clear_first);
// ray queries (gvom_query.hip): P = the fused map's frame (xy_res, z_res, drcp, fastdiv, origin, xy, zs, om, nseg, epoch, f32_sqrt;
// the rest is not read).  out4[n][4] = {status, steps, voxel, unknown}, out3[n][3] = the stop position in metres (NaN where there
// is none); out4 must be 16-byte aligned.  Reads fstate / ftags only.
hipError_t gvom_launch_raycast(hipStream_t s, const ScanParams &P, const RayQuery &Q, const int32_t *fstate, const uint32_t *ftags,
                               int32_t *out4, float *out3);
// obstacle clearance (gvom_clearance.hip): pos / neg (neg may be nullptr) are [y][x] int32 maps of xy x xy cells; a cell is an
// obstacle iff (double)pos > thr or neg > 0.  out_d2[y][x] = exact squared distance in cells to the nearest obstacle (INT32_MAX
// where there is none, or beyond max_cells2 when that is > 0), out_dist[y][x] = (float)(sqrt((double)d2) * res), +inf there.
// g: gvom_clearance_scratch_bytes(xy) of scratch (the row pass's uint16 distances).  xy <= GVOM_CLEARANCE_MAX_XY.
// shape (may be nullptr): the launch shape the call used -- {lgw (log2 of the columns per strip of k_clearance_cols), output rows
// per workgroup, dynamic LDS bytes, 64-cell chunks per row of k_clearance_rows}.
#define GVOM_CLEARANCE_MAX_XY 4096
size_t gvom_clearance_scratch_bytes(int xy);
hipError_t gvom_launch_clearance(hipStream_t s, int xy, double res, const int32_t *pos, const int32_t *neg, double thr,
                                 int32_t max_cells2, uint16_t *g, float *out_dist, int32_t *out_d2, int shape[4] = nullptr);
// the column pass alone, over row distances somebody else wrote into g (pitch (xy + 63) & ~63): gvom_launch_clearance ends in it
hipError_t gvom_launch_clearance_cols(hipStream_t s, int xy, double res, int32_t max_cells2, const uint16_t *g, float *out_dist,
                                      int32_t *out_d2, int shape[4] = nullptr);
// cost-to-go fields (gvom_costfield.hip; include/gvom_hip.h "cost-to-go fields" defines the result).  Every map is [y][x], xy x xy.
// travcost: the uint16 cost map c (0 = blocked) from the int32 positive / negative / visibility maps, the f64 roughness map and
// the clearance d2 (nullptr: no inflation).  seed: c from cost32 (clamped into 0..65535; nullptr: c is there already), D =
// INT32_MAX, both halves of flags (2 * gvom_ctg_tiles(xy)^2 words) cleared, then D = 0 at the G goals ([G][2] device int32, inside
// the window) that lie on unblocked cells, the tiles that hold or border them flagged in the first half, *seeded += their number.  relax: one round --
// the tiles flagged in fcur relax to their local fixed point (or for `inner` sweeps) accepting nothing above max_cost, clear their
// flag and flag in fnext the tiles that have to look again; *relaxed += tiles that ran, *activated += tiles that flagged any.
// dirs: the direction codes from D and c; *reached += cells with D < INT32_MAX.
struct CtgCostParams {
    double density_threshold, min_roughness, max_roughness;
    int32_t inflation_cells2, base, soft_weight, unknown_cost, rough_weight;
    int32_t use_negative, unknown_blocks;
};
int gvom_ctg_tiles(int xy);
hipError_t gvom_launch_travcost(hipStream_t s, int xy, const int32_t *pos, const int32_t *neg, const int32_t *vis, const double *rough,
                                const int32_t *d2, const CtgCostParams &C, uint16_t *c);
hipError_t gvom_launch_ctg_seed(hipStream_t s, int xy, const int32_t *cost32, uint16_t *c, int32_t *D, uint32_t *flags,
                                const int32_t *goals, int G, uint32_t *seeded);
hipError_t gvom_launch_ctg_relax(hipStream_t s, int xy, const uint16_t *c, int32_t *D, uint32_t *fcur, uint32_t *fnext,
                                 uint32_t *activated, uint32_t *relaxed, int32_t max_cost, int inner);
hipError_t gvom_launch_ctg_dirs(hipStream_t s, int xy, const uint16_t *c, const int32_t *D, uint8_t *dir, uint32_t *reached);
// rollout scoring (gvom_rollouts.hip; include/gvom_hip.h "rollout scoring" defines the result).  poses [K][T][3] float32; fstart
// [H + 1] and foffs (dx in the low, dy in the high 16 bits, both signed) are the footprint table as gvom_footprint_set stored it;
// cell_cost / cost_to_go (may be nullptr) are [y][x] maps of xy x xy cells.  summary [K][4] int32 (16-byte aligned), pose_cost [K][T].
#define GVOM_ROLLOUT_MAX_T 4096
#define GVOM_ROLLOUT_MAX_POSES ((int64_t)1 << 26)
#define GVOM_ROLLOUT_MAX_HEADINGS 1024
#define GVOM_ROLLOUT_MAX_CELLS 16384                   // per heading
#define GVOM_ROLLOUT_MAX_TABLE ((int64_t)1 << 22)      // offsets of all headings together
struct RolloutParams {
    int xy, H, T;
    float s;                // (float)(H / 2 pi): heading = rintf(yaw * s) mod H
    long long K;
    long long ox, oy;       // round(origin / xy_resolution): window cell = floor(x / xy_resolution) - ox
    double res;
};
hipError_t gvom_launch_rollouts(hipStream_t s, const RolloutParams &P, const float *poses, const int32_t *fstart, const uint32_t *foffs,
                                const uint16_t *cell_cost, const int32_t *cost_to_go, int32_t *summary, uint16_t *pose_cost);
// terrain attitude scoring (gvom_attitude.hip; include/gvom_hip.h "terrain attitude scoring" defines the result).  R = the pose frame
// as k_rollouts takes it; poses, fstart and foffs as above; wheels [H][4][2] and cos_sin [H][2] float64 are the chassis table as
// gvom_chassis_set stored it; ground is ONE [y][x] float64 map of xy x xy cells (attitude_ground writes it from a map set's height and
// inferred-height maps).  summary [K][5] int32, attitude [K][T][3] float32, status [K][T] uint8.
struct AttitudeParams {
    RolloutParams R;
    double wheelbase, track, axle_mid, belly_height;   // front_axle - rear_axle, track, 0.5 * (front_axle + rear_axle), belly_height
    float max_pitch, max_roll, min_clearance;
};
hipError_t gvom_launch_attitude_ground(hipStream_t s, int xy, int inferred, const double *height, const double *inferred_height, double *ground);
hipError_t gvom_launch_attitude(hipStream_t s, const AttitudeParams &P, const float *poses, const int32_t *fstart, const uint32_t *foffs,
                                const double *wheels, const double *cos_sin, const double *ground, int32_t *summary, float *attitude,
                                uint8_t *status);
// body clearance scoring (gvom_body.hip; include/gvom_hip.h "body clearance scoring" defines the result).  R, poses, wheels, cos_sin and
// ground as k_attitude takes them; body [S][4] float32 (bx, by, bz, r), 16-byte aligned; field float32 [n][n][zs] in the class grid's
// layout, its corner at world voxel (bx, by, bz), each within 2^40.  summary [K][4] int32, clearance [K][T] float32, pairs [K][T][2] uint8
// {status, tightest}, 2-byte aligned.
#define GVOM_BODY_MAX_SPHERES 256
struct BodyParams {
    RolloutParams R;
    double wheelbase, track, axle_mid;                 // front_axle - rear_axle, track, 0.5 * (front_axle + rear_axle)
    double z_res;                                      // (xy_resolution is R.res)
    long long bx, by, bz;
    int n, zs, S;
    float min_margin;
};
hipError_t gvom_launch_body(hipStream_t s, const BodyParams &P, const float *poses, const double *wheels, const double *cos_sin,
                            const double *ground, const float *body, const float *field, int32_t *summary, float *clearance, uint8_t *pairs);
// scan alignment scoring (gvom_align.hip; include/gvom_hip.h "scan alignment scoring" defines the result).  cloud [n][3] float32 and
// tf [K][12] float64 (rows 0..2 of each 4x4) in device memory; F = the fused map's frame as k_occupancy takes it.  grid: the class
// grid, gvom_align_grid_bytes(xy, zs) of scratch, rebuilt by every call.  counts [K][6] int32 (cleared here, then {score, occupied,
// near, free, unknown, outside}), best [4] int32 {best index, best score, n, K}.
#define GVOM_ALIGN_MAX_POINTS ((int64_t)1 << 20)
#define GVOM_ALIGN_MAX_CANDIDATES 65536
#define GVOM_ALIGN_MAX_PAIRS ((int64_t)1 << 32)
#define GVOM_ALIGN_MAX_WEIGHT 1024
#define GVOM_ALIGN_PTS_BLOCK 1024                      // returns per k_align_score workgroup (gvom_get_tuning "alignment_points_per_block")
#define GVOM_ALIGN_CAND_GROUP 32                       // candidates per k_align_score workgroup ("alignment_candidate_group")
struct AlignParams {
    double xy_res, z_res;
    double drcp[2];         // RN(1 / xy_res), RN(1 / z_res) for div_by_res()
    double origin[3];       // window origin in voxels
    long   n;
    int    K;
    int    xy, zs;
    int    rw;              // words per row of the class grid: ceil(xy / 16)
    int    fastdiv;         // as ScanParams::fastdiv
    int    dilate;
    int    w[5];            // weights of {occupied, near, free, unknown, outside}
};
size_t gvom_align_grid_bytes(int xy, int zs);
hipError_t gvom_launch_align(hipStream_t s, const OccParams &F, const AlignParams &P, const int32_t *fstate, const uint32_t *ftags,
                             const float *cloud, const double *tf, uint32_t *grid, int32_t *counts, int32_t *best);
// the same behind a class grid that is READY on the stream (k_align_field's layout: gvom_launch_align's own, or the voxel atlas's
// gvom_launch_vatlas_align_field): clears counts, k_align_score, k_align_best.  P.origin is the origin of whatever the grid shows.
hipError_t gvom_launch_align_grid(hipStream_t s, const AlignParams &P, const float *cloud, const double *tf, const uint32_t *grid,
                                  int32_t *counts, int32_t *best);
// frontier extraction (gvom_frontier.hip; include/gvom_hip.h "frontier extraction" defines the result).  Every map is [y][x], xy x xy:
// c uint16 cell costs, vis int32 visibility, D int32 cost to go (may be nullptr).  L and count are the two int32 work arrays of
// xy*xy cells.  mark: L = own index at a frontier cell / 0xffffffff elsewhere, count = 0, flags[tile] = 1 where a tile
// (gvom_frontier_tiles(xy)^2 of them, cleared by the caller) holds one, *n_frontier += frontier cells.  relax: one round, as
// gvom_launch_ctg_relax.  rows: phase 0 initialises the cap rows of parts 0 and 1 (before finish).  finish: count, the ordered ranks
// (bc: 2 * gvom_frontier_blocks(xy) words of scratch; totals[3] = {kept, dropped, cells in kept clusters}, cleared by the caller),
// the cluster map, the rows' statistics, and part 3.
int gvom_frontier_tiles(int xy);
int gvom_frontier_blocks(int xy);
hipError_t gvom_launch_frontier_mark(hipStream_t s, int xy, const uint16_t *c, const int32_t *vis, const int32_t *D, uint32_t *L,
                                     uint32_t *count, uint32_t *flags, uint32_t *n_frontier);
hipError_t gvom_launch_frontier_relax(hipStream_t s, int xy, uint32_t *L, uint32_t *fcur, uint32_t *fnext, uint32_t *activated,
                                      uint32_t *relaxed, int inner);
hipError_t gvom_launch_frontier_rows(hipStream_t s, int phase, int cap, int32_t *rows, int64_t *sums, const uint32_t *totals,
                                     const uint32_t *n_frontier, int32_t *counts);
hipError_t gvom_launch_frontier_finish(hipStream_t s, int xy, int32_t min_cells, int cap, const int32_t *D, const uint32_t *L, uint32_t *count,
                                       uint32_t *bc, uint32_t *totals, const uint32_t *n_frontier, int32_t *rows, int64_t *sums,
                                       int32_t *cmap, int32_t *counts);
// viewpoint scoring (gvom_viewpoint.hip; include/gvom_hip.h "viewpoint scoring" defines the result).  viewpoints: the `batch`
// viewpoints from Q.k0 on; bitmaps = batch x Q.bm_words words, CLEARED by the caller; rows = part 0, int32 [K][8], cleared by the
// caller before the first batch (columns 1 .. 7 are added to).  best: behind the last batch; column 0 of every row, the rows of
// invalid poses, and part 1.
hipError_t gvom_launch_viewpoints(hipStream_t s, const ScanParams &P, const ViewQuery &Q, int batch, const int32_t *fstate, const uint32_t *ftags,
                                  uint32_t *bitmaps, int32_t *rows);
hipError_t gvom_launch_viewpoint_best(hipStream_t s, const ScanParams &P, const ViewQuery &Q, const int32_t *fstate, const uint32_t *ftags,
                                      int32_t *rows, int32_t *best);
// pose fields (gvom_posefield.hip; include/gvom_hip.h "pose fields" defines the result).  c [y][x] uint16 cell costs; fstart / foffs
// the footprint table as above; C, D, action [H][y][x] volumes; pstart [H + 1] and prims [total][4] int16 (dx, dy, h_to, w) the
// primitive table as gvom_primitives_set stored it, R its largest |dx|, |dy|.  seed: phase 0 clears D and the 2 * tiles^2 flags and
// converts cost32 (may be nullptr) into c16; phase 1, behind cspace, seeds the goals [G][3] int32 (x, y, h; h < 0: every heading).
// relax: one round, as gvom_launch_ctg_relax, with gvom_pose_relax_lds(H, R) bytes of dynamic LDS.
#define GVOM_POSE_MAX_HEADINGS 64
#define GVOM_POSE_MAX_REACH 4
#define GVOM_POSE_MAX_PRIMS 64                         // per heading
#define GVOM_POSE_MAX_STATES ((int64_t)1 << 28)
int gvom_pose_tiles(int xy);
size_t gvom_pose_relax_lds(int H, int R);
hipError_t gvom_launch_cspace(hipStream_t s, int xy, int H, const uint16_t *c, const int32_t *fstart, const uint32_t *foffs, uint16_t *C);
hipError_t gvom_launch_pose_seed(hipStream_t s, int phase, int xy, int H, int R, const int32_t *cost32, uint16_t *c16, const uint16_t *C,
                                 int32_t *D, uint32_t *flags, const int32_t *goals, int G, uint32_t *seeded);
hipError_t gvom_launch_pose_relax(hipStream_t s, int xy, int H, int R, const uint16_t *C, int32_t *D, const int32_t *pstart,
                                  const int16_t *prims, uint32_t *fcur, uint32_t *fnext, uint32_t *activated, uint32_t *relaxed,
                                  int32_t max_cost, int inner);
hipError_t gvom_launch_pose_actions(hipStream_t s, int xy, int H, const uint16_t *C, const int32_t *D, const int32_t *pstart,
                                    const int16_t *prims, uint8_t *action, uint32_t *reached);
// attitude volumes (gvom_attitude_volume.hip; include/gvom_hip.h "attitude volumes" defines the result).  fstart / foffs, wheels and
// cos_sin as above.  table: uv [total][2] float64 = (u - am, v) of every footprint cell and wcell [H][12] int32 = the wheels' four cell
// offsets (dx, dy) and the footprint's box {least dx, largest dx, least dy, largest dy}, from the two tables.  volume: ground ONE [y][x] float64 map; status and tilt [H][y][x] uint8; counts [8] int32, words
// 0 .. 6 CLEARED by the caller (added to), word 7 = H.  cspace_attitude: C [H][y][x] in place.
struct AttitudeVolumeParams {
    int xy, H;
    double wheelbase, track, belly_height;             // front_axle - rear_axle, track, belly_height
    float max_pitch, max_roll, min_clearance;
};
hipError_t gvom_launch_attitude_volume_table(hipStream_t s, int H, int total, double res, double axle_mid, const int32_t *fstart,
                                             const uint32_t *foffs, const double *wheels, const double *cos_sin, double *uv, int32_t *wcell);
hipError_t gvom_launch_attitude_volume(hipStream_t s, const AttitudeVolumeParams &P, const int32_t *fstart, const uint32_t *foffs,
                                       const double *uv, const int32_t *wcell, const double *ground, uint8_t *status, uint8_t *tilt,
                                       int32_t *counts);
hipError_t gvom_launch_cspace_attitude(hipStream_t s, int xy, int H, const uint8_t *status, const uint8_t *tilt, uint32_t block_mask,
                                       uint32_t tilt_weight, uint16_t *C);
// body volumes (gvom_body_volume.hip; include/gvom_hip.h "body volumes" defines the result).  P as k_body takes it, of which R.xy, R.H,
// R.ox, R.oy and R.res say what the window is (R.K, R.T and R.s are not read); wcell the attitude volume table's [H][12] int32; cos_sin,
// ground, body and field as k_body takes them.  status, squeeze [H][y][x] uint8 and clearance [H][y][x] float32; counts [8] int32, words
// 0 .. 5 CLEARED by the caller (added to), words 6 and 7 = H and S.
hipError_t gvom_launch_body_volume(hipStream_t s, const BodyParams &P, float soft_margin, const int32_t *wcell, const double *cos_sin,
                                   const double *ground, const float *body, const float *field, uint8_t *status, uint8_t *squeeze,
                                   float *clearance, int32_t *counts);
// map atlas (gvom_atlas.hip; include/gvom_hip.h "map atlas" defines the result).  The atlas is ten planes of A x A cells behind one
// base address, A a power of two: the six f64 maps of a set (maps 3 .. 8) at k * A*A doubles, then the three i32 maps (0 .. 2) and
// the int32 stamp at k * A*A ints; world cell (X, Y) at [(Y & (A-1)) * A + (X & (A-1))].  AtlasMaps = nine [y][x] maps of n x n cells
// in set order (i[0..2] the i32 maps 0 .. 2, f[0..5] the f64 maps 3 .. 8, as bit patterns) and a stamp map; the recall skips a null
// pointer.  Every window is given RELATIVE to the extent: rx, ry = window origin - extent origin (|.| <= 2^30, the host clamps), and
// by its storage phase px, py = window origin & (A-1).  cnt = the atlas's counters, int32: [0..5] of the last integrate {written,
// kept, uninformative, outside, made UNKNOWN by the move, of those known}, [6] cells of rank >= 1.
#define GVOM_ATLAS_MIN_CELLS 64
#define GVOM_ATLAS_MAX_CELLS 4096
struct AtlasMaps {
    int32_t *i[3];
    unsigned long long *f[6];
    int32_t *stamp;
};
inline size_t gvom_atlas_bytes(int A) { return (size_t)A * A * 64; }
hipError_t gvom_launch_atlas_fill(hipStream_t s, char *atlas, int A, size_t first, size_t n);
// move: the w x hgt cells from (rx, ry) / (px, py) on become UNKNOWN; counts them, and those that were known, into cnt[4], cnt[5], cnt[6]
hipError_t gvom_launch_atlas_move(hipStream_t s, char *atlas, int A, int px, int py, int w, int hgt, int32_t *cnt);
hipError_t gvom_launch_atlas_merge(hipStream_t s, char *atlas, int A, const AtlasMaps &in, int n, int rx, int ry, int px, int py,
                                   int32_t seq, int32_t *cnt);
// recall: n x n cells into `out`; counts (may be nullptr, else CLEARED by the caller) = {cells of rank 2, of rank 1, outside the extent, seq}
hipError_t gvom_launch_atlas_recall(hipStream_t s, const char *atlas, int A, const AtlasMaps &out, int n, int rx, int ry, int px, int py,
                                    int32_t seq, int32_t *counts);
// atlas fields (gvom_atlas_field.hip; include/gvom_hip.h "atlas fields" defines the result).  The first two read the atlas's planes in
// place through the extent's storage phase px, py = extent origin & (A-1) and write UNWRAPPED [y][x] arrays of A x A cells, extent cell
// (x, y) at [y*A + x]: clearance_rows = the row pass of gvom_launch_clearance (g: A*A uint16, the pitch is A), to be followed by
// gvom_launch_clearance_cols at side A; travcost = gvom_launch_travcost's cost map under the atlas's cell rule (d2 unwrapped, nullptr:
// no inflation).  field_window: the n x n cells from (rx, ry) RELATIVE to the field's corner (|.| <= 2^30) of the three [A][A] planes
// of a field into the three [n][n] planes of a cost field; INT32_MAX, 255 and 0 outside the field.
hipError_t gvom_launch_atlas_clearance_rows(hipStream_t s, const char *atlas, int A, int px, int py, bool use_negative, double thr,
                                            uint16_t *g);
hipError_t gvom_launch_atlas_travcost(hipStream_t s, const char *atlas, int A, int px, int py, const int32_t *d2, const CtgCostParams &C,
                                      uint16_t *c);
hipError_t gvom_launch_atlas_field_window(hipStream_t s, int A, const int32_t *fD, const uint8_t *fdir, const uint16_t *fc, int n, int rx,
                                          int ry, int32_t *oD, uint8_t *odir, uint16_t *oc);
// atlas frontiers (gvom_atlas_frontier.hip; include/gvom_hip.h "atlas frontiers" defines the result): gvom_launch_frontier_mark on the
// unwrapped [y][x] planes c and D of a field of xy x xy cells, the visibility read in place from the atlas of side A: field cell (x, y)
// is extent cell (ox + x, oy + y) (|ox|, |oy| <= 2^30; outside the extent a cell is neither known nor unknown), px, py the extent's
// storage phase.  L, count, flags and n_frontier as for gvom_launch_frontier_mark; relax, rows and finish follow at side xy.
hipError_t gvom_launch_atlas_frontier_mark(hipStream_t s, int xy, const uint16_t *c, const int32_t *D, const char *atlas, int A, int ox,
                                           int oy, int px, int py, uint32_t *L, uint32_t *count, uint32_t *flags, uint32_t *n_frontier);
// voxel atlas (gvom_voxel_atlas.hip; include/gvom_hip.h "voxel atlas" defines the result).  The atlas is A x A x Z voxels at 2 bits each,
// A and Z powers of two, behind one base address; the layout is that unit's own.  Every box of voxels is given RELATIVE to the extent:
// r = box origin - extent origin (|.| <= 2^30, the host clamps); pe* = extent origin & (size - 1), the storage phase of extent voxel 0.
// cnt = the atlas's counters, uint64 [16]: the slots below (two's complement sums; the host keeps what it can compute itself).
#define GVOM_VATLAS_MIN_CELLS 64
#define GVOM_VATLAS_MAX_CELLS 4096
#define VA_CNT_MOVED_OBS 7     // [0..4] of the last integrate {first seen, free -> occupied, occupied -> free, confirmed, uninformative}
#define VA_CNT_OBSERVED 8      // [7] observed voxels the last move cleared; [8], [9] observed / occupied voxels the atlas holds
#define VA_CNT_OCCUPIED 9
struct VAtlas {
    unsigned long long *pairs;
    int A, Z;
    int lgZ, lgP;             // log2 Z, log2 (A / 64)
};
inline size_t gvom_vatlas_bytes(int A, int Z) { return (size_t)A * A / 4 * Z; }
// merge: the window rows [y0, y0 + ny) and levels [z0, z0 + nz) that lie inside the extent; of the columns, the npx STORAGE pair columns
// from bx on (mod A/64) that hold the window's columns inside the extent; npairs = ny * nz * npx, the pairs the merge visits (the launcher holds the three to it).  F = the fused map's frame as
// k_occupancy takes it.  Adds to cnt[0..4], cnt[8], cnt[9].
struct VAtlasWindow {
    int y0, ny, z0, nz;
    int rx, ry, rz;
    int pex, pey, pez;
    int bx, npx;
    uint32_t npairs;
};
// move: the pairs of storage rows [ys, ys + ny) mod A and levels [zs, zs + nz) mod Z lose the bits of storage columns [xs, xs + wx) mod A;
// npairs = ny * nz * (A / 64).  Adds the observed voxels it clears to cnt[7] and takes what it clears from cnt[8], cnt[9].
struct VAtlasSlab {
    int ys, ny, zs, nz, xs, wx;
    uint64_t npairs;
};
// box: n x n x zs voxels from r on, p* = box origin & (size - 1); out[x][y][z] uint8 = 0 never observed (and outside the extent), 1
// observed free, 2 occupied; counts int32 [4], words 0 and 1 CLEARED by the caller (added to) = {occupied, free}, words 2 and 3 =
// outside, seq as given.  zc, yb: the launcher's.
struct VAtlasBox {
    int n, zs;
    int rx, ry, rz;
    int px, py, pz;
    int outside, seq;
    int zc, yb;
};
hipError_t gvom_launch_vatlas_merge(hipStream_t s, const VAtlas &V, const VAtlasWindow &D, const OccParams &F, const int32_t *fstate,
                                    const uint32_t *ftags, unsigned long long *cnt);
hipError_t gvom_launch_vatlas_move(hipStream_t s, const VAtlas &V, const VAtlasSlab &S, unsigned long long *cnt);
hipError_t gvom_launch_vatlas_box(hipStream_t s, const VAtlas &V, VAtlasBox B, uint8_t *out, int32_t *counts);
// the same box (n, zs, r*, p*; the other fields are not read) as the class grid of scan alignment scoring, gvom_align_grid_bytes(n, zs)
// of it, in k_align_field's layout and codes: what gvom_launch_align_grid scores against.  A voxel's class is the atlas's alone (NEAR
// looks at the extent's voxels outside the box too); a box voxel outside the extent is UNKNOWN.
hipError_t gvom_launch_vatlas_align_field(hipStream_t s, const VAtlas &V, const VAtlasBox &B, int dilate, uint32_t *grid);
// the walks: P = gvom_launch_raycast's frame with the extent in the window's place (origin = E, xy = A, zs = Z, om = E & (size - 1)), Q as
// there with cap = A + Z.  raycast: out3 [n][3] = {status, steps, unknown}, pos3 [n][3] the stop position in metres, vox3 [n][3] the world
// voxel of the stop.  viewpoints / viewpoint_best: as gvom_launch_viewpoints / _viewpoint_best; boxes [K][8] int32 = {lx, ly, lz, dx, dy,
// dz, 0, 0}, the box of extent voxels of every pose (inside the extent, dx * dy * dz <= 32 * Q.bm_words).
hipError_t gvom_launch_vatlas_raycast(hipStream_t s, const ScanParams &P, const RayQuery &Q, const VAtlas &V, int32_t *out3, float *pos3, int32_t *vox3);
hipError_t gvom_launch_vatlas_viewpoints(hipStream_t s, const ScanParams &P, const ViewQuery &Q, const VAtlas &V, int batch, const int32_t *boxes,
                                         uint32_t *bitmaps, int32_t *rows);
hipError_t gvom_launch_vatlas_viewpoint_best(hipStream_t s, const ScanParams &P, const ViewQuery &Q, const VAtlas &V, int32_t *rows, int32_t *best);
// voxel atlas changes (gvom_voxel_changes.hip; include/gvom_hip.h "voxel atlas changes" defines the result).  B = the WINDOW as the box
// kernels take a box (n, zs, r*, p*; the other fields are not read), F, fstate, ftags = the fused map as the merge takes it.
// planes: gvom_vchange_planes_bytes(n, zs) of 16-byte words {appeared, vanished}, word ((y * zs + z) * nseg + q) = columns 64 q .. 64 q + 63
// of window row y and level z, nseg = ceil(n / 64); cnt uint64 [3], CLEARED by the caller = {appeared, vanished, outside the extent}.
// codes: out uint8 [n][n][zs] = 0 / 1 appeared / 2 vanished.  columns: cols uint16 [2][n][n] (appeared / vanished voxels per column,
// [y][x] inside a plane), lohi uint32 [n][n] = lowest | highest << 16 of the levels whose code is in mask; L, count, flags, n_marked as
// for gvom_launch_frontier_mark; D int32 [n][n] = squared cells to cell (n / 2, n / 2); rows4 int32 [cap][4] initialised.  clusters
// (behind gvom_launch_frontier_finish): cmap = its cluster map, totals = its totals; rows4 = {appeared, vanished, lowest, highest level}
// per kept rank below cap, zero beyond; counts[4 .. 7] = cnt[0 .. 2] (saturated to int32), seq.
size_t gvom_vchange_planes_bytes(int n, int zs);
hipError_t gvom_launch_vchange_planes(hipStream_t s, const VAtlas &V, const VAtlasBox &B, const OccParams &F, const int32_t *fstate,
                                      const uint32_t *ftags, void *planes, unsigned long long *cnt);
hipError_t gvom_launch_vchange_codes(hipStream_t s, int n, int zs, const void *planes, uint8_t *out);
hipError_t gvom_launch_vchange_columns(hipStream_t s, int xy, int zs, int mask, int cap, const void *planes, uint16_t *cols, uint32_t *lohi,
                                       uint32_t *L, uint32_t *count, uint32_t *flags, uint32_t *n_marked, int32_t *D, int32_t *rows4);
hipError_t gvom_launch_vchange_clusters(hipStream_t s, int xy, int cap, int seq, const int32_t *cmap, const uint16_t *cols, const uint32_t *lohi,
                                        const uint32_t *totals, const unsigned long long *cnt, int32_t *rows4, int32_t *counts);
// voxel distance fields (gvom_voxel_distance.hip; include/gvom_hip.h "voxel distance field" defines the result).  B = the box as the box
// kernels take it (n, zs, r*, p*, outside, seq).  The passes in y and z run on the box GROWN by the halo where a source can lie: hby rows
// below the box, nyg rows in all (>= hby + n); hbz levels below, nzg in all.  kx = 64-bit words the x pass searches on either side, hxy =
// the y walk's cap; a, b = fl64(resolution^2) of xy and z; cap2 = fl64(max_distance^2); nw = ceil(n / 64).
#define GVOM_VDIST_MAX_HALO 32767               // the halo of a cap, in voxels: squared offsets and their sums of two stay below 2^32
struct VDistFrame {
    VAtlasBox B;
    int hby, nyg, hbz, nzg;
    int kx, hxy, nw;
    int unknown;              // GVOM_DISTANCE_UNKNOWN_BLOCKS: NEVER voxels are sources
    double a, b, cap2;
};
// sample: n points against the field float32 [n][n][zs] of the box whose corner is world voxel `origin`
struct VDistSample {
    double xy_res, z_res;
    double origin[3];
    int n, zs;
    int64_t npts;
};
size_t gvom_vdist_rows_bytes(const VDistFrame &F);            // the x pass's output; 256-byte aligned behind it:
size_t gvom_vdist_cols_bytes(const VDistFrame &F);            // the y pass's output
// work = the two buffers above; out float32 [n][n][zs] metres (+inf beyond the cap); counts int32 [4], words 0 and 1 CLEARED by the caller
// = {voxels at 0, voxels with a finite distance}, words 2 and 3 = B.outside, B.seq
hipError_t gvom_launch_vdist_field(hipStream_t s, const VAtlas &V, const VDistFrame &F, void *work, float *out, int32_t *counts);
// out float32 [npts] = the field at the voxel of every point, NaN outside the box or where a coordinate is not finite; counts int32 [4]
// CLEARED by the caller = {inside the box, of those finite, of those 0, npts}
hipError_t gvom_launch_vdist_sample(hipStream_t s, const VDistSample &Q, const float *pts, const float *field, float *out, int32_t *counts);
// storage order [sy][sx] -> reference order [x][y] (window coordinates)
hipError_t gvom_launch_unwrap_f64(hipStream_t s, int xy, int om0, int om1, const double *in, int in_stride, double *out_xy);
hipError_t gvom_launch_posdens(hipStream_t s, const Map2dParams &P, const int32_t *fstate,
                               const uint32_t *ftags, const uint4 *frows,
                               double *hmaps, const uint32_t *blockcounts, int nblocks,
                               unsigned long long *host_counter, unsigned long long *dev_counter);
hipError_t gvom_launch_debug_height(hipStream_t s, int xy, int om0, int om1, const double origin[3], double xy_res,
                                    double z_res, const double *height, int hs, const double *rough,
                                    const double *sx, const double *sy, float *out7,
                                    const double *guessed, float *out3);
