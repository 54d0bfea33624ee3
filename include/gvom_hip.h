/*
 * gvom_hip.h -- C ABI of libgvom_hip.so: the MI355X (gfx950) implementation of G-VOM's
 * process_pointcloud -> combine_maps hot path.
 *
 * This is the drop-in boundary.  The reference has no FFI of its own (it is a Python class
 * that launches Numba-CUDA kernels); each entry point below replaces one *method* of the
 * reference class `Gvom` (/root/reference/scripts/gvom.py, "gvom.py:NNN") and is bound
 * from Python with ctypes by g-vom_amd/gvom.py (see INTEGRATION.md for the stub).
 * Plain pointers and sizes only; no PyTorch / numpy types.  All functions are
 * thread-safe per handle (an internal mutex replaces the reference's semaphores,
 * gvom.py:65-67,96); ctypes drops the GIL around every call.
 *
 * Array conventions at this boundary are the REFERENCE's:
 *   voxel arrays : index = x + y*xy_size + z*xy_size*xy_size        (gvom.py:1086,1146)
 *   2-D maps     : [x][y] C-order, i.e. m[x*xy_size + y]            (gvom.py:288-349)
 * (internally the library stores voxels world-anchored/toroidal as [y][z][x] and 2-D
 * maps as [y][x]; see DESIGN.md.)
 */
#ifndef GVOM_HIP_H
#define GVOM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GVOM_ABI_VERSION 10  /* 10: device-resident 3-D products (gvom_device_product and its export / release / DLPack / copy calls: occupancy
                              *    grid, voxel cloud, height clouds), "device_product_sets"; gvom_get_occupancy runs k_occupancy;
                              * 9: device-resident maps (gvom_combine_maps_device, map-set exports, DLPack), "device_map_sets";
                              * 8: RCCL loopback transport (GVOM_TRANSPORT_LOOPBACK), gvom_comm_wire_stats, gvom_comm_abort;
                              * 7: eager fusion of one-slot rings ("eager" knob, gvom_get_tuning "eager_adopted" / "eager_dropped"); a sharded scan /
                              *    combine as ONE native call (gvom_comm_process_pointcloud, gvom_comm_combine_maps_into);
                              * 6: sub-cloud interleave of the trace ("interleave" knob, automatic by a layout probe), gvom_get_tuning;
                              *    peer transport absorbs refused exports / imports (gvom_shard_renew_region, gvom_comm_peer_renewed), gvom_comm_info;
                              * 5: second transport between ranks (peer copies: gvom_comm_create2, gvom_comm_transport),
                              *    gvom_alloc_generation;
                              * 4: per-voxel statistics on sharded maps (gvom_shard_stats_*, gvom_comm_exchange_stats);
                              * 3: rank-exchange (shard) and communicator entry points, gvom_set_tuning, flags;
                              *    2: *_into outputs column-major; occupancy and PointCloud2 entry points */

/* return codes (>= 0: the reference's documented outcomes; < 0: failures) */
#define GVOM_OK                0
#define GVOM_EMPTY_CLOUD       1   /* gvom.py:107-109 "[WARNING] Processing an empty pointcloud..." */
#define GVOM_NO_OVERLAP        2   /* gvom.py:148-150 "[WARNING] The pointcloud points don't overlap..." */
#define GVOM_EMPTY_BUFFER      3   /* gvom.py:179-181 "[WARNING] The map buffer is empty..." */
#define GVOM_NO_DATA           4   /* gvom.py:364-366,381-383,397-399 "No data" */
#define GVOM_ERR_INVALID      -1   /* bad argument */
#define GVOM_ERR_HIP          -2   /* a HIP runtime call failed; see gvom_last_error() */
#define GVOM_ERR_NO_DEVICE    -3   /* no usable gfx950 device / library built without GPU */
#define GVOM_ERR_CAPACITY     -4   /* grid too large for 32-bit voxel indices, or > 64 ring slots, or every device map / product set (of a kind) exported */

#define GVOM_DTYPE_F32 0
#define GVOM_DTYPE_F64 1

typedef struct gvom_handle gvom_t;

/* The 14 positional constructor arguments of Gvom.__init__ (gvom.py:29-31), same order. */
typedef struct gvom_params {
    double  xy_resolution;
    double  z_resolution;
    int32_t xy_size;
    int32_t z_size;
    int32_t buffer_size;
    int32_t reserved0;             /* flags: GVOM_FLAG_* */
    double  min_distance;
    double  positive_obstacle_threshold;
    double  negative_obstacle_threshold;
    double  slope_obstacle_threshold;
    double  robot_height;
    double  robot_radius;
    double  ground_to_lidar_height;
    int32_t xy_eigen_dist;
    int32_t z_eigen_dist;
} gvom_params;

/* gvom_params.reserved0 flags */
#define GVOM_FLAG_VOXEL_STATISTICS 1   /* also run the per-voxel mean/covariance path (gvom.py:1172-1299,
                                        * 858-909, 1333-1378) that feeds only make_debug_voxel_map; off by
                                        * default: it is not on the north-star path and costs scan time.
                                        * The environment variable GVOM_VOXEL_STATISTICS=0/1 overrides. */
#define GVOM_FLAG_STATISTICS_ON_DEMAND 4 /* (unsharded handles, ignored with GVOM_FLAG_VOXEL_STATISTICS) the per-voxel path runs
                                        * WHILE SOMEBODY READS IT: it starts on -- the reference computes it in every scan and
                                        * combine and its node reads it every tick (gvom_ros.py:171) -- and goes off AT THE FOURTH
                                        * COMBINE IN A ROW that no read preceded: that combine merges no statistics, and their
                                        * buffers go back to the allocator (40 bytes per voxel and fused map alone).  A READ is a
                                        * call of gvom_gather_metrics, gvom_debug_voxel_map, gvom_debug_voxel_eigen or
                                        * gvom_device_product(GVOM_PRODUCT_VOXEL_CLOUD), whatever it returns; gvom_read_rows,
                                        * gvom_read_dense and every other call are not.  Only combines that find a filled last
                                        * slot count; rejected scans change nothing.  The path comes back with the next read:
                                        * that call returns GVOM_NO_DATA, the scans accepted after it carry statistics (a slot's
                                        * can be read at once), and the fused map has them from the first combine at which every
                                        * filled ring slot does.  They then RESTART FROM THE RING: a previous map without
                                        * statistics contributes its hit counts and minimum heights and nothing else, so a voxel
                                        * that only such a map knows has an all-zero statistics row (count 0) until a scan with
                                        * statistics reaches its neighbourhood; a previous row of count 0 merges no statistics
                                        * at later combines either (the reference's merge, gvom.py:858-909, would divide 0 by 0).
                                        * What the map had merged before the pause is not in them.  A reader of every fourth
                                        * combine or fewer therefore never gets data.  g-vom_amd/gvom.py's default. */
#define GVOM_FLAG_NUMBA_CUDA_TYPING 2  /* the types Numba 0.54.1 infers for a REAL CUDA device where they differ from its simulator's
                                        * (profiles/numba_cuda_typing.txt: its type inference with the CUDA target's typing context
                                        * over gvom.py:1060-1150, 1303-1329): ray_length = math.sqrt(float32) is
                                        * float32 (gvom.py:1109), slope[k] / ray_length is float32 / float32 (:1112-1114) and the loop
                                        * bound is that float32 minus 1 in float64 (:1127) -- every other difference (math.floor
                                        * giving float64, the voxel index carried as float64) is value-neutral.  Default (flag
                                        * clear): the float64 square root of Numba's simulator, which is what the golden fixtures
                                        * were generated with.  What NO flag reproduces: NVVM's default contraction of a*b + c into
                                        * FMAs on a real device (code generation, not typing; unpinnable without one). */
#define GVOM_FLAG_CUDA_F32_SQRT    GVOM_FLAG_NUMBA_CUDA_TYPING   /* (its name before ABI 8) */

/* Ring-buffer bookkeeping visible on the reference object (gvom.py:56-58,172-175). */
typedef struct gvom_state {
    int32_t buffer_index;
    int32_t last_buffer_index;
    int32_t has_combined;          /* combine_maps has produced a fused map at least once */
    int32_t reserved0;
    int64_t combined_cell_count;   /* gvom.py:217 combined_cell_count_cpu (valid if has_combined) */
    double  combined_origin[3];    /* gvom.py:184 (voxel units, integer valued) */
    double  ego_position[3];       /* gvom.py:102-104 latest ego */
} gvom_state;

/* Exact integer accounting of the last accepted scan (used for roofline arithmetic). */
typedef struct gvom_scan_stats {
    int64_t points;                /* N */
    int64_t cells;                 /* C: occupied voxels of the scan (gvom.py:147 cell_count_cpu) */
    int64_t sum_hit;               /* sum of hit over the scan's voxels  */
    int64_t sum_total;             /* sum of total over the scan's voxels (endpoint adds included) */
} gvom_scan_stats;

/* --- lifetime: replaces Gvom.__init__ (gvom.py:29-97) ------------------------------------ */
int  gvom_create(const gvom_params *params, int device_id, gvom_t **out);
/* One rank of a map sharded over `world` GPUs (see "one map sharded over the GPUs of a node" below). */
int  gvom_create_sharded(const gvom_params *params, int device_id, int rank, int world,
                         gvom_t **out);
void gvom_destroy(gvom_t *h);

/* --- Gvom.process_pointcloud (gvom.py:99-175) ---------------------------------------------
 * xyz: N rows of >= 3 consecutive float32/float64 (row_stride_bytes apart), host memory for
 * gvom_process_pointcloud, device (HBM) memory for the *_device variant.  The cloud is never
 * modified.  transform: row-major 4x4 double or NULL (gvom.py:134-135).
 * Returns GVOM_OK / GVOM_EMPTY_CLOUD / GVOM_NO_OVERLAP (ring untouched, ego still updated). */
int gvom_process_pointcloud(gvom_t *h, const void *xyz, int64_t n, int64_t row_stride_bytes,
                            int dtype, const double ego[3], const double *transform_4x4);
int gvom_process_pointcloud_device(gvom_t *h, const void *xyz_dev, int64_t n,
                                   int64_t row_stride_bytes, int dtype, const double ego[3],
                                   const double *transform_4x4);

/* Ingest side of the ROS node (gvom_ros.py:93-109): scans the packed bytes of a
 * sensor_msgs/PointCloud2 directly -- `data` holds n_points (= width*height, no row padding)
 * records of point_step bytes with little-endian fields x, y, z of type `dtype` (GVOM_DTYPE_F32 =
 * PointField.FLOAT32, GVOM_DTYPE_F64 = FLOAT64) at byte offsets off_x/off_y/off_z (multiples of
 * the field size).  Replaces ros_numpy.point_cloud2.pointcloud2_to_xyz_array + process_pointcloud;
 * records with a non-finite coordinate (which ros_numpy removes) have no effect on the map.
 * Same return codes as gvom_process_pointcloud. */
int gvom_process_pointcloud2(gvom_t *h, const void *data, int64_t n_points, int64_t point_step,
                             int64_t off_x, int64_t off_y, int64_t off_z, int dtype,
                             const double ego[3], const double *transform_4x4);

/* --- range images (an extension: the scan as a spinning multi-beam lidar emits it) -------------------------------------------
 * An Ouster-class sensor delivers H beams x W columns of raw ranges (0 = no return) and a fixed per-pixel lookup table -- a unit
 * direction and a small offset -- that turns a range into a point.  gvom_sensor_model_set hands the table over once;
 * gvom_process_range_image then takes the raw image (2 or 4 bytes per pixel instead of 12 or 24 per return, the same length
 * every scan, beam-major by construction) and unprojects it on the GPU (k_unproject, one launch in front of the scan).
 *
 * SENSOR MODEL, per handle, replaceable at any time between scans: H, W >= 1 with H*W < 2^31; dir and off: float64 [H*W][3],
 * pixel i = h*W + w (off may be NULL: zeros); range_scale: metres per raw unit (finite, > 0); min_range <= r <= max_range
 * (metres, inclusive; 0 and +infinity accept everything).  The arrays are copied to device memory inside the call (the caller
 * may free them on return); a model that replaces another is ordered behind every scan that read the old one.
 * gvom_get_tuning "range_image" (read-only): 1 when a model is set, else 0 -- which is also how a caller probes a library of
 * this ABI version for the two entry points.
 *
 * SCAN: raw[H][W], row-major, rows row_stride_bytes apart (>= a row, a multiple of the element size), of GVOM_RANGE_U16 /
 * _U32 / _F32, in host memory (on_device == 0; uploaded like a host cloud) or device memory (a device pointer, nothing is
 * copied; as for gvom_process_pointcloud_device the data must be ready when the call is made).  col_poses: NULL, or float64
 * [W][12] in HOST memory, one row-major 3x4 per column (the de-skew of a sweep: column w was measured at pose C[w]).  cloud_dtype:
 * GVOM_DTYPE_F32 / _F64, the type T of the cloud the scan runs on.  For pixel i = h*W + w, in float64, every operation rounded
 * once, in exactly this order (no fused multiply-add):
 *     r      = (double)raw[i] * range_scale
 *     valid  = raw[i] != 0  and  r is finite  and  min_range <= r <= max_range
 *     p[k]   = r * dir[i][k] + off[i][k]                                   k = 0, 1, 2   (multiply, then add)
 *     q[k]   = ((p[0]*C[w][4k] + p[1]*C[w][4k+1]) + p[2]*C[w][4k+2]) + C[w][4k+3]        (with col_poses; else q = p)
 *     xyz[i] = (T) q   for valid pixels,   (NaN, NaN, NaN)   for the others
 * and the call IS gvom_process_pointcloud_device(xyz, H*W, 3*sizeof(T), T, ego, transform_4x4): its return codes (an image
 * without a valid pixel is GVOM_NO_OVERLAP, as an all-NaN cloud is), ring behaviour, gvom_get_scan_stats (points = H*W),
 * eager fusion, statistics and layout probe.  GVOM_ERR_INVALID: no model set, a bad range_dtype / cloud_dtype / row stride,
 * and on a SHARDED handle (range images are not split over ranks). */
int gvom_sensor_model_set(gvom_t *h, int32_t H, int32_t W, const double *dir, const double *off /* may be NULL */,
                          double range_scale, double min_range, double max_range);
#define GVOM_RANGE_U16 0
#define GVOM_RANGE_U32 1
#define GVOM_RANGE_F32 2
int gvom_process_range_image(gvom_t *h, const void *raw, int on_device, int range_dtype, int64_t row_stride_bytes,
                             const double *col_poses /* host, W*12, may be NULL */, int cloud_dtype,
                             const double ego[3], const double *transform_4x4);

/* --- multi-origin scans (an extension: every return traced from its own sensor position) -------------------------------------
 * The scan calls above trace every ray from `ego`, which also places the window.  A de-skewed sweep (the sensor moved while it
 * turned) and a vehicle with several lidars have returns that were measured from DIFFERENT places: here return i is traced from
 * origins[index[i]].  `ego` keeps every other role: window origin, gvom_state.ego_position, the robot-radius fill of the fusion,
 * the return codes.
 *
 * gvom_process_pointcloud_origins is gvom_process_pointcloud (on_device == 0) / gvom_process_pointcloud_device (else) with
 * gvom.py:1097-1099 replaced, for return i, by
 *     k = index[i];  pt[0] = (float)(O[k][0] / xy_resolution);  pt[1] = (float)(O[k][1] / xy_resolution);  pt[2] = (float)(O[k][2] / z_resolution)
 * (float64 division, one rounding to float32: what the host does for `ego`).  Endpoint, min-height, the min-distance test (from
 * the WORLD origin), the transform of the cloud, ring commit, GVOM_EMPTY_CLOUD / GVOM_NO_OVERLAP, statistics and eager fusion are
 * unchanged, with the window computed from `ego`.  origins: HOST float64 [K][3], 1 <= K <= 65536, finite, world frame (the
 * frame of `ego`: transform_4x4 is NOT applied to them).  index: uint16 [n] in the memory the cloud is in (host when
 * on_device == 0, else device), or NULL: index[i] = i % K.  The reference's own behaviour for an unusual ray start follows: an
 * origin outside the window contributes endpoints only (its first step is outside), an origin equal to its return takes no step.
 * GVOM_ERR_INVALID: K out of range, a non-finite origin, a HOST index entry >= K (checked before anything is enqueued: the ring
 * is untouched), and on a SHARDED handle (multi-origin scans are not split over ranks).  A DEVICE index cannot be checked by the
 * host: a return with index[i] >= K has no effect at all -- no endpoint, no ray, no table row read.
 * The step segments of k_trace are sized from the origins at hand; the layout probe, "dirsort" and "interleave" -- which order
 * returns by direction seen from ONE sensor position -- do not run on this route, forced or not (gvom_get_tuning reports
 * interleave 1, dirsort 0 after such a scan).  gvom_get_tuning "multi_origin" (read-only): 1 -- how a caller probes a library of
 * this ABI version for the two entry points; "multi_origin_ran": 1 when the LAST scan ran the per-lane-origin trace.
 *
 * gvom_process_range_image_origins is gvom_process_range_image with every pixel traced from its COLUMN's sensor position.
 * col_poses is required (GVOM_ERR_INVALID without; also for W > 65536).  O[w] is the translation of C[w] taken through
 * transform_4x4 in the cloud transform's order, in float64, on the host:
 *     t = (C[w][3], C[w][7], C[w][11]);   O[w][k] = ((t0*tf[4k] + t1*tf[4k+1]) + t2*tf[4k+2]) + tf[4k+3]   (O[w] = t without a transform)
 * and the call IS gvom_process_pointcloud_origins on the unprojected cloud with origins = O, K = W, index = NULL (pixel
 * i = h*W + w: i % W = w).  The per-pixel offsets off[i] of the sensor model are not part of a ray's start. */
int gvom_process_pointcloud_origins(gvom_t *h, const void *xyz, int on_device, int64_t n, int64_t row_stride_bytes, int dtype,
                                    const double *origins /* host, K*3 */, int32_t K, const uint16_t *index /* may be NULL */,
                                    const double ego[3], const double *transform_4x4);
int gvom_process_range_image_origins(gvom_t *h, const void *raw, int on_device, int range_dtype, int64_t row_stride_bytes,
                                     const double *col_poses /* host, W*12, required */, int cloud_dtype,
                                     const double ego[3], const double *transform_4x4);

/* --- Gvom.combine_maps (gvom.py:177-354) --------------------------------------------------
 * Caller-allocated xy_size*xy_size outputs (any of them may be NULL to skip its copy).
 * Returns GVOM_OK or GVOM_EMPTY_BUFFER. */
/* Note on very long runs: the fused map carries its predecessor's free (ray-pass) counts along (gvom.py:996); they
 * are held as -count - 1 in int32 states and stop at 2^30 here (the reference's wrap into the row-index range). */
int gvom_combine_maps(gvom_t *h, double origin_world[3], int32_t *positive, int32_t *negative,
                      double *roughness, int32_t *visibility);

/* Zero-copy variant of combine_maps: the four maps are written by the GPU straight into a
 * pinned, device-mapped host buffer obtained from gvom_output_buffer_alloc (20*xy*xy bytes:
 * [positive i32 | negative i32 | visibility i32 | roughness f64]).  Unlike gvom_combine_maps,
 * each map is stored COLUMN-MAJOR: cell (x, y) at m[y*xy_size + x] -- the Fortran-ordered form of
 * the reference's [x, y]-indexed arrays, which is what gvom_ros.py:141-162 reads
 * (np.reshape(map, -1, order='F')); the GPU writes it as contiguous runs without a transpose and
 * streams each map out as soon as it is known.  The caller owns the buffer (and may keep several alive) until gvom_output_buffer_free.
 * COHERENCE: the synchronous calls learn of completion from a flag k_map2d's last workgroup stores behind its maps (every wave waits
 * for its stores to be acknowledged first), not from a stream synchronisation.  That is sound for COHERENT (fine-grained) pinned
 * memory, which is what gvom_output_buffer_alloc returns (hipHostMallocMapped | hipHostMallocCoherent): system-scope stores are
 * written through.  A buffer of the caller's own must be allocated the same way; gvom_combine_maps_into /
 * gvom_combine_occupancy_into / gvom_combine_begin / gvom_combine_map2d_into (and gvom_comm_combine_maps_into through it)
 * refuse (GVOM_ERR_INVALID) a pinned buffer whose flags say otherwise. */
int gvom_output_buffer_alloc(gvom_t *h, void **host_ptr);
int gvom_output_buffer_free(gvom_t *h, void *host_ptr);
int gvom_combine_maps_into(gvom_t *h, double origin_world[3], void *pinned_out);
/* ONLY WHAT CHANGED IS STORED.  Most of a window is empty, and an empty cell gets the same four values every combine (visibility 0,
 * positive 0, negative 0, roughness -1.0).  For every buffer from gvom_output_buffer_alloc the library therefore keeps a CONTENT
 * RECORD -- in device memory, one bit per map and run of 32 cells in x -- of where it last stored anything else, and
 * gvom_combine_maps_into / gvom_combine_begin (occ == NULL) do not store a run again that holds only those values now and held
 * only those values the last time the library wrote THAT buffer.  The buffer's contents after the call are exactly what a full
 * store leaves.  The first combine into a buffer stores everything, and so does the first one after anything else has written it
 * through the library (the occupancy grids, gvom_combine_map2d_into) or after the record was dropped (at most 8 buffers per
 * handle have one; the one used longest ago goes).  A buffer of the caller's own allocation is always stored in full.
 * THE CALLER'S SIDE: a recorded buffer must have no writer but the library.  Whoever writes into it and hands it to a later
 * combine calls gvom_output_forget first (any pointer is accepted; the next combine into it stores every run), or switches
 * the record off for the handle: gvom_set_tuning "delta_out" 0.
 * gvom_output_record (measurements, tests): the record of `host_ptr` as the kernel keeps it -- one byte per 32 (x) x 8 (y) tile
 * and wave of k_map2d, tile-row-major, wave w < 4: rows 2 w, 2 w + 1 of the tile, bits 0 / 1 visibility, 2 / 3 roughness; wave
 * w >= 4: rows 2 (w - 4), + 1, bits 0 / 1 positive, 2 / 3 negative; a set bit = the run holds non-default values.  Waits for the
 * handle's work, copies *n = ceil(xy/32) * ceil(xy/8) * 8 bytes to `bits` (NULL: only *n and *generation are set; cap < *n:
 * GVOM_ERR_CAPACITY).  *generation changes whenever the record restarts (all runs stored).  GVOM_NO_DATA: no record. */
int gvom_output_forget(gvom_t *h, void *host_ptr);
int gvom_output_record(gvom_t *h, void *host_ptr, uint8_t *bits, size_t cap, size_t *n, uint64_t *generation);

/* combine_maps fused with the ROS node's post-processing (gvom_ros.py:141-165):
 * advances the fusion exactly like gvom_combine_maps, but the GPU writes the five int8
 * nav_msgs/OccupancyGrid.data arrays the node publishes into the pinned buffer (from
 * gvom_output_buffer_alloc), as planes of xy*xy bytes, cell (x, y) at [y*xy_size + x]:
 *   0 hard obstacles   max(100*(positive > density_threshold), negative)          :141
 *   1 soft obstacles   100*(positive <= density_threshold)*(positive > 0)         :146
 *   2 ground certainty visibility*100                                             :151
 *   3 negative         negative                                                   :157
 *   4 roughness        ((clip(r, min, max) + min)/(max - min))*100, cast to int8 as numpy does  :162-163
 * (reproduced as written, including the "+ min" and the wrapping cast). */
int gvom_combine_occupancy_into(gvom_t *h, double origin_world[3], void *pinned_out,
                                double density_threshold, double min_roughness, double max_roughness);

/* Asynchronous combine (an extension: the reference's combine_maps, gvom.py:177-354, is synchronous).
 * gvom_combine_begin enqueues what gvom_combine_maps_into (occ == NULL) or gvom_combine_occupancy_into
 * (occ = {density_threshold, min_roughness, max_roughness}) computes and returns without waiting;
 * gvom_combine_end waits for the maps and completes the call (the fused cell count, origin_world).
 * Between the two the caller may hand the NEXT scan to gvom_process_pointcloud*: its kernels run while
 * the maps of this combine are stored to host memory (k_map2d runs on a second stream; the next fusion
 * waits for it on the device).  `pinned_out` must not be read before gvom_combine_end has returned.
 * One combine may be pending per handle; the synchronous combine entry points return GVOM_ERR_INVALID
 * while one is (and gvom_combine_begin does while another thread waits inside a synchronous combine;
 * synchronous combines of several threads simply queue up).  Results are those of the synchronous calls. */
int gvom_combine_begin(gvom_t *h, void *pinned_out, const double *occ);
int gvom_combine_end(gvom_t *h, double origin_world[3]);

/* --- device-resident maps (an extension: for consumers that run on the GPU too, e.g. a sampling planner) -----------------
 * gvom_combine_maps_device advances the fusion exactly like gvom_combine_maps (eager adoption, statistics on demand, ring) but
 * k_map2d writes a MAP SET in device memory instead of host memory, and the call returns once the work is ENQUEUED (no host
 * wait).  A set holds nine xy*xy maps of the combine, each COLUMN-MAJOR like gvom_combine_maps_into's (cell (x, y) at
 * [y*xy_size + x]; element strides {1, xy_size} for [x, y] indexing), bit-identical to what the host routes return:
 *   0 positive i32   1 negative i32   2 visibility i32   3 roughness f64          (the four returned maps)
 *   4 height f64     5 inferred height f64   6 x slope f64   7 y slope f64   8 guessed height delta f64
 *                                                              (the attributes gvom_read_map2d reads, unwrapped)
 * *set_id names the set (a sequence number); GVOM_EMPTY_BUFFER as gvom_combine_maps.  GVOM_ERR_INVALID on a sharded handle
 * or while a gvom_combine_begin is pending.  60 bytes per cell and set, at most 8 sets per handle ("device_map_sets" of
 * gvom_get_tuning: how many are allocated); a combine that needs a ninth returns GVOM_ERR_CAPACITY.  A set nobody holds an
 * export of goes back to the pool when the next device combine begins (its id is stale from then on).  The fused cell
 * count (gvom_get_state) is read once the combine's kernels have completed: the first call that needs it waits for them. */
int gvom_combine_maps_device(gvom_t *h, double origin_world[3], int64_t *set_id);
/* Consumer streams: a hipStream_t as void* (NULL: the null stream), or GVOM_STREAM_NOSYNC -- no ordering at all (the caller
 * synchronises on its own; its release records nothing). */
#define GVOM_STREAM_NOSYNC ((void *)(intptr_t)-1)
/* EXPORT map `which` (0..8) of a set to `consumer_stream`: the stream waits on the set's completion (hipStreamWaitEvent, no host
 * wait) and the set's export count goes up.  *ptr = the map's device address, strides = {1, xy_size} elements. */
int gvom_device_map_export(gvom_t *h, int64_t set_id, int which, void *consumer_stream, void **ptr, int64_t strides[2]);
/* End one export: an event is recorded on `consumer_stream` behind whatever reads it has queued, and the count goes down.  A set
 * is reused only when its count is 0, and the combine that reuses it first makes the handle's stream wait on every release
 * event of the set -- a consumer may queue reads and release at once.  Exports OUTLIVE the handle: a set with live exports
 * stays valid after gvom_destroy and is freed at its last release (through a DLPack deleter then). */
int gvom_device_map_release(gvom_t *h, int64_t set_id, void *consumer_stream);
/* DLPack: an export of map `which` to `consumer_stream` wrapped as a DLManagedTensorVersioned (versioned = 1, DLPack 1.0) or a
 * legacy DLManagedTensor (0): kDLROCM, this handle's device, shape {xy, xy}, strides {1, xy}, int32 or float64.  Its deleter
 * (C code of this library, no Python and no GIL needed, callable from any thread and after gvom_destroy) performs the release
 * on that stream.  Unused managed tensors must be deleted through their deleter as well. */
int gvom_device_map_dlpack(gvom_t *h, int64_t set_id, int which, void *consumer_stream, int versioned, void **managed);
/* Blocking copy of map `which` of a set into host memory (xy*xy elements, [y*xy_size + x]). */
int gvom_device_map_copy(gvom_t *h, int64_t set_id, int which, void *host_out);

/* --- device-resident 3-D products (an extension: the occupancy grid and the debug clouds for consumers on the GPU) ----------
 * gvom_device_product writes one PRODUCT into device memory on the handle's stream and returns once the work is ENQUEUED (no
 * host wait, no copy).  A product is a SNAPSHOT -- of the current fused map (occupancy, voxel cloud) or of the 2-D maps of the
 * last combine (the height clouds) -- that later scans and combines do not change.  Kinds, parts and layouts (all C-contiguous):
 *   GVOM_PRODUCT_OCCUPANCY              part 0  uint8 [xy, xy, z]   1 = occupied: what gvom_get_occupancy returns (k_occupancy)
 *   GVOM_PRODUCT_VOXEL_CLOUD            part 0  float32 [cap, 8]    the rows of gvom_debug_voxel_map, in unspecified order
 *                                       part 1  float32 [cap, 3]    their eigenvalues (gvom_debug_voxel_eigen), row for row
 *                                       part 2  int64 [1]           rows the map HAS (rows beyond cap are dropped, still counted)
 *   GVOM_PRODUCT_HEIGHT_CLOUD           part 0  float32 [xy*xy, 7]  gvom_debug_height_map
 *   GVOM_PRODUCT_INFERRED_HEIGHT_CLOUD  part 0  float32 [xy*xy, 3]  gvom_debug_inferred_height_map
 * max_rows: the voxel cloud's cap; <= 0 = the fused cell count (which waits for a device combine's pending count once).
 * GVOM_NO_DATA under the conditions of the host forms: nothing combined yet; no 2-D maps since the last fusion (height clouds);
 * no fused statistics (voxel cloud -- which counts as a read of the statistics, so statistics on demand stay on).
 * GVOM_ERR_INVALID on a sharded handle.  *product_id names the product (a sequence number of its own, not a map set id).
 * Products live in PRODUCT SETS that behave exactly like map sets (exports, releases, reuse behind the consumers' release
 * events, exports outliving the handle); a set is allocated when a kind is first asked for or no set of the kind is free, and
 * a product nobody holds an export of goes back to the pool when the next product of ITS KIND is asked for (its id is stale from
 * then on).  At most GVOM_MAX_PRODUCT_SETS sets PER KIND and handle (an occupancy set is xy*xy*z bytes); the call that needs
 * one more returns GVOM_ERR_CAPACITY.  gvom_get_tuning "device_product_sets": how many are allocated, all kinds together; they
 * do not count as "device_map_sets". */
#define GVOM_PRODUCT_OCCUPANCY             1
#define GVOM_PRODUCT_VOXEL_CLOUD           2
#define GVOM_PRODUCT_HEIGHT_CLOUD          3
#define GVOM_PRODUCT_INFERRED_HEIGHT_CLOUD 4
#define GVOM_MAX_PRODUCT_SETS              4
int gvom_device_product(gvom_t *h, int kind, int64_t max_rows, int64_t *product_id);
/* As gvom_device_map_export / _release / _dlpack / _copy, for part `part` of a product.  Export: *ptr, *ndim (1..3), shape and
 * strides in elements (entries beyond ndim are 1).  DLPack: kDLROCM, uint8 (unsigned-integer type code) / float32 / int64,
 * ndim up to 3.  Copy: the whole part (cap rows of a voxel cloud) into host memory, blocking. */
int gvom_device_product_export(gvom_t *h, int64_t product_id, int part, void *consumer_stream, void **ptr, int32_t *ndim,
                               int64_t shape[3], int64_t strides[3]);
int gvom_device_product_release(gvom_t *h, int64_t product_id, void *consumer_stream);
int gvom_device_product_dlpack(gvom_t *h, int64_t product_id, int part, void *consumer_stream, int versioned, void **managed);
int gvom_device_product_copy(gvom_t *h, int64_t product_id, int part, void *host_out);

/* --- obstacle clearance (an extension: what a planner asks the hard-obstacle map first -- how far is each cell from an obstacle) --
 * gvom_clearance computes, on the GPU, the exact Euclidean distance transform of the node's hard-obstacle grid (gvom_ros.py:141-142)
 * and leaves it in device memory as a product (kind GVOM_PRODUCT_CLEARANCE) that gvom_device_product_export / _release / _dlpack /
 * _copy handle like the others.  Costmap inflation is `distance < robot_radius` on the result.
 *
 * DEFINITION.  positive, negative: int32 maps of xy_size * xy_size cells.  A cell is an OBSTACLE iff (double)positive >
 * density_threshold, or negative > 0 (not with GVOM_CLEARANCE_NO_NEGATIVE in flags; not when there is no negative map): the
 * non-zero cells of the hard-obstacle grid.  Cells outside the window are not obstacles.
 *     d2[x, y]       = min over obstacle cells (ox, oy) of (x - ox)^2 + (y - oy)^2                  int32, exact
 *                      GVOM_CLEARANCE_FAR where there is no obstacle, or (max_cells2 > 0) where the minimum exceeds max_cells2
 *     distance[x, y] = (float)(sqrt((double)d2) * xy_resolution)     one float64 square root, one float64 multiply, one rounding
 *                      +infinity where d2 is GVOM_CLEARANCE_FAR
 * part 0 = distance, float32 metres; part 1 = d2, int32 squared cells; both [x, y]-indexed with element strides {1, xy_size}
 * (cell (x, y) at [y*xy_size + x]), like a device map.
 *
 * INPUT.  map_set_id >= 0: maps 0 and 1 of that live device map set (gvom_combine_maps_device); positive and negative must be
 * NULL.  The kernels run on the handle's stream behind the combine that wrote the set, and a later combine that recycles the set
 * runs behind them: the caller needs no export of the set for the duration of the call.  map_set_id < 0: the caller's arrays,
 * xy_size*xy_size int32 each with x fastest (cell (x, y) at [y*xy_size + x]); negative may be NULL.  on_device != 0: device
 * addresses, read in place (the data must be ready when the call is made); on_device == 0: host memory, copied through a staging
 * buffer of the handle before the call returns (a convenience and test route).  No scan or combine is needed on this route.
 * The call ENQUEUES and returns (no host wait on the device routes); after the first call on a handle it allocates nothing unless
 * every clearance set is exported (gvom_get_tuning "clearance_allocations": device allocations the entry point has made so far).
 * Products of this kind live in the product-set pool ("device_product_sets"): at most GVOM_MAX_PRODUCT_SETS, GVOM_ERR_CAPACITY
 * beyond; an unexported one goes back to the pool with the next gvom_clearance call.  gvom_device_product(GVOM_PRODUCT_CLEARANCE)
 * is GVOM_ERR_INVALID (this call makes them).
 * GVOM_ERR_INVALID: a sharded handle; a set id AND pointers, or neither; a stale or unknown set id; a NaN threshold; unknown flag
 * bits.  GVOM_ERR_CAPACITY: xy_size > 4096 (2 * (xy_size - 1)^2, the largest d2, fits int32 far beyond that; the kernels' row
 * masks and LDS strips are sized for 4096).
 * NOT PROVIDED: the nearest obstacle's indices or a gradient; unknown cells as obstacles; sharded handles; output into pinned
 * host memory.  k_map2d is unchanged. */
#define GVOM_PRODUCT_CLEARANCE 5      /* part 0 float32 [xy, xy] metres, part 1 int32 [xy, xy] squared cells;
                                         both [x, y]-indexed with strides (1, xy), like a device map */
#define GVOM_CLEARANCE_FAR 2147483647
#define GVOM_CLEARANCE_NO_NEGATIVE 1  /* flags */
int gvom_clearance(gvom_t *h, int64_t map_set_id, const int32_t *positive, const int32_t *negative, int on_device,
                   double density_threshold, int32_t max_cells2, int flags, int64_t *product_id);

/* --- ray queries (an extension: the first 3-D question a planner asks of a voxel map -- is the straight line from A to B free, and
 * if not, where does it stop) ---------------------------------------------------------------------------------------------------
 * gvom_raycast walks n segments through the CURRENT fused map on the GPU (k_raycast), with the mapper's own ray rule, and leaves
 * the answers in device memory as a product (kind GVOM_PRODUCT_RAYCAST) that gvom_device_product_export / _release / _dlpack /
 * _copy handle like the others.  The walk is read-only.  gvom_get_tuning "raycast" (read-only): 1 -- how a caller probes a
 * library for this entry point (an addition: GVOM_ABI_VERSION stays).
 * The CURRENT fused map -- here and for every call that reads it (gvom_device_product, gvom_score_alignments,
 * gvom_score_viewpoints, gvom_get_occupancy, gvom_read_dense) -- is the map of the most recently BEGUN combine, synchronous or
 * asynchronous (from gvom_combine_begin on, before gvom_combine_end); a scan, accepted or rejected, changes nothing a query sees
 * until the next combine (tests/test_query_cycle.py holds the calls to this at every point of the scan cycle).
 *
 * INPUT.  from [K][3] and to [n][3]: world metres, C-contiguous float32; K is 1 (every ray starts at from[0]) or n.
 * on_device == 0: host memory, copied through a staging buffer of the handle before the call returns; on_device != 0: device
 * addresses, read in place (the data must be ready when the call is made).  The call ENQUEUES on the handle's stream behind
 * whatever produced the current fused map and returns (no host wait on the device route); later scans and combines are ordered
 * behind the kernel and do not change the product, which is a snapshot.  origin_voxels (may be NULL) receives the fused map's
 * window origin W in voxels: window voxel (x, y, z) is world voxel W + (x, y, z).
 *
 * DEFINITION, per ray i.  Every operation is rounded once, there is no FMA; res = (xy_resolution, xy_resolution, z_resolution).
 *     a = from[K == 1 ? 0 : i];  b = to[i]                any non-finite component: {INVALID, 0, -1, 0}, position NaN
 *     p[k] = (float)((double)a[k] / res[k]);   e[k] = (float)((double)b[k] / res[k])
 *     increments inc[3], step length, limit: gvom.py:1105-1126 on (p, e), with the handle's sqrt typing (GVOM_FLAG_CUDA_F32_SQRT)
 *     S = the number of steps the loop test of gvom.py:1127 / 1150 admits
 *     unknown = 0
 *     for j = 1 .. S:
 *         p += inc                                        three float32 additions, gvom.py:1128-1132
 *         v[k] = floor((double)p[k] - W[k]);  outside the window: {LEFT_WINDOW, j - 1, -1, unknown}, position NaN, stop
 *         s = fused state of v                            what gvom_read_dense(GVOM_WHICH_FUSED) returns; a stale tile reads -1
 *         s >= 0:    {OCCUPIED, j, v.x + v.y*xy + v.z*xy*xy, unknown}, position[k] = (float)((double)p[k] * res[k]), stop
 *         s == -1:   unknown += 1;  with GVOM_RAY_UNKNOWN_BLOCKS: {UNKNOWN, j, voxel, unknown}, position as above, stop
 *     with GVOM_RAY_CHECK_TARGET, after S unstopped steps: v[k] = floor((double)b[k] / res[k] - W[k])  (gvom.py:1072-1080);
 *         outside the window: {LEFT_WINDOW, S, -1, unknown}, position NaN;  else examined as above with steps = S + 1 and
 *         position = b (a free target: CLEAR as below)
 *     otherwise {CLEAR, S, -1, unknown}, position NaN
 * min_distance plays no part.  The start voxel is not examined (the mapper's ray does not mark it either).  A ray that starts
 * outside the window is LEFT_WINDOW with 0 steps unless its first step lands inside.  For a float32-representable start and end
 * the voxels walked are exactly those a scan's ray from a to b adds a ray pass to: the answer is consistent with the map.
 * part 0 = int32 [n, 4] {status, steps, voxel, unknown}; part 1 = float32 [n, 3] stop position in metres; row i = ray i.
 *
 * GVOM_NO_DATA before the first combine.  GVOM_ERR_INVALID: a sharded handle; n < 1; K neither 1 nor n; NULL from / to /
 * product_id; unknown flag bits.  GVOM_ERR_CAPACITY: n > 2^26, or every set of the kind is exported.
 * Products of this kind live in the product-set pool ("device_product_sets"), sized by n: at most GVOM_MAX_PRODUCT_SETS; an
 * unexported one goes back to the pool with the next gvom_raycast call (a smaller one is given up for one that holds n rays).
 * gvom_get_tuning "raycast_allocations" (read-only): device allocations the entry point has made on this handle (its product
 * sets and the staging buffer of the host route); it does not grow in steady state at a fixed n.
 * gvom_device_product(GVOM_PRODUCT_RAYCAST) is GVOM_ERR_INVALID (this call makes them).
 * NOT PROVIDED: sharded handles; sorting or binning of the rays by the library (results stay indexed by i; rays in a coherent
 * order -- neighbours in the array pointing the same way -- share cache lines and finish together, and are faster); a per-ray
 * maximum range other than the segment's own length; hit-count or density thresholds on OCCUPIED; queries against a single ring
 * slot. */
#define GVOM_PRODUCT_RAYCAST 6   /* part 0 int32 [n, 4] {status, steps, voxel, unknown}; part 1 float32 [n, 3] stop position, metres */
#define GVOM_RAY_CLEAR 0
#define GVOM_RAY_OCCUPIED 1
#define GVOM_RAY_UNKNOWN 2
#define GVOM_RAY_LEFT_WINDOW 3
#define GVOM_RAY_INVALID 4
#define GVOM_RAY_UNKNOWN_BLOCKS 1   /* flags */
#define GVOM_RAY_CHECK_TARGET   2
int gvom_raycast(gvom_t *h, const float *from /* [K][3] */, int64_t K, const float *to /* [n][3] */, int64_t n,
                 int on_device, int flags, double origin_voxels[3], int64_t *product_id);

/* --- cost-to-go fields (an extension: the global question of a ground-vehicle planner -- from every cell, what does it cost to reach
 * the goal, and which way do I step) ------------------------------------------------------------------------------------------------
 * gvom_cost_to_go computes, on the GPU, the navigation function (cost-to-go field, wavefront) of a 2-D cost map towards a set of
 * goal cells and leaves it in device memory as a product (kind GVOM_PRODUCT_COSTFIELD) that gvom_device_product_export / _release /
 * _dlpack / _copy handle like the others.  gvom_get_tuning "cost_to_go" (read-only): 1 -- how a caller probes a library for this
 * entry point (an addition: GVOM_ABI_VERSION stays).  All arithmetic is integer: the result is exact.
 *
 * DEFINITION.
 * COST MAP   c[x, y]: int32 in 0 .. 65535, cell (x, y) at [y*xy_size + x] like every device map.  0 = the cell is BLOCKED;
 *            1 .. 65535 = the price of the cell.
 * GRAPH      8-connected, undirected.  Direction codes k = 0 .. 7 have the offsets (dx, dy) = (1,0) (1,1) (0,1) (-1,1) (-1,0) (-1,-1)
 *            (0,-1) (1,-1); odd k is a diagonal.  A step from u to its neighbour v is ADMISSIBLE iff v lies inside the window,
 *            c[u] > 0 and c[v] > 0, and -- for a diagonal -- both cells that share the corner, (u.x + dx, u.y) and (u.x, u.y + dy),
 *            are unblocked: no corner is cut.  The step weighs w(u, v) = K * (c[u] + c[v]), K = 5 straight, K = 7 diagonal (10 and
 *            14 between free cells of cost 1; at most 7 * 131070 < 2^20).
 * GOALS      n_goals >= 1 cells (x, y) in window coordinates.  A goal on a blocked cell seeds nothing; a goal outside the window
 *            is GVOM_ERR_INVALID.
 * FIELD      D[u] = the minimum over all admissible paths from u to any seeded goal of the sum of the step weights; 0 at a seeded
 *            goal.  1 <= max_cost <= 2^30 (GVOM_CTG_MAX_COST; 0 means 2^30).  D[u] = GVOM_CTG_UNREACHED (INT32_MAX) where u is
 *            blocked, has no path, or its minimum exceeds max_cost.  A candidate is accepted only if it is <= max_cost, so every
 *            intermediate stays below 2^30 + 2^20: nothing can overflow int32.
 * DIRECTION  dir[u] = the smallest k whose neighbour v is admissible with D[v] + w(u, v) == D[u]; GVOM_CTG_GOAL (8) where
 *            D[u] == 0; GVOM_CTG_NONE (255) where D[u] is unreached; GVOM_CTG_UNSETTLED (254) where no neighbour matches, which
 *            can only happen in a call that stopped before convergence.  A pure function of D and c: exact too.
 * part 0 = D, int32; part 1 = dir, uint8; part 2 = the cost map as the solver used it, uint16; all three [x, y]-indexed with
 * element strides {1, xy_size} (cell (x, y) at [y*xy_size + x]), like a clearance product.
 *
 * INPUT, one of two.
 * map_set_id < 0: the caller's int32 cost map `cost`, xy_size*xy_size with x fastest; params is not read.  on_device == 0: host
 *   memory, staged through a buffer of the handle; a value outside 0 .. 65535 is GVOM_ERR_INVALID, checked before anything is
 *   enqueued.  on_device != 0: a device address, read in place (the data must be ready when the call is made); values outside
 *   0 .. 65535 are CLAMPED into the range by the kernel (negative: blocked).
 * map_set_id >= 0: a live device map set (gvom_combine_maps_device) and *params; cost must be NULL.  k_travcost builds c from map
 *   0 (positive, int32 -- never negative in a map set), 1 (negative), 2 (visibility) and 3 (roughness, float64).  A cell is BLOCKED
 *   iff any of
 *       (double)positive > density_threshold
 *       negative > 0                                            (not with GVOM_CTG_NO_NEGATIVE in flags)
 *       inflation_cells2 > 0 and d2 <= inflation_cells2         d2: gvom_clearance's squared cells for the same threshold and
 *                                                               negative flag with max_cells2 = inflation_cells2, into scratch
 *       visibility == 0                                         (only with GVOM_CTG_UNKNOWN_BLOCKS in flags)
 *   otherwise, in int64,
 *       c = min(65535, base + soft_weight*positive + (visibility == 0 ? unknown_cost : 0) + rough_weight*q)
 *   q (roughness r, float64, every operation rounded once): 0 if rough_weight == 0 or !(r > min_roughness); otherwise
 *       q = (int)floor(((min(r, max_roughness) - min_roughness) / (max_roughness - min_roughness)) * 100.0)
 *   Constraints: base >= 1; soft_weight, unknown_cost, rough_weight in 0 .. 65535; inflation_cells2 >= 0; density_threshold not NaN;
 *   max_roughness > min_roughness, both finite, when rough_weight > 0.  Graded (distance-dependent) inflation is NOT provided: build
 *   a cost map from the clearance product and hand over its device pointer.
 * goals: HOST int32 [n_goals][2] = (x, y), 1 <= n_goals <= 65536.
 *
 * THIS CALL WAITS, unlike the other product calls: it returns when the field has converged, or when max_rounds > 0 rounds have
 * run (max_rounds == 0: until converged).  A round is one launch in which every tile of 32 x 32 cells whose surroundings changed
 * relaxes to its own fixed point; open terrain needs a handful, a maze as many as its longest shortest path crosses tiles.  A call
 * that stops early returns GVOM_OK with converged = 0: every finite D it left is then the cost of a real path -- an upper bound of
 * the true field, not necessarily the minimum -- and dir may hold GVOM_CTG_UNSETTLED.  No kernel waits on another workgroup, and
 * every loop in every kernel has a bound fixed at launch.  The handle is held for the duration of the call: scans and combines
 * issued by other threads on the same handle wait for it.
 * info (may be NULL): {converged 0 / 1, rounds run, reached cells (D < GVOM_CTG_UNREACHED), goals seeded}.
 * ORDER.  The kernels run on the handle's stream behind the combine that wrote the set; a later combine that recycles the set runs
 * behind them: the caller needs no export of the set for the duration of the call.  The product is a snapshot.
 * Products of this kind live in the product-set pool ("device_product_sets"): at most GVOM_MAX_PRODUCT_SETS, GVOM_ERR_CAPACITY
 * beyond; an unexported one goes back to the pool with the next gvom_cost_to_go call.  gvom_get_tuning "cost_to_go_allocations"
 * (read-only): device allocations the entry point has made on this handle (product sets, the work buffer, the staging buffer of the
 * host route, the inflation scratch); it does not grow in steady state.  gvom_device_product(GVOM_PRODUCT_COSTFIELD) is
 * GVOM_ERR_INVALID (this call makes them).
 * GVOM_ERR_INVALID: a sharded handle; a set id AND a cost map, or neither; a set id without params; a stale or unknown set id; a goal
 * outside the window; n_goals outside 1 .. 65536 or NULL goals; bad parameters (above; max_cost outside 0 .. 2^30; max_rounds < 0);
 * unknown flag bits; NULL product_id.  GVOM_ERR_CAPACITY: xy_size > 4096; every set of the kind exported.
 * gvom_set_tuning "cost_to_go_inner" (sweeps a tile makes at most per round; 0 = 256) and "cost_to_go_batch" (rounds enqueued
 * between two looks at the counters, at most 16; 0 = 8) change how long the call takes, never its result; gvom_get_tuning
 * "cost_to_go_tiles": tile relaxations of the last call. */
#define GVOM_PRODUCT_COSTFIELD 7   /* part 0 int32 [xy, xy] cost to go, part 1 uint8 [xy, xy] direction, part 2 uint16 [xy, xy] cell
                                      costs; all [x, y]-indexed with strides (1, xy), like a device map */
#define GVOM_CTG_UNREACHED 2147483647
#define GVOM_CTG_MAX_COST 1073741824
#define GVOM_CTG_GOAL 8
#define GVOM_CTG_UNSETTLED 254
#define GVOM_CTG_NONE 255
#define GVOM_CTG_NO_NEGATIVE 1      /* flags */
#define GVOM_CTG_UNKNOWN_BLOCKS 2
typedef struct gvom_ctg_params {
    double density_threshold;
    double min_roughness, max_roughness;
    int32_t inflation_cells2;
    int32_t base, soft_weight, unknown_cost, rough_weight;
} gvom_ctg_params;
int gvom_cost_to_go(gvom_t *h, int64_t map_set_id, const gvom_ctg_params *params, const int32_t *cost, int on_device,
                    const int32_t *goals /* [n_goals][2] */, int64_t n_goals, int32_t max_cost, int32_t max_rounds, int flags,
                    int64_t *product_id, int64_t info[4]);

/* --- rollout scoring (an extension: the inner loop of a sampling / MPPI planner -- what does the vehicle's footprint, turned to each
 * pose's heading, touch on the cost map, and where does each candidate trajectory first collide) ------------------------------------
 * gvom_score_rollouts scores, on the GPU, K trajectories of T poses each against a uint16 cost map -- a cost field's (part 2 of a
 * GVOM_PRODUCT_COSTFIELD) or the caller's -- with the FOOTPRINT TABLE gvom_footprint_set gave the handle, and leaves the result in
 * device memory as a product (kind GVOM_PRODUCT_ROLLOUTS) that gvom_device_product_export / _release / _dlpack / _copy handle like the
 * others.  gvom_get_tuning "rollouts" (read-only): 1 -- how a caller probes a library for these entry points (an addition:
 * GVOM_ABI_VERSION stays); "footprint" (read-only): 1 while a table is set.  All arithmetic that decides a result is integer but the
 * two roundings named below: the result is exact.
 *
 * DEFINITION.
 * FOOTPRINT  a table of H headings, 1 <= H <= 1024.  Heading k has the cell offsets offsets[start[k] .. start[k + 1]), each an int16
 *            pair (dx, dy); start is int32 [H + 1] with start[0] = 0; every heading has between 1 and 16384 cells and the table at
 *            most 2^22 offsets.  The library computes no geometry: it walks the table.  (The Python binding builds tables for
 *            rectangles and discs.)
 * POSES      float32 [K][T][3] = (x, y, yaw), C-contiguous, world metres and radians.  1 <= T <= 4096, K >= 1, K * T <= 2^26.
 * CENTRE     per axis c = floor((double)x / xy_resolution) - o with o = origin_cells[axis] = round(window origin / xy_resolution), the
 *            rule the binding's world_to_cells uses.  A finite coordinate with |x / xy_resolution| >= 2^30 lies outside the window,
 *            however far.  |o| <= 2^40.
 * HEADING    k = ((int)rintf(yaw * s)) mod H, made non-negative, with s = (float)(H / 2 pi) (the quotient in float64, rounded once):
 *            one float32 multiply, no contraction, round half to even.
 * INVALID    a pose is invalid if x, y or yaw is not finite or |yaw * s| < 2^24 does not hold.
 * POSE COST  with c the cost map (0 = blocked, as part 2 of a cost field): 0 if the pose is invalid, or any footprint cell (centre +
 *            offset) lies outside the window, or any footprint cell inside the window has c == 0; otherwise the maximum of c over the
 *            footprint cells (unsigned: costs >= 32768 survive).  Every pose is evaluated: nothing depends on scheduling.
 * SUMMARY    first_blocked = the smallest t with pose cost 0, or T.  status is decided at that pose: GVOM_ROLLOUT_CLEAR if there is
 *            none; GVOM_ROLLOUT_INVALID if the pose is invalid; else GVOM_ROLLOUT_COLLISION if a footprint cell inside the window has
 *            c == 0; else GVOM_ROLLOUT_LEFT_WINDOW.  path_cost = the sum of the pose costs of t < first_blocked (<= 4096 * 65535 <
 *            2^31).  terminal = D[centre cell of pose first_blocked - 1] where a cost-to-go field D was given; GVOM_CTG_UNREACHED
 *            when first_blocked == 0, when no field was given, and when that centre cell lies outside the window (a footprint need
 *            not contain its own centre).
 * part 0 = int32 [K, 4] {status, first_blocked, path_cost, terminal}; part 1 = uint16 [K, T] pose costs; row i = rollout i.
 *
 * gvom_footprint_set validates the table, copies it to the device and returns after the copy.  A later call replaces the table; the
 * copy runs on the handle's stream, behind whatever still reads the previous one.  GVOM_ERR_INVALID: NULL arguments, n_headings
 * outside 1 .. 1024, start[0] != 0, a heading with fewer than 1 or more than 16384 cells; GVOM_ERR_CAPACITY: more than 2^22 offsets.
 *
 * gvom_score_rollouts: INPUT, one of two.  costfield_id >= 0: a live GVOM_PRODUCT_COSTFIELD; its part 2 is c and its part 0 is D, read
 * on the handle's stream behind the solve that wrote them; cell_cost and cost_to_go must be NULL.  costfield_id < 0: cell_cost (uint16,
 * xy_size * xy_size, cell (x, y) at [y*xy_size + x]) and optionally cost_to_go (int32, same order; NULL: every terminal is
 * GVOM_CTG_UNREACHED).  on_device != 0: poses and map pointers are device addresses, read in place (the data must be ready when the
 * call is made); the call enqueues and returns without a host wait.  on_device == 0: poses and map pointers are host memory, staged
 * through a buffer of the handle; the call returns after the upload.  (With a cost field id, on_device says where the poses are.)
 * The product is a snapshot: later scans, combines and gvom_footprint_set calls do not change it.
 * Products of this kind live in the product-set pool ("device_product_sets"), sized by K and T: at most GVOM_MAX_PRODUCT_SETS; an
 * unexported one goes back to the pool with the next gvom_score_rollouts call (a smaller one is given up for one that holds K x T).
 * gvom_get_tuning "rollout_allocations" (read-only): device allocations the entry point has made on this handle (its product sets and
 * the staging buffer of the host route); it does not grow in steady state at a fixed K and T.
 * gvom_device_product(GVOM_PRODUCT_ROLLOUTS) is GVOM_ERR_INVALID (this call makes them).  Kinds 8 and 9 are not assigned.
 * GVOM_ERR_INVALID: a sharded handle; no footprint table set; a field id AND map pointers, or neither; an unknown or stale field id;
 * T outside 1 .. 4096; K < 1; NULL poses / origin_cells / product_id; an origin beyond 2^40 cells.  GVOM_ERR_CAPACITY: K * T > 2^26;
 * xy_size > 4096; every set of the kind exported.
 * NOT PROVIDED: the sum or mean over the footprint (the cost is the maximum); an early stop at the first collision (every pose is
 * scored); per-pose output into host memory (copy part 1); poses in any layout other than [K][T][3]; sharded handles;
 * interpolation between poses (space them a cell apart). */
#define GVOM_PRODUCT_ROLLOUTS 10   /* part 0 int32 [K, 4] {status, first_blocked, path_cost, terminal}; part 1 uint16 [K, T] pose costs */
#define GVOM_ROLLOUT_CLEAR 0
#define GVOM_ROLLOUT_COLLISION 1
#define GVOM_ROLLOUT_LEFT_WINDOW 2
#define GVOM_ROLLOUT_INVALID 3
int gvom_footprint_set(gvom_t *h, int32_t n_headings, const int32_t *start /* [n_headings + 1] */, const int16_t *offsets /* [start[n_headings]][2] */);
int gvom_score_rollouts(gvom_t *h, int64_t costfield_id, const uint16_t *cell_cost, const int32_t *cost_to_go,
                        const float *poses /* [K][T][3] */, int64_t K, int64_t T, int on_device, const int64_t origin_cells[2],
                        int64_t *product_id);

/* --- terrain attitude scoring (an extension: the off-road half of a sampling planner's inner loop -- how would the vehicle SIT on the
 * ground at each pose: nose up or down, tilted sideways, high-centred on a crest) ----------------------------------------------------
 * gvom_score_attitude scores, on the GPU, K trajectories of T poses each against ONE float64 ground map -- a device map set's height
 * and inferred-height maps, or the caller's -- with the footprint table gvom_footprint_set gave the handle and the CHASSIS
 * gvom_chassis_set gave it, and leaves the result in device memory as a product (kind GVOM_PRODUCT_ATTITUDE) that
 * gvom_device_product_export / _release / _dlpack / _copy handle like the others.  gvom_get_tuning "attitude" (read-only): 1 -- how a
 * caller probes a library for these entry points (an addition: GVOM_ABI_VERSION stays); "chassis" (read-only): 1 while a chassis is
 * set.  Every float64 operation below is ONE IEEE operation in the order written, parentheses binding, no contraction; the library
 * calls no trigonometric function (the caller supplies cos_sin): the result is exact, and every decision is made on the float32
 * values that are stored, so a consumer can re-derive it from part 1.
 *
 * DEFINITION.  res = xy_resolution, xy = xy_size, o = origin_cells.
 * GROUND     g, float64, cell (x, y) at [y*xy + x].  A cell is KNOWN iff g > -1000 && g < +inf (NaN, +-inf and exactly -1000 are
 *            unknown).  map_set_id >= 0: a live device map set; g = height (map 4) where height > -1000, otherwise the inferred
 *            height (map 5) if flags has GVOM_ATTITUDE_INFERRED_GROUND, else -1000; ground must be NULL.  map_set_id < 0: g is the
 *            caller's ground, host or device memory as on_device says.
 * POSES, CENTRE, HEADING, INVALID   those of rollout scoring above, word for word (the same s, H, rintf, the 2^30 and 2^24 bounds);
 *            H is the footprint table's.  In addition fx = q - floor(q) with q = (double)x / res, and fy likewise: where in its
 *            cell the pose lies.
 * CHASSIS    front_axle > rear_axle (the axles' body x, metres; body frame: x forward, y left), track > 0, belly_height (the
 *            belly above the wheels' contact plane), and cos_sin [H][2] = (cos, sin) of heading k's angle.  WHEELS FL, FR, RL, RR
 *            have the body coordinates (a, b) = (front_axle, +track/2), (front_axle, -track/2), (rear_axle, +track/2),
 *            (rear_axle, -track/2); at gvom_chassis_set, on the host, with (c, s) = cos_sin[k]: wx = a*c - b*s, wy = a*s + b*c,
 *            kept per heading and wheel.  Wheel cell, per axis: floor(((double)x + wx) / res) - o; it is OUTSIDE the window if it
 *            is not in [0, xy) or |quotient| < 2^30 does not hold.  z_i = g at that cell.
 * ATTITUDE   zF = 0.5*(zFL + zFR), zR = 0.5*(zRL + zRR), zL = 0.5*(zFL + zRL), zT = 0.5*(zFR + zRR);
 *            sp = (zF - zR) / (front_axle - rear_axle)   the pitch tangent, nose up positive;
 *            sr = (zL - zT) / track                      the roll tangent, left side up positive;
 *            z0 = 0.25*((zFL + zFR) + (zRL + zRR)), am = 0.5*(front_axle + rear_axle).
 * BELLY      over the footprint cells (dx, dy) of heading k that lie inside the window and whose ground is known:
 *            du = (((double)dx + 0.5) - fx) * res, dv likewise with dy and fy; u = du*c + dv*s, v = dv*c - du*s;
 *            plane = (z0 + sp*(u - am)) + sr*v; clr = (plane + belly_height) - g; belly = the least clr, +inf where there is no
 *            such cell.  (A clr that is NaN -- only heights whose sums overflow float64 make one -- is skipped.)
 * STATUS     per pose, the first that applies: GVOM_ATTITUDE_INVALID; _LEFT_WINDOW: a wheel cell or a footprint cell is outside
 *            the window; _UNKNOWN_GROUND: a wheel cell's ground is unknown; _PITCH: fabsf((float)sp) > max_pitch; _ROLL:
 *            fabsf((float)sr) > max_roll; _BELLY: (float)belly < min_clearance; _OK.  An infinite limit disables its test.
 * part 1 = float32 [K, T, 3] {(float)sp, (float)sr, (float)belly}; {0, 0, 0} where the status is INVALID, LEFT_WINDOW or
 *            UNKNOWN_GROUND.  part 2 = uint8 [K, T], the pose status.
 * part 0 = int32 [K, 5] {status, first_bad, steepest_pitch_pose, steepest_roll_pose, lowest_belly_pose}: first_bad = the smallest t
 *            whose status is not OK, or T; status = that pose's, or OK; the three indices are the lowest t < first_bad with the
 *            largest fabsf(pitch), the largest fabsf(roll) and the smallest belly (a NaN tangent ranks below every number), -1
 *            when first_bad == 0.  Row i = rollout i.
 *
 * gvom_chassis_set computes the wheel table on the host, copies it and cos_sin to the device and returns after the copy; a later
 * call replaces the chassis.  GVOM_ERR_INVALID: NULL arguments; n_headings outside 1 .. 1024; a non-finite length; front_axle <=
 * rear_axle; track <= 0; a NaN limit; a cos_sin entry that is not finite or exceeds 1 in magnitude; a wheel offset that is not finite.
 * gvom_score_attitude: on_device, staging, the snapshot, the pool (sized by K and T) and the limits are gvom_score_rollouts' -- read
 * a map set id for the field id and ground for the map pointers.  It rebuilds the ground map of a map set in a grow-only buffer of
 * the handle.  gvom_get_tuning "attitude_allocations" (read-only): device allocations the entry point has made on this handle (that
 * buffer, the staging buffer of the host route and its product sets); it does not grow in steady state at a fixed K and T.
 * gvom_device_product(GVOM_PRODUCT_ATTITUDE) is GVOM_ERR_INVALID (this call makes them).  Kind 13 is not assigned.
 * GVOM_ERR_INVALID: a sharded handle; no footprint table set, no chassis set, or a chassis whose n_headings is not the table's; a set
 * id AND a ground pointer, or neither; an unknown or stale set id; unknown flag bits; T outside 1 .. 4096; K < 1; NULL poses /
 * origin_cells / product_id; an origin beyond 2^40 cells.  GVOM_ERR_CAPACITY: K * T > 2^26; xy_size > 4096; every set of the kind
 * exported.
 * NOT PROVIDED: suspension or tyre models; three-wheel contact (the plane is the least-squares one of four heights, not a stable
 * stance); sharded handles; interpolation between poses. */
#define GVOM_PRODUCT_ATTITUDE 14   /* part 0 int32 [K, 5] {status, first_bad, steepest pitch, steepest roll, lowest belly}; part 1 float32 [K, T, 3] {pitch, roll, belly}; part 2 uint8 [K, T] pose status */
/* 13 stays unassigned: tests/align_layout_host_test.cpp holds 8, 9, 11 and 13 to "no such kind" */
#define GVOM_ATTITUDE_OK 0
#define GVOM_ATTITUDE_PITCH 1
#define GVOM_ATTITUDE_ROLL 2
#define GVOM_ATTITUDE_BELLY 3
#define GVOM_ATTITUDE_UNKNOWN_GROUND 4
#define GVOM_ATTITUDE_LEFT_WINDOW 5
#define GVOM_ATTITUDE_INVALID 6
#define GVOM_ATTITUDE_INFERRED_GROUND 1   /* flags: where the height is unknown, stand on the inferred height */
typedef struct {
    double front_axle, rear_axle, track, belly_height;   /* metres, body frame: x forward, y left */
    float max_pitch, max_roll, min_clearance;            /* tangents, tangents, metres */
} gvom_chassis_t;
int gvom_chassis_set(gvom_t *h, const gvom_chassis_t *c, int32_t n_headings, const double *cos_sin /* [n_headings][2] */);
int gvom_score_attitude(gvom_t *h, int64_t map_set_id, const double *ground, const float *poses /* [K][T][3] */, int64_t K, int64_t T,
                        int on_device, int flags, const int64_t origin_cells[2], int64_t *product_id);

/* --- scan alignment scoring (an extension: the inner loop of a correlative scan matcher -- does the pose a scan is about to be fused
 * at fit the map it is fused into) -------------------------------------------------------------------------------------------------
 * gvom_score_alignments holds, on the GPU, a float32 cloud of n returns under K candidate rigid transforms against the CURRENT fused
 * map: per candidate it counts the returns that end in an occupied voxel, next to one, in a free one, in a never-observed one and
 * outside the window, weighs the counts into an integer score and names the best candidate.  The result stays in device memory as a
 * product (kind GVOM_PRODUCT_ALIGNMENT) that gvom_device_product_export / _release / _dlpack / _copy handle like the others.  READ-ONLY:
 * nothing of the map changes.  gvom_get_tuning "alignments" (read-only): 1 -- how a caller probes a library for this entry point (an
 * addition: GVOM_ABI_VERSION stays).  A pair (candidate, return) is classed by the voxel that gvom_process_pointcloud(cloud, ego,
 * transform = candidate) would add the return's hit to: the result is exact.
 *
 * DEFINITION.  M_k = candidate k, float64 [3][4]: rows 0..2 of a 4x4, row-major; transforms is [K][3][4], C-contiguous.  p_i =
 * (x, y, z) float32; cloud is [n][3], C-contiguous.  res = (xy_resolution, xy_resolution, z_resolution), size = (xy_size, xy_size,
 * z_size), W = the fused map's window origin in voxels, s(v) = the fused state of window voxel v (-1 = never observed, which is also
 * what a stale tile reads; <= -2 = observed free; >= 0 = occupied).
 * 1 WORLD POSITION  the scan's own transform rule: w_r = (float)(((x * M[r][0] + y * M[r][1]) + z * M[r][2]) + M[r][3]), products
 *                   and sums in float64, left to right, no contraction, rounded ONCE to float32.
 * 2 VOXEL           the scan's endpoint rule: v_r = floor((double)w_r / res_r - W_r).  The pair is OUTSIDE unless 0 <= v_r < size_r
 *                   on all three axes, compared in float64: NaN, infinities, non-finite matrix entries and products that overflow
 *                   float32 fall out as OUTSIDE without a special case.  The scan's min_distance rejection is NOT applied: it
 *                   measures from the world's origin, which says nothing about a fit.
 * 3 CLASS           in this order: OCCUPIED if s(v) >= 0; NEAR if dilate == 1 and some window voxel u with max_r |u_r - v_r| <= 1 has
 *                   s(u) >= 0 (voxels outside the window never count as neighbours); FREE if s(v) <= -2; otherwise UNKNOWN.
 * 4 PER CANDIDATE   the counts {occupied, near, free, unknown, outside}, which sum to n, and score = sum of weights[c] * count[c]
 *                   (int32; weights in the order of the counts, |weight| <= 1024, so |score| <= 2^30).
 * 5 BEST            the lowest k whose score is the maximum.
 * part 0 = int32 [K, 6] {score, occupied, near, free, unknown, outside}, row k = candidate k; part 1 = int32 [4] {best index, best
 * score, n, K}.
 *
 * on_device != 0: cloud and transforms are device addresses, read in place (the data must be ready when the call is made); the call
 * enqueues and returns without a host wait.  on_device == 0: both are host memory, staged through a buffer of the handle; the call
 * returns after the upload.  The product is a snapshot of the map as it is when the call is made: later scans and combines do not
 * change it.  Products of this kind live in the product-set pool ("device_product_sets"), sized by K: at most GVOM_MAX_PRODUCT_SETS;
 * an unexported one goes back to the pool with the next call.  The call rebuilds, from the fused state, a CLASS GRID of 2 bits per
 * voxel in a grow-only buffer of the handle (xy_size * ceil(xy_size / 16) * z_size * 4 bytes; gvom_get_tuning "alignment_grid_bytes",
 * read-only); "alignment_allocations" (read-only): device allocations the entry point has made on this handle (the grid, the staging
 * buffer of the host route and its product sets) -- it does not grow in steady state.  "alignment_points_per_block" /
 * "alignment_candidate_group" (read-only): the tile of the scoring kernel.
 * gvom_device_product(GVOM_PRODUCT_ALIGNMENT) is GVOM_ERR_INVALID (this call makes them).  Kinds 8, 9 and 11 are not assigned.
 * GVOM_NO_DATA before the first combine.  GVOM_ERR_INVALID: a sharded handle; NULL cloud / transforms / weights / product_id; n < 1
 * or K < 1; dilate other than 0 or 1; |weight| > 1024.  GVOM_ERR_CAPACITY: n > 2^20; K > 65536; n * K > 2^32; a class grid of 2^32
 * words or more; every set of the kind exported.
 * NOT PROVIDED: float64 clouds; per-point weights; hit-count thresholds; a dilation of more than one voxel; sharded handles; single
 * ring slots (the fused map only); a cache of the class grid across calls. */
#define GVOM_PRODUCT_ALIGNMENT 12   /* part 0 int32 [K, 6] {score, occupied, near, free, unknown, outside}; part 1 int32 [4] {best index, best score, n, K} */
int gvom_score_alignments(gvom_t *h, const float *cloud /* [n][3] */, int64_t n, const double *transforms /* [K][3][4] */, int64_t K,
                          int on_device, int dilate, const int32_t weights[5], int64_t *product_id);

/* --- frontier extraction (an extension: where to go next when nobody supplies a goal -- the boundary between ground that has been
 * seen and can be driven on, and ground that has never been seen) -------------------------------------------------------------------
 * gvom_frontiers finds, on the GPU, the frontier cells of a cost map, clusters them, and leaves per cluster its size, box, nearest
 * member and coordinate sums in device memory as a product (kind GVOM_PRODUCT_FRONTIERS) that gvom_device_product_export / _release /
 * _dlpack / _copy handle like the others.  gvom_get_tuning "frontiers" (read-only): 1 -- how a caller probes a library for this entry
 * point (an addition: GVOM_ABI_VERSION stays).  All arithmetic is integer: the result is exact and does not depend on scheduling.
 *
 * DEFINITION.  Three maps of xy_size * xy_size cells, cell (x, y) at [y*xy_size + x]:
 *   c    uint16 cell cost, 0 = blocked, as part 2 of a cost field;
 *   vis  int32 visibility, as map 2 of a map set; a cell is KNOWN iff vis > 0;
 *   D    int32 cost to go; it may be absent.  The graph of a cost field is undirected: a field seeded AT the vehicle holds the
 *        travel cost TO every cell.
 * FRONTIER CELL u: c[u] > 0, and vis[u] > 0, and at least one of its four edge neighbours lies inside the window and has vis == 0,
 *            and, where D is given, D[u] < GVOM_CTG_UNREACHED.  Cells outside the window are not unknown.
 * CLUSTER    a connected component of the frontier cells under 8-connectivity.  Its LABEL is the smallest linear index
 *            y*xy_size + x among its members.
 * KEPT       clusters are those with at least min_cells members (min_cells >= 1).  Their RANK is their position in ascending label
 *            order, 0 .. n_kept - 1.
 * PER KEPT CLUSTER of rank r < cap, cap = max_clusters: label; cells; min x, min y, max x, max y; best cell and best D -- the member
 *            with the least D, on ties the lowest index: one unsigned 64-bit minimum over ((uint32)D << 32) | index; without D, best
 *            D = GVOM_CTG_UNREACHED and the best cell is the label --; sum x, sum y as int64 (the centroid is theirs divided by
 *            cells; the caller divides).  Clusters of rank >= cap are dropped from the rows and still counted.
 * part 0 = int32 [cap, 8] {label, cells, min x, min y, max x, max y, best cell, best D}; part 1 = int64 [cap, 2] {sum x, sum y};
 * part 2 = int32 [xy, xy], the cluster map, [x, y]-indexed with strides (1, xy) like a device map: the rank of the cell's cluster
 * (also for ranks >= cap), -1 where the cell is no frontier cell, -2 where it is one of a cluster below min_cells; part 3 = int32 [4]
 * {n_kept, frontier cells, frontier cells in kept clusters, cap}.  Rows >= min(n_kept, cap) of parts 0 and 1 are zero.
 *
 * INPUT, one of two.  costfield_id >= 0 AND map_set_id >= 0: a live GVOM_PRODUCT_COSTFIELD, whose part 2 is c and whose part 0 is D,
 * and a live device map set, whose map 2 is vis; the three pointers must be NULL; the kernels run on the handle's stream behind
 * whatever wrote the field and the set.  Both ids < 0: cell_cost and visibility are required, cost_to_go is optional; on_device != 0:
 * device addresses, read in place (the data must be ready when the call is made); on_device == 0: host arrays, staged through a
 * buffer of the handle.
 * Like gvom_cost_to_go, THIS CALL WAITS: it returns once the labels have converged.  Rounds of label relaxation over 32 x 32 tiles
 * are enqueued a batch at a time ("frontier_batch", gvom_set_tuning: rounds between two looks at the counters, 1 .. 16, 0 = 8;
 * "frontier_inner": sweeps a tile makes at most per round, 0 = 256; both change the time, never the result); the first round that
 * flags no tile ends the labelling.  Labels only go down, so it ends; the call additionally gives up with GVOM_ERR_HIP after
 * xy_size * xy_size + 1 rounds, which cannot be reached.  There is no max_rounds: a stopped labelling has labels that are not roots,
 * and its pieces are not well defined.
 * info (may be NULL): {rounds run, n_kept, frontier cells, clusters dropped by min_cells}.
 * The product is a snapshot: later scans, combines and solves do not change it.  Products of this kind live in the product-set pool
 * ("device_product_sets"), sized by the map and max_clusters: at most GVOM_MAX_PRODUCT_SETS, GVOM_ERR_CAPACITY beyond; an unexported
 * one goes back to the pool with the next call.  "frontier_allocations" (read-only): device allocations the entry point has made on
 * this handle (its work buffer of 8 bytes per cell plus flags and counters, the staging buffer of the host route and its product
 * sets); it does not grow in steady state.  "frontier_rounds" / "frontier_tiles" (read-only): rounds and tile relaxations of the last
 * call.  gvom_device_product(GVOM_PRODUCT_FRONTIERS) is GVOM_ERR_INVALID (this call makes them).  Kinds 8, 9, 11, 13 and 15 are not
 * assigned.
 * GVOM_ERR_INVALID: a sharded handle; ids and pointers mixed, or neither; only one of the two ids; a stale id; min_cells < 1;
 * max_clusters outside 1 .. 2^20; NULL product_id.  GVOM_ERR_CAPACITY: xy_size > 4096; every set of the kind exported.
 * NOT PROVIDED: 4-connected clusters; the window edge as a frontier; frontiers in 3-D; splitting of long clusters; a
 * distance-to-robot filter other than reachability; sharded handles; an early stop. */
#define GVOM_PRODUCT_FRONTIERS 16   /* part 0 int32 [cap, 8]; part 1 int64 [cap, 2] {sum x, sum y}; part 2 int32 [xy, xy] cluster map; part 3 int32 [4] */
int gvom_frontiers(gvom_t *h, int64_t costfield_id, int64_t map_set_id, const uint16_t *cell_cost, const int32_t *cost_to_go /* may be NULL */,
                   const int32_t *visibility, int on_device, int32_t min_cells, int32_t max_clusters, int64_t *product_id, int64_t info[4]);

/* --- viewpoint scoring (an extension: the next-best-view question of an exploration stack -- put my sensor at this pose, with its
 * real beam pattern: how many voxels that nobody has observed would its beams pass before they hit something) ----------------------
 * gvom_score_viewpoints casts the selected beams of the handle's sensor model (gvom_sensor_model_set) from K poses through the CURRENT
 * fused map on the GPU (k_viewpoints, k_viewpoint_best), with gvom_raycast's ray rule, and leaves per pose the number of DISTINCT
 * never-observed voxels the beams examined, the same with multiplicity, and how the beams ended, in device memory as a product (kind
 * GVOM_PRODUCT_VIEWPOINTS) that gvom_device_product_export / _release / _dlpack / _copy handle like the others.  Read-only on the map.
 * gvom_get_tuning "viewpoints" (read-only): 1 -- how a caller probes a library for this entry point (an addition: GVOM_ABI_VERSION
 * stays).
 *
 * POSES.  poses [K][12]: rows 0..2 of the 4x4 sensor-to-world matrices, row-major, float64.  on_device == 0: host memory, copied
 * through a staging buffer of the handle before the call returns; on_device != 0: a device address, read in place (the data must be
 * ready when the call is made).  The call ENQUEUES on the handle's stream behind whatever produced the current fused map and returns
 * (no host wait on the device route); later scans and combines are ordered behind the kernels and do not change the product, which is
 * a snapshot; a sensor model that replaces another is ordered behind the calls that read the old one.  origin_voxels (may be NULL)
 * receives the fused map's window origin W in voxels.
 * BEAMS.  Of the model's H x W pixels the selected ones are h = 0, stride_h, 2*stride_h, .. < H and w = 0, stride_w, .. < W; nb is
 * their number, ceil(H / stride_h) * ceil(W / stride_w).  The model's range gate and range scale play no part.
 *
 * DEFINITION, per viewpoint k with matrix C = poses[k] and selected pixel i = h*W + w.  float64, every operation rounded once, in this
 * order, no FMA -- the arithmetic of "range images" above with r = max_range:
 *     p[c] = max_range * dir[i][c] + off[i][c]                               c = 0, 1, 2
 *     q[c] = ((p[0]*C[4c] + p[1]*C[4c+1]) + p[2]*C[4c+2]) + C[4c+3]
 *     b[c] = (float)q[c];   a[c] = (float)C[4c+3]                            one origin per viewpoint: the pose's translation
 * The ray a -> b is walked exactly as gvom_raycast walks the segment a -> b ("ray queries" above: the same set-up, step count S,
 * three float32 additions per step, window lookup, a stale tile reads never observed, the handle's sqrt typing), with
 * GVOM_RAY_UNKNOWN_BLOCKS if `flags` has it and never with GVOM_RAY_CHECK_TARGET.  A beam with a non-finite component in a or b is
 * INVALID, as gvom_raycast's ray is.
 * part 0 = int32 [K, 8], row k:
 *     0  status   a GVOM_RAY_* code for the origin's own voxel v[c] = floor((double)a[c] / res[c] - W[c]): CLEAR observed free,
 *                 OCCUPIED, UNKNOWN never observed (a stale tile included), LEFT_WINDOW outside the window; INVALID: an entry of
 *                 C is not finite, and then every other column is 0 except column 7 = nb
 *     1  gain     the number of DISTINCT window voxels whose fused state is never-observed (-1) and that at least one beam of k
 *                 examined (the voxel that stops a beam under GVOM_RAY_UNKNOWN_BLOCKS included)
 *     2  visits   the sum over the beams of gvom_raycast's `unknown` column: the same voxels, with multiplicity
 *     3 .. 7      beams that ended OCCUPIED, CLEAR, LEFT_WINDOW, UNKNOWN (only with the flag), INVALID; they sum to nb
 * part 1 = int32 [4] {best, gain[best], K, nb}: best = the lowest index of the largest gain among the rows whose status is CLEAR;
 * -1 and gain 0 where no row is CLEAR.
 * All results are integers; integer sums and bit-ORs commute: the product does not depend on scheduling.  Deduplication: one bitmap
 * of the window's voxels per viewpoint (bit x + y*xy + z*xy*xy), an atomic OR per examined never-observed voxel; the beam that finds
 * the bit clear counts the voxel.  The bitmaps live in a grow-only work buffer of the handle of at most "viewpoint_bitmap_mb"
 * megabytes (gvom_set_tuning / gvom_get_tuning; default 256, 0 .. 4096, a negative value restores the default): a call walks
 * B = max(1, that / the bytes of one bitmap) viewpoints per launch (at most 32768; "viewpoint_batch", read-only: B of the last call)
 * and clears the bitmaps in front of every launch.  The setting changes the time and the memory, never the result.
 *
 * GVOM_NO_DATA before the first combine.  GVOM_ERR_INVALID: a sharded handle; no sensor model; K < 1; a stride < 1; max_range not
 * finite or <= 0; NULL poses / product_id; unknown flag bits.  GVOM_ERR_CAPACITY: K > 65536; nb > 2^22;
 * nb * (xy_size + z_size + 1) >= 2^31 (visits cannot overflow); a window of 2^31 voxels or more; every set of the kind exported.
 * Products of this kind live in the product-set pool ("device_product_sets"), sized by K: at most GVOM_MAX_PRODUCT_SETS; an
 * unexported one goes back to the pool with the next call.  "viewpoint_allocations" (read-only): device allocations the entry point
 * has made on this handle (the bitmaps, the staging buffer of the host route and its product sets); it does not grow in steady state.
 * gvom_device_product(GVOM_PRODUCT_VIEWPOINTS) is GVOM_ERR_INVALID (this call makes them).  Kind 17 is not assigned, like 8, 9, 11, 13
 * and 15.
 * NOT PROVIDED: per-beam results (that is gvom_raycast); a per-beam origin from `off` (off moves the beam's end, every beam starts at
 * the pose's translation); range weighting of the gain; a 2-D cell gain; sharded handles. */
#define GVOM_PRODUCT_VIEWPOINTS 18   /* part 0 int32 [K, 8] {status, gain, visits, beams OCCUPIED, CLEAR, LEFT_WINDOW, UNKNOWN, INVALID}; part 1 int32 [4] {best, its gain, K, nb} */
int gvom_score_viewpoints(gvom_t *h, const double *poses /* [K][12] */, int64_t K, int on_device, double max_range,
                          int32_t stride_h, int32_t stride_w, int flags, double origin_voxels[3], int64_t *product_id);

/* --- pose fields (an extension: the navigation function on (x, y, heading) -- heading-aware cost-to-go under the oriented footprint,
 * for a vehicle that cannot turn on the spot; what makes a rollout's terminal cost honest for a car) ------------------------------------
 * gvom_pose_field computes, on the GPU, from every STATE (x, y, h) of a window -- a cell and one of the H headings of the footprint
 * table gvom_footprint_set gave the handle -- the cheapest way to a goal state that the MOTION PRIMITIVES gvom_primitives_set gave the
 * handle allow, and the first primitive of it, and leaves the result in device memory as a product (kind GVOM_PRODUCT_POSEFIELD) that
 * gvom_device_product_export / _release / _dlpack / _copy handle like the others.  gvom_get_tuning "pose_field" (read-only): 1 -- how
 * a caller probes a library for these entry points (an addition: GVOM_ABI_VERSION stays); "primitives" (read-only): 1 while a table is
 * set.  All arithmetic is integer: the result is exact and does not depend on scheduling.
 *
 * DEFINITION.
 * COST MAP    c, uint16 per cell, 0 = blocked: part 2 of a live GVOM_PRODUCT_COSTFIELD, or the caller's int32 map as gvom_cost_to_go
 *             takes it (cell (x, y) at [y*xy_size + x]; a device map is clamped into 0 .. 65535, a host map outside it is refused).
 * POSE COST   C[h][cell], uint16: exactly the POSE COST of "rollout scoring" for a pose centred in `cell` with heading h -- 0 where a
 *             footprint cell of heading h lies outside the window or on a cell with c == 0, otherwise the maximum of c under the
 *             footprint.
 * PRIMITIVES  start int32 [H + 1] with start[0] = 0, prims int16 [start[H]][4], each row (dx, dy, h_to, w).  Primitive p of heading h,
 *             start[h] <= p < start[h + 1], leads from the state u = (x, y, h) to v = (x + dx, y + dy, h_to).  |dx|, |dy| <= 4;
 *             0 <= h_to < H; 1 <= w <= 255; at most 64 primitives per heading; (dx, dy, h_to) != (0, 0, h).  The graph is DIRECTED:
 *             the vehicle reverses only where the table says so.
 * ADMISSIBLE  a primitive is admissible iff v lies in the window, C[u] != 0 and C[v] != 0; its PRICE is w * (C[u] + C[v]).  The
 *             cells swept between the two ends are not examined.
 * FIELD       D, int32: the least solution of D[u] = min over the admissible primitives of u of (price + D[v]) with D = 0 at the
 *             seeded goal states; GVOM_CTG_UNREACHED elsewhere.  max_cost > 0: states dearer than max_cost read GVOM_CTG_UNREACHED
 *             (0: the limit is GVOM_CTG_MAX_COST), as in "cost-to-go fields".
 * ACTION      uint8 per state: the index, within heading h's list, of the first primitive in table order that attains the minimum;
 *             GVOM_POSE_GOAL (253) at a seeded state; GVOM_CTG_NONE (255) where D is unreached; GVOM_CTG_UNSETTLED (254) where no
 *             primitive matches, which happens only in a field stopped by max_rounds.
 * GOALS       int32 [n_goals][3] = (x, y, h) in window cells.  h < 0 seeds every heading of the cell.  A goal state with C == 0 seeds
 *             nothing.  info[3] counts the distinct states seeded.
 * part 0 = int32 D, part 1 = uint8 action, part 2 = uint16 C, each [H, xy, xy] indexed [h, x, y] with strides (xy*xy, 1, xy): every
 * plane has the memory layout of a cost field's maps.
 *
 * gvom_primitives_set validates the table, copies it to the device and returns after the copy; a later call replaces the table.
 * GVOM_ERR_INVALID: NULL arguments, n_headings outside 1 .. 64, start[0] != 0, a heading with more than 64 primitives (none is
 * allowed: a dead end), and any primitive outside the limits above.
 *
 * gvom_pose_field: the solver is gvom_cost_to_go's scheme (tiles of 8 x 8 cells x all headings relax in LDS, rounds are enqueued a
 * batch at a time, the first round that flagged no tile ends the solve), so the call WAITS for the field.  max_rounds > 0 stops after
 * that many rounds: info[0] = 0 then, every finite D is the cost of a real drive (an upper bound of the field).  max_rounds == 0 and
 * no convergence is GVOM_ERR_HIP.  info = {converged, rounds, reached states, seeded states}.  gvom_set_tuning "pose_field_inner"
 * (sweeps a tile makes at most per round; 0: 64) and "pose_field_batch" (rounds per look at the counters, at most 16; 0: 8) change
 * the time, never the result; "pose_field_rounds" / "pose_field_tiles" (read-only): rounds and tile relaxations of the last call.
 * The product is a snapshot: later scans, combines, gvom_footprint_set and gvom_primitives_set calls do not change it.  Products of
 * this kind live in the product-set pool ("device_product_sets"), sized by H and xy_size: at most GVOM_MAX_PRODUCT_SETS; an
 * unexported one goes back to the pool with the next call.  "pose_field_allocations" (read-only): device allocations the entry points
 * have made on this handle (the table, the work and staging buffers and the product sets); it does not grow in steady state.
 * gvom_device_product(GVOM_PRODUCT_POSEFIELD) is GVOM_ERR_INVALID (this call makes them).  Kind 19 is not assigned.
 * GVOM_ERR_INVALID: a sharded handle; no footprint table or no primitive table set, or tables of different H; a field id AND a cost
 * map, or neither; an unknown or stale field id; goals NULL, n_goals outside 1 .. 65536, a goal outside the window or with h >= H;
 * max_cost outside 0 .. 2^30; max_rounds < 0; a host cost outside 0 .. 65535.  GVOM_ERR_CAPACITY: H > 64; xy_size > 4096;
 * H * xy_size^2 > 2^28; every set of the kind exported.
 * NOT PROVIDED: the cells swept between a primitive's two ends (keep the primitives short, or grow the footprint's margin);
 * primitives longer than 4 cells; a heading tolerance at goals; reading the field inside gvom_score_rollouts (gather D at the
 * rollouts' last poses); incremental repair after a map change; sharded handles. */
#define GVOM_PRODUCT_POSEFIELD 20   /* part 0 int32 D, part 1 uint8 action, part 2 uint16 pose cost: [H, xy, xy], strides (xy*xy, 1, xy) */
#define GVOM_POSE_GOAL 253
int gvom_primitives_set(gvom_t *h, int32_t n_headings, const int32_t *start /* [n_headings + 1] */, const int16_t *prims /* [start[n_headings]][4] */);
int gvom_pose_field(gvom_t *h, int64_t costfield_id, const int32_t *cost, int on_device, const int32_t *goals /* [n_goals][3] */,
                    int64_t n_goals, int32_t max_cost, int32_t max_rounds, int64_t *product_id, int64_t info[4]);

/* --- attitude volumes (an extension: pitch, roll and belly limits per heading, for the pose field -- a side slope the vehicle can climb
 * nose-first but would roll over on when crossing it is open in one heading and closed in another) ------------------------------------
 * gvom_attitude_volume computes, on the GPU, how the vehicle would sit on ONE float64 ground map at EVERY state of the window -- the
 * centre of each cell at each of the H headings of the footprint table -- with the footprint table gvom_footprint_set and the chassis
 * gvom_chassis_set gave the handle, and leaves the status and the tilt of every state in device memory as a product (kind
 * GVOM_PRODUCT_ATTITUDE_VOLUME) that gvom_device_product_export / _release / _dlpack / _copy handle like the others.
 * gvom_pose_field_attitude is gvom_pose_field with such a volume taken into its pose cost volume.  gvom_get_tuning "attitude_volume"
 * (read-only): 1 -- how a caller probes a library for the two entry points (an addition: GVOM_ABI_VERSION stays).
 *
 * DEFINITION.  The arithmetic is "terrain attitude scoring" above, word for word, for a pose that lies exactly in the centre of window
 * cell (cx, cy) with heading h, written relative to the window: the result does not depend on the window's origin.  All float64, one
 * IEEE operation each in the order written, no contraction.
 * GROUND     that section's, from a map set (map_set_id >= 0, flags GVOM_ATTITUDE_INFERRED_GROUND or 0) or the caller's (host or
 *            device memory as on_device says).
 * WHEEL CELL wheel i of heading h stands in cell (cx + floor(0.5 + wx[h][i] / res), cy + floor(0.5 + wy[h][i] / res)), wx and wy the
 *            wheel table of gvom_chassis_set.  A cell outside [0, xy) is outside the window.  z_i = g at that cell.
 * ATTITUDE, BELLY   zF, zR, zL, zT, sp, sr, z0, am, du, dv, u, v, plane, clr and belly are that section's formulas with fx = fy = 0.5;
 *            KNOWN is its rule.
 * STATUS     the first that applies: GVOM_ATTITUDE_LEFT_WINDOW: a wheel cell or a footprint cell is outside the window;
 *            _UNKNOWN_GROUND: a wheel cell's ground is unknown; _PITCH, _ROLL, _BELLY: decided on (float)sp, (float)sr, (float)belly
 *            against the float32 limits as there; _OK.  GVOM_ATTITUDE_INVALID cannot occur.
 * TILT       uint8.  0 where the status is UNKNOWN_GROUND or LEFT_WINDOW.  Elsewhere tp = (double)fabsf((float)sp) / (double)max_pitch
 *            * 100.0 if max_pitch is finite, else 0; tr likewise from the roll; t = tp > tr ? tp : tr;
 *            tilt = !(t > 0) ? 0 : (t >= 100 ? 100 : (uint8)floor(t)): how much of the nearer limit the state uses, in percent.
 * part 0 = uint8 status, part 1 = uint8 tilt: [H, xy, xy], indexed [h, x, y], strides (xy*xy, 1, xy) -- every plane has a pose field
 * plane's layout.  part 2 = int32 [8]: the number of states per status code 0 .. 6, then H.
 *
 * gvom_attitude_volume: on_device and the staging of a host ground map are gvom_score_attitude's; the call is enqueued on the handle's
 * stream and returns without a host wait (after the upload of a host map).  What depends on (heading, footprint cell) only is kept in a
 * table in device memory that the FIRST call after a gvom_footprint_set / gvom_chassis_set rebuilds on the stream (those two calls
 * allocate nothing for it).  The product is a snapshot: later scans, combines, gvom_footprint_set and gvom_chassis_set calls do not
 * change it.  Products of this kind live in the product-set pool ("device_product_sets"), sized by H and xy_size: at most
 * GVOM_MAX_PRODUCT_SETS; an unexported one goes back to the pool with the next gvom_attitude_volume call.
 * "attitude_volume_allocations" (read-only): device allocations the entry point has made on this handle (the table, the ground map of
 * the map-set route, the staging buffer of the host route and its product sets); it does not grow in steady state.
 * gvom_device_product(GVOM_PRODUCT_ATTITUDE_VOLUME) is GVOM_ERR_INVALID (this call makes them).  Kind 29 is not assigned.
 * GVOM_ERR_INVALID: a sharded handle; no footprint table set, no chassis set, or a chassis whose n_headings is not the table's; a set
 * id AND a ground pointer, or neither; an unknown or stale set id; unknown flag bits; NULL product_id.  GVOM_ERR_CAPACITY: H > 64;
 * xy_size > 4096; H * xy_size^2 > 2^28; every set of the kind exported.
 *
 * gvom_pose_field_attitude is gvom_pose_field -- the same arguments, checks, codes, product, info, tuning names and pool -- with
 * volume_id naming a live GVOM_PRODUCT_ATTITUDE_VOLUME of the same H and xy_size, read on the handle's stream behind the call that
 * wrote it.  Behind the pose cost volume C of "pose fields", C'[h][cell] = 0 where C == 0 or bit `status` of block_mask is set
 * (bit k = status code k), otherwise C' = min(65535, C + tilt_weight * tilt); seeding, relaxation, actions and part 2 of the product
 * take C' for C.  In addition GVOM_ERR_INVALID: block_mask > 0x7f; tilt_weight outside 0 .. 255; a stale volume id, an id of
 * another kind, or a volume of another H or xy_size.
 * NOT PROVIDED: float32 pitch / roll / belly volumes; states between cell centres; volumes over the atlas; sharded handles. */
#define GVOM_PRODUCT_ATTITUDE_VOLUME 30   /* part 0 uint8 status, part 1 uint8 tilt: [H, xy, xy], strides (xy*xy, 1, xy); part 2 int32 [8]; kind 29 stays unassigned */
int gvom_attitude_volume(gvom_t *h, int64_t map_set_id, const double *ground, int on_device, int flags, int64_t *product_id);
int gvom_pose_field_attitude(gvom_t *h, int64_t costfield_id, const int32_t *cost, int on_device, int64_t volume_id, uint32_t block_mask,
                             int32_t tilt_weight, const int32_t *goals /* [n_goals][3] */, int64_t n_goals, int32_t max_cost,
                             int32_t max_rounds, int64_t *product_id, int64_t info[4]);

/* --- map atlas (an extension: a world-fixed memory of the 2-D maps beyond the rolling window -- what the vehicle drove over a minute
 * ago is still known when it has to plan a way back) ------------------------------------------------------------------------------------
 * The atlas is a larger, toroidally stored copy of the nine maps of a map set plus a last-written stamp, in device memory, one per
 * handle.  Each device combine's set can be merged into it on the GPU (gvom_atlas_integrate), and any window-sized part of it comes
 * back as an ordinary map set (gvom_atlas_recall) that every call taking a map_set_id accepts.  gvom_get_tuning "atlas" (read-only):
 * the side A of the configured atlas, 0 without one -- how a caller probes a library for these entry points (an addition:
 * GVOM_ABI_VERSION stays).  Everything is copied or counted: the results are exact and do not depend on scheduling.
 *
 * DEFINITION.
 * CELLS      world cell (X, Y) is the integer voxel column index a map set's origin is counted in: a set with integer origin (Ox, Oy)
 *            holds cell (Ox + x, Oy + y) at [y*xy_size + x].  gvom_device_map_origin reads the integer origin of a live set.
 * STORAGE    A x A cells, A a power of two, 64 <= A <= 4096, A >= xy_size; ten planes: the six f64 maps and the three i32 maps of a
 *            set, and an int32 stamp; cell (X, Y) at [(Y & (A-1)) * A + (X & (A-1))] of each plane (the AND is the floor-modulo, also
 *            of negative coordinates).  64 bytes per cell, 1 GiB at 4096, allocated once by gvom_atlas_configure.
 * EXTENT     the A x A world cells [Ex, Ex+A) x [Ey, Ey+A) the atlas currently stands for.  gvom_atlas_configure sets E to
 *            fixed_origin ((0, 0) where that is NULL) and every cell to UNKNOWN.
 * UNKNOWN    positive 0, negative 0, visibility 0, roughness -1.0, height -1000.0, inferred height -1000.0, x slope 0.0, y slope 0.0,
 *            guessed delta 0.0, stamp 0: what a combine writes where it knows nothing.
 * RANK       of a cell's nine values: 2 (observed) iff visibility > 0; 1 (inferred) iff visibility <= 0 and (negative > 0 or inferred
 *            height > -1000.0); 0 otherwise.
 * INTEGRATE  of a set with origin O, two steps.  MOVE (GVOM_ATLAS_FOLLOW only): the extent goes to E' = O + floor(xy_size/2) - A/2 per
 *            axis; every cell of the new extent that was not in the old one becomes UNKNOWN (the cells that left lose their storage to
 *            these); a move of A or more on an axis makes everything UNKNOWN.  With GVOM_ATLAS_FIXED the extent never moves.  MERGE:
 *            seq is incremented (the first integrate after a configure has seq 1); for every cell of the set inside the extent, with
 *            r_new the rank of the set's values and r_old the rank of the atlas's, the cell is WRITTEN iff r_new >= 1 and r_new >=
 *            r_old -- all nine values copied bit for bit, stamp = seq -- and stays as it is otherwise.  Observed ground is never
 *            overwritten by an inference or by nothing; a cell that re-enters the window unseen keeps what was known about it.
 * COUNTERS   int32, in device memory, filled by wave-combined integer atomics.  gvom_atlas_counts -- the only atlas call that WAITS --
 *            reads out[0..5] of the last integrate: {written, kept (r_new >= 1 but < r_old), uninformative (inside the extent, r_new
 *            == 0), outside the extent, cells made UNKNOWN by the move, of those how many had rank >= 1}; out[6] cells of rank >= 1 in
 *            the atlas; out[7] seq.  The first four sum to xy_size^2.
 * RECALL     for any integer origin (Rx, Ry) (NULL: the last integrated set's): a complete map set of xy_size x xy_size cells -- the
 *            atlas's nine values where a cell lies in the extent, UNKNOWN elsewhere.  The set comes from the pool of at most 8 sets
 *            gvom_combine_maps_device takes its sets from, under the same rule: an unexported set goes back to the pool when the next
 *            device combine OR RECALL begins; its ready event is recorded on the handle's stream and its id comes from the same
 *            sequence: it is a map set in every respect.  origin_world (may be NULL) = (Rx, Ry) * xy_resolution, and the last
 *            integrated set's z origin * z_resolution (0 where pointers were integrated), which is informational: heights are world
 *            metres.  With it comes a product of kind GVOM_PRODUCT_ATLAS_RECALL: part 0 int32 [xy, xy], the stamps, [x, y]-indexed
 *            with strides (1, xy) like a device map; part 1 int32 [4] {cells of rank 2, cells of rank 1, cells outside the extent, seq}.
 *            Of this kind a handle holds up to 8 product sets, one per map set, not GVOM_MAX_PRODUCT_SETS.
 * EXTENT EXPORT   gvom_atlas_extent: a product of kind GVOM_PRODUCT_ATLAS_EXTENT, the whole extent unwrapped -- [A, A], [x, y]-indexed
 *            with strides (1, A), cell (Ex + x, Ey + y) at [y*A + x]: parts 0 positive, 1 negative, 2 visibility (int32), 3 roughness,
 *            4 height (f64), 5 stamp (int32); 32 bytes per cell.  extent_origin (may be NULL) receives (Ex, Ey).  Consumers that plan
 *            at atlas scale read it in place, or on a second handle through the *_of_device calls; the cost-to-go field of the whole
 *            extent needs neither ("atlas fields" below).
 *
 * INPUT of gvom_atlas_integrate, one of two.  map_set_id >= 0: a live device map set (maps and origin_cells must be NULL); the merge
 * runs on the handle's stream behind the combine or recall that wrote it.  map_set_id < 0: `maps`, nine pointers in set order (0
 * positive .. 8 guessed delta, [y][x], xy_size^2 elements each), and their integer origin; on_device != 0: device addresses, read in
 * place (the data must be ready when the call is made); on_device == 0: host arrays, staged through a buffer of the handle.
 * Integrate, recall, extent and clear ENQUEUE on the handle's stream and return (the host route of integrate waits for its upload).
 * gvom_atlas_configure(cells, mode, fixed_origin) allocates or re-allocates; cells == 0 frees.  gvom_atlas_clear sets every cell to
 * UNKNOWN and the counters to 0; the extent and seq stay.  "atlas_allocations" (read-only): device allocations the entry points have
 * made on this handle (the planes, the counters, the staging buffer of the host route and the product sets); it does not grow in
 * steady state.  gvom_device_product(kind 22 / 24) is GVOM_ERR_INVALID (these calls make them).  Kinds 21 and 23 are not assigned.
 * GVOM_ERR_INVALID: a sharded handle; no atlas configured; cells not a power of two, outside 64 .. 4096 or below xy_size; an unknown
 * mode; id and pointers mixed, or neither; a NULL map; a stale id; an origin beyond 2^40 cells; NULL outputs.  GVOM_ERR_CAPACITY: a
 * recall with all 8 map sets exported; every product set of the kind exported.
 * NOT PROVIDED: a coarser level or pyramid; a "latest wins" policy; time decay; more than one atlas per handle; sharded
 * handles; saving to disk; DLPack views of the toroidal planes themselves.  3-D memory is the voxel atlas's ("voxel atlas" below). */
#define GVOM_PRODUCT_ATLAS_RECALL 22   /* part 0 int32 [xy, xy] stamps; part 1 int32 [4] {rank 2, rank 1, outside, seq} */
#define GVOM_PRODUCT_ATLAS_EXTENT 24   /* parts 0 .. 2 int32 positive, negative, visibility; 3, 4 f64 roughness, height; 5 int32 stamp: [A, A], strides (1, A) */
#define GVOM_ATLAS_FOLLOW 0
#define GVOM_ATLAS_FIXED  1
int gvom_device_map_origin(gvom_t *h, int64_t map_set_id, int64_t origin_cells[3]);
int gvom_atlas_configure(gvom_t *h, int32_t cells, int mode, const int64_t fixed_origin[2] /* may be NULL */);
int gvom_atlas_integrate(gvom_t *h, int64_t map_set_id, const void *const maps[9], int on_device, const int64_t origin_cells[2]);
int gvom_atlas_recall(gvom_t *h, const int64_t origin_cells[2] /* may be NULL */, int64_t *map_set_id, int64_t *product_id, double origin_world[3]);
int gvom_atlas_extent(gvom_t *h, int64_t *product_id, int64_t extent_origin[2]);
int gvom_atlas_clear(gvom_t *h);
int gvom_atlas_counts(gvom_t *h, int64_t out[8]);

/* --- atlas fields (an extension: the cost-to-go field of everything the atlas remembers, and the part of it under any window -- the
 * global navigation function a local planner takes its terminal cost from) ---------------------------------------------------------------
 * gvom_atlas_cost_to_go solves "cost-to-go fields" on the atlas's WHOLE extent, reading the toroidal planes in place: no extent export,
 * no second handle.  gvom_atlas_field_window crops the result to any window as an ordinary cost field, which gvom_score_rollouts,
 * gvom_frontiers and gvom_pose_field accept like one gvom_cost_to_go made.  gvom_get_tuning "atlas_cost_to_go" (read-only) reads 1: how
 * a caller probes a library for these entry points (additions: GVOM_ABI_VERSION stays).  Integer arithmetic throughout: the results are
 * exact and do not depend on scheduling.
 *
 * DEFINITION of gvom_atlas_cost_to_go.
 * MAP        the extent at the moment of the call, [Ex, Ex+A) x [Ey, Ey+A): extent cell (x, y) is world cell (Ex + x, Ey + y), read from
 *            [((Ey+y) & (A-1)) * A + ((Ex+x) & (A-1))] of the atlas's planes.  The graph is the FLAT A x A grid: cells on opposite edges
 *            of the extent are adjacent in storage and are NOT neighbours.
 * HARD       a cell is hard iff (double)positive > density_threshold, or negative > 0 (not with GVOM_CTG_NO_NEGATIVE in flags).  d2 =
 *            gvom_clearance's squared cells of that obstacle set on the flat A x A grid, capped at inflation_cells2: obstacles anywhere
 *            in the extent inflate, nothing inflates across the extent's edge.
 * COST       the rule of "cost-to-go fields", cell for cell, with two clarifications an atlas needs because gvom_atlas_integrate lets
 *            any bit pattern in.  "Never observed" is visibility <= 0 (the atlas's rank < 2; in a map set the same as == 0): such a
 *            cell is blocked with GVOM_CTG_UNKNOWN_BLOCKS and pays unknown_cost.  An unblocked cost is min(65535, max(1, base +
 *            soft_weight * positive + ... )) in int64, which is the same wherever positive >= 0.  A NaN roughness gives q = 0 (r >
 *            min_roughness is false).
 * FIELD, DIRECTION   exactly D and dir of gvom_cost_to_go on that cost map: the eight steps, the corner rule, K = 5 / 7, max_cost,
 *            GVOM_CTG_UNREACHED / _GOAL / _NONE / _UNSETTLED.  goals: [n_goals][2] WORLD cells (x, y), 1 <= n_goals <= 65536; a goal
 *            outside the extent is GVOM_ERR_INVALID, a goal on a blocked cell seeds nothing.
 * The call WAITS like gvom_cost_to_go -- it returns on convergence or after max_rounds (> 0) rounds, with the same promises about a field
 * that is not final -- and runs on the handle's stream behind the last integrate.  info (may be NULL): the same four fields.
 * "cost_to_go_inner" / "cost_to_go_batch" shape its rounds too; "atlas_field_tiles" (read-only): tile relaxations of the last call.
 * The product, of kind GVOM_PRODUCT_ATLAS_FIELD, is a SNAPSHOT with its own memory and its own recorded extent origin, which
 * extent_origin (may be NULL) receives: later integrates, moves of the extent, gvom_atlas_clear and a re-configure do not touch it.
 * 7 bytes per cell, 117 MB at 4096.  At most GVOM_MAX_PRODUCT_SETS fields per handle; an unexported field goes back to the pool with
 * the next gvom_atlas_cost_to_go; with every one exported the call returns GVOM_ERR_CAPACITY.  The solver's buffers at side A (counters,
 * flags, goals; with an inflation the row distances and d2, 10 bytes per cell) are the handle's, apart from gvom_cost_to_go's.
 * GVOM_ERR_INVALID: a sharded handle; no atlas configured; NULL params, goals or product_id; unknown flag bits; the parameter errors of
 * gvom_cost_to_go; a goal outside the extent.
 *
 * gvom_atlas_field_window ENQUEUES and returns.  Give exactly one of map_set_id >= 0 (a live map set: its integer origin is the
 * window's) and origin_cells = (Rx, Ry) (within 2^40).  The result is a product of kind GVOM_PRODUCT_COSTFIELD, [xy, xy] with strides
 * (1, xy): cell (x, y) holds the field's D, dir and c of world cell (Rx + x, Ry + y), and GVOM_CTG_UNREACHED, GVOM_CTG_NONE and 0 where
 * that cell lies outside the FIELD's extent (the one it was made with, wherever the atlas is now).  It lives in the cost-field pool under
 * its rule -- an unexported one goes back with the next gvom_cost_to_go OR gvom_atlas_field_window -- and is a cost field in every
 * respect.  dir is copied as it is: at the crop's border a step may point out of the window, where the path goes on in the field.
 * GVOM_ERR_INVALID: a stale or unknown field_id; a set id and origin_cells, or neither; a stale set id; an origin beyond 2^40 cells; a
 * NULL product_id.  "atlas_field_allocations" (read-only): device allocations the two entry points have made on this handle (the
 * solver's buffers and the product sets of both kinds); it does not grow in steady state.  gvom_device_product(kind 26) is
 * GVOM_ERR_INVALID.  Kind 25 is not assigned.
 * NOT PROVIDED: a pose field at atlas scale; an age or stamp term in the cost; incremental repair of a field after an integrate; a coarser
 * level; sharded handles; goals in device memory; a path walk on the device; fields that follow the extent. */
#define GVOM_PRODUCT_ATLAS_FIELD 26   /* part 0 int32 D, part 1 uint8 dir, part 2 uint16 c: [A, A], strides (1, A); kind 25 stays unassigned */
int gvom_atlas_cost_to_go(gvom_t *h, const gvom_ctg_params *params, const int64_t *goals /* [n_goals][2] WORLD cells */,
                          int64_t n_goals, int32_t max_cost, int32_t max_rounds, int flags,
                          int64_t *product_id, int64_t info[4], int64_t extent_origin[2]);
int gvom_atlas_field_window(gvom_t *h, int64_t field_id, int64_t map_set_id, const int64_t origin_cells[2], int64_t *product_id);

/* --- atlas frontiers (an extension: where unexplored ground remains anywhere the vehicle has been, when the live window has no
 * frontier left -- one call instead of a recall, a crop and gvom_frontiers per window position, and no cluster cut at a window border) ---
 * gvom_atlas_frontiers runs "frontier extraction" on the WHOLE extent of an atlas field: the field's cell costs and cost to go, and the
 * atlas's visibility plane read in place as the atlas is NOW.  Every cluster comes with its nearest member and the global cost to reach
 * it.  gvom_get_tuning "atlas_frontiers" (read-only) reads 1: how a caller probes a library for this entry point (an addition:
 * GVOM_ABI_VERSION stays).  All arithmetic is integer: the result is exact and does not depend on scheduling.
 *
 * DEFINITION.
 * MAPS       field_id names a live GVOM_PRODUCT_ATLAS_FIELD of side Af with recorded origin F: c is its part 2, D its part 0; field cell
 *            (x, y) is world cell F + (x, y) and has linear index y*Af + x.
 * VISIBILITY comes from the atlas as it is at the moment of the call, with present extent E, side A and the storage phase of E: a world
 *            cell is KNOWN iff it lies in the present extent and visibility > 0, UNKNOWN iff it lies in the present extent and
 *            visibility <= 0 (the rule of "atlas fields": gvom_atlas_integrate lets any bit pattern in), and NEITHER outside the present
 *            extent.  The field is a snapshot: the extent may have moved, or the atlas may have been re-configured to another side,
 *            since the field was made.  The product lives in the FIELD's frame.
 * FRONTIER CELL u: c[u] > 0, and u is KNOWN, and D[u] < GVOM_CTG_UNREACHED, and at least one of its four edge neighbours lies inside
 *            the field's extent and is UNKNOWN.  The graph is the FLAT Af x Af grid: cells on opposite edges of the extent are not
 *            neighbours, and neither the field's edge nor the atlas's edge is a frontier.
 * CLUSTER, KEPT, RANK, the rows, the sums, the cluster map and the counts are exactly those of "frontier extraction" with xy_size
 *            replaced by Af: part 0 int32 [cap, 8], part 1 int64 [cap, 2], part 2 int32 [Af, Af] with strides (1, Af), part 3 int32 [4].
 *            Labels and best cells are linear indices in the field's frame; extent_origin (may be NULL) receives F.
 * The call WAITS, like gvom_frontiers, and runs on the handle's stream behind the last integrate and behind whatever wrote the field.
 * "frontier_batch" and "frontier_inner" shape its rounds too; "atlas_frontier_rounds" / "atlas_frontier_tiles" (read-only): rounds and
 * tile relaxations of the last call.  info (may be NULL): the four fields of gvom_frontiers.  A field that stopped early (max_rounds) is
 * accepted: the definition uses only D < GVOM_CTG_UNREACHED.
 * The product, of kind GVOM_PRODUCT_ATLAS_FRONTIERS, is a SNAPSHOT in the product-set pool under its rule: later integrates, moves,
 * clears and solves do not change it; an unexported one goes back with the next gvom_atlas_frontiers; with every one exported the call
 * returns GVOM_ERR_CAPACITY.  The work buffer at side Af (8 bytes per cell plus flags and counters, 128 MB at 4096) is the handle's,
 * apart from gvom_frontiers' window-sized one, which this call never touches.  "atlas_frontier_allocations" (read-only): device
 * allocations the entry point has made on this handle (that buffer and its product sets); it does not grow in steady state.
 * gvom_device_product(kind 28) is GVOM_ERR_INVALID.  Kind 27 is not assigned.
 * GVOM_ERR_INVALID: a sharded handle; no atlas configured; an unknown, stale or wrong-kind field_id; min_cells < 1; max_clusters outside
 * 1 .. 2^20; a NULL product_id.
 * NOT PROVIDED: a crop of the cluster map to a window; caller-supplied planes at atlas scale (the *_of routes); frontiers without D;
 * splitting of long clusters; a stamp or age filter; incremental re-labelling after an integrate. */
#define GVOM_PRODUCT_ATLAS_FRONTIERS 28   /* the four parts of kind 16 at side A; kind 27 stays unassigned */
int gvom_atlas_frontiers(gvom_t *h, int64_t field_id, int32_t min_cells, int32_t max_clusters,
                         int64_t *product_id, int64_t info[4], int64_t extent_origin[2] /* may be NULL */);

/* --- voxel atlas (an extension: the 3-D side of the map atlas -- a world-fixed memory of the voxels' classes beyond the rolling window,
 * with ray and viewpoint queries that run on it in place) -------------------------------------------------------------------------------
 * The exploration loop  atlas field -> frontiers -> viewpoint poses -> score viewpoints  hands back goals far outside the window, where
 * every beam of gvom_score_viewpoints is LEFT_WINDOW and a line of sight along a planned way back cannot be checked.  The voxel atlas
 * keeps, per handle, a toroidally stored, world-anchored grid of A x A x Z voxels at 2 bits each and answers gvom_raycast's and
 * gvom_score_viewpoints' questions on it.  Everything is exact: a voxel's class is a function of the fused state, the merge is bit
 * operations, the walk is k_raycast's with the extent in the window's place.  An addition: GVOM_ABI_VERSION stays.  gvom_get_tuning
 * "voxel_atlas" (read-only): A, or 0 without a voxel atlas -- how a caller probes a library for these entry points;
 * "voxel_atlas_levels": Z.
 *
 * VOXELS.  World voxel (X, Y, Zv) is the integer voxel index in which the fused map's window origin W is counted: window voxel
 * (x, y, z) is world voxel W + (x, y, z).
 * CLASS of a fused state s (what gvom_read_dense(GVOM_WHICH_FUSED) returns; a stale tile reads -1):  s >= 0: OCCUPIED (2);  s == -1:
 * NEVER (0);  otherwise FREE (1).
 * STORAGE.  A is a power of two, 64 <= A <= 4096, A >= xy_size; Z is a power of two, z_size <= Z <= A; A*A*Z <= 2^32 (1 GiB).  The
 * atlas is toroidal on all three axes.  Nothing outside the library depends on the layout.
 * EXTENT.  [Ex, Ex+A) x [Ey, Ey+A) x [Ez, Ez+Z).  gvom_voxel_atlas_configure sets E to fixed_origin ((0, 0, 0) where that is NULL) and
 * every voxel to NEVER.  Every component of E and of an integrated W must stay below 2^30 in magnitude (GVOM_ERR_INVALID otherwise).
 *
 * INTEGRATE (gvom_voxel_atlas_integrate) merges the CURRENT fused map -- the map of the most recently begun combine, exactly as for
 * gvom_raycast -- in two steps.
 *   MOVE, in GVOM_ATLAS_FOLLOW mode only:  E'xy = Wxy + floor(xy_size / 2) - A / 2 (the map atlas's rule: both atlases cover the same
 *   cells when they follow the same combines),  E'z = Wz + floor(z_size / 2) - Z / 2.  Every voxel of the new extent that was not in the
 *   old one becomes NEVER; a move of a whole side or more on any axis clears everything.  GVOM_ATLAS_FIXED never moves.
 *   MERGE increments seq.  For every window voxel inside the extent, with c the class of its fused state:  c == NEVER: the atlas voxel
 *   stays as it is;  otherwise the atlas voxel becomes c.  The current window is the authority wherever it has observed something; a
 *   voxel that left the ring buffer, or re-enters the window unseen, keeps what was known.
 * COUNTS (gvom_voxel_atlas_counts, the only call that waits).  int64 out[11].  Of the last integrate: [0] first seen (old NEVER), [1]
 * free -> occupied, [2] occupied -> free, [3] confirmed (same class), [4] uninformative (inside the extent, c == NEVER), [5] outside the
 * extent -- [0] .. [5] sum to xy_size^2 * z_size --, [6] voxels made NEVER by the move, [7] of those, how many were observed.  Of the
 * atlas: [8] observed voxels, [9] occupied voxels, [10] seq.  All are integer sums of population counts, exact whatever the schedule.
 * BOX (gvom_voxel_atlas_box).  Any integer origin (Bx, By, Bz) -- NULL: the last integrated window's W, and GVOM_NO_DATA where nothing
 * has been integrated since gvom_voxel_atlas_configure -- gives a product of kind
 * GVOM_PRODUCT_VOXEL_BOX: part 0 uint8 [xy, xy, z] in the occupancy grid's layout, the class codes 0 / 1 / 2, 0 outside the extent;
 * part 1 int32 [4] {occupied, free, voxels outside the extent, seq}.  part 0 == 2 is an occupancy grid of remembered space.
 * origin_out (may be NULL) receives B.
 * RAYS.  gvom_voxel_atlas_raycast is gvom_raycast's DEFINITION word for word with  W := E,  the window's sizes (A, A, Z),  "fused state
 * of v" := the atlas class of v (OCCUPIED stops, NEVER counts as unknown),  LEFT_WINDOW := left the extent,  and the step cap A + Z + 1.
 * The ray set-up, the float32 additions, the literal float64 lookup, the sqrt typing, the flags and the INVALID rule are the same.
 * Product kind GVOM_PRODUCT_VOXEL_ATLAS_RAYS: part 0 int32 [n, 3] {status, steps, unknown}; part 1 float32 [n, 3] stop position; part 2
 * int32 [n, 3] the WORLD voxel of the stop, (0, 0, 0) where gvom_raycast reports voxel -1 (a window voxel index would not fit int32 at
 * A = 4096).  n <= 2^26; host and device routes, no host wait on the device route; a snapshot product, as for gvom_raycast.
 * extent_voxels (may be NULL) receives E.
 * VIEWPOINTS.  gvom_voxel_atlas_score_viewpoints takes gvom_score_viewpoints' arguments and has its definition with the same
 * substitutions; kind GVOM_PRODUCT_VOXEL_ATLAS_VIEWPOINTS in the layout of kind 18.  Only the result is defined: the gain counts
 * DISTINCT world voxels.  The library deduplicates in one bitmap per pose over a box that it proves to contain every voxel a beam of
 * that pose can examine -- from the model's largest |direction| and |offset| per axis, max_range, the pose's matrix and translation
 * (directions need not be unit vectors), widened by the float32 rounding of the walk and clipped to the extent.  The bitmaps live under
 * the "viewpoint_bitmap_mb" budget with gvom_score_viewpoints' batching; the setting changes time and memory, never the result.  The
 * boxes are the host's to prove: the device route reads the poses back (K x 96 bytes) and so WAITS for the handle's stream, and the
 * first call after a gvom_sensor_model_set reads the model back once.
 * GVOM_ERR_CAPACITY: K > 65536; more than 2^22 selected beams; beams * (A + Z + 1) >= 2^31; a per-pose box of 2^31 bits or more.
 *
 * GVOM_NO_DATA before the first combine (integrate and the queries).  GVOM_ERR_INVALID: a sharded handle; no voxel atlas configured;
 * sizes outside the rules above; an unknown mode; an origin at or beyond 2^30; NULL outputs; unknown flag bits; gvom_raycast's and
 * gvom_score_viewpoints' argument errors.  Products live in the product-set pool: at most GVOM_MAX_PRODUCT_SETS per kind; an unexported
 * one goes back to the pool with the next call of its kind.  gvom_voxel_atlas_configure(cells, levels, mode, fixed_origin) allocates or
 * re-allocates; cells == 0 frees.  gvom_voxel_atlas_clear sets every voxel to NEVER and the counters to 0; the extent and seq stay.
 * "voxel_atlas_allocations" (read-only): device allocations the entry points have made on this handle (the atlas, its counters, the
 * staging buffer, bitmaps and product sets); it does not grow in steady state.  "voxel_atlas_viewpoint_batch" (read-only, a
 * diagnostic): poses per kernel launch of the last gvom_voxel_atlas_score_viewpoints, 0 before the first -- what the
 * "viewpoint_bitmap_mb" budget came to.  gvom_device_product(kind 32 / 34 / 36) is
 * GVOM_ERR_INVALID (these calls make them).  Kinds 31, 33 and 35 are not assigned.
 * NOT PROVIDED: stamps or time decay; hit counts; a stored "near" plane ("voxel atlas alignment" below derives the class per call);
 * integrating a caller's dense grid; more than one voxel atlas per handle; sharded handles; saving to disk. */
#define GVOM_PRODUCT_VOXEL_BOX 32               /* part 0 uint8 [xy, xy, z] class codes; part 1 int32 [4] {occupied, free, outside, seq} */
#define GVOM_PRODUCT_VOXEL_ATLAS_RAYS 34        /* part 0 int32 [n, 3] {status, steps, unknown}; part 1 float32 [n, 3]; part 2 int32 [n, 3] world voxel */
#define GVOM_PRODUCT_VOXEL_ATLAS_VIEWPOINTS 36  /* the two parts of kind 18 */
#define GVOM_VOXEL_NEVER 0
#define GVOM_VOXEL_FREE 1
#define GVOM_VOXEL_OCCUPIED 2
int gvom_voxel_atlas_configure(gvom_t *h, int32_t cells, int32_t levels, int mode, const int64_t fixed_origin[3] /* may be NULL */);
int gvom_voxel_atlas_integrate(gvom_t *h);
int gvom_voxel_atlas_clear(gvom_t *h);
int gvom_voxel_atlas_counts(gvom_t *h, int64_t out[11]);
int gvom_voxel_atlas_box(gvom_t *h, const int64_t origin[3] /* may be NULL */, int64_t *product_id, int64_t origin_out[3] /* may be NULL */);
int gvom_voxel_atlas_raycast(gvom_t *h, const float *from /* [K][3] */, int64_t K, const float *to /* [n][3] */, int64_t n,
                             int on_device, int flags, int64_t extent_voxels[3], int64_t *product_id);
int gvom_voxel_atlas_score_viewpoints(gvom_t *h, const double *poses /* [K][12] */, int64_t K, int on_device, double max_range,
                                      int32_t stride_h, int32_t stride_w, int flags, int64_t extent_voxels[3], int64_t *product_id);

/* --- voxel atlas alignment (an extension: relocalise on remembered space -- scan alignment scoring against the voxel atlas, for a scan
 * whose returns end outside the rolling window) ----------------------------------------------------------------------------------------
 * gvom_score_alignments reads only the current fused map: a scan held against what the vehicle saw a minute ago finds every return
 * OUTSIDE.  gvom_voxel_atlas_score_alignments holds the cloud against any window-sized BOX of the voxel atlas instead.  Everything is
 * exact.  An addition: GVOM_ABI_VERSION stays.  gvom_get_tuning "voxel_atlas_alignments" (read-only): 1 -- how a caller probes a library
 * for this entry point.
 *
 * DEFINITION.  gvom_voxel_atlas_score_alignments is gvom_score_alignments' DEFINITION ("scan alignment scoring") word for word, with
 * three substitutions.
 * window := the BOX  [Bx, Bx+xy_size) x [By, By+xy_size) x [Bz, Bz+z_size) in world voxels: the size of the mapper's window, at any
 *            integer origin that gvom_voxel_atlas_box accepts.  A NULL origin means the last integrated window's W, and the call returns
 *            GVOM_NO_DATA where nothing has been integrated since gvom_voxel_atlas_configure, exactly as the box call does.  The window
 *            origin of the endpoint rule  floor((double)w / res - W)  becomes B, and OUTSIDE means outside the box.
 * class of a voxel := a function of the ATLAS alone, never of where the box lies, in this order:  OCCUPIED if the atlas class is
 *            GVOM_VOXEL_OCCUPIED;  NEAR if dilate == 1 and an occupied voxel OF THE EXTENT lies within one voxel on every axis -- voxels
 *            outside the box but inside the extent count; voxels outside the extent are NEVER and do not count;  FREE if the atlas class
 *            is GVOM_VOXEL_FREE;  UNKNOWN otherwise.  A box voxel outside the extent is UNKNOWN.
 * Everything else is unchanged: the transform rule, the float64 inside test, n, K, the pair and weight limits, the score and the lowest
 *            index of the best score.  res and the division form are the mapper's.
 * CONSEQUENCES.  Two boxes give a world voxel the same class.  After ONE integrate into a fresh atlas, with B = W, the result equals
 * gvom_score_alignments' bit for bit, dilate 1 included: nothing outside the window is known yet.  The call is read-only on the atlas.
 * It enqueues and returns: the handle knows the extent on the host, so there is no host wait on the device route, and the host route
 * waits only for its upload.
 * The product, of kind GVOM_PRODUCT_VOXEL_ATLAS_ALIGNMENT, has the two parts of kind 12: part 0 int32 [K, 6] {score, occupied, near,
 * free, unknown, outside}, part 1 int32 [4] {best index, best score, n, K}; a snapshot in the product-set pool under its rule.
 * origin_out (may be NULL) receives B.  The class grid is rebuilt from the atlas's bit planes in every call, in the buffer that
 * gvom_score_alignments uses ("alignment_grid_bytes"; its allocation counts in "alignment_allocations", the product sets and the host
 * route's staging buffer in "voxel_atlas_allocations"; neither grows in steady state).  gvom_device_product(kind 38) is
 * GVOM_ERR_INVALID.  Kind 37 is not assigned.
 * The refusals are gvom_score_alignments' (GVOM_ERR_INVALID: NULL cloud / transforms / weights / product_id, n < 1, K < 1, dilate other
 * than 0 or 1, |weight| > 1024;  GVOM_ERR_CAPACITY: n > 2^20, K > 65536, n * K > 2^32, a class grid of 2^32 words or more, every set of
 * the kind exported) and the voxel atlas calls' (GVOM_ERR_INVALID: a sharded handle, no voxel atlas configured;  GVOM_NO_DATA before the
 * first combine, and with a NULL origin before the first integrate).
 * NOT PROVIDED: boxes of other sizes than the window; a cache of the class grid keyed on the atlas's seq; float64 clouds; sharded
 * handles; a coarse-to-fine search driver. */
#define GVOM_PRODUCT_VOXEL_ATLAS_ALIGNMENT 38   /* the two parts of kind 12; kind 37 stays unassigned */
int gvom_voxel_atlas_score_alignments(gvom_t *h, const float *cloud /* [n][3] */, int64_t n, const double *transforms /* [K][3][4] */, int64_t K,
                                      int on_device, int dilate, const int32_t weights[5], const int64_t origin[3] /* may be NULL */,
                                      int64_t origin_out[3] /* may be NULL */, int64_t *product_id);

/* --- voxel distance field (an extension: exact 3-D clearance from the voxel atlas -- how far every voxel of a box is from the nearest
 * remembered obstacle, under overhangs that a 2-D column reduction flattens away) ---------------------------------------------------------
 * gvom_clearance is the distance transform of the 2-D obstacle mask; the 3-D side answered only "what class is this voxel" and "where
 * does this ray stop".  gvom_voxel_atlas_distance_field gives the truncated Euclidean distance field of a window-sized box of the voxel
 * atlas, in metres, exact under the definition below; gvom_voxel_distance_sample reads such a field at world points (body spheres, scan
 * returns).  An addition: GVOM_ABI_VERSION stays.  gvom_get_tuning "voxel_distance_field" (read-only): 1 -- how a caller probes a
 * library for these entry points.
 *
 * BOX.  [Bx, Bx+xy_size) x [By, By+xy_size) x [Bz, Bz+z_size) in world voxels, at any integer origin that gvom_voxel_atlas_box accepts.
 * A NULL origin means the last integrated window's W; GVOM_NO_DATA exactly where gvom_voxel_atlas_box returns it.  Part 0 has the
 * class grid's layout, out[x][y][z]: it lines up voxel for voxel with the box call's classes and with the occupancy grid.
 * SOURCES.  Every world voxel whose atlas class is GVOM_VOXEL_OCCUPIED; with GVOM_DISTANCE_UNKNOWN_BLOCKS also every voxel whose class
 * is GVOM_VOXEL_NEVER.  A voxel outside the extent is NEVER, as for the box call: under the flag everything outside the extent is a
 * source.  Sources are NOT restricted to the box: a remembered obstacle just beyond a face of the box decides the distances near it.
 * VALUE.  For a box voxel v,
 *     d2(v) = min over sources s of  fl64( fl64(a * n) + fl64(b * m) ),   n = (sx-vx)^2 + (sy-vy)^2,  m = (sz-vz)^2,
 * n and m exact integers converted to double,  a = fl64(xy_resolution * xy_resolution),  b = fl64(z_resolution * z_resolution), from
 * the handle's double parameters, no contraction.  out(v) = (float)sqrt(d2) -- a float64 root, rounded once to float32 -- where
 * d2 <= cap2 = fl64(max_distance * max_distance), else +infinity.  Distances run between voxel centres; a source voxel reads 0.
 * max_distance is mandatory, finite and > 0: the field is truncated.
 * EXACTNESS.  The result inside the box is exact with respect to the WHOLE extent: a source further than the halo on an axis cannot be
 * within the cap.  Hxy = the largest h with fl64(a * (double)(h*h)) <= cap2, Hz the same with b; the host computes both in exactly
 * this arithmetic ("voxel_distance_halo_xy" / "voxel_distance_halo_z", read-only: those of the last call).  Both terms are monotone in
 * |dx|, |dy| and |dz| and fl64 is monotone, so the minimum commutes with a separable evaluation -- integer passes in x and y that give
 * n_min per level, then a float64 pass over fl64(a * n_min(dz)) + fl64(b * dz^2) -- and the minimum of a set of doubles is unique even
 * where the nearest source is not: the result does not depend on the schedule.
 * COUNTS.  Part 1, int32 [4]: voxels at distance 0; voxels with a finite distance; box voxels outside the extent; the atlas's seq.
 * SAMPLE.  gvom_voxel_distance_sample takes a live product of kind GVOM_PRODUCT_VOXEL_DISTANCE of this handle and n world points in
 * metres, float32 [n][3], 1 <= n <= 2^26, in host memory or (on_device) in device memory.  The voxel of a point is
 * floor((double)p / resolution) per axis, a float64 division.  Part 0, float32 [n]: the field's value at that voxel; NaN where the voxel
 * lies outside the field's box or a coordinate is not finite.  Part 1, int32 [4]: {points inside the box, of those finite, of those at
 * 0, n}.  Read-only on the field; the gather runs on the handle's stream, in front of whatever reuses the field's set later, so the
 * caller may release the field as soon as the call returns (as gvom_score_rollouts treats its cost field).
 *
 * Neither call waits for the GPU (the host route of the sample call waits for its upload).  GVOM_ERR_INVALID: a sharded handle; no voxel
 * atlas configured; NULL product_id; a NaN, non-positive or infinite max_distance; unknown flag bits; NULL points; n < 1; a
 * field_product_id that is not a live product of kind 40 of this handle.  GVOM_ERR_CAPACITY, with the handle unchanged: a halo of more
 * than 32767 voxels; n > 2^26; working buffers -- the halo-grown intermediates of the x and y passes -- beyond the budget
 * "voxel_distance_mb" megabytes (gvom_set_tuning; default 256, at most 4096, < 0: the default); every set of the kind exported.  The
 * working buffer is grow-only; it and the product sets count in "voxel_atlas_allocations", which does not grow in steady state.
 * gvom_device_product(kind 40 / 42) is GVOM_ERR_INVALID.  Kinds 39 and 41 are not assigned.
 * NOT PROVIDED: a signed distance inside obstacles; nearest-source indices and gradients; interpolation between voxels in the sample
 * call; an unbounded field; incremental updates between integrates; sharded handles; a field of the whole extent. */
#define GVOM_PRODUCT_VOXEL_DISTANCE 40          /* part 0 float32 [xy, xy, z] metres, part 1 int32 [4]; kind 39 is not assigned */
#define GVOM_PRODUCT_VOXEL_DISTANCE_SAMPLES 42  /* part 0 float32 [n], part 1 int32 [4]; kind 41 is not assigned */
#define GVOM_DISTANCE_UNKNOWN_BLOCKS 1          /* flags */
int gvom_voxel_atlas_distance_field(gvom_t *h, const int64_t origin[3] /* may be NULL */, double max_distance, int flags,
                                    int64_t *product_id, int64_t origin_out[3] /* may be NULL */);
int gvom_voxel_distance_sample(gvom_t *h, int64_t field_product_id, const float *points /* [n][3] */, int64_t n, int on_device,
                               int64_t *product_id);

/* --- body clearance scoring (an extension: rollouts against the 3-D distance field -- does the body pass under the branch, the gate bar,
 * the bridge once the vehicle sits on that ground, nose up on the ramp or tilted on the side slope) -----------------------------------------
 * gvom_score_rollouts says what the footprint touches on the 2-D cost map and gvom_score_attitude how the vehicle sits on the ground.
 * gvom_score_body places a BODY of spheres, set once with gvom_body_set, at K trajectories of T poses each on ONE float64 ground map, reads
 * a voxel distance field at every sphere's centre -- one kernel, one gather per sphere -- and leaves the result in device memory as a
 * product (kind GVOM_PRODUCT_BODY) that gvom_device_product_export / _release / _dlpack / _copy handle like the others.  gvom_get_tuning
 * "body" (read-only): 1 -- how a caller probes a library for these entry points (an addition: GVOM_ABI_VERSION stays); "body_spheres"
 * (read-only): S while a table is set, else 0.  Every float64 operation below is ONE IEEE operation in the order written, parentheses
 * binding, no contraction; sqrt and / are the correctly rounded float64 ones; the library calls no trigonometric function: the result is
 * exact, and every decision is taken on the float32 values that are stored.
 *
 * DEFINITION.  res = xy_resolution, zres = z_resolution, xy = xy_size, o = origin_cells.
 * BODY       S spheres, 1 <= S <= 256, float32 [S][4] = (bx, by, bz, r): (bx, by) in the chassis's body frame (x forward, y left, origin
 *            at the pose), bz the height above the wheels' contact plane, r >= 0 the radius, all metres.
 * POSES, CENTRE, HEADING, INVALID   those of rollout scoring above, word for word; H is the footprint table's and (c, s) = cos_sin[k]
 *            comes from gvom_chassis_set.  A footprint table and a chassis with equal H must be set, as for gvom_score_attitude.
 * GROUND     terrain attitude scoring's GROUND, word for word: map_set_id >= 0 with GVOM_ATTITUDE_INFERRED_GROUND or 0 in flags (ground
 *            must be NULL), or the caller's float64 map with origin_cells.  The wheel cells, zFL .. zRR, sp, sr, z0 and am are that
 *            section's, word for word.  Only the four wheel cells are tested against the window: the footprint cells are not walked.
 * FIELD      one of two.  field_product_id >= 0: a live product of kind GVOM_PRODUCT_VOXEL_DISTANCE of this handle; (Bx, By, Bz) is the box
 *            origin it was made with, field and field_origin must be NULL.  field_product_id < 0: the caller's float32
 *            [xy_size][xy_size][z_size] in the class grid's layout, out[x][y][z], with (Bx, By, Bz) = field_origin[3] in world voxels,
 *            each within 2^40; host or device memory as on_device says, like the ground.  READ-ONLY on the field: the kernel runs on the
 *            handle's stream in front of whatever reuses the field's set, so the caller may release the field as soon as the call
 *            returns (gvom_voxel_distance_sample's rule).
 * FRAME      per pose, float64:  lu = sqrt(1.0 + sp*sp);  ln = sqrt((1.0 + sp*sp) + sr*sr);
 *            e1 = (e1u, 0, e1w) = (1.0/lu, 0, sp/lu)          along the chassis, nose up positive;
 *            n  = (nu, nv, nw)  = (-sp/ln, -sr/ln, 1.0/ln)    the contact plane's normal;
 *            e2 = n x e1 = (e2u, e2v, e2w) = (nv*e1w, nw*e1u - nu*e1w, -(nv*e1u))   to the left;
 *            q0 = z0 - sp*am                                  the contact plane's height under the pose.
 * SPHERE CENTRE   for (bx, by, bz), each widened to double:
 *            Cu = (bx*e1u + by*e2u) + bz*nu;  Cv = by*e2v + bz*nv;  Cw = ((bx*e1w + by*e2w) + bz*nw) + q0;
 *            X = (double)x + (Cu*c - Cv*s);  Y = (double)y + (Cu*s + Cv*c);  Z = Cw.
 *            Its voxel: floor(X / res) - Bx, floor(Y / res) - By, floor(Z / zres) - Bz.  It is OUTSIDE the box if it is not in range or
 *            |quotient| < 2^30 does not hold on some axis (NaN included).  The world height of the maps is (min_height + z + origin_z) *
 *            z_resolution, so the ground under a wheel lies in the voxel floor(g / zres): the frames agree without an offset.
 * MARGIN     m_i = d_i - r_i, one float32 subtraction, d_i the field's value at the sphere's voxel (+inf stays +inf).  clearance = the
 *            least m_i; a NaN m_i is skipped by the minimum (a caller's field may contain NaN, a product's cannot).  tightest = the
 *            lowest i that attains the least margin; 255 with clearance = +inf if every margin was skipped.
 * STATUS     per pose, the first that applies: GVOM_BODY_INVALID; _LEFT_WINDOW: a wheel cell is outside the window; _UNKNOWN_GROUND: a
 *            wheel cell's ground is unknown; _LEFT_BOX: a sphere's voxel is outside the box; _COLLISION: clearance < min_margin, a
 *            float32 comparison; _OK.  min_margin is finite.
 * part 1 = float32 [K, T] clearance, 0 where the status is INVALID, LEFT_WINDOW, UNKNOWN_GROUND or LEFT_BOX.
 * part 2 = uint8 [K, T, 2] {status, tightest}, tightest = 0 in those four cases.
 * part 0 = int32 [K, 4] {status, first_bad, tightest_pose, tightest_sphere}: first_bad = the smallest t whose status is not OK, or T;
 *            status = that pose's, or OK; tightest_pose = the lowest t < first_bad with the least clearance and tightest_sphere that
 *            pose's tightest, both -1 when first_bad == 0.  Row i = rollout i.  Every pose is evaluated: nothing depends on scheduling.
 * WHAT THE NUMBER MEANS   the field runs between voxel centres, and the ground is remembered as occupied voxels too: a body is clear of
 *            every remembered voxel centre where clearance >= the voxel's half diagonal.  Spheres model the body above the belly, not
 *            the wheels.
 *
 * gvom_body_set validates the table, copies it to the device on the handle's stream -- behind whatever still reads the previous one --
 * and returns after the copy.  A later call replaces the table; products made with the old table are unchanged.  GVOM_ERR_INVALID: NULL
 * arguments, S outside 1 .. 256, a non-finite entry, r < 0.
 * gvom_score_body: on_device, staging, the snapshot, the pool (sized by K and T) and the limits (T in 1 .. 4096, K * T <= 2^26, xy_size
 * <= 4096) are gvom_score_attitude's; on_device says where the poses, the ground and the field pointers lie.  gvom_get_tuning
 * "body_allocations" (read-only): device allocations the two entry points have made on this handle (the table, the ground map of the
 * map-set route, the staging buffer of the host route and the product sets); it does not grow in steady state at a fixed K, T and route.
 * gvom_device_product(GVOM_PRODUCT_BODY) is GVOM_ERR_INVALID (this call makes them).  Kind 43 is not assigned.
 * GVOM_ERR_INVALID: a sharded handle; no footprint table, no chassis, or unequal H; no body table; a set id AND a ground pointer, or
 * neither; an unknown or stale set id; a field id AND a field pointer or origin, or neither; a stale field id or one of another kind; a
 * NULL field_origin on the pointer route or one beyond 2^40 voxels; a NaN or infinite min_margin; unknown flag bits; T outside 1 .. 4096;
 * K < 1; NULL poses / origin_cells / product_id; an origin beyond 2^40 cells.  GVOM_ERR_CAPACITY: K * T > 2^26; xy_size > 4096; every set
 * of the kind exported.
 * NOT PROVIDED: interpolation in the field; capsules or boxes; poses with their own z; suspension; sharded handles; interpolation
 * between poses. */
#define GVOM_PRODUCT_BODY 44   /* part 0 int32 [K, 4] {status, first_bad, tightest_pose, tightest_sphere}; part 1 float32 [K, T] clearance; part 2 uint8 [K, T, 2] {status, tightest} */
/* 43 stays unassigned: tests/body_layout_host_test.cpp holds it to "no such kind" */
#define GVOM_BODY_OK 0
#define GVOM_BODY_COLLISION 1
#define GVOM_BODY_LEFT_BOX 2
#define GVOM_BODY_UNKNOWN_GROUND 3
#define GVOM_BODY_LEFT_WINDOW 4
#define GVOM_BODY_INVALID 5
int gvom_body_set(gvom_t *h, const float *spheres /* [S][4] */, int32_t S);
int gvom_score_body(gvom_t *h, int64_t field_product_id, const float *field, const int64_t field_origin[3], int64_t map_set_id,
                    const double *ground, const float *poses /* [K][T][3] */, int64_t K, int64_t T, int on_device, int flags,
                    const int64_t origin_cells[2], float min_margin, int64_t *product_id);

/* --- body volumes (an extension: 3-D body clearance per heading at every cell of the window, and the pose field that plans through it --
 * the gate bar the low vehicle drives under is no wall, and the tall vehicle goes round) --------------------------------------------------
 * gvom_score_body says whether the sphere body passes at poses a caller already chose.  gvom_body_volume evaluates the same arithmetic at
 * EVERY state (cell centre, heading) of the window -- one kernel, no pose array -- and leaves the result in device memory as a product
 * (kind GVOM_PRODUCT_BODY_VOLUME) that gvom_device_product_export / _release / _dlpack / _copy handle like the others.
 * gvom_pose_field_volumes is gvom_pose_field with an attitude volume, a body volume, or both taken into its pose cost volume.
 * gvom_get_tuning "body_volume" (read-only): 1 -- how a caller probes a library for these entry points (an addition: GVOM_ABI_VERSION
 * stays).  Every float64 operation below is ONE IEEE operation in the order written, no contraction: the result is exact, and every
 * decision is taken on the float32 values that are stored.
 *
 * DEFINITION.  res = xy_resolution, xy = xy_size, o = origin_cells, |o| <= 2^40.
 * STATE      (cx, cy, h): the centre of window cell (cx, cy) at heading h of the footprint table; (c, s) = cos_sin[h] of gvom_chassis_set.
 *            A footprint table, a chassis of equal H and a body table (gvom_body_set) must be set.  GVOM_BODY_INVALID cannot occur.
 * GROUND, FIELD   "body clearance scoring"'s, word for word: a map set (flags GVOM_ATTITUDE_INFERRED_GROUND or 0) or the caller's float64
 *            map; a live GVOM_PRODUCT_VOXEL_DISTANCE or the caller's float32 field with field_origin[3].  READ-ONLY on the field: the
 *            caller may release it as soon as the call returns.
 * WHEEL CELLS, STANCE   "attitude volumes"' rule, word for word: wheel i of heading h stands in cell (cx + floor(0.5 + wx[h][i] / res),
 *            cy + floor(0.5 + wy[h][i] / res)), window-relative; z_i = g at that cell; KNOWN, sp, sr, z0 and am are that section's.  Only
 *            the four wheel cells are tested against the window: the footprint cells are not walked.
 * FRAME, SPHERE CENTRE, MARGIN   "body clearance scoring"'s, word for word: e1, n, e2, q0; Cu, Cv, Cw; m_i, clearance and tightest.  The
 *            pose's world position is X0 = ((double)(ox + cx) + 0.5) * res, Y0 = ((double)(oy + cy) + 0.5) * res;
 *            X = X0 + (Cu*c - Cv*s);  Y = Y0 + (Cu*s + Cv*c);  Z = Cw.  The voxel and the OUTSIDE rule are that section's.
 * STATUS     the first that applies: GVOM_BODY_LEFT_WINDOW: a wheel cell is outside the window; _UNKNOWN_GROUND: a wheel cell's ground is
 *            unknown; _LEFT_BOX: a sphere's voxel is outside the box; _COLLISION: clearance < min_margin, a float32 comparison; _OK.
 * SQUEEZE    uint8: how much of the band between soft_margin and min_margin the state has used up.  0 where the status is LEFT_WINDOW,
 *            UNKNOWN_GROUND or LEFT_BOX.  Elsewhere, with m = min_margin, f = soft_margin (finite, f >= m), k = clearance, all float32:
 *            0 if k >= f; 100 if k <= m or f == m; otherwise t = ((double)f - (double)k) / ((double)f - (double)m) * 100.0 and
 *            squeeze = !(t > 0) ? 0 : (t >= 100 ? 100 : (uint8)floor(t)).  A clearance of +inf gives 0.
 * part 0 = uint8 status, part 1 = uint8 squeeze, part 2 = float32 clearance (0 where the status is LEFT_WINDOW, UNKNOWN_GROUND or
 * LEFT_BOX): each [H, xy, xy], indexed [h, x, y], strides (xy*xy, 1, xy) -- every plane has a pose field plane's layout.
 * part 3 = int32 [8]: the number of states per status code 0 .. 5, then H, then S.
 *
 * gvom_body_volume: on_device, the flags and the staging of a host field and ground map are gvom_score_body's; the call is enqueued on the
 * handle's stream and returns without a host wait (after the upload of host inputs).  The wheel offsets come from the attitude volume's
 * table, rebuilt by the same rule (the first call of either entry point after a gvom_footprint_set / gvom_chassis_set).  The product is a
 * snapshot: later scans, combines, integrates, gvom_footprint_set, gvom_chassis_set and gvom_body_set calls do not change it.  Products
 * of this kind live in the product-set pool ("device_product_sets"), sized by H and xy_size: at most GVOM_MAX_PRODUCT_SETS.
 * "body_volume_allocations" (read-only): device allocations the entry point has made on this handle (the ground map of the map-set
 * route, the staging buffer of the host route and its product sets); it does not grow in steady state.
 * gvom_device_product(GVOM_PRODUCT_BODY_VOLUME) is GVOM_ERR_INVALID (this call makes them).  Kind 45 is not assigned.
 * Errors: the union of gvom_score_body's and gvom_attitude_volume's.  GVOM_ERR_INVALID: a sharded handle; no footprint table, no
 * chassis, or unequal H; no body table; a set id AND a ground pointer, or neither; an unknown or stale set id; a field id AND a field
 * pointer or origin, or neither; a stale field id or one of another kind; a NULL field_origin on the pointer route or one beyond 2^40
 * voxels; a NaN or infinite min_margin; a NaN or infinite soft_margin; soft_margin < min_margin; unknown flag bits; NULL origin_cells /
 * product_id; an origin beyond 2^40 cells.  GVOM_ERR_CAPACITY: H > 64; xy_size > 4096; H * xy_size^2 > 2^28; every set of the kind
 * exported.
 *
 * gvom_pose_field_volumes is gvom_pose_field -- the same arguments, checks, codes, product, info, tuning names and pool -- with two
 * optional volumes.  Either volume id may be -1 (none); its mask and weight must then be 0.  Behind the pose cost volume C of "pose
 * fields", the attitude volume gives C' as gvom_pose_field_attitude does (C' = C without one).  Then C''[h][cell] = 0 where C' == 0 or bit
 * `status` of body_block_mask is set (bit k = GVOM_BODY_* code k), otherwise C'' = min(65535, C' + squeeze_weight * squeeze); seeding,
 * relaxation, actions and part 2 of the product take C''.  With body_volume_id = -1 the result is gvom_pose_field_attitude's bit for bit;
 * with both -1 it is gvom_pose_field's.  In addition GVOM_ERR_INVALID: attitude_block_mask > 0x7f; body_block_mask > 0x3f; tilt_weight or
 * squeeze_weight outside 0 .. 255; a mask or weight that is not 0 beside an id of -1; a stale volume id, an id of another kind, or a
 * volume of another H or xy_size.
 * NOT PROVIDED: interpolation in the field; states between cell centres; swept volumes between a primitive's ends; body volumes over the
 * atlas extent; a float32 clearance taken into the cost other than through squeeze; sharded handles. */
#define GVOM_PRODUCT_BODY_VOLUME 46   /* parts 0, 1 uint8 status, squeeze, part 2 float32 clearance: [H, xy, xy], strides (xy*xy, 1, xy); part 3 int32 [8] */
/* 45 stays unassigned: tests/body_volume_layout_host_test.cpp holds it to "no such kind" */
int gvom_body_volume(gvom_t *h, int64_t field_product_id, const float *field, const int64_t field_origin[3], int64_t map_set_id,
                     const double *ground, int on_device, int flags, const int64_t origin_cells[2], float min_margin, float soft_margin,
                     int64_t *product_id);
int gvom_pose_field_volumes(gvom_t *h, int64_t costfield_id, const int32_t *cost, int on_device, int64_t attitude_volume_id,
                            uint32_t attitude_block_mask, int32_t tilt_weight, int64_t body_volume_id, uint32_t body_block_mask,
                            int32_t squeeze_weight, const int32_t *goals /* [n_goals][3] */, int64_t n_goals, int32_t max_cost,
                            int32_t max_rounds, int64_t *product_id, int64_t info[4]);

/* --- voxel atlas changes (an extension: what is different since I was last here -- the voxels of the current fused map that contradict
 * what the voxel atlas remembers, as codes, per column, and clustered into objects that appeared or vanished) --------------------------------
 * gvom_voxel_atlas_integrate counts how many voxels went free -> occupied and occupied -> free with every merge; it does not say where
 * they are or which object they form.  gvom_voxel_atlas_changes answers that BEFORE the merge, read-only: it compares the CURRENT fused map
 * -- selected exactly as gvom_voxel_atlas_integrate selects it -- with the atlas as it is at the moment of the call, with no move applied,
 * and changes neither.  The intended loop is combine, changes, integrate.  An addition: GVOM_ABI_VERSION stays.  gvom_get_tuning
 * "voxel_changes" (read-only): 1 -- how a caller probes a library for this entry point.  All arithmetic is integer -- population counts,
 * sums, minima and maxima: the result is exact and does not depend on scheduling.
 *
 * DEFINITION.  W = the window origin of the current fused map, xy = xy_size, z = z_size; v = (x, y, l) a window voxel, c(v) the CLASS
 * ("voxel atlas") of its fused state, a(v) the atlas's class of world voxel W + v (NEVER outside the extent).
 * CODE       GVOM_CHANGE_APPEARED (1): W + v lies inside the extent, c == OCCUPIED and a == FREE.  GVOM_CHANGE_VANISHED (2): inside the
 *            extent, c == FREE and a == OCCUPIED.  0 otherwise: first-seen, confirmed, uninformative and outside voxels are no changes.
 * MASK       1, 2 or 3: the codes that mark a column (bit 0 appeared, bit 1 vanished).
 * MARKED     column (x, y) is MARKED iff it holds at least one voxel whose code is in mask.
 * CLUSTERS   the 8-connected components of the marked columns.  LABEL, KEPT (>= min_cells columns), RANK and cap (= max_clusters) are
 *            word for word those of "frontier extraction", with "frontier cell" read as "marked column".
 * DISTANCE   the plane that gvom_frontiers calls D is d2(x, y) = (x - cx)^2 + (y - cy)^2 with cx = cy = xy / 2 (integer division): a
 *            cluster's "best cell" is its column nearest the vehicle, ties broken by the lowest index y * xy + x, and "best D" is that
 *            squared distance in cells.
 * The product, of kind GVOM_PRODUCT_VOXEL_CHANGES, is a SNAPSHOT in the product-set pool under its rule (at most GVOM_MAX_PRODUCT_SETS of
 * the kind, sized by xy, z and max_clusters).  Its parts:
 *   part 0  int32 [cap, 8]     per kept cluster of rank below cap {label, columns, min x, min y, max x, max y, nearest column, its d2}
 *   part 1  int64 [cap, 2]     {sum x, sum y} over the cluster's columns
 *   part 2  int32 [xy, xy]     the cluster map: rank, -1 unmarked, -2 below min_cells; [x, y]-indexed, strides (1, xy)
 *   part 3  int32 [8]          {n_kept, marked columns, marked columns in kept clusters, cap, appeared voxels, vanished voxels, window
 *                              voxels outside the extent, the atlas's seq}.  Words 4 and 5 count ALL coded voxels, whatever mask is
 *   part 4  int32 [cap, 4]     per kept cluster of rank below cap {appeared voxels, vanished voxels, lowest window level, highest window
 *                              level}: the voxel totals count both codes whatever mask is, the levels only voxels whose code is in mask.
 *                              Zero rows beyond min(n_kept, cap), as in parts 0 and 1
 *   part 5  uint8 [xy, xy, z]  the codes, in the occupancy grid's layout (the layout of a voxel box's class grid)
 *   part 6  uint16 [2, xy, xy] appeared (plane 0) and vanished (plane 1) voxels per column: [k, x, y]-indexed, strides (xy*xy, 1, xy) --
 *                              every plane has a pose field plane's layout
 * Parts 0 to 2 and words 0 to 3 of part 3 are what the frontier kernels write, unchanged.
 *
 * gvom_voxel_atlas_changes(h, mask, min_cells, max_clusters, &product_id, origin_out, info): info is gvom_frontiers' info {rounds, kept
 * clusters, marked columns, clusters below min_cells}; origin_out (may be NULL) receives W.  Like gvom_frontiers the call WAITS for the
 * labelling.  GVOM_NO_DATA before the first combine.  An atlas that was never integrated is valid and yields no change (everything it
 * holds is NEVER).  GVOM_ERR_INVALID: a sharded handle; no voxel atlas configured; mask outside 1 .. 3; min_cells < 1; max_clusters
 * outside 1 .. GVOM_FRONTIER_MAX_CLUSTERS; W at or beyond 2^30 voxels; NULL product_id.  GVOM_ERR_CAPACITY: xy_size > 4096; every set of
 * the kind exported.  The device allocations of the call (its product sets, the labelling's work buffer, the bit planes) are counted in
 * "voxel_atlas_allocations" and do not grow in steady state.  gvom_device_product(GVOM_PRODUCT_VOXEL_CHANGES) is GVOM_ERR_INVALID (this
 * call makes them).  Kind 47 is not assigned.
 * NOT PROVIDED: 26-connected clusters in 3-D; a level band (changes between two heights only); a change query fused into the integrate;
 * changes against a box other than the current window; sharded handles. */
#define GVOM_CHANGE_APPEARED 1
#define GVOM_CHANGE_VANISHED 2
#define GVOM_PRODUCT_VOXEL_CHANGES 48   /* parts 0 .. 3 as kind 16 with part 3 int32 [8]; part 4 int32 [cap, 4]; part 5 uint8 [xy, xy, z]; part 6 uint16 [2, xy, xy]; kind 47 stays unassigned */
int gvom_voxel_atlas_changes(gvom_t *h, int mask, int32_t min_cells, int32_t max_clusters, int64_t *product_id,
                             int64_t origin_out[3] /* may be NULL */, int64_t info[4] /* may be NULL */);

/* --- one map sharded over the GPUs of a node (one rank = one process = one GPU) -------------------
 * No counterpart in the reference (it has no multi-GPU path); semantics = SURVEY 8(e):
 * the rays are data-parallel, the per-voxel accumulators (hit / total: int32 sum, min-height: f32 min)
 * are reduced onto the rank that owns the voxel's storage row, everything after is per voxel / per
 * column on the owner.  Rank r owns storage rows [r*xy/world, (r+1)*xy/world) of the world-anchored y
 * axis (xy must be a multiple of 4*world).  The result is bit-identical to one GPU fed with the
 * concatenated cloud.
 *
 * Per scan:  gvom_shard_scan_local   trace this rank's share (it may be empty) over the whole window;
 *                                    returns, per owner rank d, how many dirty quads (4 rows x 64 sx at
 *                                    one sz = 1 KiB of ray-pass counts + a 4-byte id) and endpoints
 *                                    ({voxel, min-height sample}, 8 bytes) are packed for d
 *            -- the transport exchanges the counts, then moves SEND regions to the owners' RECV
 *               regions (gvom_shard_buffer; RCCL: gvom_comm_exchange_scan) --
 *            gvom_shard_recv_reserve  size the endpoint receive regions from the counts
 *            gvom_shard_scan_merge    add the received contributions, encode this rank's rows, commit
 *                                     iff `accept` (any rank saw an in-grid return: gvom.py:147-150)
 * Per combine: gvom_combine_fuse (fusion + column reductions + positive-obstacle densities of this
 *            rank's rows) -> all-gather of GVOM_BUF_HEIGHT_MAPS rows -> gvom_combine_map2d_into (all rows
 *            of slope / roughness / guess / positive / negative / visibility on every rank).
 * gvom_process_pointcloud* / gvom_combine_maps* return GVOM_ERR_INVALID on a sharded handle. */
int gvom_shard_scan_local(gvom_t *h, const void *xyz, int on_device, int64_t n, int64_t row_stride_bytes,
                          int dtype, const double ego[3], const double *transform_4x4,
                          int64_t *send_quads, int64_t *send_eps, int *any_ingrid);
#define GVOM_XBUF_SEND_IDS   0   /* uint32 quad ids for rank `peer`                      */
#define GVOM_XBUF_SEND_QUADS 1   /* 1 KiB per quad, same order                          */
#define GVOM_XBUF_SEND_EPS   2   /* {uint32 voxel, uint32 min-height sample} per endpoint */
#define GVOM_XBUF_RECV_IDS   3
#define GVOM_XBUF_RECV_QUADS 4
#define GVOM_XBUF_RECV_EPS   5   /* valid after gvom_shard_recv_reserve                  */
#define GVOM_XBUF_SEND_RETURNS 6 /* statistics handles: returns {x, y, z} of the cloud's type for rank `peer` */
#define GVOM_XBUF_RECV_RETURNS 7 /* valid after gvom_shard_stats_reserve                 */
int gvom_shard_buffer(gvom_t *h, int which, int peer, void **ptr, int64_t *capacity_bytes);
int gvom_shard_recv_reserve(gvom_t *h, const int64_t *recv_eps);
int gvom_shard_scan_merge(gvom_t *h, const int64_t *recv_quads, const int64_t *recv_eps, int accept);
/* Per-voxel statistics on a sharded map (GVOM_FLAG_VOXEL_STATISTICS; 2*xy_eigen_dist + 1 <= rows per rank): a return adds
 * to every occupied voxel of its neighbourhood (gvom.py:1188-1220), so besides the endpoints every rank gets the returns
 * whose neighbourhood reaches into its rows: send_returns[d] after gvom_shard_scan_local, GVOM_XBUF_SEND_RETURNS ->
 * the peers' GVOM_XBUF_RECV_RETURNS (gvom_comm_exchange_stats) sized by gvom_shard_stats_reserve, before
 * gvom_shard_scan_merge.  All ranks must pass clouds of one type (float32 or float64). */
int gvom_shard_stats_counts(gvom_t *h, int64_t *send_returns);
int gvom_shard_stats_reserve(gvom_t *h, const int64_t *recv_returns, int dtype /* GVOM_DTYPE_*: the scan's cloud type */);
/* For the transport: region `which` (GVOM_XBUF_SEND_*, or -1 = GVOM_BUF_HEIGHT_MAPS) moves, contents included, into a FRESH
 * allocation of the same size (its gvom_region_generation changes); the old allocation is parked, never freed while the
 * process lives (another process may have it mapped). */
int gvom_shard_renew_region(gvom_t *h, int which);
int gvom_combine_fuse(gvom_t *h, int64_t *local_cells);
int gvom_set_combined_cell_count(gvom_t *h, int64_t global_cells);
#define GVOM_BUF_HEIGHT_MAPS  0   /* [sy][height row | inferred-height row | positive-density row], f64 */
#define GVOM_BUF_FUSED_CELLS  3   /* one int64: occupied voxels of this rank's rows of the fused map */
int gvom_sync(gvom_t *h);
int gvom_device_buffer(gvom_t *h, int which, void **ptr, int64_t *bytes, int64_t *row_stride_bytes);
int gvom_combine_map2d_into(gvom_t *h, double origin_world[3], void *pinned_out);

/* --- transport between the ranks of a sharded map: RCCL over xGMI, bound directly ------------------
 * name: the same string on every rank and unique to this communicator on the node (rank 0 creates
 * /dev/shm/<name> for the ncclUniqueId and the small host-side exchanges).  gvom_comm_exchange_host:
 * all[r*k + j] = rank r's mine[j] (k <= 208 = 3 * 64 ranks + 16).  gvom_comm_exchange_scan / gvom_comm_allgather_rows run
 * on the handle's stream and do not synchronise.  device < 0: host-only communicator (rendezvous +
 * gvom_comm_exchange_host / gvom_comm_barrier, no RCCL and no HIP call; the device collectives return
 * GVOM_ERR_INVALID) -- the CPU tests run the multi-process rendezvous with it. */
typedef struct gvom_comm gvom_comm_t;
int  gvom_comm_create(int rank, int world, int device, const char *name, gvom_comm_t **out);   /* = create2(..., GVOM_TRANSPORT_RCCL) */
/* Transports for the DEVICE data (the host-side vectors always travel through the shared-memory segment):
 * RCCL  grouped ncclSend / ncclRecv and an in-place ncclAllGather on the handle's stream, no host synchronisation;
 * PEER  peer copies: every rank exports its send regions (hipIpcGetMemHandle), the receiver maps them (lazy peer
 *       access) and pulls its bytes with hipMemcpyAsync on its own handle's stream, bracketed by two host barriers --
 *       xGMI between the GPUs of a node, plain device copies when several ranks share ONE GPU (which RCCL refuses:
 *       this is the transport a one-GPU box can run several rank processes with);
 * AUTO  RCCL; if librccl cannot be loaded, or ncclCommInitRank fails on any rank or does not return within
 *       GVOM_RCCL_INIT_TIMEOUT_S (default 90 s after the last rank has arrived), every rank uses PEER.
 * gvom_comm_transport: the transport in use (GVOM_TRANSPORT_RCCL, GVOM_TRANSPORT_PEER or GVOM_TRANSPORT_LOOPBACK).
 * Failure semantics: a rank whose device exchange failed marks the communicator (for every rank) as broken, and a rank
 * whose process has gone is noticed by whoever waits for it next: the others' next gvom_comm_exchange_host / _barrier
 * returns GVOM_ERR_HIP with a message naming the rank instead of waiting GVOM_COMM_TIMEOUT_S.  A broken communicator stays
 * broken: destroy it. */
#define GVOM_TRANSPORT_RCCL 0
#define GVOM_TRANSPORT_PEER 1
#define GVOM_TRANSPORT_AUTO 2
/* LOOPBACK  RCCL on a box with ONE GPU: the ranks are threads of one process that share the device (RCCL refuses two ranks of
 *       one communicator on one device), each with a 1-rank communicator of its own.  What RCCL moves with ncclSend on the
 *       sender and ncclRecv on the receiver, the RECEIVER moves with ncclSend(the peer's send region, itself) +
 *       ncclRecv(its receive region, itself) in one group on its handle's stream -- same group handling, capacity checks,
 *       ncclUint8 byte counts and position in front of the unpack kernels as GVOM_TRANSPORT_RCCL -- bracketed by two host
 *       barriers; the combine's rows the same way, followed by the in-place ncclAllGather of the 1-rank communicator.
 *       All ranks must live in one process (plain device addresses travel through the segment). */
#define GVOM_TRANSPORT_LOOPBACK 3
int  gvom_comm_create2(int rank, int world, int device, const char *name, int transport, gvom_comm_t **out);
int  gvom_comm_transport(gvom_comm_t *c);
/* Peer transport, asynchronous form (GVOM_PEER_ASYNC=1 on every rank, and every rank able to register the segment with HIP;
 * otherwise the host-synchronised form): an exchange enqueues its copies and returns; the GPUs write exchange numbers into the segment.
 * Call gvom_comm_before_scan before gvom_shard_scan_local and gvom_comm_before_combine before gvom_combine_fuse: they wait
 * (normally not at all) until every peer has pulled what this rank is about to overwrite.  No-ops on the other transports. */
int  gvom_comm_before_scan(gvom_comm_t *c);
int  gvom_comm_before_combine(gvom_comm_t *c);
int  gvom_comm_peer_async(gvom_comm_t *c);          /* 1: the peer transport runs in its asynchronous form */
/* peer transport bookkeeping: {bytes pulled, copies, exports made, refused hipIpc* calls that were repeated} */
int  gvom_comm_peer_stats(gvom_comm_t *c, int64_t out[4]);
/* Peer transport and the HSA runtime's inter-process memory.  Requires HSA_ENABLE_IPC_MODE_LEGACY=0 in the environment of
 * every rank on hosts whose driver only supports dmabuf IPC (the communicator says so on stderr when it is unset); every
 * measurement in profiles/ was taken with it.  hipIpcGetMemHandle / hipIpcOpenMemHandle can REFUSE an allocation ("invalid
 * argument" / "invalid device pointer": seen once in several hundred exports under a test that exports a fresh allocation
 * every scan, never in steady state).  The library absorbs it: a refused export moves the region into a fresh allocation
 * (gvom_shard_renew_region) and exports that; a refused open is reported through the segment, the owner does the same, and
 * every rank tries again -- up to three fresh allocations, inside the exchange, before the call fails and the communicator
 * is marked broken.  gvom_comm_peer_renewed: how often that happened on this rank. */
int64_t gvom_comm_peer_renewed(gvom_comm_t *c);
/* What the communicator itself knows of the job: out = {ranks in RCCL's communicator (ncclCommCount; -1 without RCCL), this
 * rank's number there (ncclCommUserRank), HIP device, transport in use}; busid (optional): the device's PCI bus id. */
int  gvom_comm_info(gvom_comm_t *c, int64_t out[4], char *busid, size_t busid_len);
/* RCCL calls this rank has issued so far: {ncclSend + ncclRecv calls, their bytes, groups closed, ncclAllGather calls} */
int  gvom_comm_wire_stats(gvom_comm_t *c, int64_t out[4]);
/* A rank whose caller cannot go on marks the communicator broken for every rank (see "Failure semantics" above). */
int  gvom_comm_abort(gvom_comm_t *c);
void gvom_comm_destroy(gvom_comm_t *c);
int  gvom_comm_exchange_host(gvom_comm_t *c, const int64_t *mine, int k, int64_t *all);
int  gvom_comm_barrier(gvom_comm_t *c);
int  gvom_comm_exchange_scan(gvom_comm_t *c, gvom_t *h, const int64_t *send_quads, const int64_t *send_eps,
                             const int64_t *recv_quads, const int64_t *recv_eps);
int  gvom_comm_exchange_stats(gvom_comm_t *c, gvom_t *h, const int64_t *send_returns, const int64_t *recv_returns,
                              int bytes_per_return);
int  gvom_comm_allgather_rows(gvom_comm_t *c, gvom_t *h);
/* A whole sharded scan / combine in ONE call (handles without per-voxel statistics): the sequences documented above --
 * gvom_comm_before_scan, gvom_shard_scan_local, the host exchange of the counts, gvom_shard_recv_reserve,
 * gvom_comm_exchange_scan, gvom_shard_scan_merge; gvom_comm_before_combine, gvom_combine_fuse, gvom_comm_allgather_rows,
 * gvom_combine_map2d_into -- run natively, every rank calling with ITS share of the cloud (n may be 0).
 * out = {accepted (some rank saw a return in the grid, gvom.py:147-150), returns of all ranks, bytes this rank sent, received}.
 * gvom_comm_combine_maps_into returns GVOM_EMPTY_BUFFER while the ring is empty (gvom.py:179-181). */
int  gvom_comm_process_pointcloud(gvom_comm_t *c, gvom_t *h, const void *xyz, int on_device, int64_t n, int64_t row_stride_bytes,
                                  int dtype, const double ego[3], const double *transform_4x4, int64_t out[4]);
int  gvom_comm_combine_maps_into(gvom_comm_t *c, gvom_t *h, double origin_world[3], void *pinned_out);
int  gvom_comm_rank(gvom_comm_t *c);
int  gvom_comm_world(gvom_comm_t *c);
const char *gvom_comm_last_error(gvom_comm_t *c);

/* --- accessors of the reference object ------------------------------------------------- */
/* 1 if ring slot `slot` holds a scan (origin_buffer[slot] is not None, gvom.py:201). */
int gvom_slot_filled(gvom_t *h, int slot);
int gvom_get_state(gvom_t *h, gvom_state *out);
int gvom_get_scan_stats(gvom_t *h, gvom_scan_stats *out);
/* Gvom.get_map_as_occupancy_grid (gvom.py:356-361): uint8[xy][xy][z] C-order (== the
 * reference's order='F' reshape of the lookup table), 1 where occupied. */
int gvom_get_occupancy(gvom_t *h, uint8_t *out_xyz);
/* Gvom.make_debug_voxel_map (gvom.py:363-378; kernels :1333-1378 eigenvalues, :454-473): one row of
 * 8 float32 per occupied fused voxel {x, y, z, hit/total, hit, l0-l1, l1-l2, l2}; row order is
 * unspecified (as in the reference).  *rows = number of occupied voxels; at most max_rows are written.
 * GVOM_NO_DATA unless the handle computes the per-voxel statistics (GVOM_FLAG_VOXEL_STATISTICS / _ON_DEMAND), has combined and the
 * fused map carries them. */
int gvom_debug_voxel_map(gvom_t *h, float *out, int64_t max_rows, int64_t *rows);
/* The same with the three eigenvalues of every row (reference attribute voxels_eigenvalues,
 * gvom.py:1333-1378): eigen[row][3] = {l0, l1, l2}, row for row with `out`. */
int gvom_debug_voxel_eigen(gvom_t *h, float *out, float *eigen, int64_t max_rows, int64_t *rows);
/* Gvom.make_debug_height_map (gvom.py:380-394, kernel :426-438): float32[xy*xy][7]. */
int gvom_debug_height_map(gvom_t *h, float *out);
/* Gvom.make_debug_inferred_height_map (gvom.py:396-410, kernel :442-450): float32[xy*xy][3]. */
int gvom_debug_inferred_height_map(gvom_t *h, float *out);

/* --- test hooks: dense equivalents in the reference's voxel order ------------------------
 * which: 0..buffer_size-1 = ring slot (index_buffer/hit_count_buffer/... gvom.py:59-64),
 *        GVOM_WHICH_FUSED = current fused map (combined_* gvom.py:69-75).
 * state: 0 where occupied, -1 never observed, -m-1 free with m ray passes (gvom.py:1154-1160);
 * hit/total 0 and min_h 1.0f where not occupied.  origin: voxel units.  NULLs are skipped.
 * Returns GVOM_NO_DATA if the slot / fused map is empty. */
#define GVOM_WHICH_FUSED (-1)
int gvom_read_dense(gvom_t *h, int which, int32_t *state, int32_t *hit, int32_t *total,
                    float *min_h, double origin[3], int64_t *cell_count);
/* Reference attributes metrics_buffer[slot] / combined_metrics (gvom.py:54-83,234,281; handles with
 * GVOM_FLAG_VOXEL_STATISTICS): gvom_read_rows gives the compact row of every occupied voxel in the
 * reference's voxel order (-1 elsewhere), gvom_gather_metrics the 10 statistics {mean xyz, covariance
 * xx xy xz yy yz zz, count} of selected rows: float64 for a ring slot, float32 for the fused map. */
int gvom_read_rows(gvom_t *h, int which, int32_t *rows_dense);
int gvom_gather_metrics(gvom_t *h, int which, const int32_t *rows, int64_t n, void *out);
/* which2d: internal float64 maps of the last combine, [x][y] C-order like the reference's
 * attributes (gvom.py:85-88,310-313). */
#define GVOM_MAP_HEIGHT          0
#define GVOM_MAP_INFERRED_HEIGHT 1
#define GVOM_MAP_SLOPE_X         2
#define GVOM_MAP_SLOPE_Y         3
#define GVOM_MAP_ROUGHNESS       4
#define GVOM_MAP_GUESSED_DELTA   5
int gvom_read_map2d(gvom_t *h, int which2d, double *out);

/* --- measurement ------------------------------------------------------------------------
 * Device time (HIP events on the library's own stream) of the kernels of the last
 * process_pointcloud / combine_maps call, in milliseconds, by stage.  Stages:
 * 0 trace (transform+hit+DDA), 1 encode, 2 min-height, 3 fuse (+column reductions), 4 maps2d. */
#define GVOM_N_STAGES 5
int gvom_last_stage_ms(gvom_t *h, float ms[GVOM_N_STAGES]);
/* Enables/disables per-stage event timing (adds one host sync per call when on). */
int gvom_set_profiling(gvom_t *h, int on);
/* Host-side phase times (microseconds per call, averaged; enabled by GVOM_HOST_TIMING=1):
 * [0] scan launches [1] scan wait [2] combine launches [3] combine wait [4] output copies. */
int gvom_host_timing(gvom_t *h, double us[8]);
/* Performance knobs that never change a result.  name: "segs" (step segments per ray in the trace
 * kernel), "period" (committing steps between two flushes of a wave's LDS line cache), "ep_row"
 * (dispatch row of the endpoint blocks; -1: inside segment 0's waves), "prio" (steps of remaining walk per issue-priority
 * level of a trace wave, s_setprio; 0: the hardware's own arbitration); 0 / 0 / -2 / -1 = automatic.
 * "interleave": K = 2 .. 64 (a power of two that divides the number of returns) declares the cloud to be K equally long
 * sub-clouds behind one another -- K sensors at one place, K sweeps -- whose returns of equal position are neighbours in
 * space; the trace then puts those neighbours into neighbouring lanes of one wave (merged steps, shared accumulator lines:
 * 512^2 x 128, 4 x 262,144 returns: 11.5 M -> 4.1 M memory-side atomic requests, 549 -> 355 us).  0 (default): automatic -- a
 * one-wave probe kernel in front of the trace looks for that structure (64 sampled returns per candidate K <= 4) on the second
 * cloud of a length and every 32nd after it, and the following clouds of that length are traced accordingly; clouds whose
 * length changes from scan to scan are not looked at for sub-clouds (they are probed every 8th scan for the "dirsort" verdict only); 1: off.  Only WHO traces which return changes, never a result.
 * "eager": the EAGER FUSION of one-slot rings (buffer_size 1, unsharded, xy_size % 16 == 0; with per-voxel statistics their merge is
 * enqueued with the scan as well).  The scan launches
 * ONE kernel behind the trace that encodes the ring slot AND fuses it with the previous fused map (the work of the scan's
 * encode pass and of the next combine's fusion, in one pass over the scan's accumulators), into spare buffers -- speculating
 * that the next call is gvom_combine_maps*, the reference node's pattern (gvom_ros.py:82-115: one combine per scan).  That
 * call adopts the result iff no scan came in between; otherwise it is dropped and the combine fuses the encoded slot as
 * before.  -1 (default): automatic -- off after three dropped speculations in a row, on again once combines follow scans;
 * 1: always; 0: never.  gvom_get_tuning "eager_adopted" / "eager_dropped": how often either happened.
 * "dirsort": the DIRECTIONAL ORDER of clouds that are in no spatial order (BASELINE config c1's uniformly random points; any cloud
 * shuffled, merged or filtered out of its sensor order).  The trace's cost follows the accumulator lines a 64-ray bundle touches per
 * step, and 64 random returns touch 64; a counting sort by direction bin seen from the sensor (two small kernels in front of the
 * trace: 6 cube faces x 16 x 16 cells) gives every wave 64 rays that point the same way: c1's trace 65 -> 16 us + 15 us of sorting.
 * The same remedy serves organised clouds in azimuth-major ("firing") order, whose bundles are VERTICAL fans (the scan the
 * beam-major order traces in 37 us takes 280): they are sorted by (sin-elevation row, azimuth sector) -- 256 x 32 bins -- inside
 * which the returns keep the order they came in, and the beam-major fans come back (43 us + the sort).
 * 0 (default): automatic -- the layout probe also looks, in 64 samples, whether a return and its successor point more than ~6
 * degrees apart (mode 1: cube cells) or a return and the one 63 places behind it differ by more than ~3 degrees in elevation
 * (mode 2: elevation rows), and the following clouds of that length are traced accordingly; 1 / 2: always, in that mode; -1: never.
 * gvom_get_tuning("dirsort"): the mode the last scan ran in (0: the cloud's own order).  Only WHO traces which return changes.
 * "fastdiv": k_trace divides every float32 coordinate by xy_resolution / z_resolution (gvom.py:1072-1080, 1101-1103); with the
 * reciprocal r = RN(1 / d), q = x * r, e = fma(-q, d, x), fma(e, r, q) IS the IEEE quotient for every float32 x iff it is for the
 * 2^23 float32 significands, which gvom_create checks on the host for both resolutions (once per value and process); a
 * resolution that fails the check, float64 clouds and hosts without hardware fma keep the divide.  -1 (default): use it where
 * verified; 0: always divide.  gvom_get_tuning("fastdiv"): bit 0 / 1 = in use for xy_resolution / z_resolution.
 * "encfuse" (A/B of that kernel's shape: low 4 bits waves per column block, bit 4 blocks in dispatch order -- no XCD per row band
 * in the 32-sx form, no XCD pairing in the 16-sx one --, bit 5 the 16-sx form on every grid; gvom_get_tuning "encfuse_width" /
 * "encfuse_waves", read-only: sx and waves per column block of the last k_encfuse launched, 0 before the first), "fuse1" (1: one-slot
 * fusions through the general kernel), "flag_kernel" (1: round 3's completion-flag kernel).
 * "occupancy_clear" (A/B of k_occupancy's dead tile columns: 0, default, the kernel writes every byte of the grid; 1 the grid is
 * cleared with hipMemsetAsync and only tile columns with a live tile are written.  Same grid either way).
 * "delta_out" (1, default: gvom_combine_maps_into / gvom_combine_begin store only the runs of the four maps that changed, see
 * gvom_output_forget; 0: every run, every time, and no record is kept.  Same buffer contents either way; also readable).
 * "output_records" (read-only, gvom_get_tuning): output buffers that have a content record now.
 * "range_image" (read-only, gvom_get_tuning): 1 when a sensor model is set (gvom_sensor_model_set), else 0.
 * "multi_origin" / "multi_origin_ran" (read-only, gvom_get_tuning): see "multi-origin scans" above.
 * "clearance_allocations" (read-only, gvom_get_tuning): see "obstacle clearance" above.
 * "clearance_lgw" / "clearance_rows_per_tile" / "clearance_lds_bytes" / "clearance_chunks" (read-only, gvom_get_tuning): the
 * launch shape of the LAST gvom_clearance on this handle, as the launch itself chose it from xy_size and max_cells2 -- log2 of the
 * columns per strip of the column pass (3 .. 6), output rows per workgroup of that pass (16 .. 256), its dynamic LDS in bytes (at
 * most 65536), and the 64-cell chunks per map row of the row pass (at most 64).  All 0 before the first call.  The shape never
 * changes a result; the names exist so that tests can show which launch regimes they ran.
 * "raycast" / "raycast_allocations" (read-only, gvom_get_tuning): see "ray queries" above.
 * "cost_to_go" / "cost_to_go_allocations" / "cost_to_go_tiles" (read-only), "cost_to_go_inner" / "cost_to_go_batch": see
 * "cost-to-go fields" above.
 * "rollouts" / "footprint" / "rollout_allocations" (read-only, gvom_get_tuning): see "rollout scoring" above.
 * "attitude" / "chassis" / "attitude_allocations" (read-only, gvom_get_tuning): see "terrain attitude scoring" above.
 * "body" / "body_spheres" / "body_allocations" (read-only, gvom_get_tuning): see "body clearance scoring" above.
 * "alignments" / "alignment_allocations" / "alignment_grid_bytes" / "alignment_points_per_block" / "alignment_candidate_group"
 * (read-only, gvom_get_tuning): see "scan alignment scoring" above.
 * "viewpoints" / "viewpoint_allocations" / "viewpoint_batch" (read-only, gvom_get_tuning), "viewpoint_bitmap_mb": see "viewpoint
 * scoring" above.
 * "attitude_volume" / "attitude_volume_allocations" (read-only, gvom_get_tuning): see "attitude volumes" above.
 * "body_volume" / "body_volume_allocations" (read-only, gvom_get_tuning): see "body volumes" above.
 * "voxel_distance_field" / "voxel_distance_halo_xy" / "voxel_distance_halo_z" (read-only, gvom_get_tuning), "voxel_distance_mb": see
 * "voxel distance field" above.
 * "voxel_changes" (read-only, gvom_get_tuning): see "voxel atlas changes" above.
 * (Test hooks are not part of this library: include/gvom_hip_test.h, lib/libgvom_hip_test.so.) */
int gvom_set_tuning(gvom_t *h, const char *name, int value);
/* The value the LAST scan ran with ("segs", "period", "ep_row", "prio", "interleave": what automatic resolved to).
 * "fuse_kernel" (read-only): the kernel of the last fusion -- 1 k_fuse1, 2 k_fuse4<2>, 3 k_fuse4<4>, 4 k_fuse (chunks of up to
 * 16 levels), 5 k_fuse (taller chunks), 6 an adopted eager k_encfuse; + 16 where the fusion descriptors were read from memory
 * (more sources than fit the kernel arguments); 0 before the first fusion. */
int gvom_get_tuning(gvom_t *h, const char *name, int *value);
/* Raw HIP stream the library launches on (hipStream_t as void*), for external event timing. */
void *gvom_stream(gvom_t *h);
/* differs between any two handles of the process and changes whenever a SEND region of `h` (GVOM_XBUF_SEND_*: the only
 * grow-only buffers another rank reads) has been re-allocated: tells a cache of addresses derived from gvom_shard_buffer
 * when to look again */
uint64_t gvom_alloc_generation(gvom_t *h);
/* the same for one region (which = GVOM_XBUF_SEND_*, or -1 for GVOM_BUF_HEIGHT_MAPS): changes exactly when the allocation the
 * region lies in is replaced, and differs between handles */
uint64_t gvom_region_generation(gvom_t *h, int which);

const char *gvom_last_error(gvom_t *h);      /* never NULL */
int gvom_backend_info(char *buf, size_t len); /* "gfx950 ..." device + build string */
int gvom_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GVOM_HIP_H */
