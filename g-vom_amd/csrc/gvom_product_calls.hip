// gvom_product_calls.hip -- the calls that MAKE a device product: gvom_device_product (occupancy grid, voxel cloud, the two height
// clouds), gvom_clearance, gvom_raycast, gvom_cost_to_go, gvom_score_rollouts (with gvom_footprint_set, which sets its table),
// gvom_score_attitude (with gvom_chassis_set), gvom_score_body (with gvom_body_set), gvom_score_alignments, gvom_frontiers, gvom_score_viewpoints, gvom_pose_field / gvom_pose_field_attitude / gvom_pose_field_volumes (with
// gvom_primitives_set), gvom_attitude_volume and gvom_body_volume, and the frame builders they and the debug reads (gvom_debug.hip) give the kernels.  Every call takes its set
// through product_acquire and hands it out through product_publish (gvom_sets.hip).  What several calls do alike stands once, in
// front of the entry points, and serves the atlas calls (gvom_atlas_calls.hip) and the voxel atlas's walk queries (gvom_voxel_atlas_calls.hip:
// check_rays / rays_fill, check_views / views_* and check_align / align_fill) too: the argument checks (check_*, *_of), the staging
// of host inputs (stage_host), the frames (metric_frame, rollout_frame), the vehicle on the ground of the four calls that stand it there
// (check_standing, the Ground and the Field a call reads, the chassis as the kernels take it) and, for the calls that wait, the round driver (solve_rounds;
// its arithmetic and the work buffers' layouts are gvom_solvework.h's), the work buffers and the epilogue (goal_solve_finish).  What
// is left in each body is what is particular to that product: its own checks, in the order they always had, and its launches.
#include "gvom_host.h"

namespace gvom_host {
// what every kernel that reads a fused map takes of its frame: size, ring-window phase, slab rows, segment count, tile epoch
template <class P> static void fused_frame(const gvom_handle *h, const Fused &F, P &p, int &y_lo, int &y_hi)
{
    memset(&p, 0, sizeof p);
    p.xy = h->prm.xy_size; p.zs = h->prm.z_size;
    window_phase(h, F.origin, p.om);
    y_lo = h->sy_lo; y_hi = h->sy_hi;
    p.nseg = h->nseg; p.epoch = F.epoch;
}

void occ_params(const gvom_handle *h, const Fused &F, OccParams &P) { fused_frame(h, F, P, P.y_lo, P.y_hi); }

void cloud_params(const gvom_handle *h, const Fused &F, Map2dParams &P)
{
    fused_frame(h, F, P, P.y_lo, P.y_hi);
    P.xy_res = h->prm.xy_resolution; P.z_res = h->prm.z_resolution;
}

// the frame of the fused map F as k_raycast reads it (gvom_launch_raycast names the fields), and what of a query depends on it
static void raycast_params(const gvom_handle *h, const Fused &F, ScanParams &P, RayQuery &Q)
{
    const gvom_params &p = h->prm;
    fused_frame(h, F, P, P.sy_lo, P.sy_hi);
    metric_frame(h, F, P);
    P.f32_sqrt = h->f32_sqrt ? 1 : 0;
    bool far = false;
    for (int k = 0; k < 3; ++k) {
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

// what k_rollouts, and k_attitude in its P.R, take of a call of K trajectories of T poses
static void rollout_frame(const gvom_handle *h, int64_t K, int64_t T, const int64_t origin_cells[2], RolloutParams &R)
{
    memset(&R, 0, sizeof R);
    R.xy = h->prm.xy_size; R.H = h->footprint.H; R.T = (int)T; R.K = K;
    R.s = (float)((double)h->footprint.H / 6.283185307179586476925286766559);
    R.ox = origin_cells[0]; R.oy = origin_cells[1];
    R.res = h->prm.xy_resolution;
}

// ---- the argument checks more than one entry point makes (gvom_host.h) ----------------------------------------------------------------
int refuse(gvom_handle *h, const char *fn, const std::string &what, int code) { h->err = std::string(fn) + ": " + what; return code; }

static int product_of_kind(gvom_handle *h, const char *fn, int64_t id, int kind, const char *what, DevSet **f)
{
    *f = find_set(h->psets, id);
    return *f && (*f)->kind == kind ? GVOM_OK : refuse(h, fn, what);
}

// ---- the vehicle on the ground: what gvom_score_attitude, gvom_score_body, gvom_attitude_volume and gvom_body_volume do alike ---------
// the standing checks, in the order each of the four has them; volume: at most 64 headings too (GVOM_POSE_MAX_HEADINGS)
static int check_standing(gvom_handle *h, const char *fn, bool volume)
{
    if (h->sharded) return refuse(h, fn, "sharded handles are not supported");
    if (h->footprint.H < 1) return refuse(h, fn, "no footprint table is set (gvom_footprint_set)");
    if (h->chassis.H < 1) return refuse(h, fn, "no chassis is set (gvom_chassis_set)");
    if (volume && h->footprint.H > GVOM_POSE_MAX_HEADINGS) return refuse(h, fn, "footprint tables of more than 64 headings are not supported", GVOM_ERR_CAPACITY);
    if (h->chassis.H != h->footprint.H) return refuse(h, fn, "the chassis was set for another number of headings than the footprint table has");
    return GVOM_OK;
}
static int check_states(gvom_handle *h, const char *fn, int64_t H, int64_t xy) { return H * xy * xy > GVOM_POSE_MAX_STATES ? refuse(h, fn, "more than 2^28 states (headings x xy_size^2)", GVOM_ERR_CAPACITY) : GVOM_OK; }

// THE GROUND a call reads: the caller's map (a staged host map takes dev over), or a map set's, which k_attitude_ground writes into the
// call's own grow-only buffer.  ground_reserve, in front of the call's uploads: room for it in the call's record, counted there;
// ground_write, behind the call's set_wait_releases: the pass itself, on the handle's stream
struct Ground { DevSet *m = nullptr; double *own = nullptr; const double *dev = nullptr; };
static int ground_reserve(gvom_handle *h, Ground &g, GroundCall &call, const double *ground)
{
    const size_t xy = (size_t)h->prm.xy_size;
    if (const int rc = g.m ? stage_buf(h, call, call.ground, xy * xy * 8) : GVOM_OK) return rc;
    g.own = g.m ? (double *)call.ground.p : nullptr;
    g.dev = g.m ? g.own : ground;
    return GVOM_OK;
}
static int ground_write(gvom_handle *h, const Ground &g, int flags)
{
    if (g.m) HIPCHK(h, gvom_launch_attitude_ground(h->stream, h->prm.xy_size, (flags & GVOM_ATTITUDE_INFERRED_GROUND) ? 1 : 0, part_ptr<const double>(g.m, 4),
                                                  part_ptr<const double>(g.m, 5), g.own));
    return GVOM_OK;
}

// THE FIELD of gvom_score_body and gvom_body_volume, whose arguments are past check_one_source: a voxel distance product's (f) or the
// caller's pointer with its origin.  B = its corner in world voxels, n and zs = its sides
struct Field { DevSet *f = nullptr; int64_t B[3]; int n, zs; };
static int field_of(gvom_handle *h, const char *fn, int64_t id, const int64_t origin[3], Field &F)
{
    if (const int rc = id >= 0 ? product_of_kind(h, fn, id, GVOM_PRODUCT_VOXEL_DISTANCE, "unknown or stale distance field id", &F.f) : GVOM_OK) return rc;
    F.n = F.f ? F.f->xy : h->prm.xy_size; F.zs = F.f ? F.f->zs : h->prm.z_size;
    for (int k = 0; k < 3; ++k) {
        if (!F.f && (origin[k] < -((int64_t)1 << 40) || origin[k] > ((int64_t)1 << 40))) return refuse(h, fn, "a field origin beyond 2^40 voxels");
        F.B[k] = F.f ? F.f->origin[k] : origin[k];
    }
    return GVOM_OK;
}

// the chassis as AttitudeParams, AttitudeVolumeParams and BodyParams take it: the lengths (axle_mid where the params have one), the limits
static void chassis_lengths(const gvom_handle *h, double &wheelbase, double &track, double *axle_mid)
{
    const gvom_chassis_t &c = h->chassis.c;
    wheelbase = c.front_axle - c.rear_axle; track = c.track;
    if (axle_mid) *axle_mid = 0.5 * (c.front_axle + c.rear_axle);
}
template <class P> static void chassis_limits(const gvom_chassis_t &c, P &p) { p.belly_height = c.belly_height; p.max_pitch = c.max_pitch; p.max_roll = c.max_roll; p.min_clearance = c.min_clearance; }

// what k_body and k_volume_body take beside P.R: the chassis lengths, the field's box and the sphere count
static void body_params(const gvom_handle *h, const Field &F, float min_margin, BodyParams &P)
{
    chassis_lengths(h, P.wheelbase, P.track, &P.axle_mid);
    P.z_res = h->prm.z_resolution;
    P.bx = F.B[0]; P.by = F.B[1]; P.bz = F.B[2];
    P.n = F.n; P.zs = F.zs; P.S = h->body.S; P.min_margin = min_margin;
}

int check_one_source(gvom_handle *h, const char *fn, bool id, bool also, bool missing, const char *by_id, const char *both, const char *other)
{
    if (id && also) return refuse(h, fn, std::string("give ") + by_id + " or " + both + ", not both");
    if (!id && missing) return refuse(h, fn, std::string("give ") + by_id + " or " + other);
    return GVOM_OK;
}

int check_goals(gvom_handle *h, const char *fn, const void *goals, int64_t n_goals, int32_t max_cost, int32_t max_rounds)
{
    if (!goals || n_goals < 1 || n_goals > GVOM_CTG_MAX_GOALS) return refuse(h, fn, "between 1 and 65536 goals");
    if (max_cost < 0 || max_cost > GVOM_CTG_MAX_COST) return refuse(h, fn, "max_cost outside 0 .. 2^30");
    if (max_rounds < 0) return refuse(h, fn, "max_rounds must not be negative");
    return GVOM_OK;
}

int check_rollout_shape(gvom_handle *h, const char *fn, int64_t K, int64_t T, const int64_t origin_cells[2])
{
    if (T < 1 || T > GVOM_ROLLOUT_MAX_T) return refuse(h, fn, "T outside 1 .. 4096");
    if (K < 1) return refuse(h, fn, "K must be at least 1");
    if (K > GVOM_ROLLOUT_MAX_POSES / T) return refuse(h, fn, "more than 2^26 poses in one call", GVOM_ERR_CAPACITY);
    for (int k = 0; k < 2; ++k)
        if (origin_cells[k] < -((int64_t)1 << 40) || origin_cells[k] > ((int64_t)1 << 40)) return refuse(h, fn, "an origin beyond 2^40 cells");
    return GVOM_OK;
}

int check_side(gvom_handle *h, const char *fn) { return h->prm.xy_size > GVOM_CLEARANCE_MAX_XY ? refuse(h, fn, "maps of more than 4096 cells a side are not supported", GVOM_ERR_CAPACITY) : GVOM_OK; }

int check_clusters(gvom_handle *h, const char *fn, int32_t min_cells, int32_t max_clusters)
{
    if (min_cells < 1) return refuse(h, fn, "min_cells must be at least 1");
    if (max_clusters < 1 || max_clusters > GVOM_FRONTIER_MAX_CLUSTERS) return refuse(h, fn, "max_clusters outside 1 .. 2^20");
    return GVOM_OK;
}

// ---- the walk queries: what gvom_raycast / _score_viewpoints / _score_alignments and their atlas twins do alike (gvom_host.h) ---------------
int check_rays(gvom_handle *h, const char *fn, const float *from, int64_t K, const float *to, int64_t n, int flags)
{
    if (!from || !to) return refuse(h, fn, "from and to must not be NULL");
    if (n < 1) return refuse(h, fn, "n must be at least 1");
    if (K != 1 && K != n) return refuse(h, fn, "K must be 1 or n");
    if (flags & ~(GVOM_RAY_UNKNOWN_BLOCKS | GVOM_RAY_CHECK_TARGET)) return refuse(h, fn, "unknown flag bits");
    if (n > GVOM_RAYCAST_MAX_RAYS) return refuse(h, fn, "more than 2^26 rays in one call", GVOM_ERR_CAPACITY);
    return GVOM_OK;
}

int rays_fill(gvom_handle *h, CallState &call, const float *from, int64_t K, const float *to, int64_t n, int on_device, int flags, RayQuery &Q)
{
    Q.from = from; Q.to = to; Q.n = (long)n;
    Q.one_origin = K == 1 ? 1 : 0;
    Q.unknown_blocks = (flags & GVOM_RAY_UNKNOWN_BLOCKS) ? 1 : 0;
    Q.check_target = (flags & GVOM_RAY_CHECK_TARGET) ? 1 : 0;
    HIPCHK(h, join_second_stream(h));
    if (on_device) return GVOM_OK;
    const HostPart parts[2] = {{from, (size_t)K * 12}, {to, (size_t)n * 12}};                // host segments: staged, and up before the call returns
    const void *dev[2];
    if (const int rc = stage_host(h, call, parts, 2, true, dev)) return rc;
    Q.from = (const float *)dev[0]; Q.to = (const float *)dev[1];
    return GVOM_OK;
}

int check_views(gvom_handle *h, const char *fn, const double *poses, int64_t K, double max_range, int32_t stride_h, int32_t stride_w, int flags,
                int64_t span, const char *spans, ViewBeams *B)
{
    if (!poses) return refuse(h, fn, "poses must not be NULL");
    if (h->range_image.H <= 0) return refuse(h, fn, "no sensor model (gvom_sensor_model_set)");
    if (K < 1) return refuse(h, fn, "K must be at least 1");
    if (stride_h < 1 || stride_w < 1) return refuse(h, fn, "the beam strides must be at least 1");
    if (!std::isfinite(max_range) || !(max_range > 0.0)) return refuse(h, fn, "max_range must be finite and > 0");
    if (flags & ~GVOM_RAY_UNKNOWN_BLOCKS) return refuse(h, fn, "unknown flag bits");
    if (K > GVOM_VIEWPOINT_MAX_POSES) return refuse(h, fn, "more than 65536 viewpoints in one call", GVOM_ERR_CAPACITY);
    B->nh = ((int64_t)h->range_image.H + stride_h - 1) / stride_h; B->nw = ((int64_t)h->range_image.W + stride_w - 1) / stride_w; B->nb = B->nh * B->nw;
    if (B->nb > GVOM_VIEWPOINT_MAX_BEAMS) return refuse(h, fn, "more than 2^22 selected beams", GVOM_ERR_CAPACITY);
    if (B->nb * (span + 1) >= ((int64_t)1 << 31)) return refuse(h, fn, std::string("beams x (") + spans + " + 1) reaches 2^31", GVOM_ERR_CAPACITY);
    return GVOM_OK;
}

int64_t views_batch(const gvom_handle *h, int64_t bits, int64_t K, size_t *bm_words)
{
    *bm_words = (((size_t)bits + 31) / 32 + 63) & ~(size_t)63;                  // whole 256-byte lines
    const int64_t batch = (int64_t)(((size_t)h->viewpoints.mb << 20) / (*bm_words * 4));
    return std::max<int64_t>(1, std::min<int64_t>(batch, std::min<int64_t>(K, GVOM_VIEWPOINT_MAX_BATCH)));
}

void views_fill(const gvom_handle *h, const RayQuery &R, const ViewBeams &B, int64_t K, double max_range, int32_t stride_h, int32_t stride_w, int flags,
                size_t bm_words, ViewQuery &Q)
{
    memset(&Q, 0, sizeof Q);
    Q.dir = (const double *)h->range_image.model.p; Q.off = Q.dir + (size_t)h->range_image.H * h->range_image.W * 3;
    Q.max_range = max_range;
    Q.W = h->range_image.W; Q.stride_h = stride_h; Q.stride_w = stride_w;
    Q.nh = (int)B.nh; Q.nw = (int)B.nw; Q.nwc = (int)((B.nw + 63) / 64); Q.nb = (int)B.nb; Q.K = (int)K;
    Q.unknown_blocks = (flags & GVOM_RAY_UNKNOWN_BLOCKS) ? 1 : 0;
    Q.lit = R.lit; Q.cap = R.cap; Q.bm_words = (uint32_t)bm_words;
}

int views_run(gvom_handle *h, Buf &bitmaps, ViewQuery &Q, int64_t batch, int32_t *rows, const std::function<hipError_t(int)> &launch_batch,
              const std::function<hipError_t()> &launch_best)
{
    const int64_t K = Q.K;
    HIPCHK(h, hipMemsetAsync(rows, 0, (size_t)K * 32, h->stream));
    for (int64_t k0 = 0; k0 < K; k0 += batch) {
        const int nk = (int)std::min<int64_t>(batch, K - k0);
        Q.k0 = (int)k0;
        HIPCHK(h, hipMemsetAsync(bitmaps.p, 0, (size_t)nk * Q.bm_words * 4, h->stream));
        HIPCHK(h, launch_batch(nk));
    }
    Q.k0 = 0;
    HIPCHK(h, launch_best());
    return GVOM_OK;
}

int check_align(gvom_handle *h, const char *fn, const float *cloud, int64_t n, const double *transforms, int64_t K, int dilate, const int32_t weights[5],
                size_t *grid_bytes)
{
    if (!cloud || !transforms || !weights) return refuse(h, fn, "cloud, transforms and weights must not be NULL");
    if (n < 1) return refuse(h, fn, "n must be at least 1");
    if (K < 1) return refuse(h, fn, "K must be at least 1");
    if (dilate != 0 && dilate != 1) return refuse(h, fn, "dilate must be 0 or 1");
    for (int c = 0; c < 5; ++c)
        if (weights[c] < -GVOM_ALIGN_MAX_WEIGHT || weights[c] > GVOM_ALIGN_MAX_WEIGHT) return refuse(h, fn, "a weight outside -1024 .. 1024");
    if (n > GVOM_ALIGN_MAX_POINTS) return refuse(h, fn, "more than 2^20 returns in one call", GVOM_ERR_CAPACITY);
    if (K > GVOM_ALIGN_MAX_CANDIDATES) return refuse(h, fn, "more than 65536 candidates in one call", GVOM_ERR_CAPACITY);
    if (n * K > GVOM_ALIGN_MAX_PAIRS) return refuse(h, fn, "more than 2^32 pairs in one call", GVOM_ERR_CAPACITY);
    *grid_bytes = gvom_align_grid_bytes(h->prm.xy_size, h->prm.z_size);
    if (*grid_bytes / 4 > 0xffffffffull) return refuse(h, fn, "the class grid of this map has 2^32 words or more", GVOM_ERR_CAPACITY);
    return GVOM_OK;
}

int align_fill(gvom_handle *h, CallState &call, const float *cloud, int64_t n, const double *transforms, int64_t K, int on_device, int dilate,
               const int32_t weights[5], AlignParams &P, const float **cdev, const double **tdev)
{
    const int xy = h->prm.xy_size;
    P.n = (long)n; P.K = (int)K; P.xy = xy; P.zs = h->prm.z_size; P.rw = (xy + 15) / 16; P.dilate = dilate;
    for (int c = 0; c < 5; ++c) P.w[c] = weights[c];
    *cdev = cloud; *tdev = transforms;
    HIPCHK(h, join_second_stream(h));
    if (on_device) return GVOM_OK;
    const HostPart parts[2] = {{transforms, (size_t)K * 96}, {cloud, (size_t)n * 12}};      // host inputs: staged, and up before the call returns
    const void *dev[2];
    if (const int rc = stage_host(h, call, parts, 2, true, dev)) return rc;
    *tdev = (const double *)dev[0]; *cdev = (const float *)dev[1];
    return GVOM_OK;
}

int check_host_cost(gvom_handle *h, const char *fn, const int32_t *cost, size_t n2)
{
    for (size_t k = 0; k < n2; ++k)
        if (cost[k] < 0 || cost[k] > 65535) return refuse(h, fn, "a host cost map holds a value outside 0 .. 65535");
    return GVOM_OK;
}

int cost_field_of(gvom_handle *h, const char *fn, int64_t id, DevSet **f) { return product_of_kind(h, fn, id, GVOM_PRODUCT_COSTFIELD, "unknown or stale cost field id", f); }
int atlas_field_of(gvom_handle *h, const char *fn, int64_t id, DevSet **f) { return product_of_kind(h, fn, id, GVOM_PRODUCT_ATLAS_FIELD, "unknown or stale atlas field id", f); }

int map_set_of(gvom_handle *h, int64_t id, DevSet **m)
{
    if ((*m = find_set(h->dsets, id))) return GVOM_OK;
    h->err = "unknown or stale device map set id";
    return GVOM_ERR_INVALID;
}

// ---- host inputs (gvom_host.h) -----------------------------------------------------------------------------------------------------------
int stage_host(gvom_handle *h, CallState &call, const HostPart *parts, int n, bool sync, const void **dev)
{
    size_t at[4], need = 0;
    for (int i = 0; i < n; ++i) {
        at[i] = need;
        if (parts[i].src) need += i + 1 < n ? align256(parts[i].bytes) : parts[i].bytes;
    }
    if (const int rc = stage_buf(h, call, need)) return rc;
    const Buf &b = call.stage;
    for (int i = 0; i < n; ++i) {
        dev[i] = parts[i].src ? (char *)b.p + at[i] : nullptr;
        if (parts[i].src) HIPCHK(h, hipMemcpyAsync((char *)b.p + at[i], parts[i].src, parts[i].bytes, hipMemcpyHostToDevice, h->stream));
    }
    if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
    return GVOM_OK;
}

int ctg_cost_params(gvom_handle *h, const char *fn, const gvom_ctg_params *params, int flags, CtgCostParams *C)
{
    const gvom_ctg_params &p = *params;
    const bool ok = p.density_threshold == p.density_threshold && p.inflation_cells2 >= 0 && p.base >= 1 &&
                    p.soft_weight >= 0 && p.soft_weight <= 65535 && p.unknown_cost >= 0 && p.unknown_cost <= 65535 &&
                    p.rough_weight >= 0 && p.rough_weight <= 65535 &&
                    (p.rough_weight == 0 || (isfinite(p.min_roughness) && isfinite(p.max_roughness) && p.max_roughness > p.min_roughness));
    if (!ok) return refuse(h, fn, "bad cost parameters (NaN threshold, base < 1, a weight outside 0 .. 65535, a negative inflation, or an empty / non-finite roughness range)");
    memset(C, 0, sizeof *C);
    C->density_threshold = p.density_threshold; C->min_roughness = p.min_roughness; C->max_roughness = p.max_roughness;
    C->inflation_cells2 = p.inflation_cells2; C->base = p.base; C->soft_weight = p.soft_weight; C->unknown_cost = p.unknown_cost;
    C->rough_weight = p.rough_weight;
    C->use_negative = (flags & GVOM_CTG_NO_NEGATIVE) ? 0 : 1; C->unknown_blocks = (flags & GVOM_CTG_UNKNOWN_BLOCKS) ? 1 : 0;
    return GVOM_OK;
}

// ---- the calls that wait (gvom_host.h) ---------------------------------------------------------------------------------------------------
template <class Enqueue> int solve_rounds(gvom_handle *h, uint32_t *cnt, uint32_t *fl, uint32_t *pin, int ntiles, int batch, int64_t limit,
                                          Enqueue enqueue, SolveRounds *out)
{
    int64_t rounds = 0, tiles = 0;
    bool converged = false;
    while (!converged && rounds < limit) {
        const int nb = solve_batch_len(batch, limit, rounds);
        if (rounds) HIPCHK(h, hipMemsetAsync(cnt, 0, SOLVE_CNT_BATCH_BYTES, h->stream));
        for (int r = 0; r < nb; ++r) {
            const int64_t k = rounds + r;
            HIPCHK(h, enqueue(k, fl + (k & 1) * ntiles, fl + ((k + 1) & 1) * ntiles, cnt + r, cnt + SOLVE_CNT_RAN + r));
        }
        HIPCHK(h, hipMemcpyAsync(pin, cnt, SOLVE_CNT_BATCH_BYTES, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        const SolveLook look = solve_look(pin, nb);
        converged = look.converged; rounds += look.ran; tiles += look.tiles;
    }
    out->converged = converged; out->rounds = rounds; out->tiles = tiles;
    return GVOM_OK;
}

int solve_work_reserve(gvom_handle *h, SolveCall &call, size_t bytes)
{
    SolveWork &w = call.solve;
    if (const int rc = stage_buf(h, call, w.work, bytes)) return rc;
    if (!w.pin) HIPCHK(h, hipHostMalloc((void **)&w.pin.p, 256, hipHostMallocDefault));
    return GVOM_OK;
}

int goal_work_start(gvom_handle *h, const GoalWorkPtrs &G, const void *goals, size_t bytes)
{
    HIPCHK(h, hipMemcpyAsync(G.goals, goals, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(G.cnt, 0, 256, h->stream));
    return GVOM_OK;
}

int goal_solve_finish(gvom_handle *h, const char *fn, SolveWork &w, DevSet *set, int64_t *product_id, const SolveRounds &S, int32_t max_rounds,
                      int64_t info[4])
{
    if (const int rc = product_publish(h, set, product_id)) return rc;     // (`ready` goes in front of the counters' way back)
    HIPCHK(h, hipMemcpyAsync(w.pin, w.work.p, 256, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (!S.converged && max_rounds == 0) { set->id = *product_id = -1; return refuse(h, fn, "the field did not settle", GVOM_ERR_HIP); }   // (nobody gets it)
    w.last_rounds = (int)std::min<int64_t>(S.rounds, INT32_MAX);
    w.last_tiles = (int)std::min<int64_t>(S.tiles, INT32_MAX);
    if (info) { info[0] = S.converged ? 1 : 0; info[1] = S.rounds; info[2] = w.pin[CTG_CNT_REACHED]; info[3] = w.pin[CTG_CNT_SEEDED]; }
    return GVOM_OK;
}

int ctg_solve(gvom_handle *h, SolveWork &w, const GoalWorkPtrs &G, int n, const int32_t *cost32, uint16_t *c16, int32_t *D, uint8_t *dir,
              int n_goals, int32_t max_cost, int32_t max_rounds, SolveRounds *out)
{
    const int nt = gvom_ctg_tiles(n);
    HIPCHK(h, gvom_launch_ctg_seed(h->stream, n, cost32, c16, D, G.fl, G.goals, n_goals, G.cnt + CTG_CNT_SEEDED));
    const int32_t cap = max_cost == 0 ? GVOM_CTG_MAX_COST : max_cost;
    const int inner = h->cost_to_go.solve.tune_inner > 0 ? h->cost_to_go.solve.tune_inner : 256;
    const int batch = h->cost_to_go.solve.tune_batch > 0 ? h->cost_to_go.solve.tune_batch : 8;
    // by induction over the tile crossings of a shortest path the solve ends after at most (crossings + 1) rounds of tiles that
    // reach their fixed point; the limit below is beyond anything n <= 4096 can need and only keeps the loop finite
    const int64_t limit = max_rounds > 0 ? (int64_t)max_rounds : (int64_t)1 << 22;
    const int rc = solve_rounds(h, G.cnt, G.fl, w.pin, nt * nt, batch, limit, [&](int64_t, uint32_t *fin, uint32_t *fout, uint32_t *any, uint32_t *ran) {
        return gvom_launch_ctg_relax(h->stream, n, c16, D, fin, fout, any, ran, cap, inner);
    }, out);
    if (rc) return rc;
    HIPCHK(h, gvom_launch_ctg_dirs(h->stream, n, c16, D, dir, G.cnt + CTG_CNT_REACHED));
    return GVOM_OK;
}

int frontier_work(gvom_handle *h, SolveCall &call, int n, FrWork *W)
{
    const FrOffsets o = fr_offsets(n, gvom_frontier_tiles(n), gvom_frontier_blocks(n));
    if (const int rc = solve_work_reserve(h, call, o.end)) return rc;
    char *p = (char *)call.solve.work.p;
    *W = FrWork{(uint32_t *)p, (uint32_t *)(p + o.flags), (uint32_t *)(p + o.bc), (uint32_t *)(p + o.L), (uint32_t *)(p + o.count), o.bc};
    return GVOM_OK;
}

int frontier_solve(gvom_handle *h, const char *fn, SolveWork &w, int n, const int32_t *D, const FrWork &W, int32_t min_cells,
                   int32_t max_clusters, DevSet *set, int64_t *product_id, int64_t info[4], const std::function<hipError_t()> &more)
{
    const int nt = gvom_frontier_tiles(n);
    uint32_t *const cnt = W.cnt;
    int32_t *rows = part_ptr<int32_t>(set, 0), *cmap = part_ptr<int32_t>(set, 2), *counts = part_ptr<int32_t>(set, 3);
    int64_t *sums = part_ptr<int64_t>(set, 1);
    HIPCHK(h, gvom_launch_frontier_rows(h->stream, 0, max_clusters, rows, sums, cnt + FR_CNT_KEPT, cnt + FR_CNT_CELLS, counts));
    const int inner = h->frontiers.solve.tune_inner > 0 ? h->frontiers.solve.tune_inner : 256;
    const int batch = h->frontiers.solve.tune_batch > 0 ? h->frontiers.solve.tune_batch : 8;
    // labels only go down and there are n * n of them: a round that lowers none flags no tile, so fewer than n * n + 1 rounds lower
    // one.  The limit cannot be reached and only keeps the loop finite
    SolveRounds S;
    int rc = solve_rounds(h, cnt, W.fl, w.pin, nt * nt, batch, (int64_t)n * n + 1, [&](int64_t, uint32_t *fin, uint32_t *fout, uint32_t *any, uint32_t *ran) {
        return gvom_launch_frontier_relax(h->stream, n, W.L, fin, fout, any, ran, inner);
    }, &S);
    if (rc) return rc;
    if (!S.converged) return refuse(h, fn, "the labels did not settle", GVOM_ERR_HIP);                  // (the set keeps id -1: nobody gets it)
    HIPCHK(h, gvom_launch_frontier_finish(h->stream, n, min_cells, max_clusters, D, W.L, W.count, W.bc, cnt + FR_CNT_KEPT, cnt + FR_CNT_CELLS, rows,
                                          sums, cmap, counts));
    if (more) HIPCHK(h, more());
    if ((rc = product_publish(h, set, product_id))) return rc;             // (`ready` goes in front of the counters' way back)
    HIPCHK(h, hipMemcpyAsync(w.pin, cnt, 256, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    w.last_rounds = (int)std::min<int64_t>(S.rounds, INT32_MAX);
    w.last_tiles = (int)std::min<int64_t>(S.tiles, INT32_MAX);
    if (info) { info[0] = S.rounds; info[1] = w.pin[FR_CNT_KEPT]; info[2] = w.pin[FR_CNT_CELLS]; info[3] = w.pin[FR_CNT_KEPT + 1]; }
    return GVOM_OK;
}
}  // namespace gvom_host

extern "C" {
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
    static const char *const elsewhere[GVOM_PRODUCT_POSEFIELD + 1] = {                                  // by kind: who makes it instead
        nullptr, nullptr, nullptr, nullptr, nullptr, "a clearance product is made by gvom_clearance", "a raycast product is made by gvom_raycast",
        "a cost field is made by gvom_cost_to_go", nullptr, nullptr, "rollouts are made by gvom_score_rollouts", nullptr,
        "alignment scores are made by gvom_score_alignments", nullptr, "attitude scores are made by gvom_score_attitude", nullptr,
        "frontiers are made by gvom_frontiers", nullptr, "viewpoint scores are made by gvom_score_viewpoints", nullptr, "pose fields are made by gvom_pose_field"};
    const char *const maker = kind >= 0 && kind <= GVOM_PRODUCT_POSEFIELD ? elsewhere[kind] : nullptr;
    if (maker || kind < 1 || kind > GVOM_N_PRODUCT_KINDS) return refuse(h, "gvom_device_product", maker ? maker : "unknown product kind");
    if (h->sharded) return refuse(h, "gvom_device_product", "sharded handles are not supported");
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
    DevSet *set = nullptr;
    int rc = product_acquire(h, kind, set_bytes(kind, xy, zs, cap), set_bytes(kind, xy, zs, cap + cap / 2), "gvom_device_product", nullptr, &set);   // (a cloud grows with the map: headroom)
    if (rc) return rc;
    set->cap = cap;
    const Fused &F = h->fused[h->cur];
    HIPCHK(h, join_second_stream(h));
    if ((rc = set_wait_releases(h, set))) return rc;
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
        HIPCHK(h, hipMemsetAsync(set->mem, 0, 8, h->stream));
        HIPCHK(h, gvom_launch_voxel_cloud(h->stream, P, (double)F.origin[0], (double)F.origin[1], (double)F.origin[2], F.state, F.tags,
                                          (const uint4 *)F.rows.p, (const float *)F.metrics.p, part_ptr<float>(set, 0), part_ptr<float>(set, 1), cap,
                                          part_ptr<unsigned long long>(set, 2)));
        break;
    }
    case GVOM_PRODUCT_HEIGHT_CLOUD: HIPCHK(h, launch_height_cloud(h, F, (float *)set->mem, nullptr)); break;
    default: HIPCHK(h, launch_height_cloud(h, F, nullptr, (float *)set->mem)); break;
    }
    return product_publish(h, set, product_id);
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
    const char *const fn = "gvom_clearance";
    int rc;
    if (h->sharded) return refuse(h, fn, "sharded handles are not supported");
    if (flags & ~GVOM_CLEARANCE_NO_NEGATIVE) return refuse(h, "gvom_clearance", "unknown flag bits");
    if (density_threshold != density_threshold) return refuse(h, "gvom_clearance", "the density threshold is not a number");
    if ((rc = check_one_source(h, fn, map_set_id >= 0, positive || negative, !positive, "a map set id", "map pointers", "a positive map")) || (rc = check_side(h, fn))) return rc;
    const int xy = h->prm.xy_size;
    const size_t n2 = (size_t)xy * xy;
    const int32_t *pos = positive, *neg = negative;
    if (map_set_id >= 0) {
        DevSet *m = nullptr;
        if ((rc = map_set_of(h, map_set_id, &m))) return rc;
        pos = part_ptr<const int32_t>(m, 0); neg = part_ptr<const int32_t>(m, 1);
    }
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *set = nullptr;
    const size_t bytes = set_bytes(GVOM_PRODUCT_CLEARANCE, xy, 0, 0);
    rc = product_acquire(h, GVOM_PRODUCT_CLEARANCE, bytes, bytes, fn, &h->clearance, &set);
    if (rc) return rc;
    if ((rc = stage_buf(h, h->clearance, h->clearance.g, gvom_clearance_scratch_bytes(xy)))) return rc;
    HIPCHK(h, join_second_stream(h));
    if (map_set_id < 0 && !on_device) {                                     // host maps: staged, and up before the call returns
        if ((rc = stage_buf(h, h->clearance, 2 * n2 * 4))) return rc;
        int32_t *st = (int32_t *)h->clearance.stage.p;
        HIPCHK(h, hipMemcpyAsync(st, positive, n2 * 4, hipMemcpyHostToDevice, h->stream));
        if (negative) HIPCHK(h, hipMemcpyAsync(st + n2, negative, n2 * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        pos = st; neg = negative ? st + n2 : nullptr;
    }
    if (flags & GVOM_CLEARANCE_NO_NEGATIVE) neg = nullptr;
    if ((rc = set_wait_releases(h, set))) return rc;
    HIPCHK(h, gvom_launch_clearance(h->stream, xy, h->prm.xy_resolution, pos, neg, density_threshold, max_cells2,
                                    (uint16_t *)h->clearance.g.p, part_ptr<float>(set, 0), part_ptr<int32_t>(set, 1), h->clearance.shape));
    return product_publish(h, set, product_id);
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
    const char *const fn = "gvom_raycast";
    int rc;
    if (h->sharded) return refuse(h, fn, "sharded handles are not supported");
    if ((rc = check_rays(h, fn, from, K, to, n, flags))) return rc;
    if (!h->has_combined) return GVOM_NO_DATA;
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *set = nullptr;
    const size_t bytes = set_bytes(GVOM_PRODUCT_RAYCAST, 0, 0, n);
    if ((rc = product_acquire(h, GVOM_PRODUCT_RAYCAST, bytes, bytes, fn, &h->raycast, &set))) return rc;
    set->cap = n;
    const Fused &F = h->fused[h->cur];
    ScanParams P;
    RayQuery Q;
    memset(&Q, 0, sizeof Q);
    raycast_params(h, F, P, Q);
    if ((rc = rays_fill(h, h->raycast, from, K, to, n, on_device, flags, Q))) return rc;
    if ((rc = set_wait_releases(h, set))) return rc;
    HIPCHK(h, gvom_launch_raycast(h->stream, P, Q, F.state, F.tags, part_ptr<int32_t>(set, 0), part_ptr<float>(set, 1)));
    if ((rc = product_publish(h, set, product_id))) return rc;
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
    const char *const fn = "gvom_cost_to_go";
    int rc;
    if (h->sharded) return refuse(h, fn, "sharded handles are not supported");
    if (flags & ~(GVOM_CTG_NO_NEGATIVE | GVOM_CTG_UNKNOWN_BLOCKS)) return refuse(h, "gvom_cost_to_go", "unknown flag bits");
    if ((rc = check_one_source(h, fn, map_set_id >= 0, cost, !cost, "a map set id", "a cost map", "a cost map"))) return rc;
    if (map_set_id >= 0 && !params) return refuse(h, "gvom_cost_to_go", "a map set needs the cost parameters");
    if ((rc = check_goals(h, fn, goals, n_goals, max_cost, max_rounds)) || (rc = check_side(h, fn))) return rc;
    const int xy = h->prm.xy_size;
    const size_t n2 = (size_t)xy * xy;
    for (int64_t k = 0; k < 2 * n_goals; ++k)
        if (goals[k] < 0 || goals[k] >= xy) return refuse(h, "gvom_cost_to_go", "a goal lies outside the window");
    CtgCostParams C;
    memset(&C, 0, sizeof C);
    DevSet *m = nullptr;
    if (map_set_id >= 0) {
        if ((rc = ctg_cost_params(h, fn, params, flags, &C)) || (rc = map_set_of(h, map_set_id, &m))) return rc;
    } else if (!on_device && (rc = check_host_cost(h, fn, cost, n2))) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *set = nullptr;
    const size_t bytes = set_bytes(GVOM_PRODUCT_COSTFIELD, xy, 0, 0);
    if ((rc = product_acquire(h, GVOM_PRODUCT_COSTFIELD, bytes, bytes, fn, &h->cost_to_go, &set))) return rc;
    const int nt = gvom_ctg_tiles(xy);
    const GoalWork lay = goal_work(nt * nt, 8, 0);
    if ((rc = solve_work_reserve(h, h->cost_to_go, lay.end))) return rc;
    const GoalWorkPtrs G = goal_work_ptrs(h->cost_to_go.solve, lay);
    HIPCHK(h, join_second_stream(h));
    const void *cost32 = map_set_id < 0 ? cost : nullptr;
    if (map_set_id < 0 && !on_device) {                                     // a host cost map: staged
        const HostPart part = {cost, n2 * 4};
        if ((rc = stage_host(h, h->cost_to_go, &part, 1, false, &cost32))) return rc;
    }
    const size_t clr_g = align256(gvom_clearance_scratch_bytes(xy)), clr_map = align256(n2 * 4);
    if (m && C.inflation_cells2 > 0 && (rc = stage_buf(h, h->cost_to_go, h->cost_to_go.clr, clr_g + 2 * clr_map))) return rc;
    if ((rc = goal_work_start(h, G, goals, (size_t)n_goals * 8)) || (rc = set_wait_releases(h, set))) return rc;
    int32_t *D = part_ptr<int32_t>(set, 0);
    uint16_t *c16 = part_ptr<uint16_t>(set, 2);
    if (m) {
        const int32_t *mp = part_ptr<const int32_t>(m, 0), *mn = part_ptr<const int32_t>(m, 1);
        const int32_t *cd2 = nullptr;
        if (C.inflation_cells2 > 0) {
            char *q = (char *)h->cost_to_go.clr.p;
            HIPCHK(h, gvom_launch_clearance(h->stream, xy, h->prm.xy_resolution, mp, C.use_negative ? mn : nullptr, C.density_threshold,
                                            C.inflation_cells2, (uint16_t *)q, (float *)(q + clr_g), (int32_t *)(q + clr_g + clr_map)));
            cd2 = (const int32_t *)(q + clr_g + clr_map);
        }
        HIPCHK(h, gvom_launch_travcost(h->stream, xy, mp, mn, part_ptr<const int32_t>(m, 2), part_ptr<const double>(m, 3), cd2, C, c16));
    }
    SolveRounds S;
    if ((rc = ctg_solve(h, h->cost_to_go.solve, G, xy, (const int32_t *)cost32, c16, D, part_ptr<uint8_t>(set, 1), (int)n_goals, max_cost, max_rounds, &S))) return rc;
    return goal_solve_finish(h, fn, h->cost_to_go.solve, set, product_id, S, max_rounds, info);
}
// ---- rollout scoring (gvom_footprint_set, gvom_score_rollouts) -------------------------------------------------------------------
// K trajectories of T poses each, scored by k_rollouts (gvom_rollouts.hip) against a uint16 cost map with the footprint table of the
// handle: a product of kind GVOM_PRODUCT_ROLLOUTS sized by K and T.  The kernel runs on the handle's stream -- behind the solve
// that wrote the cost field it reads, and in front of whatever recycles that field later.  Enqueues and returns.
VIS int gvom_footprint_set(gvom_t *h, int32_t n_headings, const int32_t *start, const int16_t *offsets)
{
    if (!h) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!start || !offsets) return refuse(h, "gvom_footprint_set", "start and offsets must not be NULL");
    if (n_headings < 1 || n_headings > GVOM_ROLLOUT_MAX_HEADINGS) return refuse(h, "gvom_footprint_set", "between 1 and 1024 headings");
    if (start[0] != 0) return refuse(h, "gvom_footprint_set", "start[0] must be 0");
    for (int k = 0; k < n_headings; ++k) {
        const int64_t m = (int64_t)start[k + 1] - start[k];
        if (m < 1 || m > GVOM_ROLLOUT_MAX_CELLS) return refuse(h, "gvom_footprint_set", "every heading needs between 1 and 16384 cells");
        if (start[k + 1] > GVOM_ROLLOUT_MAX_TABLE) return refuse(h, "gvom_footprint_set", "more than 2^22 offsets in the table", GVOM_ERR_CAPACITY);
    }
    HIPCHK(h, hipSetDevice(h->device));
    const size_t sb = (size_t)(n_headings + 1) * 4, offs_at = align256(sb), ob = (size_t)start[n_headings] * 4;
    h->footprint.H = 0;                                                     // (no table while this one is on its way)
    if (h->footprint.tab.bytes < offs_at + ob) HIPCHK(h, hipStreamSynchronize(h->stream));   // the kernels that read the table it outgrows
    const int rc = ensure(h, h->footprint.tab, offs_at + ob);
    if (rc) return rc;
    // on the handle's stream: behind whatever still reads the previous table
    HIPCHK(h, hipMemcpyAsync(h->footprint.tab.p, start, sb, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync((char *)h->footprint.tab.p + offs_at, offsets, ob, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->footprint.offs_at = offs_at; h->footprint.H = n_headings;
    h->footprint.total = start[n_headings]; ++h->footprint.gen;             // (gvom_attitude_volume rebuilds its table)
    return GVOM_OK;
}

VIS int gvom_score_rollouts(gvom_t *h, int64_t costfield_id, const uint16_t *cell_cost, const int32_t *cost_to_go, const float *poses,
                            int64_t K, int64_t T, int on_device, const int64_t origin_cells[2], int64_t *product_id)
{
    if (!h || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *product_id = -1;
    const char *const fn = "gvom_score_rollouts";
    int rc;
    if (h->sharded) return refuse(h, fn, "sharded handles are not supported");
    if (h->footprint.H < 1) return refuse(h, "gvom_score_rollouts", "no footprint table is set (gvom_footprint_set)");
    if (!poses || !origin_cells) return refuse(h, "gvom_score_rollouts", "poses and origin_cells must not be NULL");
    if ((rc = check_one_source(h, fn, costfield_id >= 0, cell_cost || cost_to_go, !cell_cost, "a cost field id", "map pointers", "a cell-cost map")) ||
        (rc = check_rollout_shape(h, fn, K, T, origin_cells)) || (rc = check_side(h, fn))) return rc;
    const int xy = h->prm.xy_size;
    const size_t n2 = (size_t)xy * xy;
    const uint16_t *c16 = cell_cost;
    const int32_t *D = cost_to_go;
    if (costfield_id >= 0) {
        DevSet *f = nullptr;
        if ((rc = cost_field_of(h, fn, costfield_id, &f))) return rc;
        c16 = part_ptr<const uint16_t>(f, 2); D = part_ptr<const int32_t>(f, 0);
    }
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *set = nullptr;
    const size_t bytes = set_bytes(GVOM_PRODUCT_ROLLOUTS, 0, 0, K, T);
    rc = product_acquire(h, GVOM_PRODUCT_ROLLOUTS, bytes, bytes, fn, &h->rollouts, &set);
    if (rc) return rc;
    set->cap = K; set->cols = T;
    const float *pdev = poses;
    HIPCHK(h, join_second_stream(h));
    if (!on_device) {                                                       // host poses (and maps): staged, and up before the call returns
        const HostPart parts[3] = {{cell_cost, n2 * 2}, {cost_to_go, n2 * 4}, {poses, (size_t)K * T * 12}};
        const void *dev[3];
        if ((rc = stage_host(h, h->rollouts, parts, 3, true, dev))) return rc;
        if (dev[0]) c16 = (const uint16_t *)dev[0];
        if (dev[1]) D = (const int32_t *)dev[1];
        pdev = (const float *)dev[2];
    }
    if ((rc = set_wait_releases(h, set))) return rc;
    RolloutParams P;
    rollout_frame(h, K, T, origin_cells, P);
    HIPCHK(h, gvom_launch_rollouts(h->stream, P, pdev, (const int32_t *)h->footprint.tab.p, (const uint32_t *)((char *)h->footprint.tab.p + h->footprint.offs_at),
                                   c16, D, part_ptr<int32_t>(set, 0), part_ptr<uint16_t>(set, 1)));
    return product_publish(h, set, product_id);
}

// ---- terrain attitude scoring (gvom_chassis_set, gvom_score_attitude) -------------------------------------------------------------
// K trajectories of T poses each, scored by k_attitude (gvom_attitude.hip) against one float64 ground map with the footprint table and
// the chassis of the handle: a product of kind GVOM_PRODUCT_ATTITUDE sized by K and T.  With a map set, k_attitude_ground first
// writes the ground map from the set's height and inferred-height maps into a grow-only buffer of the handle.  The kernels run on
// the handle's stream -- behind the combine that wrote the set, and in front of whatever recycles it later.  Enqueues and returns.
VIS int gvom_chassis_set(gvom_t *h, const gvom_chassis_t *c, int32_t n_headings, const double *cos_sin)
{
    if (!h) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!c || !cos_sin) return refuse(h, "gvom_chassis_set", "the chassis and cos_sin must not be NULL");
    if (n_headings < 1 || n_headings > GVOM_ROLLOUT_MAX_HEADINGS) return refuse(h, "gvom_chassis_set", "between 1 and 1024 headings");
    if (!(isfinite(c->front_axle) && isfinite(c->rear_axle) && isfinite(c->track) && isfinite(c->belly_height))) return refuse(h, "gvom_chassis_set", "a length is not finite");
    if (!(c->front_axle > c->rear_axle)) return refuse(h, "gvom_chassis_set", "front_axle must lie in front of rear_axle");
    if (!(c->track > 0.0)) return refuse(h, "gvom_chassis_set", "track must be greater than 0");
    if (c->max_pitch != c->max_pitch || c->max_roll != c->max_roll || c->min_clearance != c->min_clearance) return refuse(h, "gvom_chassis_set", "a limit is not a number");
    for (int k = 0; k < 2 * n_headings; ++k)
        if (!(fabs(cos_sin[k]) <= 1.0)) return refuse(h, "gvom_chassis_set", "a cos_sin entry is not finite or exceeds 1 in magnitude");
    const size_t wb = (size_t)n_headings * 64, cs_at = align256(wb), cb = (size_t)n_headings * 16;
    std::vector<double> tab((cs_at + cb) / 8, 0.0);
    const double half = c->track / 2, ab[4][2] = {{c->front_axle, half}, {c->front_axle, -half}, {c->rear_axle, half}, {c->rear_axle, -half}};
    for (int k = 0; k < n_headings; ++k) {
        const double co = cos_sin[2 * k], si = cos_sin[2 * k + 1];
        for (int i = 0; i < 4; ++i) {
            const double wx = ab[i][0] * co - ab[i][1] * si, wy = ab[i][0] * si + ab[i][1] * co;
            if (!(isfinite(wx) && isfinite(wy))) return refuse(h, "gvom_chassis_set", "a wheel offset is not finite");
            tab[(size_t)(k * 4 + i) * 2] = wx; tab[(size_t)(k * 4 + i) * 2 + 1] = wy;
        }
        tab[cs_at / 8 + 2 * k] = co; tab[cs_at / 8 + 2 * k + 1] = si;
    }
    HIPCHK(h, hipSetDevice(h->device));
    h->chassis.H = 0;                                                       // (no chassis while this one is on its way)
    if (h->chassis.tab.bytes < cs_at + cb) HIPCHK(h, hipStreamSynchronize(h->stream));   // the kernels that read the table it outgrows
    const int rc = ensure(h, h->chassis.tab, cs_at + cb);
    if (rc) return rc;
    // on the handle's stream: behind whatever still reads the previous table
    HIPCHK(h, hipMemcpyAsync(h->chassis.tab.p, tab.data(), cs_at + cb, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->chassis.cs_at = cs_at; h->chassis.H = n_headings; h->chassis.c = *c;
    ++h->chassis.gen;                                                       // (gvom_attitude_volume rebuilds its table)
    return GVOM_OK;
}

VIS int gvom_score_attitude(gvom_t *h, int64_t map_set_id, const double *ground, const float *poses, int64_t K, int64_t T, int on_device,
                            int flags, const int64_t origin_cells[2], int64_t *product_id)
{
    if (!h || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *product_id = -1;
    const char *const fn = "gvom_score_attitude";
    int rc;
    if ((rc = check_standing(h, fn, false))) return rc;
    if (!poses || !origin_cells) return refuse(h, fn, "poses and origin_cells must not be NULL");
    if (flags & ~GVOM_ATTITUDE_INFERRED_GROUND) return refuse(h, fn, "unknown flag bits");
    if ((rc = check_one_source(h, fn, map_set_id >= 0, ground, !ground, "a map set id", "a ground map", "a ground map"))) return rc;
    if ((rc = check_rollout_shape(h, fn, K, T, origin_cells)) || (rc = check_side(h, fn))) return rc;
    const int xy = h->prm.xy_size;
    const size_t n2 = (size_t)xy * xy;
    Ground g;
    if (map_set_id >= 0 && (rc = map_set_of(h, map_set_id, &g.m))) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *set = nullptr;
    const size_t bytes = set_bytes(GVOM_PRODUCT_ATTITUDE, 0, 0, K, T);
    if ((rc = product_acquire(h, GVOM_PRODUCT_ATTITUDE, bytes, bytes, fn, &h->attitude, &set))) return rc;
    set->cap = K; set->cols = T;
    if ((rc = ground_reserve(h, g, h->attitude, ground))) return rc;
    const float *pdev = poses;
    HIPCHK(h, join_second_stream(h));
    if (!on_device) {                                                       // host poses (and ground): staged, and up before the call returns
        const HostPart parts[2] = {{ground, n2 * 8}, {poses, (size_t)K * T * 12}};
        const void *dev[2];
        if ((rc = stage_host(h, h->attitude, parts, 2, true, dev))) return rc;
        if (dev[0]) g.dev = (const double *)dev[0];
        pdev = (const float *)dev[1];
    }
    if ((rc = set_wait_releases(h, set)) || (rc = ground_write(h, g, flags))) return rc;
    AttitudeParams P;
    memset(&P, 0, sizeof P);
    rollout_frame(h, K, T, origin_cells, P.R);
    chassis_lengths(h, P.wheelbase, P.track, &P.axle_mid);
    chassis_limits(h->chassis.c, P);
    HIPCHK(h, gvom_launch_attitude(h->stream, P, pdev, (const int32_t *)h->footprint.tab.p, (const uint32_t *)((char *)h->footprint.tab.p + h->footprint.offs_at),
                                   (const double *)h->chassis.tab.p, (const double *)((char *)h->chassis.tab.p + h->chassis.cs_at), g.dev,
                                   part_ptr<int32_t>(set, 0), part_ptr<float>(set, 1), part_ptr<uint8_t>(set, 2)));
    return product_publish(h, set, product_id);
}

// ---- body clearance scoring (gvom_body_set, gvom_score_body) ----------------------------------------------------------------------
// K trajectories of T poses each, scored by k_body (gvom_body.hip) against one float64 ground map and one voxel distance field with the
// chassis and the sphere table of the handle: a product of kind GVOM_PRODUCT_BODY sized by K and T.  The ground of a map set is
// k_attitude_ground's, in a grow-only buffer of the handle.  The kernels run on the handle's stream -- behind the passes that wrote the
// field and the combine that wrote the set, and in front of whatever recycles either later.  Enqueues and returns.
VIS int gvom_body_set(gvom_t *h, const float *spheres, int32_t S)
{
    if (!h) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    const char *const fn = "gvom_body_set";
    if (!spheres) return refuse(h, fn, "spheres must not be NULL");
    if (S < 1 || S > GVOM_BODY_MAX_SPHERES) return refuse(h, fn, "between 1 and 256 spheres");
    for (int k = 0; k < 4 * S; ++k)
        if (!std::isfinite(spheres[k])) return refuse(h, fn, "an entry is not finite");
    for (int k = 0; k < S; ++k)
        if (spheres[4 * k + 3] < 0.0f) return refuse(h, fn, "a radius is negative");
    HIPCHK(h, hipSetDevice(h->device));
    h->body.S = 0;                                                          // (no body while this one is on its way)
    const int rc = stage_buf(h, h->body, h->body.tab, (size_t)GVOM_BODY_MAX_SPHERES * 16);        // (allocated once: it holds every S)
    if (rc) return rc;
    // on the handle's stream: behind whatever still reads the previous table
    HIPCHK(h, hipMemcpyAsync(h->body.tab.p, spheres, (size_t)S * 16, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->body.S = S;
    return GVOM_OK;
}

VIS int gvom_score_body(gvom_t *h, int64_t field_product_id, const float *field, const int64_t field_origin[3], int64_t map_set_id,
                        const double *ground, const float *poses, int64_t K, int64_t T, int on_device, int flags, const int64_t origin_cells[2],
                        float min_margin, int64_t *product_id)
{
    if (!h || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *product_id = -1;
    const char *const fn = "gvom_score_body";
    int rc;
    if ((rc = check_standing(h, fn, false))) return rc;
    if (h->body.S < 1) return refuse(h, fn, "no body is set (gvom_body_set)");
    if (!poses || !origin_cells) return refuse(h, fn, "poses and origin_cells must not be NULL");
    if (flags & ~GVOM_ATTITUDE_INFERRED_GROUND) return refuse(h, fn, "unknown flag bits");
    if (!std::isfinite(min_margin)) return refuse(h, fn, "min_margin must be finite");
    if ((rc = check_one_source(h, fn, map_set_id >= 0, ground, !ground, "a map set id", "a ground map", "a ground map"))) return rc;
    if ((rc = check_one_source(h, fn, field_product_id >= 0, field || field_origin, !field, "a distance field id", "a field pointer", "a field pointer"))) return rc;
    if (field_product_id < 0 && !field_origin) return refuse(h, fn, "a field pointer needs field_origin");
    if ((rc = check_rollout_shape(h, fn, K, T, origin_cells)) || (rc = check_side(h, fn))) return rc;
    const int xy = h->prm.xy_size;
    const size_t n2 = (size_t)xy * xy;
    Ground g;
    Field F;
    if ((map_set_id >= 0 && (rc = map_set_of(h, map_set_id, &g.m))) || (rc = field_of(h, fn, field_product_id, field_origin, F))) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *set = nullptr;
    const size_t bytes = set_bytes(GVOM_PRODUCT_BODY, 0, 0, K, T);
    if ((rc = product_acquire(h, GVOM_PRODUCT_BODY, bytes, bytes, fn, &h->body, &set))) return rc;
    set->cap = K; set->cols = T;
    if ((rc = ground_reserve(h, g, h->body, ground))) return rc;
    const float *pdev = poses;
    const float *fdev = F.f ? part_ptr<const float>(F.f, 0) : field;
    HIPCHK(h, join_second_stream(h));
    if (!on_device) {                                                       // host poses (field and ground): staged, and up before the call returns
        const HostPart parts[3] = {{field, n2 * (size_t)F.zs * 4}, {ground, n2 * 8}, {poses, (size_t)K * T * 12}};
        const void *dev[3];
        if ((rc = stage_host(h, h->body, parts, 3, true, dev))) return rc;
        if (dev[0]) fdev = (const float *)dev[0];
        if (dev[1]) g.dev = (const double *)dev[1];
        pdev = (const float *)dev[2];
    }
    if ((rc = set_wait_releases(h, set)) || (rc = ground_write(h, g, flags))) return rc;
    BodyParams P;
    memset(&P, 0, sizeof P);
    rollout_frame(h, K, T, origin_cells, P.R);
    body_params(h, F, min_margin, P);
    HIPCHK(h, gvom_launch_body(h->stream, P, pdev, (const double *)h->chassis.tab.p, (const double *)((char *)h->chassis.tab.p + h->chassis.cs_at), g.dev,
                               (const float *)h->body.tab.p, fdev, part_ptr<int32_t>(set, 0), part_ptr<float>(set, 1), part_ptr<uint8_t>(set, 2)));
    return product_publish(h, set, product_id);
}

// ---- scan alignment scoring (gvom_score_alignments) ------------------------------------------------------------------------------
// n returns under K candidate transforms against the CURRENT fused map (gvom_align.hip): k_align_field rebuilds the class grid in a
// grow-only buffer of the handle, k_align_score counts, k_align_best weighs -- on the handle's stream behind whatever produced the
// map, read-only; the result is a product of kind GVOM_PRODUCT_ALIGNMENT sized by K.  Enqueues and returns; later scans and combines
// run behind the kernels on the same stream and never touch the product.
VIS int gvom_score_alignments(gvom_t *h, const float *cloud, int64_t n, const double *transforms, int64_t K, int on_device, int dilate,
                              const int32_t weights[5], int64_t *product_id)
{
    if (!h || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *product_id = -1;
    const char *const fn = "gvom_score_alignments";
    int rc;
    size_t gb;
    if (h->sharded) return refuse(h, fn, "sharded handles are not supported");
    if ((rc = check_align(h, fn, cloud, n, transforms, K, dilate, weights, &gb))) return rc;
    if (!h->has_combined) return GVOM_NO_DATA;
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *set = nullptr;
    const size_t bytes = set_bytes(GVOM_PRODUCT_ALIGNMENT, 0, 0, K);
    if ((rc = product_acquire(h, GVOM_PRODUCT_ALIGNMENT, bytes, bytes, fn, &h->alignment, &set))) return rc;
    set->cap = K;
    if ((rc = stage_buf(h, h->alignment, h->alignment.grid, gb))) return rc;
    const Fused &F = h->fused[h->cur];
    OccParams O;
    occ_params(h, F, O);
    AlignParams P;
    memset(&P, 0, sizeof P);
    metric_frame(h, F, P);
    const float *cdev;
    const double *tdev;
    if ((rc = align_fill(h, h->alignment, cloud, n, transforms, K, on_device, dilate, weights, P, &cdev, &tdev))) return rc;
    if ((rc = set_wait_releases(h, set))) return rc;
    HIPCHK(h, gvom_launch_align(h->stream, O, P, F.state, F.tags, cdev, tdev, (uint32_t *)h->alignment.grid.p, part_ptr<int32_t>(set, 0),
                                part_ptr<int32_t>(set, 1)));
    return product_publish(h, set, product_id);
}

// ---- frontier extraction (gvom_frontiers) -----------------------------------------------------------------------------------------
// The frontier cells of a cost map, clustered, ranked and summarised (gvom_frontier.hip), as a product of kind GVOM_PRODUCT_FRONTIERS
// sized by the map and max_clusters.  The kernels run on the handle's stream behind whatever wrote the field and the map set they
// read, and whatever recycles those later runs behind them.  Like gvom_cost_to_go this call WAITS: rounds of k_frontier_relax are
// enqueued a batch at a time, the batch's per-round counters come back through pinned memory, and the first round that flagged no
// tile ends the labelling (the rounds enqueued behind it found nothing to do): frontier_solve above, everything behind the marking.
VIS int gvom_frontiers(gvom_t *h, int64_t costfield_id, int64_t map_set_id, const uint16_t *cell_cost, const int32_t *cost_to_go,
                       const int32_t *visibility, int on_device, int32_t min_cells, int32_t max_clusters, int64_t *product_id, int64_t info[4])
{
    if (!h || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *product_id = -1;
    for (int k = 0; info && k < 4; ++k) info[k] = 0;
    const char *const fn = "gvom_frontiers";
    int rc;
    if (h->sharded) return refuse(h, fn, "sharded handles are not supported");
    const bool ids = costfield_id >= 0 && map_set_id >= 0;
    if ((costfield_id >= 0) != (map_set_id >= 0)) return refuse(h, "gvom_frontiers", "the ids route needs a cost field id AND a map set id");
    if (ids && (cell_cost || cost_to_go || visibility)) return refuse(h, "gvom_frontiers", "give the two ids or map pointers, not both");
    if (!ids && (!cell_cost || !visibility)) return refuse(h, "gvom_frontiers", "give the two ids, or a cell-cost map and a visibility map");
    if ((rc = check_clusters(h, fn, min_cells, max_clusters)) || (rc = check_side(h, fn))) return rc;
    const int xy = h->prm.xy_size;
    const size_t n2 = (size_t)xy * xy;
    const uint16_t *c16 = cell_cost;
    const int32_t *D = cost_to_go, *vis = visibility;
    if (ids) {
        DevSet *f = nullptr, *m = nullptr;
        if ((rc = cost_field_of(h, fn, costfield_id, &f)) || (rc = map_set_of(h, map_set_id, &m))) return rc;
        c16 = part_ptr<const uint16_t>(f, 2); D = part_ptr<const int32_t>(f, 0); vis = part_ptr<const int32_t>(m, 2);
    }
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *set = nullptr;
    const size_t bytes = set_bytes(GVOM_PRODUCT_FRONTIERS, xy, 0, max_clusters);
    if ((rc = product_acquire(h, GVOM_PRODUCT_FRONTIERS, bytes, bytes, fn, &h->frontiers, &set))) return rc;
    set->cap = max_clusters;
    FrWork W;
    if ((rc = frontier_work(h, h->frontiers, xy, &W))) return rc;
    HIPCHK(h, join_second_stream(h));
    if (!ids && !on_device) {                                               // host maps: staged
        const HostPart parts[3] = {{cell_cost, n2 * 2}, {visibility, n2 * 4}, {cost_to_go, n2 * 4}};
        const void *dev[3];
        if ((rc = stage_host(h, h->frontiers, parts, 3, false, dev))) return rc;
        c16 = (const uint16_t *)dev[0]; vis = (const int32_t *)dev[1]; D = (const int32_t *)dev[2];
    }
    HIPCHK(h, hipMemsetAsync(W.cnt, 0, W.clear_bytes, h->stream));          // the counters and both halves of the flags
    if ((rc = set_wait_releases(h, set))) return rc;
    HIPCHK(h, gvom_launch_frontier_mark(h->stream, xy, c16, vis, D, W.L, W.count, W.fl, W.cnt + FR_CNT_CELLS));
    return frontier_solve(h, fn, h->frontiers.solve, xy, D, W, min_cells, max_clusters, set, product_id, info);
}

// ---- viewpoint scoring (gvom_score_viewpoints) -------------------------------------------------------------------------------------
// The selected beams of the handle's sensor model cast from K poses through the CURRENT fused map (gvom_viewpoint.hip), read-only, on
// the handle's stream behind whatever produced that map; the result is a product of kind GVOM_PRODUCT_VIEWPOINTS sized by K.  The
// viewpoints are walked a batch at a time -- as many as have their bitmaps in "viewpoint_bitmap_mb" megabytes --, the bitmaps cleared
// on the stream in front of every batch; the kernel boundary orders the batches.  Enqueues and returns.  gvom_sensor_model_set drains
// the stream under this mutex before it replaces the model: no kernel of an earlier call reads a model that is being overwritten.
VIS int gvom_score_viewpoints(gvom_t *h, const double *poses, int64_t K, int on_device, double max_range, int32_t stride_h, int32_t stride_w,
                              int flags, double origin_voxels[3], int64_t *product_id)
{
    if (!h || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *product_id = -1;
    const char *const fn = "gvom_score_viewpoints";
    int rc;
    ViewBeams B;
    if (h->sharded) return refuse(h, fn, "sharded handles are not supported");
    const int xy = h->prm.xy_size, zs = h->prm.z_size;
    if ((rc = check_views(h, fn, poses, K, max_range, stride_h, stride_w, flags, (int64_t)xy + zs, "xy_size + z_size", &B))) return rc;
    const int64_t V = (int64_t)xy * xy * zs;
    if (V >= ((int64_t)1 << 31)) return refuse(h, fn, "the window has 2^31 voxels or more", GVOM_ERR_CAPACITY);
    if (!h->has_combined) return GVOM_NO_DATA;
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *set = nullptr;
    const size_t bytes = set_bytes(GVOM_PRODUCT_VIEWPOINTS, 0, 0, K);
    if ((rc = product_acquire(h, GVOM_PRODUCT_VIEWPOINTS, bytes, bytes, fn, &h->viewpoints, &set))) return rc;
    set->cap = K;
    size_t bm_words;
    const int64_t batch = views_batch(h, V, K, &bm_words);
    if ((rc = stage_buf(h, h->viewpoints, h->viewpoints.bitmaps, (size_t)batch * bm_words * 4))) return rc;
    const Fused &F = h->fused[h->cur];
    ScanParams P;
    RayQuery R;
    memset(&R, 0, sizeof R);
    raycast_params(h, F, P, R);
    ViewQuery Q;
    views_fill(h, R, B, K, max_range, stride_h, stride_w, flags, bm_words, Q);
    Q.poses = poses;
    HIPCHK(h, join_second_stream(h));
    if (!on_device) {                                                       // host poses: staged, and up before the call returns
        const HostPart part = {poses, (size_t)K * 96};
        const void *dev;
        if ((rc = stage_host(h, h->viewpoints, &part, 1, true, &dev))) return rc;
        Q.poses = (const double *)dev;
    }
    if ((rc = set_wait_releases(h, set))) return rc;
    int32_t *rows = part_ptr<int32_t>(set, 0);
    rc = views_run(h, h->viewpoints.bitmaps, Q, batch, rows,
                   [&](int nk) { return gvom_launch_viewpoints(h->stream, P, Q, nk, F.state, F.tags, (uint32_t *)h->viewpoints.bitmaps.p, rows); },
                   [&]() { return gvom_launch_viewpoint_best(h->stream, P, Q, F.state, F.tags, rows, part_ptr<int32_t>(set, 1)); });
    if (rc) return rc;
    h->viewpoints.last_batch = (int)batch;
    if ((rc = product_publish(h, set, product_id))) return rc;
    for (int k = 0; origin_voxels && k < 3; ++k) origin_voxels[k] = (double)F.origin[k];
    return GVOM_OK;
}

// ---- pose fields (gvom_primitives_set, gvom_pose_field) ----------------------------------------------------------------------------
// The navigation function on (x, y, heading) of a cost map -- a cost field's or the caller's -- under the handle's footprint table and
// primitive table, as a product of kind GVOM_PRODUCT_POSEFIELD.  The kernels (gvom_posefield.hip) run on the handle's stream: the pose
// cost volume first, then gvom_cost_to_go's loop -- rounds of k_pose_relax a batch at a time, the batch's counters back through pinned
// memory, the first round that flagged no tile ends the solve.  Like gvom_cost_to_go this call WAITS.
VIS int gvom_primitives_set(gvom_t *h, int32_t n_headings, const int32_t *start, const int16_t *prims)
{
    if (!h) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!start || !prims) return refuse(h, "gvom_primitives_set", "start and prims must not be NULL");
    if (n_headings < 1 || n_headings > GVOM_POSE_MAX_HEADINGS) return refuse(h, "gvom_primitives_set", "between 1 and 64 headings");
    if (start[0] != 0) return refuse(h, "gvom_primitives_set", "start[0] must be 0");
    int R = 0;
    for (int k = 0; k < n_headings; ++k) {
        const int64_t m = (int64_t)start[k + 1] - start[k];
        if (m < 0 || m > GVOM_POSE_MAX_PRIMS) return refuse(h, "gvom_primitives_set", "every heading has at most 64 primitives");
        for (int p = start[k]; p < start[k + 1]; ++p) {
            const int dx = prims[4 * p], dy = prims[4 * p + 1], hto = prims[4 * p + 2], w = prims[4 * p + 3];
            const bool ok = abs(dx) <= GVOM_POSE_MAX_REACH && abs(dy) <= GVOM_POSE_MAX_REACH && hto >= 0 && hto < n_headings && w >= 1 && w <= 255 &&
                            !(dx == 0 && dy == 0 && hto == k);
            if (!ok) return refuse(h, "gvom_primitives_set", "a primitive outside the limits (|dx|, |dy| <= 4, 0 <= h_to < H, 1 <= w <= 255, not a self loop)");
            R = std::max(R, std::max(abs(dx), abs(dy)));
        }
    }
    HIPCHK(h, hipSetDevice(h->device));
    const size_t sb = (size_t)(n_headings + 1) * 4, prims_at = align256(sb), pb = (size_t)start[n_headings] * 8;
    h->pose_field.H = 0;                                                    // (no table while this one is on its way)
    const int rc = stage_buf(h, h->pose_field, h->pose_field.tab, prims_at + (size_t)GVOM_POSE_MAX_HEADINGS * GVOM_POSE_MAX_PRIMS * 8);   // (the largest table: never grows again)
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->pose_field.tab.p, start, sb, hipMemcpyHostToDevice, h->stream));
    if (pb) HIPCHK(h, hipMemcpyAsync((char *)h->pose_field.tab.p + prims_at, prims, pb, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->pose_field.prims_at = prims_at; h->pose_field.H = n_headings; h->pose_field.R = R;
    return GVOM_OK;
}

// the two volumes k_cspace_attitude takes into the pose cost volume behind k_cspace, in this order (parts 0 and 1 of either are the
// elementwise rule's status and weight byte): what a call says of one, and what the checks and their texts need to know of it
struct PoseVolume { bool present; int64_t id; uint32_t mask; int32_t weight; };
static const struct { int kind; uint32_t mask_limit; const char *mask_name, *mask_top, *weight_name, *noun; } POSE_VOLUMES[2] = {
    {GVOM_PRODUCT_ATTITUDE_VOLUME, 0x7fu, "block_mask", "0x7f", "tilt_weight", "attitude"},
    {GVOM_PRODUCT_BODY_VOLUME, 0x3fu, "body_block_mask", "0x3f", "squeeze_weight", "body"}};

// the one host path of gvom_pose_field, gvom_pose_field_attitude and gvom_pose_field_volumes (fn says which)
static int pose_field_call(gvom_t *h, const char *fn, int64_t costfield_id, const int32_t *cost, int on_device, const PoseVolume (&volumes)[2],
                           const int32_t *goals, int64_t n_goals, int32_t max_cost, int32_t max_rounds, int64_t *product_id, int64_t info[4])
{
    if (!h || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *product_id = -1;
    for (int k = 0; info && k < 4; ++k) info[k] = 0;
    int rc;
    if (h->sharded) return refuse(h, fn, "sharded handles are not supported");
    if (h->footprint.H < 1) return refuse(h, fn, "no footprint table is set (gvom_footprint_set)");
    if (h->pose_field.H < 1) return refuse(h, fn, "no primitive table is set (gvom_primitives_set)");
    if (h->footprint.H > GVOM_POSE_MAX_HEADINGS) return refuse(h, fn, "footprint tables of more than 64 headings are not supported", GVOM_ERR_CAPACITY);
    if (h->pose_field.H != h->footprint.H) return refuse(h, fn, "the primitives were set for another number of headings than the footprint table has");
    if ((rc = check_one_source(h, fn, costfield_id >= 0, cost, !cost, "a cost field id", "a cost map", "a cost map"))) return rc;
    if ((rc = check_goals(h, fn, goals, n_goals, max_cost, max_rounds)) || (rc = check_side(h, fn))) return rc;
    const int xy = h->prm.xy_size, H = h->pose_field.H, R = h->pose_field.R;
    const size_t n2 = (size_t)xy * xy;
    if ((rc = check_states(h, fn, H, xy))) return rc;
    for (int64_t k = 0; k < n_goals; ++k) {
        if (goals[3 * k] < 0 || goals[3 * k] >= xy || goals[3 * k + 1] < 0 || goals[3 * k + 1] >= xy) return refuse(h, fn, "a goal lies outside the window");
        if (goals[3 * k + 2] >= H) return refuse(h, fn, "a goal's heading is not one of the table's");
    }
    DevSet *f = nullptr;
    if (costfield_id >= 0) {
        if ((rc = cost_field_of(h, fn, costfield_id, &f))) return rc;
    } else if (!on_device && (rc = check_host_cost(h, fn, cost, n2))) return rc;
    DevSet *vol[2] = {nullptr, nullptr};
    for (int i = 0; i < 2; ++i) {
        const PoseVolume &v = volumes[i];
        const auto &is = POSE_VOLUMES[i];
        if (!v.present) continue;
        if (v.mask > is.mask_limit) return refuse(h, fn, std::string(is.mask_name) + " outside 0 .. " + is.mask_top);
        if (v.weight < 0 || v.weight > 255) return refuse(h, fn, std::string(is.weight_name) + " outside 0 .. 255");
        if ((rc = product_of_kind(h, fn, v.id, is.kind, (std::string("unknown or stale ") + is.noun + " volume id").c_str(), &vol[i]))) return rc;
        if (vol[i]->cap != H || vol[i]->xy != xy) return refuse(h, fn, std::string("the ") + is.noun + " volume was made for another number of headings or another window side");
    }
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *set = nullptr;
    const size_t bytes = set_bytes(GVOM_PRODUCT_POSEFIELD, xy, 0, H);
    if ((rc = product_acquire(h, GVOM_PRODUCT_POSEFIELD, bytes, bytes, fn, &h->pose_field, &set))) return rc;
    set->cap = H;
    const int nt = gvom_pose_tiles(xy);
    const GoalWork lay = goal_work(nt * nt, 12, n2 * 2);                     // (the tail: the uint16 cost map converted from cost32)
    if ((rc = solve_work_reserve(h, h->pose_field, lay.end))) return rc;
    const GoalWorkPtrs G = goal_work_ptrs(h->pose_field.solve, lay);
    uint16_t *c16w = (uint16_t *)G.tail;
    HIPCHK(h, join_second_stream(h));
    const void *cost32 = f ? nullptr : cost;
    if (!f && !on_device) {                                                 // a host cost map: staged
        const HostPart part = {cost, n2 * 4};
        if ((rc = stage_host(h, h->pose_field, &part, 1, false, &cost32))) return rc;
    }
    const uint16_t *c16 = f ? part_ptr<const uint16_t>(f, 2) : c16w;
    if ((rc = goal_work_start(h, G, goals, (size_t)n_goals * 12)) || (rc = set_wait_releases(h, set))) return rc;
    int32_t *D = part_ptr<int32_t>(set, 0);
    uint16_t *C = part_ptr<uint16_t>(set, 2);
    const int32_t *pstart = (const int32_t *)h->pose_field.tab.p;
    const int16_t *prims = (const int16_t *)((char *)h->pose_field.tab.p + h->pose_field.prims_at);
    HIPCHK(h, gvom_launch_pose_seed(h->stream, 0, xy, H, R, (const int32_t *)cost32, c16w, C, D, G.fl, G.goals, (int)n_goals, G.cnt + CTG_CNT_SEEDED));
    HIPCHK(h, gvom_launch_cspace(h->stream, xy, H, c16, (const int32_t *)h->footprint.tab.p, (const uint32_t *)((char *)h->footprint.tab.p + h->footprint.offs_at), C));
    for (int i = 0; i < 2; ++i)
        if (vol[i]) HIPCHK(h, gvom_launch_cspace_attitude(h->stream, xy, H, part_ptr<const uint8_t>(vol[i], 0), part_ptr<const uint8_t>(vol[i], 1),
                                                          volumes[i].mask, (uint32_t)volumes[i].weight, C));
    HIPCHK(h, gvom_launch_pose_seed(h->stream, 1, xy, H, R, (const int32_t *)cost32, c16w, C, D, G.fl, G.goals, (int)n_goals, G.cnt + CTG_CNT_SEEDED));
    const int32_t cap = max_cost == 0 ? GVOM_CTG_MAX_COST : max_cost;
    const int inner = h->pose_field.solve.tune_inner > 0 ? h->pose_field.solve.tune_inner : 64;
    const int batch = h->pose_field.solve.tune_batch > 0 ? h->pose_field.solve.tune_batch : 8;
    // a state's final value is in memory at the latest one round after the round in which its successor's was, so
    // the solve ends after at most (primitives on a cheapest drive + 1) rounds of tiles that reach their fixed point; the limit below
    // is beyond that for 2^28 states and only keeps the loop finite
    const int64_t limit = max_rounds > 0 ? (int64_t)max_rounds : (int64_t)1 << 29;
    SolveRounds S;
    rc = solve_rounds(h, G.cnt, G.fl, h->pose_field.solve.pin, nt * nt, batch, limit, [&](int64_t, uint32_t *fin, uint32_t *fout, uint32_t *any, uint32_t *ran) {
        return gvom_launch_pose_relax(h->stream, xy, H, R, C, D, pstart, prims, fin, fout, any, ran, cap, inner);
    }, &S);
    if (rc) return rc;
    HIPCHK(h, gvom_launch_pose_actions(h->stream, xy, H, C, D, pstart, prims, part_ptr<uint8_t>(set, 1), G.cnt + CTG_CNT_REACHED));
    return goal_solve_finish(h, fn, h->pose_field.solve, set, product_id, S, max_rounds, info);
}

VIS int gvom_pose_field(gvom_t *h, int64_t costfield_id, const int32_t *cost, int on_device, const int32_t *goals, int64_t n_goals,
                        int32_t max_cost, int32_t max_rounds, int64_t *product_id, int64_t info[4])
{
    const PoseVolume none[2] = {};
    return pose_field_call(h, "gvom_pose_field", costfield_id, cost, on_device, none, goals, n_goals, max_cost, max_rounds, product_id, info);
}

VIS int gvom_pose_field_attitude(gvom_t *h, int64_t costfield_id, const int32_t *cost, int on_device, int64_t volume_id, uint32_t block_mask,
                                 int32_t tilt_weight, const int32_t *goals, int64_t n_goals, int32_t max_cost, int32_t max_rounds,
                                 int64_t *product_id, int64_t info[4])
{
    const PoseVolume v[2] = {{true, volume_id, block_mask, tilt_weight}, {}};
    return pose_field_call(h, "gvom_pose_field_attitude", costfield_id, cost, on_device, v, goals, n_goals, max_cost, max_rounds, product_id, info);
}

VIS int gvom_pose_field_volumes(gvom_t *h, int64_t costfield_id, const int32_t *cost, int on_device, int64_t attitude_volume_id,
                                uint32_t attitude_block_mask, int32_t tilt_weight, int64_t body_volume_id, uint32_t body_block_mask,
                                int32_t squeeze_weight, const int32_t *goals, int64_t n_goals, int32_t max_cost, int32_t max_rounds,
                                int64_t *product_id, int64_t info[4])
{
    const char *const fn = "gvom_pose_field_volumes";
    if (!h || !product_id) return GVOM_ERR_INVALID;
    if ((attitude_volume_id < 0 && (attitude_block_mask != 0u || tilt_weight != 0)) || (body_volume_id < 0 && (body_block_mask != 0u || squeeze_weight != 0))) {
        std::lock_guard<std::mutex> lk(h->mu);
        *product_id = -1;
        for (int k = 0; info && k < 4; ++k) info[k] = 0;
        return refuse(h, fn, "a mask or a weight that is not 0 beside a volume id of -1");
    }
    const PoseVolume v[2] = {{attitude_volume_id >= 0, attitude_volume_id, attitude_block_mask, tilt_weight},
                             {body_volume_id >= 0, body_volume_id, body_block_mask, squeeze_weight}};
    return pose_field_call(h, fn, costfield_id, cost, on_device, v, goals, n_goals, max_cost, max_rounds, product_id, info);
}

// the table of "attitude volumes" (attitude_volume.tab: (u - am, v) of every footprint cell and per heading the wheels' cell offsets and the footprint's
// box), shared by gvom_attitude_volume and gvom_body_volume: the first call of either after a gvom_footprint_set / gvom_chassis_set
// rebuilds it.  reserve: room for it, in front of the call's uploads; rebuild: k_volume_attitude_table on the handle's stream, behind
// whatever still reads the previous table
static bool volume_table_stale(const gvom_t *h) { return h->attitude_volume.fp_gen != h->footprint.gen || h->attitude_volume.at_gen != h->chassis.gen; }
static int volume_table_reserve(gvom_t *h, int H)
{
    if (!volume_table_stale(h)) return GVOM_OK;
    const size_t tab_bytes = align256((size_t)h->footprint.total * 16) + (size_t)H * 48;
    if (h->attitude_volume.tab.bytes < tab_bytes) HIPCHK(h, hipStreamSynchronize(h->stream));   // the kernels that read the table it outgrows
    return stage_buf(h, h->attitude_volume, h->attitude_volume.tab, tab_bytes);
}
static int volume_table_rebuild(gvom_t *h, int H)
{
    if (!volume_table_stale(h)) return GVOM_OK;
    const gvom_chassis_t &c = h->chassis.c;
    const size_t wcell_at = align256((size_t)h->footprint.total * 16);
    HIPCHK(h, gvom_launch_attitude_volume_table(h->stream, H, h->footprint.total, h->prm.xy_resolution, 0.5 * (c.front_axle + c.rear_axle),
                                                (const int32_t *)h->footprint.tab.p, (const uint32_t *)((char *)h->footprint.tab.p + h->footprint.offs_at),
                                                (const double *)h->chassis.tab.p, (const double *)((char *)h->chassis.tab.p + h->chassis.cs_at),
                                                (double *)h->attitude_volume.tab.p, (int32_t *)((char *)h->attitude_volume.tab.p + wcell_at)));
    h->attitude_volume.wcell_at = wcell_at; h->attitude_volume.fp_gen = h->footprint.gen; h->attitude_volume.at_gen = h->chassis.gen;
    return GVOM_OK;
}

// ---- attitude volumes (gvom_attitude_volume) ----------------------------------------------------------------------------------------
// The status and the tilt of terrain attitude scoring at every state (cell centre, heading) of the window, by k_volume_attitude
// (gvom_attitude_volume.hip) against one float64 ground map with the footprint table and the chassis of the handle: a product of kind
// GVOM_PRODUCT_ATTITUDE_VOLUME sized by H.  What depends on (heading, footprint cell) only -- and the wheels' cell offsets -- is a
// table of the handle that the first call after a gvom_footprint_set / gvom_chassis_set rebuilds on the stream.  With a map set,
// k_attitude_ground first writes the ground map into a grow-only buffer of the handle.  Enqueues and returns.
VIS int gvom_attitude_volume(gvom_t *h, int64_t map_set_id, const double *ground, int on_device, int flags, int64_t *product_id)
{
    if (!h || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *product_id = -1;
    const char *const fn = "gvom_attitude_volume";
    int rc;
    if ((rc = check_standing(h, fn, true))) return rc;
    if (flags & ~GVOM_ATTITUDE_INFERRED_GROUND) return refuse(h, fn, "unknown flag bits");
    if ((rc = check_one_source(h, fn, map_set_id >= 0, ground, !ground, "a map set id", "a ground map", "a ground map")) || (rc = check_side(h, fn))) return rc;
    const int xy = h->prm.xy_size, H = h->footprint.H;
    const size_t n2 = (size_t)xy * xy;
    if ((rc = check_states(h, fn, H, xy))) return rc;
    Ground g;
    if (map_set_id >= 0 && (rc = map_set_of(h, map_set_id, &g.m))) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *set = nullptr;
    const size_t bytes = set_bytes(GVOM_PRODUCT_ATTITUDE_VOLUME, xy, 0, H);
    if ((rc = product_acquire(h, GVOM_PRODUCT_ATTITUDE_VOLUME, bytes, bytes, fn, &h->attitude_volume, &set))) return rc;
    set->cap = H;
    if ((rc = volume_table_reserve(h, H)) || (rc = ground_reserve(h, g, h->attitude_volume, ground))) return rc;
    HIPCHK(h, join_second_stream(h));
    if (!g.m && !on_device) {                                               // a host ground map: staged, and up before the call returns
        const HostPart part = {ground, n2 * 8};
        const void *dev;
        if ((rc = stage_host(h, h->attitude_volume, &part, 1, true, &dev))) return rc;
        g.dev = (const double *)dev;
    }
    if ((rc = volume_table_rebuild(h, H)) || (rc = set_wait_releases(h, set)) || (rc = ground_write(h, g, flags))) return rc;
    AttitudeVolumeParams P;
    memset(&P, 0, sizeof P);
    P.xy = xy; P.H = H;
    chassis_lengths(h, P.wheelbase, P.track, nullptr);
    chassis_limits(h->chassis.c, P);
    int32_t *counts = part_ptr<int32_t>(set, 2);
    HIPCHK(h, hipMemsetAsync(counts, 0, 32, h->stream));
    HIPCHK(h, gvom_launch_attitude_volume(h->stream, P, (const int32_t *)h->footprint.tab.p, (const uint32_t *)((char *)h->footprint.tab.p + h->footprint.offs_at), (const double *)h->attitude_volume.tab.p,
                                          (const int32_t *)((char *)h->attitude_volume.tab.p + h->attitude_volume.wcell_at), g.dev, part_ptr<uint8_t>(set, 0), part_ptr<uint8_t>(set, 1), counts));
    return product_publish(h, set, product_id);
}

// ---- body volumes (gvom_body_volume) -------------------------------------------------------------------------------------------------
// The status, the squeeze and the clearance of body clearance scoring at every state (cell centre, heading) of the window, by
// k_volume_body (gvom_body_volume.hip) against one float64 ground map and one voxel distance field with the chassis and the sphere table
// of the handle: a product of kind GVOM_PRODUCT_BODY_VOLUME sized by H.  The wheels' cell offsets are the attitude volume's table (above).
// The field and ground routes are gvom_score_body's.  Enqueues and returns.
VIS int gvom_body_volume(gvom_t *h, int64_t field_product_id, const float *field, const int64_t field_origin[3], int64_t map_set_id,
                         const double *ground, int on_device, int flags, const int64_t origin_cells[2], float min_margin, float soft_margin,
                         int64_t *product_id)
{
    if (!h || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *product_id = -1;
    const char *const fn = "gvom_body_volume";
    int rc;
    if ((rc = check_standing(h, fn, true))) return rc;
    if (h->body.S < 1) return refuse(h, fn, "no body is set (gvom_body_set)");
    if (!origin_cells) return refuse(h, fn, "origin_cells must not be NULL");
    if (flags & ~GVOM_ATTITUDE_INFERRED_GROUND) return refuse(h, fn, "unknown flag bits");
    if (!std::isfinite(min_margin)) return refuse(h, fn, "min_margin must be finite");
    if (!std::isfinite(soft_margin)) return refuse(h, fn, "soft_margin must be finite");
    if (soft_margin < min_margin) return refuse(h, fn, "soft_margin must not be less than min_margin");
    if ((rc = check_one_source(h, fn, map_set_id >= 0, ground, !ground, "a map set id", "a ground map", "a ground map"))) return rc;
    if ((rc = check_one_source(h, fn, field_product_id >= 0, field || field_origin, !field, "a distance field id", "a field pointer", "a field pointer"))) return rc;
    if (field_product_id < 0 && !field_origin) return refuse(h, fn, "a field pointer needs field_origin");
    for (int k = 0; k < 2; ++k)
        if (origin_cells[k] < -((int64_t)1 << 40) || origin_cells[k] > ((int64_t)1 << 40)) return refuse(h, fn, "an origin beyond 2^40 cells");
    if ((rc = check_side(h, fn))) return rc;
    const int xy = h->prm.xy_size, H = h->footprint.H;
    const size_t n2 = (size_t)xy * xy;
    if ((rc = check_states(h, fn, H, xy))) return rc;
    Ground g;
    Field F;
    if ((map_set_id >= 0 && (rc = map_set_of(h, map_set_id, &g.m))) || (rc = field_of(h, fn, field_product_id, field_origin, F))) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *set = nullptr;
    const size_t bytes = set_bytes(GVOM_PRODUCT_BODY_VOLUME, xy, 0, H);
    if ((rc = product_acquire(h, GVOM_PRODUCT_BODY_VOLUME, bytes, bytes, fn, &h->body_volume, &set))) return rc;
    set->cap = H;
    if ((rc = volume_table_reserve(h, H)) || (rc = ground_reserve(h, g, h->body_volume, ground))) return rc;
    const float *fdev = F.f ? part_ptr<const float>(F.f, 0) : field;
    HIPCHK(h, join_second_stream(h));
    if (!on_device && (field || ground)) {                                  // a host field and / or ground map: staged, and up before the call returns
        const HostPart parts[2] = {{field, n2 * (size_t)F.zs * 4}, {ground, n2 * 8}};
        const void *dev[2];
        if ((rc = stage_host(h, h->body_volume, parts, 2, true, dev))) return rc;
        if (dev[0]) fdev = (const float *)dev[0];
        if (dev[1]) g.dev = (const double *)dev[1];
    }
    if ((rc = volume_table_rebuild(h, H)) || (rc = set_wait_releases(h, set)) || (rc = ground_write(h, g, flags))) return rc;
    BodyParams P;
    memset(&P, 0, sizeof P);
    P.R.xy = xy; P.R.H = H; P.R.res = h->prm.xy_resolution; P.R.ox = origin_cells[0]; P.R.oy = origin_cells[1];
    body_params(h, F, min_margin, P);
    int32_t *counts = part_ptr<int32_t>(set, 3);
    HIPCHK(h, hipMemsetAsync(counts, 0, 32, h->stream));
    HIPCHK(h, gvom_launch_body_volume(h->stream, P, soft_margin, (const int32_t *)((char *)h->attitude_volume.tab.p + h->attitude_volume.wcell_at),
                                      (const double *)((char *)h->chassis.tab.p + h->chassis.cs_at), g.dev, (const float *)h->body.tab.p, fdev,
                                      part_ptr<uint8_t>(set, 0), part_ptr<uint8_t>(set, 1), part_ptr<float>(set, 2), counts));
    return product_publish(h, set, product_id);
}
}  // extern "C"
