// gvom_voxel_atlas_calls.hip -- the voxel atlas's entry points (include/gvom_hip.h "voxel atlas"): gvom_voxel_atlas_configure, _integrate,
// _clear, _counts, _box, _changes, _raycast, _score_viewpoints and _score_alignments.  The kernels are gvom_voxel_atlas.hip's (gvom_voxel_changes.hip's for _changes, which waits like gvom_frontiers); everything runs on the handle's stream --
// an integrate behind whatever produced the current fused map, a query behind the integrates before it -- and only gvom_voxel_atlas_counts
// waits for it (the viewpoint call waits where it has to read poses or the sensor model back: the boxes of its bitmaps are proved here, on
// the host).  The products go through the pool path of every product call (product_acquire / product_publish, gvom_sets.hip), host inputs
// through stage_host, the checks through refuse (gvom_host.h).  The three walk queries share their checks, the filling of their queries,
// the staging and the viewpoint batch loop with gvom_raycast, gvom_score_viewpoints and gvom_score_alignments ("THE WALK QUERIES",
// gvom_host.h); theirs alone are the frame (walk_frame), the boxes of the poses, the box origin and the launches.
#include "gvom_host.h"

namespace {
const int64_t VA_FAR = (int64_t)1 << 30;                   // E and W stay below this in magnitude; a box this far from the extent lies outside it

int need_atlas(gvom_handle *h, const char *fn)
{
    if (h->sharded) return refuse(h, fn, "sharded handles are not supported");
    return h->voxel_atlas.A ? GVOM_OK : refuse(h, fn, "no voxel atlas is configured (gvom_voxel_atlas_configure)");
}

int lg2(int v) { int k = 0; while ((1 << k) < v) ++k; return k; }

VAtlas atlas_of(const gvom_handle *h)
{
    VAtlas V;
    V.pairs = h->voxel_atlas.mem; V.A = h->voxel_atlas.A; V.Z = h->voxel_atlas.Z;
    V.lgZ = lg2(h->voxel_atlas.Z); V.lgP = lg2(h->voxel_atlas.A / 64);
    return V;
}

int side(const gvom_handle *h, int k) { return k < 2 ? h->voxel_atlas.A : h->voxel_atlas.Z; }
int window_side(const gvom_handle *h, int k) { return k < 2 ? h->prm.xy_size : h->prm.z_size; }
bool near_origin(const int64_t o[3]) { return o[0] > -VA_FAR && o[0] < VA_FAR && o[1] > -VA_FAR && o[1] < VA_FAR && o[2] > -VA_FAR && o[2] < VA_FAR; }

// box origin - extent origin on axis k, clamped to +-2^30 (|E| < 2^30: the comparisons cannot overflow)
int rel_of(const gvom_handle *h, const int64_t B[3], int k)
{
    const int64_t e = h->voxel_atlas.E[k];
    if (B[k] >= e + VA_FAR) return (int)VA_FAR;
    if (B[k] <= e - VA_FAR) return -(int)VA_FAR;
    return (int)(B[k] - e);
}

// the part [lo, lo + n) of a box side of `len` voxels at relative origin r that lies inside the extent's side of `size`
void clip(int r, int len, int size, int *lo, int *n)
{
    const int64_t a = std::max<int64_t>(0, -(int64_t)r), b = std::min<int64_t>(len, (int64_t)size - r);
    *lo = b > a ? (int)a : 0;
    *n = b > a ? (int)(b - a) : 0;
}

// the window-sized box at world voxel B against the extent: per axis its relative origin and the part [lo, lo + n) inside the extent.
// Returns how many of its voxels lie inside
int64_t box_clip(const gvom_handle *h, const int64_t B[3], int r[3], int lo[3], int n[3])
{
    for (int k = 0; k < 3; ++k) {
        r[k] = rel_of(h, B, k);
        clip(r[k], window_side(h, k), side(h, k), &lo[k], &n[k]);
    }
    return (int64_t)n[0] * n[1] * n[2];
}

// the window-sized box at world voxel B as the box kernels take it: relative to the extent, with its storage phase.  Returns how many of
// its voxels lie inside the extent
int64_t box_frame(const gvom_handle *h, const int64_t B[3], VAtlasBox &X)
{
    memset(&X, 0, sizeof X);
    X.n = h->prm.xy_size; X.zs = h->prm.z_size;
    int r[3], lo[3], n[3];
    const int64_t inside = box_clip(h, B, r, lo, n);
    X.rx = r[0]; X.ry = r[1]; X.rz = r[2];
    X.px = (int)(B[0] & (h->voxel_atlas.A - 1)); X.py = (int)(B[1] & (h->voxel_atlas.A - 1)); X.pz = (int)(B[2] & (h->voxel_atlas.Z - 1));
    return inside;
}

// THE BOX ORIGIN of the calls that take one: `origin`, or (NULL) the last integrated window; GVOM_NO_DATA before the first combine, and
// for NULL before the first integrate
int box_origin(const gvom_handle *h, const int64_t origin[3], int64_t B[3])
{
    if (!h->has_combined || (!origin && h->voxel_atlas.seq == 0)) return GVOM_NO_DATA;
    for (int k = 0; k < 3; ++k) B[k] = origin ? origin[k] : h->voxel_atlas.last[k];
    return GVOM_OK;
}

// the end of a call whose product lies at world voxel `at`: recorded in the set, handed to the caller, published.  The box calls hand
// it out in front of the publication, the two extent calls (`after`) only behind a publication that succeeded: as each always did
int publish_at(gvom_handle *h, DevSet *set, const int64_t at[3], int64_t out[3], int64_t *product_id, bool after = false)
{
    for (int k = 0; k < 3; ++k) set->origin[k] = at[k];
    for (int k = 0; !after && out && k < 3; ++k) out[k] = at[k];
    if (const int rc = product_publish(h, set, product_id)) return rc;
    for (int k = 0; after && out && k < 3; ++k) out[k] = at[k];
    return GVOM_OK;
}

// the CURRENT fused map -- the map of the most recently begun combine -- as gvom_voxel_atlas_integrate and gvom_voxel_atlas_changes take
// it: GVOM_NO_DATA before the first combine, refused where its window lies at or beyond 2^30 voxels
int current_map(gvom_handle *h, const char *fn, const Fused **F)
{
    if (!h->has_combined) return GVOM_NO_DATA;
    *F = &h->fused[h->cur];
    return near_origin((*F)->origin) ? GVOM_OK : refuse(h, fn, "the window's origin lies at or beyond 2^30 voxels");
}

// follow mode: the extent goes to `to`; the voxels that entered it become NEVER -- the slab of columns over every row and level, the slab
// of rows over the remaining columns, the slab of levels over the remaining rows and columns: every cleared voxel is counted once.  A move
// of a whole side or more on an axis is the first slab alone, A wide
int move_extent(gvom_handle *h, const int64_t to[3])
{
    const VAtlas V = atlas_of(h);
    const int A = V.A, Z = V.Z;
    int w[3], s[3];                                                          // per axis: how many storage coordinates entered, from where on
    bool all = false;
    for (int k = 0; k < 3; ++k) {
        const int64_t d = to[k] - h->voxel_atlas.E[k], ad = d < 0 ? -d : d;
        const int size = side(h, k);
        all = all || ad >= size;
        w[k] = (int)std::min<int64_t>(ad, size);
        s[k] = (int)((d > 0 ? to[k] + size - w[k] : to[k]) & (size - 1));
    }
    const int64_t total = (int64_t)A * A * Z;
    h->voxel_atlas.moved = all ? total : total - (int64_t)(A - w[0]) * (A - w[1]) * (Z - w[2]);
    auto slab = [&](int ys, int ny, int zs, int nz, int xs, int wx) {
        VAtlasSlab S;
        S.ys = ys; S.ny = ny; S.zs = zs; S.nz = nz; S.xs = xs; S.wx = wx;
        S.npairs = (uint64_t)ny * (uint64_t)nz * (uint64_t)(A / 64);
        return gvom_launch_vatlas_move(h->stream, V, S, h->voxel_atlas.cnt);
    };
    if (all) HIPCHK(h, slab(0, A, 0, Z, 0, A));
    else {
        const int ox = (s[0] + w[0]) & (A - 1), oy = (s[1] + w[1]) & (A - 1);      // where the columns / rows that stayed begin
        HIPCHK(h, slab(0, A, 0, Z, s[0], w[0]));
        HIPCHK(h, slab(s[1], w[1], 0, Z, ox, A - w[0]));
        HIPCHK(h, slab(oy, A - w[1], s[2], w[2], ox, A - w[0]));
    }
    for (int k = 0; k < 3; ++k) h->voxel_atlas.E[k] = to[k];
    return GVOM_OK;
}

// the frame of the walk kernels: gvom_raycast's (gvom_launch_raycast names the fields) with the extent in the window's place
void walk_frame(const gvom_handle *h, ScanParams &P, RayQuery &Q)
{
    memset(&P, 0, sizeof P);
    memset(&Q, 0, sizeof Q);
    P.xy = h->voxel_atlas.A; P.zs = h->voxel_atlas.Z;
    P.xy_res = h->prm.xy_resolution; P.z_res = h->prm.z_resolution;
    P.drcp[0] = 1.0 / h->prm.xy_resolution; P.drcp[1] = 1.0 / h->prm.z_resolution;
    P.fastdiv = h->tune_fastdiv == 0 ? 0 : h->fastdiv_ok;
    P.f32_sqrt = h->f32_sqrt ? 1 : 0;
    bool far = false;
    for (int k = 0; k < 3; ++k) {
        P.origin[k] = (double)h->voxel_atlas.E[k];
        P.om[k] = (int)(h->voxel_atlas.E[k] & (side(h, k) - 1));
        far = far || h->voxel_atlas.E[k] <= -((int64_t)1 << 24) || h->voxel_atlas.E[k] >= ((int64_t)1 << 24);
    }
    Q.lit = far ? 1 : 0;                                                    // (Z <= A: the integer extent test holds for every near origin)
    Q.cap = (uint32_t)h->voxel_atlas.A + (uint32_t)h->voxel_atlas.Z;
}

// the sensor model's largest finite |direction| and |offset| per axis, read back once per gvom_sensor_model_set (which drains the stream
// and leaves the model complete in device memory).  A pixel with a non-finite entry casts no beam: it bounds nothing.
int model_bounds(gvom_handle *h)
{
    if (h->voxel_atlas.model_gen == h->range_image.gen) return GVOM_OK;
    const size_t n = (size_t)h->range_image.H * h->range_image.W;
    std::vector<double> m(n * 6);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(m.data(), h->range_image.model.p, n * 48, hipMemcpyDeviceToHost));
    for (int e = 0; e < 3; ++e) h->voxel_atlas.dmax[e] = h->voxel_atlas.omax[e] = 0.0;
    const double *d = m.data(), *o = d + n * 3;
    for (size_t i = 0; i < n; ++i) {
        bool fin = true;
        for (int e = 0; e < 3; ++e) fin = fin && std::isfinite(d[3 * i + e]) && std::isfinite(o[3 * i + e]);
        for (int e = 0; fin && e < 3; ++e) {
            h->voxel_atlas.dmax[e] = std::max(h->voxel_atlas.dmax[e], fabs(d[3 * i + e]));
            h->voxel_atlas.omax[e] = std::max(h->voxel_atlas.omax[e], fabs(o[3 * i + e]));
        }
    }
    h->voxel_atlas.model_gen = h->range_image.gen;
    return GVOM_OK;
}

// THE BOX OF A POSE: extent voxels {lx, ly, lz, dx, dy, dz} that hold every voxel a beam of the pose c (rows 0..2 of its matrix) can
// examine.  A beam's end in the sensor frame is p = max_range * dir + off, |p[j]| <= M[j] = max_range * dmax[j] + omax[j]; in the world
// q[e] = sum_j c[e][j] p[j] + t[e], so |q[e] - t[e]| <= sum_j |c[e][j]| M[j] = R[e] (no assumption on the matrix or on |dir|).  The walk
// starts at (float)(t / res), advances along the segment towards (float)(q / res) and takes steps only while the length walked is below
// the segment's length - 1 + one step (gvom.py:1127, 1150): less than one voxel beyond the end on any axis.  Its positions are float32
// sums: at most cap additions, each rounded by half an ulp at the largest magnitude met, as are the two end points and the increments.
// So with m = 3 + (cap + 4) * ulp32(largest |coordinate| in voxels) every examined voxel v[e] lies in
// [floor((t[e] - R[e]) / res[e] - m), floor((t[e] + R[e]) / res[e] + m)], which is clipped to the extent.  Returns the box's voxels.
int64_t pose_box(const gvom_handle *h, const double *c, double max_range, int32_t box[8])
{
    for (int e = 0; e < 8; ++e) box[e] = e >= 3 && e < 6 ? 1 : 0;
    for (int e = 0; e < 12; ++e)
        if (!std::isfinite(c[e])) return 1;                                  // an invalid pose casts no beam
    const double cap = (double)h->voxel_atlas.A + h->voxel_atlas.Z + 1.0;
    int64_t bits = 1;
    for (int e = 0; e < 3; ++e) {
        double R = 0.0;
        for (int j = 0; j < 3; ++j) R += fabs(c[4 * e + j]) * (max_range * h->voxel_atlas.dmax[j] + h->voxel_atlas.omax[j]);
        R = R * (1.0 + 1e-9) + 1e-300;                                       // (the sum's own rounding)
        const double res = e < 2 ? h->prm.xy_resolution : h->prm.z_resolution, t = c[4 * e + 3];
        const int size = side(h, e);
        const double E = (double)h->voxel_atlas.E[e];
        const double lo_w = (t - R) / res, hi_w = (t + R) / res;
        const double mag = std::max(std::max(fabs(lo_w), fabs(hi_w)), fabs(E) + size);
        const double m = 3.0 + (cap + 4.0) * mag * 0x1p-23;
        const double lo = floor(lo_w - m) - E, hi = floor(hi_w + m) - E;       // extent voxels, as doubles (possibly huge, infinite or NaN)
        int l = 0, u = size - 1;                                              // NaN: the whole side
        if (lo > 0.0) l = lo < (double)size ? (int)lo : size;
        if (hi < (double)(size - 1)) u = hi >= 0.0 ? (int)hi : -1;
        if (u < l) { l = 0; u = 0; }                                          // the beams never meet the extent on this axis: any box does
        box[e] = l; box[3 + e] = u - l + 1;
        bits *= box[3 + e];
    }
    return bits;
}

// THE HALO OF A CAP: the largest h with fl64(c * (double)(h * h)) <= cap2 -- a source further away on the axis cannot be within the cap --
// in the arithmetic of the distance itself; GVOM_VDIST_MAX_HALO + 1 where it is larger than that.  The float64 root is a first guess only
int64_t distance_halo(double c, double cap2)
{
    const double guess = sqrt(cap2 / c);
    if (!(guess < (double)(GVOM_VDIST_MAX_HALO + 1))) return GVOM_VDIST_MAX_HALO + 1;
    int64_t h = (int64_t)guess;
    while (c * (double)((h + 1) * (h + 1)) <= cap2) ++h;
    while (h > 0 && c * (double)(h * h) > cap2) --h;
    return h;
}
}  // namespace

extern "C" {
VIS int gvom_voxel_atlas_configure(gvom_t *h, int32_t cells, int32_t levels, int mode, const int64_t fixed_origin[3])
{
    if (!h) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    const char *const fn = "gvom_voxel_atlas_configure";
    if (h->sharded) return refuse(h, fn, "sharded handles are not supported");
    if (cells != 0) {
        if (cells < GVOM_VATLAS_MIN_CELLS || cells > GVOM_VATLAS_MAX_CELLS || (cells & (cells - 1))) return refuse(h, fn, "the side must be a power of two in 64 .. 4096");
        if (cells < h->prm.xy_size) return refuse(h, fn, "the voxel atlas must be at least as wide as the window (xy_size)");
        if (levels < 1 || levels > cells || (levels & (levels - 1))) return refuse(h, fn, "the levels must be a power of two, at most the side");
        if (levels < h->prm.z_size) return refuse(h, fn, "the voxel atlas must be at least as high as the window (z_size)");
        if ((int64_t)cells * cells * levels > ((int64_t)1 << 32)) return refuse(h, fn, "more than 2^32 voxels");
        if (mode != GVOM_ATLAS_FOLLOW && mode != GVOM_ATLAS_FIXED) return refuse(h, fn, "unknown mode");
        if (fixed_origin && !near_origin(fixed_origin)) return refuse(h, fn, "an origin at or beyond 2^30 voxels");
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (cells != h->voxel_atlas.A || (cells && levels != h->voxel_atlas.Z)) {   // another size, or none: the kernels that use the old one first
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (h->voxel_atlas.mem) HIPCHK(h, hipFree(h->voxel_atlas.mem.p));
        h->voxel_atlas.mem.p = nullptr; h->voxel_atlas.A = h->voxel_atlas.Z = 0;
        if (cells == 0) return GVOM_OK;
        HIPCHK(h, hipMalloc((void **)&h->voxel_atlas.mem.p, gvom_vatlas_bytes(cells, levels)));
        ++h->voxel_atlas.allocs;
    }
    if (cells == 0) return GVOM_OK;
    if (!h->voxel_atlas.cnt) { HIPCHK(h, hipMalloc((void **)&h->voxel_atlas.cnt.p, 256)); ++h->voxel_atlas.allocs; }
    if (!h->voxel_atlas.pin) HIPCHK(h, hipHostMalloc((void **)&h->voxel_atlas.pin.p, 256, hipHostMallocDefault));
    h->voxel_atlas.A = cells; h->voxel_atlas.Z = levels; h->voxel_atlas.follow = mode == GVOM_ATLAS_FOLLOW ? 1 : 0;
    for (int k = 0; k < 3; ++k) { h->voxel_atlas.E[k] = fixed_origin ? fixed_origin[k] : 0; h->voxel_atlas.last[k] = 0; }
    h->voxel_atlas.seq = h->voxel_atlas.outside = h->voxel_atlas.moved = 0;
    HIPCHK(h, join_second_stream(h));
    HIPCHK(h, hipMemsetAsync(h->voxel_atlas.cnt, 0, 256, h->stream));
    HIPCHK(h, hipMemsetAsync(h->voxel_atlas.mem, 0, gvom_vatlas_bytes(cells, levels), h->stream));
    return GVOM_OK;
}

VIS int gvom_voxel_atlas_clear(gvom_t *h)
{
    if (!h) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    const int rc = need_atlas(h, "gvom_voxel_atlas_clear");
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, join_second_stream(h));
    HIPCHK(h, hipMemsetAsync(h->voxel_atlas.cnt, 0, 256, h->stream));
    HIPCHK(h, hipMemsetAsync(h->voxel_atlas.mem, 0, gvom_vatlas_bytes(h->voxel_atlas.A, h->voxel_atlas.Z), h->stream));
    h->voxel_atlas.outside = h->voxel_atlas.moved = 0;
    return GVOM_OK;
}

// The CURRENT fused map merged into the atlas by k_vatlas_merge, behind the move of a following extent: on the handle's stream behind
// whatever produced that map, as gvom_raycast reads it; later scans and combines are ordered behind the kernel.  Enqueues and returns.
VIS int gvom_voxel_atlas_integrate(gvom_t *h)
{
    if (!h) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    const char *const fn = "gvom_voxel_atlas_integrate";
    int rc = need_atlas(h, fn);
    if (rc) return rc;
    const Fused *cur = nullptr;
    if ((rc = current_map(h, fn, &cur))) return rc;
    const Fused &F = *cur;
    int64_t to[3];
    for (int k = 0; k < 3; ++k) to[k] = F.origin[k] + window_side(h, k) / 2 - side(h, k) / 2;
    if (h->voxel_atlas.follow && !near_origin(to)) return refuse(h, fn, "the extent would lie at or beyond 2^30 voxels");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, join_second_stream(h));
    HIPCHK(h, hipMemsetAsync(h->voxel_atlas.cnt, 0, 64, h->stream));        // the counters of the last integrate and its move
    h->voxel_atlas.moved = 0;
    if (h->voxel_atlas.follow && (rc = move_extent(h, to))) return rc;
    const VAtlas V = atlas_of(h);
    VAtlasWindow D;
    memset(&D, 0, sizeof D);
    int r[3], lo[3], n[3];
    const int64_t inside = box_clip(h, F.origin, r, lo, n);
    D.rx = r[0]; D.ry = r[1]; D.rz = r[2];
    D.pex = (int)(h->voxel_atlas.E[0] & (V.A - 1)); D.pey = (int)(h->voxel_atlas.E[1] & (V.A - 1)); D.pez = (int)(h->voxel_atlas.E[2] & (V.Z - 1));
    if (inside > 0) {
        D.y0 = lo[1]; D.ny = n[1]; D.z0 = lo[2]; D.nz = n[2];
        const int s0 = (r[0] + lo[0] + D.pex) & (V.A - 1);                  // storage column of the first window column inside the extent
        D.bx = s0 >> 6;
        D.npx = std::min(V.A / 64, ((s0 & 63) + n[0] + 63) / 64);
        const int64_t pairs = (int64_t)D.ny * D.nz * D.npx;
        if (pairs >= ((int64_t)1 << 31)) return refuse(h, fn, "the window is too large for one merge", GVOM_ERR_CAPACITY);
        D.npairs = (uint32_t)pairs;
    }
    OccParams P;
    occ_params(h, F, P);
    ++h->voxel_atlas.seq;
    for (int k = 0; k < 3; ++k) h->voxel_atlas.last[k] = F.origin[k];
    h->voxel_atlas.outside = (int64_t)h->prm.xy_size * h->prm.xy_size * h->prm.z_size - inside;
    HIPCHK(h, gvom_launch_vatlas_merge(h->stream, V, D, P, F.state, F.tags, h->voxel_atlas.cnt));
    return GVOM_OK;
}

VIS int gvom_voxel_atlas_counts(gvom_t *h, int64_t out[11])
{
    if (!h || !out) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    const int rc = need_atlas(h, "gvom_voxel_atlas_counts");
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(h->voxel_atlas.pin, h->voxel_atlas.cnt, 128, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int k = 0; k < 5; ++k) out[k] = (int64_t)h->voxel_atlas.pin[k];
    out[5] = h->voxel_atlas.outside; out[6] = h->voxel_atlas.moved;
    out[7] = (int64_t)h->voxel_atlas.pin[VA_CNT_MOVED_OBS]; out[8] = (int64_t)h->voxel_atlas.pin[VA_CNT_OBSERVED]; out[9] = (int64_t)h->voxel_atlas.pin[VA_CNT_OCCUPIED];
    out[10] = h->voxel_atlas.seq;
    return GVOM_OK;
}

// A window-sized box of the atlas as the class grid out[x][y][z] (k_vatlas_box), a product of kind GVOM_PRODUCT_VOXEL_BOX.  Enqueues and returns.
VIS int gvom_voxel_atlas_box(gvom_t *h, const int64_t origin[3], int64_t *product_id, int64_t origin_out[3])
{
    if (!h || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *product_id = -1;
    const char *const fn = "gvom_voxel_atlas_box";
    int rc = need_atlas(h, fn);
    if (rc) return rc;
    int64_t B[3];
    if ((rc = box_origin(h, origin, B))) return rc;
    const int xy = h->prm.xy_size, zs = h->prm.z_size;
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *set = nullptr;
    const size_t bytes = set_bytes(GVOM_PRODUCT_VOXEL_BOX, xy, zs, 0);
    if ((rc = product_acquire(h, GVOM_PRODUCT_VOXEL_BOX, bytes, bytes, fn, &h->voxel_atlas, &set))) return rc;
    HIPCHK(h, join_second_stream(h));
    if ((rc = set_wait_releases(h, set))) return rc;
    VAtlasBox X;
    X.outside = (int)((int64_t)xy * xy * zs - box_frame(h, B, X));
    X.seq = (int)std::min<int64_t>(h->voxel_atlas.seq, INT32_MAX);
    int32_t *counts = part_ptr<int32_t>(set, 1);
    HIPCHK(h, hipMemsetAsync(counts, 0, 16, h->stream));
    HIPCHK(h, gvom_launch_vatlas_box(h->stream, atlas_of(h), X, part_ptr<uint8_t>(set, 0), counts));
    return publish_at(h, set, B, origin_out, product_id);
}

// What the CURRENT fused map contradicts of what the atlas remembers (include/gvom_hip.h "voxel atlas changes"), read-only on both:
// k_vchange_planes, _codes and _columns (gvom_voxel_changes.hip) on the handle's stream behind whatever produced that map and the
// integrates before the call; the columns kernel leaves the labelling's work buffer as k_frontier_mark does, so everything behind it is
// frontier_solve (gvom_product_calls.hip) on a work buffer of the handle's own (voxel_atlas.solve.work), with k_vchange_clusters in front of the
// publication.  Like gvom_frontiers this call WAITS.
VIS int gvom_voxel_atlas_changes(gvom_t *h, int mask, int32_t min_cells, int32_t max_clusters, int64_t *product_id, int64_t origin_out[3],
                                 int64_t info[4])
{
    if (!h || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *product_id = -1;
    for (int k = 0; info && k < 4; ++k) info[k] = 0;
    const char *const fn = "gvom_voxel_atlas_changes";
    int rc = need_atlas(h, fn);
    if (rc) return rc;
    if (mask < 1 || mask > 3) return refuse(h, fn, "mask must be 1 (appeared), 2 (vanished) or 3 (both)");
    if ((rc = check_clusters(h, fn, min_cells, max_clusters)) || (rc = check_side(h, fn))) return rc;
    const Fused *cur = nullptr;
    if ((rc = current_map(h, fn, &cur))) return rc;
    const Fused &F = *cur;
    const int xy = h->prm.xy_size, zs = h->prm.z_size;
    const size_t n2 = (size_t)xy * xy;
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *set = nullptr;
    const size_t bytes = set_bytes(GVOM_PRODUCT_VOXEL_CHANGES, xy, zs, max_clusters);
    if ((rc = product_acquire(h, GVOM_PRODUCT_VOXEL_CHANGES, bytes, bytes, fn, &h->voxel_atlas, &set))) return rc;
    set->cap = max_clusters;
    FrWork W;
    if ((rc = frontier_work(h, h->voxel_atlas, xy, &W))) return rc;
    const size_t planes_at = 256, lohi_at = planes_at + align256(gvom_vchange_planes_bytes(xy, zs)), d_at = lohi_at + align256(n2 * 4);
    if ((rc = stage_buf(h, h->voxel_atlas, h->voxel_atlas.chg, d_at + n2 * 4))) return rc;   // (no kernel of an earlier call is left: every call waits)
    char *const work = (char *)h->voxel_atlas.chg.p;
    unsigned long long *const cnt = (unsigned long long *)work;
    void *const planes = work + planes_at;
    uint32_t *const lohi = (uint32_t *)(work + lohi_at);
    int32_t *const D = (int32_t *)(work + d_at);
    HIPCHK(h, join_second_stream(h));
    HIPCHK(h, hipMemsetAsync(W.cnt, 0, W.clear_bytes, h->stream));          // the labelling's counters and both halves of the flags
    HIPCHK(h, hipMemsetAsync(cnt, 0, 256, h->stream));
    if ((rc = set_wait_releases(h, set))) return rc;
    VAtlasBox X;
    box_frame(h, F.origin, X);
    OccParams P;
    occ_params(h, F, P);
    uint16_t *const cols = part_ptr<uint16_t>(set, 6);
    int32_t *const rows4 = part_ptr<int32_t>(set, 4);
    HIPCHK(h, gvom_launch_vchange_planes(h->stream, atlas_of(h), X, P, F.state, F.tags, planes, cnt));
    HIPCHK(h, gvom_launch_vchange_codes(h->stream, xy, zs, planes, part_ptr<uint8_t>(set, 5)));
    HIPCHK(h, gvom_launch_vchange_columns(h->stream, xy, zs, mask, max_clusters, planes, cols, lohi, W.L, W.count, W.fl, W.cnt + FR_CNT_CELLS, D, rows4));
    const int seq = (int)std::min<int64_t>(h->voxel_atlas.seq, INT32_MAX);
    for (int k = 0; k < 3; ++k) set->origin[k] = F.origin[k];
    for (int k = 0; origin_out && k < 3; ++k) origin_out[k] = F.origin[k];
    return frontier_solve(h, fn, h->voxel_atlas.solve, xy, D, W, min_cells, max_clusters, set, product_id, info, [&]() {
        return gvom_launch_vchange_clusters(h->stream, xy, max_clusters, seq, part_ptr<const int32_t>(set, 2), cols, lohi, W.cnt + FR_CNT_KEPT, cnt, rows4,
                                            part_ptr<int32_t>(set, 3));
    });
}

// gvom_raycast on the atlas: n segments walked by k_vatlas_raycast, read-only, behind the integrates before the call; the result is a
// product of kind GVOM_PRODUCT_VOXEL_ATLAS_RAYS sized by n.  Enqueues and returns (the host route waits for its upload).
VIS int gvom_voxel_atlas_raycast(gvom_t *h, const float *from, int64_t K, const float *to, int64_t n, int on_device, int flags,
                                 int64_t extent_voxels[3], int64_t *product_id)
{
    if (!h || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *product_id = -1;
    const char *const fn = "gvom_voxel_atlas_raycast";
    int rc = need_atlas(h, fn);
    if (rc) return rc;
    if ((rc = check_rays(h, fn, from, K, to, n, flags))) return rc;
    if (!h->has_combined) return GVOM_NO_DATA;
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *set = nullptr;
    const size_t bytes = set_bytes(GVOM_PRODUCT_VOXEL_ATLAS_RAYS, 0, 0, n);
    if ((rc = product_acquire(h, GVOM_PRODUCT_VOXEL_ATLAS_RAYS, bytes, bytes, fn, &h->voxel_atlas, &set))) return rc;
    set->cap = n;
    ScanParams P;
    RayQuery Q;
    walk_frame(h, P, Q);
    if ((rc = rays_fill(h, h->voxel_atlas, from, K, to, n, on_device, flags, Q))) return rc;
    if ((rc = set_wait_releases(h, set))) return rc;
    HIPCHK(h, gvom_launch_vatlas_raycast(h->stream, P, Q, atlas_of(h), part_ptr<int32_t>(set, 0), part_ptr<float>(set, 1), part_ptr<int32_t>(set, 2)));
    return publish_at(h, set, h->voxel_atlas.E, extent_voxels, product_id, true);
}

// gvom_score_viewpoints on the atlas: the selected beams of the handle's sensor model cast from K poses by k_vatlas_viewpoints, a batch of
// poses at a time -- as many as have their bitmaps in "viewpoint_bitmap_mb" megabytes, every bitmap as large as the largest box of the
// call --, the bitmaps cleared on the stream in front of every batch; then k_vatlas_viewpoint_best.  The boxes are proved on the host
// (pose_box): the poses of the device route are read back first.
VIS int gvom_voxel_atlas_score_viewpoints(gvom_t *h, const double *poses, int64_t K, int on_device, double max_range, int32_t stride_h,
                                          int32_t stride_w, int flags, int64_t extent_voxels[3], int64_t *product_id)
{
    if (!h || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *product_id = -1;
    const char *const fn = "gvom_voxel_atlas_score_viewpoints";
    int rc = need_atlas(h, fn);
    if (rc) return rc;
    ViewBeams beams;
    if ((rc = check_views(h, fn, poses, K, max_range, stride_h, stride_w, flags, (int64_t)h->voxel_atlas.A + h->voxel_atlas.Z, "cells + levels", &beams))) return rc;
    if (!h->has_combined) return GVOM_NO_DATA;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, join_second_stream(h));
    if ((rc = model_bounds(h))) return rc;
    std::vector<double> back;
    const double *hp = poses;
    if (on_device) {                                                        // the boxes need the poses: read back behind whatever wrote them
        back.resize((size_t)K * 12);
        HIPCHK(h, hipMemcpyAsync(back.data(), poses, (size_t)K * 96, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        hp = back.data();
    }
    std::vector<int32_t> boxes((size_t)K * 8);
    int64_t most = 1;
    for (int64_t k = 0; k < K; ++k) {
        const int64_t bits = pose_box(h, hp + k * 12, max_range, boxes.data() + k * 8);
        if (bits >= ((int64_t)1 << 31)) return refuse(h, fn, "the box of a pose holds 2^31 voxels or more (a shorter max_range, or a smaller atlas)", GVOM_ERR_CAPACITY);
        most = std::max(most, bits);
    }
    DevSet *set = nullptr;
    const size_t bytes = set_bytes(GVOM_PRODUCT_VOXEL_ATLAS_VIEWPOINTS, 0, 0, K);
    if ((rc = product_acquire(h, GVOM_PRODUCT_VOXEL_ATLAS_VIEWPOINTS, bytes, bytes, fn, &h->voxel_atlas, &set))) return rc;
    set->cap = K;
    size_t bm_words;                                                        // every bitmap as large as the largest box of the call
    const int64_t batch = views_batch(h, most, K, &bm_words);
    if ((rc = stage_buf(h, h->voxel_atlas, h->voxel_atlas.bitmaps, (size_t)batch * bm_words * 4))) return rc;
    ScanParams P;
    RayQuery R;
    walk_frame(h, P, R);
    ViewQuery Q;
    views_fill(h, R, beams, K, max_range, stride_h, stride_w, flags, bm_words, Q);
    const HostPart parts[2] = {{on_device ? nullptr : poses, (size_t)K * 96}, {boxes.data(), (size_t)K * 32}};
    const void *dev[2];
    if ((rc = stage_host(h, h->voxel_atlas, parts, 2, true, dev))) return rc;
    Q.poses = on_device ? poses : (const double *)dev[0];
    const int32_t *dboxes = (const int32_t *)dev[1];
    if ((rc = set_wait_releases(h, set))) return rc;
    const VAtlas V = atlas_of(h);
    int32_t *rows = part_ptr<int32_t>(set, 0);
    rc = views_run(h, h->voxel_atlas.bitmaps, Q, batch, rows,
                   [&](int nk) { return gvom_launch_vatlas_viewpoints(h->stream, P, Q, V, nk, dboxes, (uint32_t *)h->voxel_atlas.bitmaps.p, rows); },
                   [&]() { return gvom_launch_vatlas_viewpoint_best(h->stream, P, Q, V, rows, part_ptr<int32_t>(set, 1)); });
    if (rc) return rc;
    h->voxel_atlas.last_batch = (int)batch;
    return publish_at(h, set, h->voxel_atlas.E, extent_voxels, product_id, true);
}

// gvom_score_alignments on the atlas: k_vatlas_align_field turns the box at B into the class grid -- in the handle's class-grid buffer,
// gvom_score_alignments' own: both rebuild it in every call, on the one stream -- and gvom_launch_align_grid scores against it with
// origin = B.  The resolutions and the division form are the current fused map's frame.  Read-only on the atlas; enqueues and returns
// (the host route waits for its upload).
VIS int gvom_voxel_atlas_score_alignments(gvom_t *h, const float *cloud, int64_t n, const double *transforms, int64_t K, int on_device, int dilate,
                                          const int32_t weights[5], const int64_t origin[3], int64_t origin_out[3], int64_t *product_id)
{
    if (!h || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *product_id = -1;
    const char *const fn = "gvom_voxel_atlas_score_alignments";
    int rc = need_atlas(h, fn);
    if (rc) return rc;
    size_t gb;
    if ((rc = check_align(h, fn, cloud, n, transforms, K, dilate, weights, &gb))) return rc;
    int64_t B[3];
    if ((rc = box_origin(h, origin, B))) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *set = nullptr;
    const size_t bytes = set_bytes(GVOM_PRODUCT_VOXEL_ATLAS_ALIGNMENT, 0, 0, K);
    if ((rc = product_acquire(h, GVOM_PRODUCT_VOXEL_ATLAS_ALIGNMENT, bytes, bytes, fn, &h->voxel_atlas, &set))) return rc;
    set->cap = K;
    if ((rc = stage_buf(h, h->alignment, h->alignment.grid, gb))) return rc;
    AlignParams P;
    memset(&P, 0, sizeof P);
    metric_frame(h, h->fused[h->cur], P);
    for (int k = 0; k < 3; ++k) P.origin[k] = (double)B[k];
    const float *cdev;
    const double *tdev;
    if ((rc = align_fill(h, h->voxel_atlas, cloud, n, transforms, K, on_device, dilate, weights, P, &cdev, &tdev))) return rc;
    if ((rc = set_wait_releases(h, set))) return rc;
    VAtlasBox X;
    box_frame(h, B, X);
    uint32_t *const grid = (uint32_t *)h->alignment.grid.p;
    HIPCHK(h, gvom_launch_vatlas_align_field(h->stream, atlas_of(h), X, dilate, grid));
    HIPCHK(h, gvom_launch_align_grid(h->stream, P, cdev, tdev, grid, part_ptr<int32_t>(set, 0), part_ptr<int32_t>(set, 1)));
    return publish_at(h, set, B, origin_out, product_id);
}

// The distance field of the box at B (include/gvom_hip.h "voxel distance field"): the three passes of gvom_voxel_distance.hip on the
// handle's stream, behind the integrates before the call; read-only on the atlas.  The halos are the host's to compute, in the
// definition's own arithmetic; the passes in y and z run on the box grown by them, clipped to where a source can lie -- the extent, one
// voxel further under the flag (everything outside is a source there, and the nearest such voxel on an axis is the first one), never
// less than the box itself.  Enqueues and returns.
VIS int gvom_voxel_atlas_distance_field(gvom_t *h, const int64_t origin[3], double max_distance, int flags, int64_t *product_id, int64_t origin_out[3])
{
    if (!h || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *product_id = -1;
    const char *const fn = "gvom_voxel_atlas_distance_field";
    int rc = need_atlas(h, fn);
    if (rc) return rc;
    if (!std::isfinite(max_distance) || !(max_distance > 0.0)) return refuse(h, fn, "max_distance must be finite and > 0");
    if (flags & ~GVOM_DISTANCE_UNKNOWN_BLOCKS) return refuse(h, fn, "unknown flag bits");
    int64_t B[3];
    if ((rc = box_origin(h, origin, B))) return rc;
    const int xy = h->prm.xy_size, zs = h->prm.z_size;
    VDistFrame F;
    memset(&F, 0, sizeof F);
    F.a = h->prm.xy_resolution * h->prm.xy_resolution; F.b = h->prm.z_resolution * h->prm.z_resolution;
    F.cap2 = max_distance * max_distance;
    if (!std::isfinite(F.cap2) || !(F.a > 0.0) || !(F.b > 0.0)) return refuse(h, fn, "max_distance squared is not finite", GVOM_ERR_CAPACITY);
    const int64_t hxy = distance_halo(F.a, F.cap2), hz = distance_halo(F.b, F.cap2);
    if (hxy > GVOM_VDIST_MAX_HALO || hz > GVOM_VDIST_MAX_HALO) return refuse(h, fn, "max_distance reaches further than 32767 voxels", GVOM_ERR_CAPACITY);
    F.B.outside = (int)((int64_t)xy * xy * zs - box_frame(h, B, F.B));
    F.B.seq = (int)std::min<int64_t>(h->voxel_atlas.seq, INT32_MAX);
    F.unknown = (flags & GVOM_DISTANCE_UNKNOWN_BLOCKS) ? 1 : 0;
    F.hxy = (int)hxy; F.kx = (int)((hxy + 63) / 64) + 1; F.nw = (xy + 63) / 64;
    // rows of the extent (and the one beyond it) below and above the box, as far as the halo reaches: (r + f) below, (size + f) - (r + n) above
    auto grown = [&](int r, int n, int size, int64_t halo, int *below, int *all) {
        const int64_t e0 = -(int64_t)r - F.unknown, e1 = (int64_t)size + F.unknown - r;   // where a source can lie, in box coordinates: [e0, e1)
        const int64_t lo = e1 > -halo ? std::max<int64_t>(0, std::min<int64_t>(halo, -e0)) : 0;
        const int64_t hi = e0 < n + halo ? std::max<int64_t>(0, std::min<int64_t>(halo, e1 - n)) : 0;
        *below = (int)lo; *all = (int)(lo + n + hi);
    };
    grown(F.B.ry, xy, h->voxel_atlas.A, hxy, &F.hby, &F.nyg);
    grown(F.B.rz, zs, h->voxel_atlas.Z, hz, &F.hbz, &F.nzg);
    const size_t rows_bytes = align256(gvom_vdist_rows_bytes(F)), work_bytes = rows_bytes + gvom_vdist_cols_bytes(F);
    if (work_bytes > ((size_t)h->voxel_atlas.mb << 20))
        return refuse(h, fn, "the working buffers of this cap need " + std::to_string((work_bytes >> 20) + 1) + " MB, more than \"voxel_distance_mb\" allows", GVOM_ERR_CAPACITY);
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *set = nullptr;
    const size_t bytes = set_bytes(GVOM_PRODUCT_VOXEL_DISTANCE, xy, zs, 0);
    if ((rc = product_acquire(h, GVOM_PRODUCT_VOXEL_DISTANCE, bytes, bytes, fn, &h->voxel_atlas, &set))) return rc;
    HIPCHK(h, join_second_stream(h));
    if (h->voxel_atlas.dist.bytes < work_bytes) HIPCHK(h, hipStreamSynchronize(h->stream));   // the passes that still run on the buffer it outgrows
    if ((rc = stage_buf(h, h->voxel_atlas, h->voxel_atlas.dist, work_bytes))) return rc;
    if ((rc = set_wait_releases(h, set))) return rc;
    int32_t *counts = part_ptr<int32_t>(set, 1);
    HIPCHK(h, hipMemsetAsync(counts, 0, 16, h->stream));
    HIPCHK(h, gvom_launch_vdist_field(h->stream, atlas_of(h), F, h->voxel_atlas.dist.p, part_ptr<float>(set, 0), counts));
    h->voxel_atlas.halo[0] = (int)hxy; h->voxel_atlas.halo[1] = (int)hz;
    return publish_at(h, set, B, origin_out, product_id);
}

// The field of a live distance product gathered at n world points by k_vdist_sample, on the handle's stream: behind the passes that
// wrote the field and in front of whatever reuses its set.  Enqueues and returns (the host route waits for its upload).
VIS int gvom_voxel_distance_sample(gvom_t *h, int64_t field_product_id, const float *points, int64_t n, int on_device, int64_t *product_id)
{
    if (!h || !product_id) return GVOM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    *product_id = -1;
    const char *const fn = "gvom_voxel_distance_sample";
    int rc;
    if (h->sharded) return refuse(h, fn, "sharded handles are not supported");
    if (!points) return refuse(h, fn, "points must not be NULL");
    if (n < 1) return refuse(h, fn, "n must be at least 1");
    if (n > GVOM_VDIST_MAX_POINTS) return refuse(h, fn, "more than 2^26 points in one call", GVOM_ERR_CAPACITY);
    DevSet *const f = find_set(h->psets, field_product_id);
    if (!f || f->kind != GVOM_PRODUCT_VOXEL_DISTANCE) return refuse(h, fn, "unknown or stale distance field id");
    HIPCHK(h, hipSetDevice(h->device));
    DevSet *set = nullptr;
    const size_t bytes = set_bytes(GVOM_PRODUCT_VOXEL_DISTANCE_SAMPLES, 0, 0, n);
    if ((rc = product_acquire(h, GVOM_PRODUCT_VOXEL_DISTANCE_SAMPLES, bytes, bytes, fn, &h->voxel_atlas, &set))) return rc;
    set->cap = n;
    const float *pdev = points;
    HIPCHK(h, join_second_stream(h));
    if (!on_device) {                                                       // host points: staged, and up before the call returns
        const HostPart parts[1] = {{points, (size_t)n * 12}};
        const void *dev[1];
        if ((rc = stage_host(h, h->voxel_atlas, parts, 1, true, dev))) return rc;
        pdev = (const float *)dev[0];
    }
    if ((rc = set_wait_releases(h, set))) return rc;
    VDistSample Q;
    memset(&Q, 0, sizeof Q);
    Q.xy_res = h->prm.xy_resolution; Q.z_res = h->prm.z_resolution;
    for (int k = 0; k < 3; ++k) Q.origin[k] = (double)f->origin[k];
    Q.n = f->xy; Q.zs = f->zs; Q.npts = n;
    int32_t *counts = part_ptr<int32_t>(set, 1);
    HIPCHK(h, hipMemsetAsync(counts, 0, 16, h->stream));
    HIPCHK(h, gvom_launch_vdist_sample(h->stream, Q, pdev, part_ptr<const float>(f, 0), part_ptr<float>(set, 0), counts));
    for (int k = 0; k < 3; ++k) set->origin[k] = f->origin[k];
    return product_publish(h, set, product_id);
}
}  // extern "C"
