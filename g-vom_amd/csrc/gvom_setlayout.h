// gvom_setlayout.h -- what a device set (DevSet, gvom_host.h) holds: the one table of the layouts of a map set and of every product
// kind (host side; no HIP in here: tests/setlayout_host_test.cpp compiles it alone).  set_bytes() sizes the one allocation of a set,
// set_part() says where a part of it lies and what it is; the pool, the exports and the DLPack capsules (gvom_sets.hip) and the
// launches (gvom_product_calls.hip) go through these two.  kind 0 = the nine maps of one combine, [y][x] order: the six f64 maps (3
// roughness, 4 height, 5 inferred height, 6 / 7 x / y slope, 8 guessed delta) at k * S doubles, each 256-byte aligned, then the three
// i32 maps (0 positive, 1 negative, 2 visibility) behind them at k * S ints, each 128-byte aligned; S = dev_map_stride(xy), 60 bytes
// per cell.  GVOM_PRODUCT_* otherwise, every part at a 256-byte boundary:
//   occupancy        V bytes, out[x][y][z]
//   voxel cloud      256-byte header (the uint64 row counter k_voxel_cloud adds to), then cap x 8 and cap x 3 floats
//   height clouds    xy*xy x 7 / x 3 floats
//   clearance        xy*xy floats (metres), then xy*xy int32 (squared cells), both [y][x]
//   raycast          cap x 4 int32 {status, steps, voxel, unknown}, then cap x 3 floats (stop position); cap = the rays of the call
//                    that wrote it
//   cost field       xy*xy int32 (cost to go), then xy*xy uint8 (direction), then xy*xy uint16 (cell costs), all [y][x]
//   rollouts (10)    cap x 4 int32 {status, first_blocked, path_cost, terminal}, then cap x cols uint16 (pose costs); cap = the
//                    rollouts K and cols = the poses per rollout T of the call that wrote it.  Kinds 8, 9 and 11 are not assigned
//   alignment (12)   cap x 6 int32 {score, occupied, near, free, unknown, outside}, then 4 int32 {best index, best score, n, K};
//                    cap = the candidates K of the call that wrote it
//   attitude (14)    cap x 5 int32 {status, first_bad, steepest_pitch_pose, steepest_roll_pose, lowest_belly_pose}, then cap x cols x 3
//                    floats {pitch, roll, belly}, then cap x cols uint8 (pose status); cap = K and cols = T as for rollouts.  Kind 13
//                    is not assigned
//   frontiers (16)   cap x 8 int32 {label, cells, min x, min y, max x, max y, best cell, best D}, then cap x 2 int64 {sum x, sum y},
//                    then xy*xy int32 (the cluster map, [y][x]), then 4 int32 {n_kept, frontier cells, those in kept clusters, cap};
//                    cap = max_clusters of the call that wrote it.  Kind 15 is not assigned
//   viewpoints (18)  cap x 8 int32 {status, gain, visits, beams OCCUPIED, CLEAR, LEFT_WINDOW, UNKNOWN, INVALID}, then 4 int32 {best
//                    index, its gain, K, beams per viewpoint}; cap = the viewpoints K of the call that wrote it.  Kind 17 is not assigned
//   pose field (20)  cap x xy*xy int32 (cost to go), then cap x xy*xy uint8 (action), then cap x xy*xy uint16 (pose costs): volumes
//                    [h][y][x], every plane laid out like a cost field's maps; cap = the headings H of the call that wrote it.  Kind 19
//                    is not assigned
//   recall (22)      xy*xy int32 (the stamps of a recalled map set, [y][x] like a device map), then 4 int32 {cells of rank 2, of rank 1,
//                    outside the extent, seq}.  Kind 21 is not assigned
//   extent (24)      the atlas's whole extent unwrapped, cap x cap cells, cap = the atlas's side A: the f64 maps roughness and height,
//                    then the int32 maps positive, negative, visibility and stamp, all [y][x].  Kind 23 is not assigned
//   atlas field (26) a cost field at the atlas's scale, cap x cap cells, cap = the side A of the atlas that made it: cap*cap int32 (cost
//                    to go), then cap*cap uint8 (direction), then cap*cap uint16 (cell costs), all [y][x] over the field's own extent.
//                    Kind 25 is not assigned
//   atlas frontiers (28)  the four parts of frontiers (16) with the window's side replaced by cols = the side of the atlas FIELD the call
//                    was given: cap x 8 int32, cap x 2 int64, cols*cols int32 (the cluster map, [y][x] over the field's extent), 4 int32;
//                    cap = max_clusters of the call that wrote it.  Kind 27 is not assigned
//   attitude volume (30)  cap x xy*xy uint8 (status), then cap x xy*xy uint8 (tilt): volumes [h][y][x], every plane laid out like a pose
//                    field's; then 8 int32 {states per status 0 .. 6, H}; cap = the headings H of the call that wrote it.  Kind 29 is
//                    not assigned
//   voxel box (32)   xy*xy*zs bytes, out[x][y][z] like the occupancy grid: the class codes 0 / 1 / 2 of a box of the voxel atlas; then 4 int32
//                    {occupied, free, outside the extent, seq}.  Kind 31 is not assigned
//   atlas rays (34)  cap x 3 int32 {status, steps, unknown}, then cap x 3 floats (stop position), then cap x 3 int32 (the world voxel of the
//                    stop); cap = the rays of the call that wrote it.  Kind 33 is not assigned
//   atlas viewpoints (36)  the two parts of viewpoints (18).  Kind 35 is not assigned
//   atlas alignment (38)   the two parts of alignment (12).  Kind 37 is not assigned
//   voxel distance (40)    xy*xy*zs floats, out[x][y][z] like the voxel box: metres to the nearest source, +inf beyond the cap; then 4 int32
//                    {voxels at 0, voxels with a finite distance, outside the extent, seq}.  Kind 39 is not assigned
//   distance samples (42)  cap floats (the field at the voxel of every point, NaN outside its box), then 4 int32 {inside the box, of those
//                    finite, of those 0, n}; cap = the points of the call that wrote it.  Kind 41 is not assigned
//   body (44)        cap x 4 int32 {status, first_bad, tightest_pose, tightest_sphere}, then cap x cols floats (pose clearance), then cap x
//                    cols x 2 uint8 {pose status, tightest sphere}; cap = K and cols = T as for rollouts.  Kind 43 is not assigned
//   body volume (46) cap x xy*xy uint8 (status), then cap x xy*xy uint8 (squeeze), then cap x xy*xy floats (clearance): volumes [h][y][x],
//                    every plane laid out like a pose field's; then 8 int32 {states per status 0 .. 5, H, S}; cap = the headings H of the
//                    call that wrote it.  Kind 45 is not assigned
//   voxel changes (48)  the four parts of frontiers (16) with part 3 grown to 8 int32 {n_kept, marked columns, those in kept clusters, cap,
//                    appeared voxels, vanished voxels, window voxels outside the extent, seq}; then cap x 4 int32 {appeared voxels, vanished
//                    voxels, lowest level, highest level} per kept cluster; then xy*xy*zs bytes, out[x][y][z] like the voxel box: the change
//                    codes 0 / 1 / 2; then 2 x xy*xy uint16 (appeared / vanished voxels per column): planes [k][y][x], each laid out like a
//                    pose field's; cap = max_clusters of the call that wrote it.  Kind 47 is not assigned
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "../../include/gvom_hip.h"

namespace gvom_host {
enum { kDLInt = 0, kDLUInt = 1, kDLFloat = 2 };            // DLPack type codes (DLDataTypeCode, as the DLPack specification defines them)

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// what of a set its layout depends on (DevSet, gvom_host.h, is one of these)
struct SetShape {
    char *mem = nullptr;
    int xy = 0;
    int kind = 0, zs = 0;                      // GVOM_PRODUCT_* (0: a map set); z_size (occupancy)
    // voxel cloud: rows the allocation holds; raycast: rays of the product; a map set: the elements from one map to the next,
    // dev_map_stride(xy) of gvom_internal.h (which needs the HIP runtime: it comes in through here) -- a multiple of 32, >= xy*xy
    int64_t cap = 0;
    int64_t cols = 0;                          // rollouts, attitude, body: poses per rollout (T); atlas frontiers: the side of the field
};
struct SetPart { void *ptr; int ndim; int64_t shape[3], strides[3]; uint8_t code, bits; size_t bytes; };

inline size_t set_bytes(int kind, int xy, int zs, int64_t cap, int64_t cols = 0)
{
    const size_t n2 = (size_t)xy * xy;
    switch (kind) {
    case 0: return (size_t)cap * 60;
    case GVOM_PRODUCT_OCCUPANCY: return n2 * zs;
    case GVOM_PRODUCT_VOXEL_CLOUD: return 256 + align256((size_t)cap * 32) + align256((size_t)cap * 12);
    case GVOM_PRODUCT_HEIGHT_CLOUD: return n2 * 28;
    case GVOM_PRODUCT_INFERRED_HEIGHT_CLOUD: return n2 * 12;
    case GVOM_PRODUCT_CLEARANCE: return align256(n2 * 4) + n2 * 4;
    case GVOM_PRODUCT_RAYCAST: return align256((size_t)cap * 16) + (size_t)cap * 12;
    case GVOM_PRODUCT_COSTFIELD: return align256(n2 * 4) + align256(n2) + n2 * 2;
    case GVOM_PRODUCT_ROLLOUTS: return align256((size_t)cap * 16) + (size_t)cap * (size_t)cols * 2;
    case GVOM_PRODUCT_ALIGNMENT: return align256((size_t)cap * 24) + 16;
    case GVOM_PRODUCT_ATTITUDE: return align256((size_t)cap * 20) + align256((size_t)cap * (size_t)cols * 12) + (size_t)cap * (size_t)cols;
    case GVOM_PRODUCT_FRONTIERS: return align256((size_t)cap * 32) + align256((size_t)cap * 16) + align256(n2 * 4) + 16;
    case GVOM_PRODUCT_VIEWPOINTS: return align256((size_t)cap * 32) + 16;
    case GVOM_PRODUCT_POSEFIELD: return align256((size_t)cap * n2 * 4) + align256((size_t)cap * n2) + (size_t)cap * n2 * 2;
    case GVOM_PRODUCT_ATLAS_RECALL: return align256(n2 * 4) + 16;
    case GVOM_PRODUCT_ATLAS_EXTENT: return (size_t)cap * (size_t)cap * 32;
    case GVOM_PRODUCT_ATLAS_FIELD: return align256((size_t)cap * (size_t)cap * 4) + align256((size_t)cap * (size_t)cap) + (size_t)cap * (size_t)cap * 2;
    case GVOM_PRODUCT_ATLAS_FRONTIERS: return align256((size_t)cap * 32) + align256((size_t)cap * 16) + align256((size_t)cols * (size_t)cols * 4) + 16;
    case GVOM_PRODUCT_ATTITUDE_VOLUME: return 2 * align256((size_t)cap * n2) + 32;
    case GVOM_PRODUCT_VOXEL_BOX: return align256(n2 * zs) + 16;
    case GVOM_PRODUCT_VOXEL_ATLAS_RAYS: return 2 * align256((size_t)cap * 12) + (size_t)cap * 12;
    case GVOM_PRODUCT_VOXEL_ATLAS_VIEWPOINTS: return align256((size_t)cap * 32) + 16;
    case GVOM_PRODUCT_VOXEL_ATLAS_ALIGNMENT: return align256((size_t)cap * 24) + 16;
    case GVOM_PRODUCT_VOXEL_DISTANCE: return align256(n2 * zs * 4) + 16;
    case GVOM_PRODUCT_VOXEL_DISTANCE_SAMPLES: return align256((size_t)cap * 4) + 16;
    case GVOM_PRODUCT_BODY: return align256((size_t)cap * 16) + align256((size_t)cap * (size_t)cols * 4) + (size_t)cap * (size_t)cols * 2;
    case GVOM_PRODUCT_BODY_VOLUME: return 2 * align256((size_t)cap * n2) + align256((size_t)cap * n2 * 4) + 32;
    case GVOM_PRODUCT_VOXEL_CHANGES:
        return align256((size_t)cap * 32) + 2 * align256((size_t)cap * 16) + align256(n2 * 4) + 256 + align256(n2 * zs) + n2 * 4;
    }
    return 0;
}

// false: the set has no such part
inline bool set_part(const SetShape *s, int part, SetPart *d)
{
    const int64_t xy = s->xy, n2 = xy * xy;
    memset(d, 0, sizeof *d);
    d->ndim = 2; d->code = kDLFloat; d->bits = 32;
    d->shape[2] = d->strides[2] = 1;
    auto rows = [&](void *ptr, int64_t n, int64_t cols) { d->ptr = ptr; d->shape[0] = n; d->shape[1] = cols; d->strides[0] = cols; d->strides[1] = 1; };
    switch (s->kind) {
    case 0: {                                              // map `part` of a map set: [x, y] indexing, column-major
        if (part < 0 || part > 8) return false;
        const size_t S = (size_t)s->cap;
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
    case GVOM_PRODUCT_ROLLOUTS:
        if (part == 0) { rows(s->mem, s->cap, 4); d->code = kDLInt; }
        else if (part == 1) { rows(s->mem + align256((size_t)s->cap * 16), s->cap, s->cols); d->code = kDLUInt; d->bits = 16; }
        else return false;
        break;
    case GVOM_PRODUCT_ALIGNMENT:
    case GVOM_PRODUCT_VOXEL_ATLAS_ALIGNMENT:               // (38: the same two parts)
        if (part == 0) { rows(s->mem, s->cap, 6); d->code = kDLInt; }
        else if (part == 1) { d->ptr = s->mem + align256((size_t)s->cap * 24); d->ndim = 1; d->shape[0] = 4; d->strides[0] = 1; d->shape[1] = d->strides[1] = 1; d->code = kDLInt; }
        else return false;
        break;
    case GVOM_PRODUCT_ATTITUDE: {
        char *const att = s->mem + align256((size_t)s->cap * 20);
        if (part == 0) { rows(s->mem, s->cap, 5); d->code = kDLInt; }
        else if (part == 1) {
            d->ptr = att; d->ndim = 3;
            d->shape[0] = s->cap; d->shape[1] = s->cols; d->shape[2] = 3;
            d->strides[0] = s->cols * 3; d->strides[1] = 3; d->strides[2] = 1;
        }
        else if (part == 2) { rows(att + align256((size_t)s->cap * (size_t)s->cols * 12), s->cap, s->cols); d->code = kDLUInt; d->bits = 8; }
        else return false;
        break;
    }
    case GVOM_PRODUCT_FRONTIERS:
    case GVOM_PRODUCT_ATLAS_FRONTIERS: {                   // (28: the same four parts, the cluster map at the side of the atlas field)
        const int64_t side = s->kind == GVOM_PRODUCT_FRONTIERS ? xy : s->cols;
        char *const sums = s->mem + align256((size_t)s->cap * 32), *const cmap = sums + align256((size_t)s->cap * 16);
        if (part == 0) { rows(s->mem, s->cap, 8); d->code = kDLInt; }
        else if (part == 1) { rows(sums, s->cap, 2); d->code = kDLInt; d->bits = 64; }
        else if (part == 2) { d->ptr = cmap; d->shape[0] = d->shape[1] = side; d->strides[0] = 1; d->strides[1] = side; d->code = kDLInt; }   // [x, y] indexing, column-major, like a device map
        else if (part == 3) { d->ptr = cmap + align256((size_t)(side * side) * 4); d->ndim = 1; d->shape[0] = 4; d->strides[0] = 1; d->shape[1] = d->strides[1] = 1; d->code = kDLInt; }
        else return false;
        break;
    }
    case GVOM_PRODUCT_VIEWPOINTS:
    case GVOM_PRODUCT_VOXEL_ATLAS_VIEWPOINTS:              // (36: the same two parts)
        if (part == 0) { rows(s->mem, s->cap, 8); d->code = kDLInt; }
        else if (part == 1) { d->ptr = s->mem + align256((size_t)s->cap * 32); d->ndim = 1; d->shape[0] = 4; d->strides[0] = 1; d->shape[1] = d->strides[1] = 1; d->code = kDLInt; }
        else return false;
        break;
    case GVOM_PRODUCT_POSEFIELD: {                         // [h, x, y] indexing: every plane column-major, like a device map
        if (part < 0 || part > 2) return false;
        const size_t vol = (size_t)s->cap * (size_t)n2;
        d->ptr = s->mem + (part ? align256(vol * 4) : 0) + (part == 2 ? align256(vol) : 0);
        d->ndim = 3;
        d->shape[0] = s->cap; d->shape[1] = d->shape[2] = xy;
        d->strides[0] = n2; d->strides[1] = 1; d->strides[2] = xy;
        d->code = part ? kDLUInt : kDLInt; d->bits = part == 0 ? 32 : (part == 1 ? 8 : 16);
        break;
    }
    case GVOM_PRODUCT_ATLAS_RECALL:
        if (part == 0) { d->ptr = s->mem; d->shape[0] = d->shape[1] = xy; d->strides[0] = 1; d->strides[1] = xy; d->code = kDLInt; }   // [x, y] indexing, column-major, like a device map
        else if (part == 1) { d->ptr = s->mem + align256((size_t)n2 * 4); d->ndim = 1; d->shape[0] = 4; d->strides[0] = 1; d->shape[1] = d->strides[1] = 1; d->code = kDLInt; }
        else return false;
        break;
    case GVOM_PRODUCT_ATLAS_EXTENT: {                      // [x, y] indexing over the extent, column-major: parts 0 .. 2 and 5 int32, 3 and 4 f64
        if (part < 0 || part > 5) return false;
        const size_t a2 = (size_t)s->cap * (size_t)s->cap;
        static const int at[6] = {0, 1, 2, 0, 1, 3};       // the part's place among the int32 maps / the f64 maps
        const bool f64 = part == 3 || part == 4;
        d->ptr = f64 ? s->mem + (size_t)at[part] * a2 * 8 : s->mem + 16 * a2 + (size_t)at[part] * a2 * 4;
        d->shape[0] = d->shape[1] = s->cap; d->strides[0] = 1; d->strides[1] = s->cap;
        d->code = f64 ? kDLFloat : kDLInt; d->bits = f64 ? 64 : 32;
        break;
    }
    case GVOM_PRODUCT_ATLAS_FIELD: {                       // [x, y] indexing over the field's extent, column-major, like a cost field's maps
        if (part < 0 || part > 2) return false;
        const size_t a2 = (size_t)s->cap * (size_t)s->cap;
        d->ptr = s->mem + (part ? align256(a2 * 4) : 0) + (part == 2 ? align256(a2) : 0);
        d->shape[0] = d->shape[1] = s->cap; d->strides[0] = 1; d->strides[1] = s->cap;
        d->code = part ? kDLUInt : kDLInt; d->bits = part == 0 ? 32 : (part == 1 ? 8 : 16);
        break;
    }
    case GVOM_PRODUCT_ATTITUDE_VOLUME: {                   // parts 0 and 1 [h, x, y] indexing: every plane column-major, like a pose field's
        if (part < 0 || part > 2) return false;
        const size_t vol = (size_t)s->cap * (size_t)n2;
        d->ptr = s->mem + (size_t)part * align256(vol);
        if (part == 2) { d->ndim = 1; d->shape[0] = 8; d->strides[0] = 1; d->shape[1] = d->strides[1] = 1; d->code = kDLInt; break; }
        d->ndim = 3;
        d->shape[0] = s->cap; d->shape[1] = d->shape[2] = xy;
        d->strides[0] = n2; d->strides[1] = 1; d->strides[2] = xy;
        d->code = kDLUInt; d->bits = 8;
        break;
    }
    case GVOM_PRODUCT_VOXEL_BOX:
        if (part == 0) {
            d->ptr = s->mem; d->ndim = 3; d->code = kDLUInt; d->bits = 8;
            d->shape[0] = d->shape[1] = xy; d->shape[2] = s->zs;
            d->strides[0] = xy * s->zs; d->strides[1] = s->zs; d->strides[2] = 1;
        }
        else if (part == 1) { d->ptr = s->mem + align256((size_t)n2 * s->zs); d->ndim = 1; d->shape[0] = 4; d->strides[0] = 1; d->shape[1] = d->strides[1] = 1; d->code = kDLInt; }
        else return false;
        break;
    case GVOM_PRODUCT_VOXEL_ATLAS_RAYS:
        if (part < 0 || part > 2) return false;
        rows(s->mem + (size_t)part * align256((size_t)s->cap * 12), s->cap, 3);
        if (part != 1) d->code = kDLInt;
        break;
    case GVOM_PRODUCT_VOXEL_DISTANCE:
        if (part == 0) {
            d->ptr = s->mem; d->ndim = 3;
            d->shape[0] = d->shape[1] = xy; d->shape[2] = s->zs;
            d->strides[0] = xy * s->zs; d->strides[1] = s->zs; d->strides[2] = 1;
        }
        else if (part == 1) { d->ptr = s->mem + align256((size_t)n2 * s->zs * 4); d->ndim = 1; d->shape[0] = 4; d->strides[0] = 1; d->shape[1] = d->strides[1] = 1; d->code = kDLInt; }
        else return false;
        break;
    case GVOM_PRODUCT_VOXEL_DISTANCE_SAMPLES:
        if (part == 0) { d->ptr = s->mem; d->ndim = 1; d->shape[0] = s->cap; d->strides[0] = 1; d->shape[1] = d->strides[1] = 1; }
        else if (part == 1) { d->ptr = s->mem + align256((size_t)s->cap * 4); d->ndim = 1; d->shape[0] = 4; d->strides[0] = 1; d->shape[1] = d->strides[1] = 1; d->code = kDLInt; }
        else return false;
        break;
    case GVOM_PRODUCT_BODY: {
        char *const clr = s->mem + align256((size_t)s->cap * 16);
        if (part == 0) { rows(s->mem, s->cap, 4); d->code = kDLInt; }
        else if (part == 1) rows(clr, s->cap, s->cols);
        else if (part == 2) {
            d->ptr = clr + align256((size_t)s->cap * (size_t)s->cols * 4); d->ndim = 3; d->code = kDLUInt; d->bits = 8;
            d->shape[0] = s->cap; d->shape[1] = s->cols; d->shape[2] = 2;
            d->strides[0] = s->cols * 2; d->strides[1] = 2; d->strides[2] = 1;
        }
        else return false;
        break;
    }
    case GVOM_PRODUCT_BODY_VOLUME: {                       // parts 0 .. 2 [h, x, y] indexing: every plane column-major, like a pose field's
        if (part < 0 || part > 3) return false;
        const size_t vol = (size_t)s->cap * (size_t)n2;
        d->ptr = s->mem + (size_t)(part < 2 ? part : 2) * align256(vol) + (part == 3 ? align256(vol * 4) : 0);
        if (part == 3) { d->ndim = 1; d->shape[0] = 8; d->strides[0] = 1; d->shape[1] = d->strides[1] = 1; d->code = kDLInt; break; }
        d->ndim = 3;
        d->shape[0] = s->cap; d->shape[1] = d->shape[2] = xy;
        d->strides[0] = n2; d->strides[1] = 1; d->strides[2] = xy;
        if (part < 2) { d->code = kDLUInt; d->bits = 8; }
        break;
    }
    case GVOM_PRODUCT_VOXEL_CHANGES: {                     // parts 0 .. 3 as frontiers (16), part 3 with 8 words
        if (part < 0 || part > 6) return false;
        char *const sums = s->mem + align256((size_t)s->cap * 32), *const cmap = sums + align256((size_t)s->cap * 16);
        char *const counts = cmap + align256((size_t)n2 * 4), *const rows4 = counts + 256;
        char *const codes = rows4 + align256((size_t)s->cap * 16), *const cols = codes + align256((size_t)n2 * s->zs);
        if (part == 0) { rows(s->mem, s->cap, 8); d->code = kDLInt; }
        else if (part == 1) { rows(sums, s->cap, 2); d->code = kDLInt; d->bits = 64; }
        else if (part == 2) { d->ptr = cmap; d->shape[0] = d->shape[1] = xy; d->strides[0] = 1; d->strides[1] = xy; d->code = kDLInt; }   // [x, y] indexing, column-major, like a device map
        else if (part == 3) { d->ptr = counts; d->ndim = 1; d->shape[0] = 8; d->strides[0] = 1; d->shape[1] = d->strides[1] = 1; d->code = kDLInt; }
        else if (part == 4) { rows(rows4, s->cap, 4); d->code = kDLInt; }
        else if (part == 5) {
            d->ptr = codes; d->ndim = 3; d->code = kDLUInt; d->bits = 8;
            d->shape[0] = d->shape[1] = xy; d->shape[2] = s->zs;
            d->strides[0] = xy * s->zs; d->strides[1] = s->zs; d->strides[2] = 1;
        }
        else {                                             // [k, x, y] indexing: every plane column-major, like a pose field's
            d->ptr = cols; d->ndim = 3; d->code = kDLUInt; d->bits = 16;
            d->shape[0] = 2; d->shape[1] = d->shape[2] = xy;
            d->strides[0] = n2; d->strides[1] = 1; d->strides[2] = xy;
        }
        break;
    }
    default: return false;
    }
    d->bytes = (size_t)(d->shape[0] * d->shape[1] * d->shape[2]) * (d->bits / 8);
    return true;
}
}  // namespace gvom_host
