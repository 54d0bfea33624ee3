// gvom_travcost.h -- the traversal cost of ONE cell (include/gvom_hip.h "cost-to-go fields", COST), shared by k_travcost
// (gvom_costfield.hip: a map set, [y][x]) and k_atlas_travcost (gvom_atlas_field.hip: the atlas's toroidal planes), so that the two
// rules cannot drift apart.  ATLAS = false is the map-set rule as it has always been.  ATLAS = true adds what "atlas fields" says an
// atlas needs, because gvom_atlas_integrate lets any bit pattern in: never observed is visibility <= 0 (the atlas's rank < 2; == 0 in
// a map set), and an unblocked cost is at least 1 (only a negative `positive` could take it lower).  A NaN roughness gives q = 0 under
// both: r > min_roughness is false.  s: the cell's index in the four maps; u: its index in d2 (the same in a map set, the unwrapped
// one beside toroidal planes).  A map that a parameter switches off is not read.
#pragma once
#include "gvom_device.h"

struct TravParams {
    double thr, rmin, rmax;
    int32_t infl2, base, soft, unknown, rough;
    int32_t use_neg, unknown_blocks;
};

template <bool ATLAS, typename IDX>
__device__ __forceinline__ uint16_t trav_cell(const TravParams &P, const int32_t *__restrict__ pos, const int32_t *__restrict__ neg,
                                              const int32_t *__restrict__ vis, const double *__restrict__ rough,
                                              const int32_t *__restrict__ d2, const IDX s, const IDX u)
{
    const int32_t p = pos[s], v = vis[s];
    bool blocked = (double)p > P.thr;
    if (P.use_neg) blocked = blocked || neg[s] > 0;
    if (P.infl2 > 0) blocked = blocked || d2[u] <= P.infl2;
    if (P.unknown_blocks) blocked = blocked || (ATLAS ? v <= 0 : v == 0);
    int64_t q = 0;
    if (P.rough > 0) {
        const double r = rough[s];
        if (r > P.rmin) q = (int64_t)floor(((py_mind(r, P.rmax) - P.rmin) / (P.rmax - P.rmin)) * 100.0);
    }
    int64_t cost = (int64_t)P.base + (int64_t)P.soft * p + ((ATLAS ? v <= 0 : v == 0) ? (int64_t)P.unknown : 0) + (int64_t)P.rough * q;
    cost = cost > 65535 ? 65535 : cost;
    if (ATLAS) cost = cost < 1 ? 1 : cost;
    return blocked ? (uint16_t)0 : (uint16_t)cost;
}
