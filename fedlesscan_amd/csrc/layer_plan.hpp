// layer_plan.hpp — the host planner of the layer-table folds
// (fa_fedavg_*_layers): how the layers of a model tile one launch.  Plain host
// arithmetic, free of HIP (as octet_grid.hpp), behind fa_layers_plan.
//
// A layer whose every row is 16-B aligned is tiled as the row-table folds tile
// their one row: 16-byte units (4 fp32, 8 16-bit, 2 float64 columns), `units`
// of them per lane spaced kBlock lanes apart, the lane after the last full
// unit folding the trailing columns -- octet_grid's tile count.  Any other
// layer is tiled one column per lane, kBlock columns per tile.  tile0 is the
// prefix sum over the layers; a layer of 0 columns has 0 tiles.  Every layer
// starts at a multiple of 64 elements of the flat output (128 to 512 bytes),
// so an aligned output base keeps every layer's stores 16-B aligned.
#pragma once
#include <stdint.h>

#include "fedavg_hip.h"
#include "octet_grid.hpp"

constexpr int64_t kLayerOutAlign = 64;  // elements

inline int64_t layer_tiles(int64_t cols, bool aligned, int units, int unit_lg) {
    if (cols <= 0) return 0;
    if (!aligned) return (cols + kBlock - 1) / kBlock;
    return octet_grid(cols, units, 0, 1, unit_lg).tiles;
}

inline int64_t layers_total_tiles(const int64_t* cols, const int32_t* aligned, int64_t L, int units, int unit_lg) {
    int64_t t = 0;
    for (int64_t l = 0; l < L; ++l) t += layer_tiles(cols[l], aligned[l] != 0, units, unit_lg);
    return t;
}

// Units per lane: the most of 4, 2, 1 whose balanced grid (at most one block
// per CU) over the model's total tiles still covers 7/8 of the CUs, else 1 --
// pick_pairs' rule with the model's tiles in place of one row's.  Reasoned,
// not measured: the bytes in flight come from the width first.
inline int pick_layer_units(const int64_t* cols, const int32_t* aligned, int64_t L, int unit_lg, int64_t cus) {
    for (int c = 4; c > 1; c >>= 1)
        if (tile_grid(layers_total_tiles(cols, aligned, L, c, unit_lg), -1, cus) * 8 >= cus * 7) return c;
    return 1;
}

// plan[l] for `units` units per lane; returns the tile total, *elems = the
// length of the flat output
inline int64_t fill_layer_plan(const int64_t* cols, const int32_t* aligned, int64_t L, int units, int unit_lg,
                               fa_layer_plan* plan, int64_t* elems) {
    int64_t t = 0, off = 0;
    for (int64_t l = 0; l < L; ++l) {
        plan[l].cols = cols[l];
        plan[l].offset = off;
        plan[l].tile0 = t;
        plan[l].aligned = aligned[l] != 0;
        t += layer_tiles(cols[l], aligned[l] != 0, units, unit_lg);
        off += (cols[l] + kLayerOutAlign - 1) / kLayerOutAlign * kLayerOutAlign;
    }
    *elems = off;
    return t;
}
