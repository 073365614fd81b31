// octet_grid.hpp — the launch geometry of the 16-bit octet kernels (bf16 and
// float16: 8 columns per 16-byte load).  Plain host arithmetic, free of HIP, so
// that a host program can check it (tools/octet_grid_check.cpp).
#pragma once
#include <stdint.h>

constexpr int kBlock = 256;  // lanes per block of every fold kernel

// Tiles of C octets per lane over P columns (the tile of the lane that folds
// the P % 8 tail columns included), and the grid over them on `cus` compute
// units:
//   per_cu == 0  one block per tile
//   per_cu > 0   per_cu blocks per CU, at most one per tile
//   per_cu < 0   -per_cu blocks per CU, then the fewest blocks that finish in
//                the same number of passes (balanced passes)
// lg: the columns of a 16-byte unit as a power of two (3: an octet; 1: a pair
// of float64, the float64 pair kernels).
struct OctetGrid {
    int64_t tiles, grid;
};
// The grid over `tiles` tiles by the per_cu rule above (0 tiles: an empty grid).
// octet_grid applies it to the tiles of one row; the layer-table folds
// (layer_plan.hpp) to the tiles of all the layers of a model.
inline int64_t tile_grid(int64_t tiles, int per_cu, int64_t cus) {
    if (tiles <= 0) return 0;
    if (per_cu == 0) return tiles;
    int64_t g = (int64_t)(per_cu > 0 ? per_cu : -per_cu) * cus;
    if (g > tiles) g = tiles;
    if (per_cu < 0) {
        const int64_t passes = (tiles + g - 1) / g;
        g = (tiles + passes - 1) / passes;
    }
    return g;
}
inline OctetGrid octet_grid(int64_t P, int C, int per_cu, int64_t cus, int lg = 3) {
    const int64_t per_block = (int64_t)kBlock * C, units = (P >> lg) + ((P & (((int64_t)1 << lg) - 1)) ? 1 : 0);
    const int64_t tiles = (units + per_block - 1) / per_block;
    return {tiles, tile_grid(tiles, per_cu, cus)};
}
