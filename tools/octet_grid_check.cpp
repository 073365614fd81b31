// octet_grid_check.cpp — host check of octet_grid (csrc/octet_grid.hpp) against
// the grid arithmetic it replaced, kept here verbatim from the launchers that
// each wrote it out (launch_bf16_gs / launch_f16_gs, rows16_grid and
// launch_fold_f16, the one-block-per-tile macros).  Built and run by
// tests/test_host_stress.py; no GPU.
#include <stdio.h>

#include <initializer_list>

#include "octet_grid.hpp"

static int64_t g_cus;
static int64_t cu_count() { return g_cus; }

// launch_bf16_gs / launch_f16_gs
template <int C>
static void old_gs(int per_cu, int64_t P, int64_t& tiles_out, int64_t& g_out) {
    const int64_t per_block = (int64_t)kBlock * C, units = (P >> 3) + ((P & 7) ? 1 : 0);
    const int64_t tiles = (units + per_block - 1) / per_block;
    int64_t g = (int64_t)(per_cu > 0 ? per_cu : -per_cu) * cu_count();
    if (g > tiles) g = tiles;
    if (per_cu < 0) {
        const int64_t passes = (tiles + g - 1) / g;
        g = (tiles + passes - 1) / passes;
    }
    tiles_out = tiles;
    g_out = g;
}

// rows16_grid (launch_fold_f16 wrote the same lines with C = kFoldF16C)
template <int C>
static void rows16_grid(int64_t P, int64_t& tiles, int64_t& g) {
    const int64_t per_block = (int64_t)kBlock * C, units = (P >> 3) + ((P & 7) ? 1 : 0);
    tiles = (units + per_block - 1) / per_block;
    g = cu_count();
    if (g > tiles) g = tiles;
    const int64_t passes = (tiles + g - 1) / g;
    g = (tiles + passes - 1) / passes;
}

// FA_BF / FA_HF: one block per tile
template <int C>
static int64_t old_v8(int64_t P) {
    const int64_t per_block = (int64_t)kBlock * (C), units = (P >> 3) + ((P & 7) ? 1 : 0);
    return (units + per_block - 1) / per_block;
}

static int bad = 0;
static void expect(const char* what, int C, int per_cu, int64_t P, OctetGrid got, int64_t tiles, int64_t g) {
    if (got.tiles == tiles && got.grid == g) return;
    ++bad;
    fprintf(stderr, "%s C=%d per_cu=%d cus=%lld P=%lld: octet_grid (%lld, %lld), was (%lld, %lld)\n", what, C, per_cu,
            (long long)g_cus, (long long)P, (long long)got.tiles, (long long)got.grid, (long long)tiles, (long long)g);
}

template <int C>
static void check_c() {
    const int64_t edge = (int64_t)kBlock * C * 8;
    const int64_t Ps[] = {1, 7, 8, 9, 2047 * 8, edge - 1, edge, edge + 1, 1000000, 100000000};
    for (int64_t cus : {1, 8, 256}) {
        g_cus = cus;
        for (int64_t P : Ps) {
            int64_t tiles, g;
            for (int per_cu : {-1, 1, 4, -2}) {
                old_gs<C>(per_cu, P, tiles, g);
                expect("gs", C, per_cu, P, octet_grid(P, C, per_cu, cus), tiles, g);
            }
            rows16_grid<C>(P, tiles, g);
            expect("rows16", C, -1, P, octet_grid(P, C, -1, cus), tiles, g);
            expect("v8", C, 0, P, octet_grid(P, C, 0, cus), old_v8<C>(P), old_v8<C>(P));
        }
    }
}

int main() {
    check_c<1>();
    check_c<2>();
    check_c<4>();
    check_c<8>();
    if (bad) return 1;
    puts("octet_grid_check: ok");
    return 0;
}
