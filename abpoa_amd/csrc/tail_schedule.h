// Where the helper walks of the direction-plane backtrack start (backtrack_dir.h): the start row of helper 1..3 as a function of the graph's row count alone.
// The kernels call it, tests/tail_schedule.cpp walks it on the host over every row count.  Host and device code, no HIP runtime call.
#pragma once
#include "engine.h"

namespace abpoa_hip {

constexpr int SPEC_TILE = 64;           // rows between two writes of the row loop's progress word (rows_fast.h: once per tile switch)
constexpr int SPEC_MAIN_ROWS = 64;      // fewest rows between helper 1's start row and the sink: the main walk has SPEC_MAIN_ROWS .. SPEC_MAIN_ROWS + SPEC_TILE - 1

// late start (all four walks begin behind the row loop): quarters of the graph
__host__ __device__ inline int spec_late_start_row(const int gn, const int r) { return (int)(((long long)gn * (SPEC_WK - r)) / SPEC_WK); }

__host__ __device__ inline int spec_isqrt(const int x) {      // floor(sqrt(x)), x < 2^24 (exact in a float)
    int s = (int)__builtin_sqrtf((float)x);
    while (s * s > x) --s;
    while ((s + 1) * (s + 1) <= x) ++s;
    return s;
}
// the highest row R <= raw with R + 1 a multiple of SPEC_TILE: the tile switch that completes R releases it at once
__host__ __device__ inline int spec_tile_row(const int raw) { return ((raw + 1) & ~(SPEC_TILE - 1)) - 1; }

// EARLY START (the helpers walk while the row loop still runs).  D_r = gn - 1 - R_r is the time helper r has, in rows of the row loop, before the last row is
// done; a step of a walk costs about a third of a row, so a helper is done in time when the rows it walks, R_r - R_(r+1), are under three times D_r.
//   * helper 1: the last tile boundary that leaves the main walk SPEC_MAIN_ROWS rows, D_1 in [64, 127]: all that is left behind the last row is that walk.
//   * helper 3: D_3 = gn / 3 -- it walks two thirds of the graph in the time of one third, two rows of walk per row of time;
//   * helper 2: D_2 = sqrt(D_1 D_3), so that helpers 1 and 2 have the same ratio of walk to time, (D_2 - D_1) / D_1 = (D_3 - D_2) / D_2: 1.0 at 768 rows at
//     most, 1.5 - 2.5 at 2 400, 3 from about 3 000 rows on where D_1 is 64;
//   * all three on tile boundaries (rounded down: more time, and a longer walk for the helper above), strictly decreasing, 1 <= R <= gn - 2;
//   * helpers 1 and 2 never walk more than three rows per row of their time: the helper below moves up a tile at a time until that holds.  In graphs of more
//     than 3 000 rows this leaves helper 3 the rows it cannot walk in time, and the main walk waits for it, as it always could.
// 0: no such row (graphs far below dir_walk_pair's 768 rows) -- the helper reports "no helper".
__host__ __device__ inline int spec_early_start_row(const int gn, const int r) {
    const int r1 = ((gn - SPEC_MAIN_ROWS) & ~(SPEC_TILE - 1)) - 1;
    if (gn < 2 * SPEC_TILE + SPEC_MAIN_ROWS || gn >= (1 << 24) / (SPEC_MAIN_ROWS + SPEC_TILE)) return 0;
    if (r == 1) return r1;
    const int d1 = gn - 1 - r1, d3 = gn / 3 > d1 ? gn / 3 : d1, d2 = spec_isqrt(d1 * d3);
    int r2 = spec_tile_row(gn - 1 - d2); if (r2 > r1 - SPEC_TILE) r2 = r1 - SPEC_TILE;
    if (r1 - r2 > ((3 * d1) & ~(SPEC_TILE - 1))) r2 = r1 - ((3 * d1) & ~(SPEC_TILE - 1));      // (3 d1 >= 192: at least a tile below r1)
    if (r == 2) return r2 >= 1 ? r2 : 0;
    int r3 = spec_tile_row(gn - 1 - d3); if (r3 > r2 - SPEC_TILE) r3 = r2 - SPEC_TILE;
    if (r2 - r3 > ((3 * (gn - 1 - r2)) & ~(SPEC_TILE - 1))) r3 = r2 - ((3 * (gn - 1 - r2)) & ~(SPEC_TILE - 1));
    return r3 >= 1 ? r3 : 0;
}
__host__ __device__ inline int spec_start_row(const bool early, const int gn, const int r) { return early ? spec_early_start_row(gn, r) : spec_late_start_row(gn, r); }

}  // namespace abpoa_hip
