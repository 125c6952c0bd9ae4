// Stand-alone harness for tests/test_tail_schedule.py: the start rows of the backtrack's helper walks (abpoa_amd/csrc/tail_schedule.h), the very function
// the kernels call, on every row count from dir_walk_pair's 768 rows to 70 000.  No GPU, no HIP runtime call.  Exit status 0 and "tail schedule ok" when all hold.
//   tail_schedule                the checks
//   tail_schedule N [N ...]      prints "N R1 R2 R3" for each row count (tests/test_gpu_tail_final_pass.py picks its read lengths with it)
#include <stdio.h>
#include <stdlib.h>
#include "tail_schedule.h"

using namespace abpoa_hip;

static int n_bad = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++n_bad <= 20) { fprintf(stderr, "FAILED %s: ", #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

int main(int argc, char **argv) {
    if (argc > 1) {
        for (int a = 1; a < argc; ++a) { const int n = atoi(argv[a]); printf("%d %d %d %d\n", n, spec_start_row(true, n, 1), spec_start_row(true, n, 2), spec_start_row(true, n, 3)); }
        return 0;
    }
    static_assert(SPEC_WK == 4 && SPEC_PM_ROWS == 256, "three helpers, tables of 256 rows");
    static_assert(SPEC_TILE == 64 && SPEC_MAIN_ROWS == 64, "tile-aligned start rows, a main walk of 64 .. 127 rows");
    int first_three = 0;
    for (int n = 768; n <= 70000; ++n) {
        int R[SPEC_WK];
        R[0] = n - 1;      // (the sink's row: where the main walk starts, one edge above its first cell)
        for (int r = 1; r < SPEC_WK; ++r) R[r] = spec_start_row(true, n, r);
        for (int r = 1; r < SPEC_WK; ++r) {
            CHECK(R[r] >= 1 && R[r] <= n - 2, "n %d helper %d start row %d", n, r, R[r]);
            CHECK(R[r] < R[r - 1], "n %d helper %d start row %d not below %d", n, r, R[r], R[r - 1]);
            CHECK((R[r] + 1) % SPEC_TILE == 0, "n %d helper %d start row %d is not the last row of a tile", n, r, R[r]);
            CHECK(R[r] == spec_early_start_row(n, r), "n %d helper %d", n, r);
            // late start: quarters of the graph, as before
            CHECK(spec_start_row(false, n, r) == (int)(((long long)n * (4 - r)) / 4), "n %d helper %d late start row %d", n, r, spec_start_row(false, n, r));
        }
        const int main_rows = n - 1 - R[1];
        CHECK(main_rows >= SPEC_MAIN_ROWS && main_rows <= SPEC_MAIN_ROWS + SPEC_TILE - 1, "n %d main walk of %d rows", n, main_rows);
        if (!first_three && R[1] > R[2] && R[2] > R[3] && R[3] >= 1) first_three = n;
        // the header's own arithmetic (a step costs a third of a row; helper r is released n - 1 - R_r rows before the end): helpers 1 and 2 are done before
        // the row loop is in every graph, helper 3 in graphs of up to 3 000 rows (beyond, the rows nobody can walk in time are its)
        for (int r = 1; r < SPEC_WK; ++r) {
            const int walk = R[r] - (r + 1 < SPEC_WK ? R[r + 1] : 0), time3 = 3 * (n - 1 - R[r]);
            if (n <= 3000 || r < 3) CHECK(walk <= time3, "n %d helper %d walks %d rows in the time of %d steps", n, r, walk, time3);
        }
    }
    CHECK(first_three == 768, "three distinct start rows first at %d rows", first_three);
    // below the helpers' threshold the function still answers (nobody asks it there): a row inside the graph or 0 = "no helper", never a row out of range
    for (int n = 1; n < 768; ++n) for (int r = 1; r < SPEC_WK; ++r) { const int R = spec_start_row(true, n, r); CHECK(R == 0 || (R >= 1 && R <= n - 2), "n %d helper %d start row %d", n, r, R); }
    for (int x = 0; x < (1 << 24); x += (x < 70000 ? 1 : 997)) { const long long s = spec_isqrt(x); CHECK(s * s <= x && (s + 1) * (s + 1) > x, "isqrt(%d) = %lld", x, s); }
    if (n_bad) { fprintf(stderr, "%d checks failed\n", n_bad); return 1; }
    printf("tail schedule ok\n");
    return 0;
}
