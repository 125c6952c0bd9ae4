// CPU harness of tests/test_batch_plan.py: the host arithmetic of the flat batch driver (abpoa_amd/csrc/batch_plan.cpp) -- the direction-word tables against
// a naive double loop, eligibility for the fast row loops, the plan and the arenas of first and retry passes against the per-alignment routing rule
// (abpoa_amd/csrc/routing.h), the two blob layouts, and the unpacking of a saved arena into trace planes.  No GPU, no HIP runtime call; built with
// -fsanitize=undefined,address.  The LDS plan's sizes depend on lds_fixed_bytes_dp / _bt, which are stand-ins here: what is asserted of a routing is what
// DESIGN.md section 1 documents (w = b + f * length; wide row loop for 40 <= w <= 215, 343 in the long-read form; local row loop up to 575 columns; linear
// gaps on the narrow loop only) and what holds for any plan.
#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "engine_options.h"
#include "batch_plan.h"
#include "routing.h"

// (the snapshot a set_option replaces is left alone on purpose -- engine_options.h -- so the leak check would report every switch this harness flips)
extern "C" const char *__asan_default_options() { return "detect_leaks=0"; }

namespace abpoa_hip {
int lds_fixed_bytes_dp() { return 1024; }
int lds_fixed_bytes_bt() { return 2048; }
}  // namespace abpoa_hip
using namespace abpoa_hip;

static int g_fail = 0, g_checked = 0;
static std::string g_case;
#define CHECK(cond) do { g_checked++; if (!(cond)) { fprintf(stderr, "FAILED %s:%d [%s] %s\n", __FILE__, __LINE__, g_case.c_str(), #cond); g_fail++; } } while (0)

static std::vector<int32_t> g_mat;
static abpoa_hip_scoring_t scoring(int gap_mode, int align_mode = ABPOA_HIP_GLOBAL_MODE, int m = 5) {      // the reference's defaults: 2 / -4, 4 + 2 k, 24 + k, -b 10 -f 0.01
    abpoa_hip_scoring_t sc;
    g_mat.assign((size_t)m * m, -4); for (int i = 0; i < m; ++i) g_mat[(size_t)i * m + i] = 2;
    sc.m = m; sc.mat = g_mat.data(); sc.max_mat = 2; sc.min_mis = 4;
    sc.gap_open1 = gap_mode == ABPOA_HIP_LINEAR_GAP ? 0 : 4; sc.gap_ext1 = 2;
    sc.gap_open2 = gap_mode == ABPOA_HIP_CONVEX_GAP ? 24 : 0; sc.gap_ext2 = gap_mode == ABPOA_HIP_CONVEX_GAP ? 1 : 0;
    sc.align_mode = align_mode; sc.gap_mode = gap_mode; sc.wb = align_mode == ABPOA_HIP_LOCAL_MODE ? -1 : 10; sc.wf = 0.01f; sc.zdrop = 0; sc.ret_cigar = 1; sc.rev_cigar = 0;
    return sc;
}

// ---------------------------------------------------------------------------------------------------------------- tables
struct Csr {
    std::vector<int32_t> off{0}, pred;
    void row(std::vector<int> p) { for (int x : p) pred.push_back(x); off.push_back((int32_t)pred.size()); }
    int n() const { return (int)off.size() - 1; }
};
static Csr chain(int n) { Csr g; g.row({}); for (int r = 1; r < n; ++r) g.row({r - 1}); return g; }

// the tables by their definition (engine.h DevBatch.row_sdist / row_pd): per row the largest distance to a successor, capped at 255, 255 below the sink; per
// row a byte for each of the first eight predecessors, its distance or 255 where there is none or it is more than 254 rows back
static bool tables_check(const Csr &g) {
    const int n = g.n();
    std::vector<uint8_t> sd((size_t)n, 0xAB); std::vector<uint32_t> pd(2 * (size_t)n, 0xABABABABu);
    const bool words = fill_dir_tables(n, g.off.data(), g.pred.data(), sd.data(), pd.data());
    bool want_words = true;
    for (int p = 0; p < n; ++p) {
        int far = 0;
        for (int r = p + 1; r < n; ++r) for (int k = g.off[r]; k < g.off[r + 1]; ++k) if (g.pred[k] == p) far = std::max(far, r == n - 1 ? 255 : std::min(255, r - p));
        CHECK(sd[p] == far);
        uint8_t got[8]; memcpy(got, &pd[2 * (size_t)p], 8);      // (little-endian: byte t of the pair of dwords)
        const int np = g.off[p + 1] - g.off[p];
        for (int t = 0; t < 8; ++t) { const int dist = t < np ? p - g.pred[g.off[p] + t] : 255; CHECK(got[t] == (dist <= 254 ? dist : 255)); }
        if (np > DIR_K_MAX && p < n - 1) want_words = false;
    }
    CHECK(words == want_words);
    return words;
}

static void table_cases() {
    g_case = "tables: chain";
    {   Csr g = chain(40); CHECK(tables_check(g));
        std::vector<uint8_t> sd(40); std::vector<uint32_t> pd(80); fill_dir_tables(40, g.off.data(), g.pred.data(), sd.data(), pd.data());
        CHECK(sd[0] == 1 && sd[37] == 1 && sd[38] == 255 && sd[39] == 0 && pd[0] == 0xFFFFFFFFu && pd[2] == 0xFFFFFF01u && pd[3] == 0xFFFFFFFFu); }
    g_case = "tables: predecessors 1, 16, 254, 255 and 300 rows back";
    {   Csr g; g.row({}); for (int r = 1; r < 400; ++r) { if (r == 350) g.row({349, 334, 96, 95, 50}); else g.row({r - 1}); }
        CHECK(tables_check(g));
        std::vector<uint8_t> sd(400); std::vector<uint32_t> pd(800); fill_dir_tables(400, g.off.data(), g.pred.data(), sd.data(), pd.data());
        CHECK(pd[700] == 0xFFFE1001u && pd[701] == 0xFFFFFFFFu);      // 1, 16, 254, then "too far" twice
        CHECK(sd[334] == 16 && sd[96] == 254 && sd[95] == 255 && sd[50] == 255 && sd[349] == 1); }
    g_case = "tables: nine predecessors";
    {   Csr a, b; a.row({}); b.row({});
        for (int r = 1; r < 30; ++r) { if (r == 20) { a.row({10, 11, 12, 13, 14, 15, 16, 17}); b.row({10, 11, 12, 13, 14, 15, 16, 17, 19}); } else { a.row({r - 1}); b.row({r - 1}); } }
        CHECK(tables_check(a)); CHECK(tables_check(b));
        std::vector<uint8_t> sa(30), sb(30); std::vector<uint32_t> pa(60), pb(60);
        fill_dir_tables(30, a.off.data(), a.pred.data(), sa.data(), pa.data()); fill_dir_tables(30, b.off.data(), b.pred.data(), sb.data(), pb.data());
        CHECK(pa[40] == pb[40] && pa[41] == pb[41] && pa[40] == 0x0708090Au && pa[41] == 0x03040506u); }
    g_case = "tables: predecessor of the sink";
    {   Csr g = chain(10); g.pred.push_back(3); g.off[10] += 1;      // the sink (row 9) also names row 3
        CHECK(tables_check(g));
        std::vector<uint8_t> sd(10); std::vector<uint32_t> pd(20); fill_dir_tables(10, g.off.data(), g.pred.data(), sd.data(), pd.data());
        CHECK(sd[3] == 255 && sd[8] == 255 && sd[2] == 1); }
    g_case = "tables: sink with 20 predecessors";
    {   Csr g; g.row({}); for (int r = 1; r < 30; ++r) g.row({r - 1});
        std::vector<int> all; for (int r = 29; r >= 10; --r) all.push_back(r);
        g.row(all); CHECK(tables_check(g)); }
    g_case = "tables: non-sink row with 16 predecessors";
    {   Csr g; g.row({}); for (int r = 1; r < 30; ++r) g.row({r - 1});
        std::vector<int> all; for (int r = 29; r >= 14; --r) all.push_back(r);
        g.row(all); g.row({30}); CHECK(!tables_check(g));
        Csr h; h.row({}); for (int r = 1; r < 30; ++r) h.row({r - 1});
        all.pop_back(); h.row(all); h.row({30}); CHECK(tables_check(h)); }      // 15 = DIR_K_MAX: words apply
}

// ---------------------------------------------------------------------------------------------------------------- eligibility
static void eligibility_cases() {
    const int qlens[2] = {300, 200}; BatchShape sh[2]; AlnDesc desc[2]; ArenaCells cells[2];
    for (int i = 0; i < 2; ++i) sh[i] = BatchShape{qlens[i] + 2, qlens[i], qlens[i] + 1, qlens[i] + 1};
    auto run = [&](const abpoa_hip_scoring_t &sc, bool fresh, int inactive_row, int moved_row) {
        const PoolTotals T = describe_batch(&sc, 2, sh, desc, cells);
        std::vector<uint8_t> act((size_t)T.rows, 1); std::vector<int32_t> l((size_t)T.rows), r((size_t)T.rows, 0);
        for (int i = 0; i < 2; ++i) for (int k = 0; k < desc[i].n_rows; ++k) l[desc[i].row0 + k] = desc[i].n_rows;
        if (inactive_row >= 0) act[desc[1].row0 + inactive_row] = 0;
        if (moved_row >= 0) r[desc[1].row0 + moved_row] = 7;
        memset(&desc[0].flags, 0x55, 8);
        mark_fast_ok(&sc, fresh, 2, desc, act.data(), l.data(), r.data());
        CHECK(desc[0].pad0 == 0 && desc[1].pad0 == 0);
        return (desc[0].flags & ALN_FAST_OK ? 1 : 0) | (desc[1].flags & ALN_FAST_OK ? 2 : 0);
    };
    const abpoa_hip_scoring_t aff = scoring(ABPOA_HIP_AFFINE_GAP), loc = scoring(ABPOA_HIP_AFFINE_GAP, ABPOA_HIP_LOCAL_MODE);
    abpoa_hip_scoring_t glob_unbanded = aff; glob_unbanded.wb = -1;
    g_case = "eligibility";
    CHECK(run(aff, true, -1, -1) == 3 && run(aff, false, -1, -1) == 3);
    CHECK(run(aff, true, 5, -1) == 1 && run(aff, false, 201, -1) == 1);      // an inactive row: off the fast loops, the other alignment stays
    CHECK(run(aff, false, -1, 100) == 1);                                     // kept band, one row not at its reset value
    CHECK(run(aff, true, -1, 100) == 3);                                      // a fresh band ignores the band state
    CHECK(run(loc, false, -1, 100) == 3 && run(loc, true, 0, -1) == 1);       // unbanded local: on, band state not read
    CHECK(run(glob_unbanded, true, -1, -1) == 0);                             // unbanded global: off
}

// ---------------------------------------------------------------------------------------------------------------- passes
struct Want { int narrow = -1, wide = -1, local = -1, general = -1; };      // per alignment of the launch: bit i of a mask that must hold, -1 = not asserted
static int g_routed = 0;
static void pass_checks(const char *name, const abpoa_hip_scoring_t &sc, const std::vector<int> &qlens, const Want &want, const std::vector<int> &n_rows_of = {}) {
    const int n = (int)qlens.size();
    std::vector<BatchShape> sh((size_t)n);
    for (int i = 0; i < n; ++i) { const int gn = n_rows_of.empty() ? qlens[i] + 2 : n_rows_of[i]; sh[i] = BatchShape{gn, qlens[i], gn - 1, gn - 1}; }
    for (int variant = 0; variant < 4; ++variant) {      // plain | trace | ABPOA_HIP_DIR_WIDE=1 | ABPOA_HIP_NODIR=1
        g_case = std::string(name) + (variant == 0 ? "" : variant == 1 ? " (trace)" : variant == 2 ? " (DIR_WIDE)" : " (NODIR)");
        const unsigned flags = BS_FRESH_BAND | (variant == 1 ? BS_TRACE : 0);
        if (variant == 2) CHECK(set_option("ABPOA_HIP_DIR_WIDE", "1") == 0);
        if (variant == 3) CHECK(set_option("ABPOA_HIP_NODIR", "1") == 0);
        std::vector<AlnDesc> desc((size_t)n), pass((size_t)n); std::vector<ArenaCells> cells((size_t)n), cells55((size_t)n);
        CHECK(set_option("ABPOA_HIP_ARENA_PCT", "55") == 0);
        describe_batch(&sc, n, sh.data(), desc.data(), cells55.data());
        CHECK(set_option("ABPOA_HIP_ARENA_PCT", nullptr) == 0);
        const PoolTotals T = describe_batch(&sc, n, sh.data(), desc.data(), cells.data());
        std::vector<uint8_t> act((size_t)T.rows, 1);
        mark_fast_ok(&sc, true, n, desc.data(), act.data(), nullptr, nullptr);
        const bool dir = dir_words_for_run(&sc, flags);
        const bool words_fit = sc.wb >= 0 && sc.align_mode == ABPOA_HIP_GLOBAL_MODE && dir_plane_usable(sc.gap_mode, sc.gap_open1, sc.gap_ext1, sc.gap_open2, sc.gap_ext2);
        CHECK(dir == (words_fit && variant != 1 && variant != 3));
        int64_t pools = 0;
        for (int i = 0; i < n; ++i) {
            const int pn = desc[i].bits == 16 ? 16 : 8; const int64_t row = padded_width(desc[i].qlen, pn) * record_values(sc.gap_mode);
            CHECK(desc[i].row0 == pools && desc[i].poff0 == pools + i && desc[i].cigar_cap == desc[i].n_rows + desc[i].qlen + 8); pools += desc[i].n_rows;
            CHECK(desc[i].w == (sc.wb < 0 ? desc[i].qlen : sc.wb + (int)(sc.wf * (float)desc[i].qlen)));
            CHECK(cells[i].est <= cells[i].full && cells[i].dir_est <= cells[i].dir_full && cells[i].est == desc[i].plane_cap);
            // ABPOA_HIP_ARENA_PCT=55: a smaller first-pass arena wherever the band is narrower than the row, never below one row; full width untouched
            CHECK(cells55[i].est >= row && cells55[i].est <= cells[i].est && cells55[i].full == cells[i].full && cells55[i].dir_full == cells[i].dir_full);
            if (cells[i].est < cells[i].full) CHECK(cells55[i].est < cells[i].est && cells55[i].dir_est < cells[i].dir_est);
        }
        CHECK(T.rows == pools);
        std::vector<int> todo; for (int i = 0; i < n; ++i) todo.push_back(i);
        for (int first = 1; first >= 0; --first) {
            if (!first) todo.erase(todo.begin());      // a retry pass of the launch's other alignments
            if (todo.empty()) break;
            DevBatch b; memset(&b, 0x77, sizeof(b));
            plan_pass(&sc, flags, dir, desc.data(), todo, b);
            CHECK(b.n == (int)todo.size() && b.m == sc.m && b.wb == sc.wb && b.gap_mode == sc.gap_mode && b.align_mode == sc.align_mode && b.e1 == sc.gap_ext1 && b.o1 == sc.gap_open1);
            CHECK(b.want_trace == (variant == 1) && b.fresh_band == 1 && b.want_lr == (variant == 1) && b.ret_cigar == 1 && b.rev_cigar == 0 && b.dbg == 0 && b.planes == nullptr);
            CHECK(b.dir_mode == (dir ? (variant == 2 ? 2 : 1) : 0));
            int n_fast = -1; const int64_t total = assign_arenas(b, first != 0, cells.data(), todo, desc.data(), pass.data(), &n_fast);
            int tails = 0; int64_t at = 0;
            for (size_t t = 0; t < todo.size(); ++t) {
                const int i = todo[t]; const AlnDesc &d = pass[t];
                CHECK(memcmp(&d, &desc[i], sizeof(d)) == 0);
                const bool nar = for_narrow_kernel(b, d), wid = for_wide_kernel(b, d), loc = for_local_kernel(b, d), gen = for_general_kernel(b, d);
                CHECK((int)nar + (int)wid + (int)loc + (int)gen == 1);
                CHECK(for_tail_kernel(b, d) == (nar || wid || loc)); tails += for_tail_kernel(b, d) ? 1 : 0;
                if (b.lds.narrow_off) CHECK(!nar);
                if (b.lds.wide_on == 0) CHECK(!wid);
                if (!gen) CHECK(b.bits_mask & (d.bits == 16 ? 1 : 2));
                if (want.narrow >= 0) CHECK(nar == ((want.narrow >> i) & 1));
                if (want.wide >= 0) CHECK(wid == ((want.wide >> i) & 1));
                if (want.local >= 0) CHECK(loc == ((want.local >> i) & 1));
                if (want.general >= 0) CHECK(gen == ((want.general >> i) & 1));
                const bool dir_a = takes_fast(b, d) && takes_dir(b, d);
                if (!dir) CHECK(!dir_a);
                if (dir && variant == 2) CHECK(dir_a == (nar || wid));
                if (dir && variant != 2) CHECK(dir_a == nar);
                CHECK(d.plane_cap == (dir_a ? (first ? cells[i].dir_est : cells[i].dir_full) : (first ? cells[i].est : cells[i].full)));
                CHECK(d.plane_off == at && at % 256 == 0);
                const int64_t need = d.plane_cap * (d.bits / 8) + 64 * 8 * 4;      // the arena and 64 records of slack
                at += (need + 255) / 256 * 256;
                g_routed++;
            }
            CHECK(n_fast == tails && at == total);
        }
        if (variant == 2) CHECK(set_option("ABPOA_HIP_DIR_WIDE", nullptr) == 0);
        if (variant == 3) CHECK(set_option("ABPOA_HIP_NODIR", nullptr) == 0);
    }
}

static void pass_cases() {      // -b 10 -f 0.01: w = 10 + length / 100
    const abpoa_hip_scoring_t aff = scoring(ABPOA_HIP_AFFINE_GAP), cvx = scoring(ABPOA_HIP_CONVEX_GAP), lin = scoring(ABPOA_HIP_LINEAR_GAP);
    const abpoa_hip_scoring_t loc = scoring(ABPOA_HIP_AFFINE_GAP, ABPOA_HIP_LOCAL_MODE, 27);
    Want w; w.narrow = 1; w.wide = 2; w.general = 0;
    pass_checks("w 20 beside w 84", aff, {1000, 7400}, w);
    pass_checks("w 39 beside w 40", aff, {2900, 3000}, w);
    pass_checks("w 39 beside w 40, convex", cvx, {2900, 3000}, w);
    abpoa_hip_scoring_t b143 = aff; b143.wb = 143;                // (-b 143: these half-widths at 7.2 kb .. 20.1 kb, inside the fast loops' query range)
    Want xl; xl.wide = 7;                                       // 215, 216 and 343 take the wide loop (the long-read form from 216 on), 344 does not
    pass_checks("w 215, 216, 343, 344", b143, {7200, 7300, 20000, 20100}, xl);
    g_case = "NOXL"; CHECK(set_option("ABPOA_HIP_NOXL", "1") == 0);
    Want noxl; noxl.wide = 1;                                   // without the long-read form the wide loop ends at 215
    pass_checks("w 215, 216, 343, 344 without the long-read form", b143, {7200, 7300, 20000, 20100}, noxl);
    g_case = "NOXL"; CHECK(set_option("ABPOA_HIP_NOXL", nullptr) == 0);
    Want l; l.narrow = 1; l.wide = 0; l.general = 2;            // linear gaps: the narrow loop only
    pass_checks("linear w 39 beside w 40", lin, {2900, 3000}, l);
    Want lo; lo.local = 1; lo.general = 2; lo.narrow = 0; lo.wide = 0;
    pass_checks("local 575 beside 576", loc, {575, 576}, lo);
    // an int16 alignment beside an int32 one: the score width follows rows and length (abpoa_hip_score_bits)
    {   int32_t inf; CHECK(abpoa_hip_score_bits(&aff, 1002, 1000, &inf) == 16 && abpoa_hip_score_bits(&aff, 60000, 1000, &inf) == 32);
        Want m; m.narrow = 3; m.general = 0;
        pass_checks("int16 beside int32", aff, {1000, 1000}, m, {1002, 60000}); }
    CHECK(g_routed > 100);
}

// ---------------------------------------------------------------------------------------------------------------- layouts
static void layout_cases() {
    g_case = "layouts";
    const abpoa_hip_scoring_t sc = scoring(ABPOA_HIP_AFFINE_GAP);
    for (int n : {1, 3, 7}) {
        std::vector<BatchShape> sh; for (int i = 0; i < n; ++i) sh.push_back(BatchShape{101 + 37 * i, 99 + 37 * i, 150 + i, 160 + i});
        std::vector<AlnDesc> desc((size_t)n); std::vector<ArenaCells> cells((size_t)n);
        const PoolTotals T = describe_batch(&sc, n, sh.data(), desc.data(), cells.data());
        const InLayout I = layout_in(n, sc.m, T); const OutLayout O = layout_out(n, T);
        // every region in order, with the bytes it must hold: its pool and its slack (+ n on the offset pools, + 1 on the predecessor pool, + 1 and 512 entries
        // on out_row, + 1 on the query)
        const size_t in_at[14] = {I.desc, I.mat, I.query, I.base, I.sdist, I.pd, I.nid, I.rem, I.act, I.poff, I.pred, I.ooff, I.out, I.bytes};
        const size_t in_need[13] = {sizeof(AlnDesc) * n, 4u * sc.m * sc.m, (size_t)T.q + 1, (size_t)T.rows, (size_t)T.rows, 8 * (size_t)T.rows, 4 * (size_t)T.rows, 4 * (size_t)T.rows,
                                    (size_t)T.rows, 4 * (size_t)(T.rows + n), 4 * (size_t)(T.preds + 1), 4 * (size_t)(T.rows + n), 4 * (size_t)(T.outs + 1 + 512)};
        CHECK(in_at[0] == 0);
        for (int k = 0; k < 13; ++k) CHECK(in_at[k] % 256 == 0 && in_at[k + 1] >= in_at[k] + in_need[k] && in_at[k + 1] - in_at[k] < in_need[k] + 256);
        // output blob: records and cigars first, then left, right, then the per-row trace arrays
        const size_t out_at[9] = {O.rec, O.cig, O.left, O.right, O.bsn, O.esn, O.coff, O.rmi, O.bytes};
        const size_t out_need[8] = {sizeof(AlnOut) * n, 8 * (size_t)T.cig, 4 * (size_t)T.rows, 4 * (size_t)T.rows, 4 * (size_t)T.rows, 4 * (size_t)T.rows, 8 * (size_t)T.rows, 4 * (size_t)T.rows};
        CHECK(out_at[0] == 0);
        for (int k = 0; k < 8; ++k) CHECK(out_at[k] % 256 == 0 && out_at[k + 1] >= out_at[k] + out_need[k] && out_at[k + 1] - out_at[k] < out_need[k] + 256);
        // the three downloads are prefixes: up to left, up to dp_beg_sn, everything
        CHECK(O.download_bytes(true, 0) == O.left && O.download_bytes(false, BS_WANT_BAND_STATE) == O.left && O.download_bytes(true, BS_FRESH_BAND) == O.left);
        CHECK(O.download_bytes(true, BS_WANT_BAND_STATE) == O.bsn);
        CHECK(O.download_bytes(true, BS_TRACE) == O.bytes && O.download_bytes(false, BS_TRACE | BS_WANT_BAND_STATE) == O.bytes);
        // the slots of every problem lie inside their regions, one behind the other
        std::vector<uint8_t> hi(I.bytes), ho(O.bytes);
        for (int i = 0; i < n; ++i) {
            const ProblemSlots s = problem_slots(I, O, desc[i], hi.data(), ho.data()); const AlnDesc &d = desc[i];
            const ProblemSlots e = i + 1 < n ? problem_slots(I, O, desc[i + 1], hi.data(), ho.data()) : ProblemSlots{hi.data() + I.query + T.q, hi.data() + I.base + T.rows,
                    (int32_t *)(hi.data() + I.nid) + T.rows, (int32_t *)(hi.data() + I.rem) + T.rows, hi.data() + I.act + T.rows, (int32_t *)(hi.data() + I.poff) + T.rows + n,
                    (int32_t *)(hi.data() + I.pred) + T.preds, (int32_t *)(hi.data() + I.ooff) + T.rows + n, (int32_t *)(hi.data() + I.out) + T.outs,
                    (int32_t *)(ho.data() + O.left) + T.rows, (int32_t *)(ho.data() + O.right) + T.rows};
            CHECK(s.query + d.qlen == e.query && s.row_base + d.n_rows == e.row_base && s.row_node_id + d.n_rows == e.row_node_id && s.row_remain + d.n_rows == e.row_remain);
            CHECK(s.row_active + d.n_rows == e.row_active && s.pred_off + d.n_rows + 1 == e.pred_off && s.pred_row + sh[i].n_pred == e.pred_row);
            CHECK(s.out_off + d.n_rows + 1 == e.out_off && s.out_row + sh[i].n_out == e.out_row && s.left + d.n_rows == e.left && s.right + d.n_rows == e.right);
            if (i == 0) CHECK(s.query == hi.data() + I.query && s.pred_off == (int32_t *)(hi.data() + I.poff) && s.left == (int32_t *)(ho.data() + O.left));
        }
        DevBatch b; memset(&b, 0, sizeof(b)); uint8_t *di = hi.data(), *dout = ho.data(), planes[1];
        bind_pools(b, I, O, di, dout, planes);
        CHECK((const uint8_t *)b.aln == di + I.desc && (const uint8_t *)b.mat == di + I.mat && b.query == di + I.query && b.row_base == di + I.base && b.row_sdist == di + I.sdist);
        CHECK((const uint8_t *)b.row_pd == di + I.pd && (const uint8_t *)b.row_node_id == di + I.nid && (const uint8_t *)b.row_remain == di + I.rem && b.row_active == di + I.act);
        CHECK((const uint8_t *)b.pred_off == di + I.poff && (const uint8_t *)b.pred_row == di + I.pred && (const uint8_t *)b.out_off == di + I.ooff && (const uint8_t *)b.out_row == di + I.out);
        CHECK((uint8_t *)b.out == dout + O.rec && (uint8_t *)b.cigar == dout + O.cig && (uint8_t *)b.left == dout + O.left && (uint8_t *)b.right == dout + O.right);
        CHECK((uint8_t *)b.dp_beg_sn == dout + O.bsn && (uint8_t *)b.dp_end_sn == dout + O.esn && (uint8_t *)b.row_cell_off == dout + O.coff && (uint8_t *)b.row_max_i == dout + O.rmi);
        CHECK(b.planes == planes);
    }
}

// ---------------------------------------------------------------------------------------------------------------- trace unpacking
static void free_trace(abpoa_hip_trace_t &T) { free(T.dp_beg); free(T.dp_end); free(T.dp_beg_sn); free(T.dp_end_sn); free(T.row_off); free(T.planes); free(T.row_max_i); }
static int64_t plane_at(const abpoa_hip_trace_t &T, int64_t k) { return T.bits == 16 ? (int64_t)((const int16_t *)T.planes)[k] : (int64_t)((const int32_t *)T.planes)[k]; }

// A three-row alignment (source, one node, sink) of an affine job: rows 0 and 1 one vector wide, the sink never computed.  The arena is written by hand in
// the format `cw` names: row 0 at cell 0, row 1 behind a gap of 4 cells
static void trace_case(int bits, int cw, bool banded, bool row1_computed) {
    g_case = "trace unpacking, " + std::to_string(bits) + " bits, cw " + std::to_string(cw) + (banded ? "" : ", no band") + (row1_computed ? "" : ", row 1 never computed");
    const int P = 3, pn = bits == 16 ? 16 : 8, W = pn, S = bits / 8;
    AlnDesc d; memset(&d, 0, sizeof(d)); d.n_rows = 3; d.qlen = 11; d.bits = bits;
    const int32_t bsn[3] = {0, row1_computed ? 0 : -1, 0}, esn[3] = {0, row1_computed ? 0 : -1, 0}, rmi[3] = {9, 4, 6};
    const int stride = cw > 0 ? cw : P;                 // cells of the score width per column
    const int64_t coff[3] = {0, (int64_t)W * stride + 4, 0};
    std::vector<uint32_t> store(256, 0xDEADBEEFu); uint8_t *arena = (uint8_t *)store.data();      // (32-bit aligned, as the saved arenas are)
    auto put = [&](int64_t cell, int64_t v) { if (bits == 16) ((int16_t *)arena)[cell] = (int16_t)v; else ((int32_t *)arena)[cell] = (int32_t)v; };
    auto val = [&](int rr, int pl, int x) { return (int64_t)(1000 * rr + 100 * pl + x - 7); };
    auto word = [&](int x) { return (uint32_t)(0x8001u + 0x10203u * (uint32_t)x); };      // (high bit of the low half set: the sign must not leak into plane 1)
    for (int rr = 0; rr < 2; ++rr) for (int pl = 0; pl < P; ++pl) for (int x = 0; x < W; ++x) {
        if (cw == 0) put(coff[rr] + (int64_t)pl * W + x, val(rr, pl, x));
        if (cw > 0) put(coff[rr] + (int64_t)x * cw + pl, val(rr, pl, x));
    }
    if (cw < 0) for (int x = 0; x < W; ++x) { uint8_t *src = arena + coff[1] * S; if (cw == -2) ((uint16_t *)src)[x] = (uint16_t)word(x); else ((uint32_t *)src)[x] = word(x); }
    abpoa_hip_trace_t T; memset(&T, 0, sizeof(T));
    unpack_trace(d, P, banded, cw, bsn, esn, coff, rmi, arena, &T);
    CHECK(T.bits == bits && T.n_planes == P);
    const int64_t row_cells = (int64_t)W * P;
    CHECK(T.row_off[0] == 0 && T.row_off[1] == row_cells && T.row_off[2] == (row1_computed ? 2 : 1) * row_cells && T.row_off[3] == T.row_off[2]);
    CHECK(T.dp_beg_sn[0] == 0 && T.dp_end_sn[0] == 0 && T.dp_beg[0] == 0 && T.dp_end[0] == pn - 1 && T.row_max_i[0] == -2);
    if (row1_computed) CHECK(T.dp_beg_sn[1] == 0 && T.dp_end_sn[1] == 0 && T.dp_beg[1] == 0 && T.dp_end[1] == (banded ? pn - 1 : d.qlen) && T.row_max_i[1] == 4);
    else CHECK(T.dp_beg_sn[1] == -1 && T.dp_end_sn[1] == -1 && T.dp_beg[1] == -1 && T.dp_end[1] == -1 && T.row_max_i[1] == -2);
    CHECK(T.dp_beg_sn[2] == -1 && T.dp_end_sn[2] == -1 && T.dp_beg[2] == -1 && T.dp_end[2] == -1 && T.row_max_i[2] == -2);      // the sink: never computed
    int bad = 0;
    for (int rr = 0; rr < (row1_computed ? 2 : 1); ++rr) for (int pl = 0; pl < P; ++pl) for (int x = 0; x < W; ++x) {
        const int64_t got = plane_at(T, T.row_off[rr] + (int64_t)pl * W + x); int64_t exp;
        if (cw >= 0) exp = val(rr, pl, x);
        else if (rr == 0) exp = 0;                                                                   // row 0 has no words
        else if (pl == 0) exp = bits == 16 ? (int64_t)(int16_t)(cw == -2 ? (uint16_t)word(x) : word(x)) : (int64_t)(int32_t)(cw == -2 ? (uint32_t)(uint16_t)word(x) : word(x));
        else if (pl == 1 && bits == 16 && cw == -4) exp = (int64_t)(int16_t)(word(x) >> 16);         // 32-bit words in 16-bit planes: the high half
        else exp = 0;
        if (got != exp) bad++;
    }
    CHECK(bad == 0);
    free_trace(T);
}

static void trace_cases() {
    for (int bits : {16, 32}) for (int cw : {0, 4, 8, -2, -4}) for (int banded = 0; banded < 2; ++banded) for (int computed = 0; computed < 2; ++computed)
        trace_case(bits, cw, banded != 0, computed != 0);
}

int main() {
    // (the harness owns every switch it tests: nothing inherited from the environment)
    for (const char *sw : {"ABPOA_HIP_NODIR", "ABPOA_HIP_NOWIDE", "ABPOA_HIP_WIDE_LO", "ABPOA_HIP_NOFAST", "ABPOA_HIP_NOXL", "ABPOA_HIP_RING_ROWS", "ABPOA_HIP_DIR_WIDE",
                           "ABPOA_HIP_DIRTRACE", "ABPOA_HIP_DBG", "ABPOA_HIP_ARENA_PCT", "ABPOA_HIP_VERBOSE"}) unsetenv(sw);
    refresh_options();
    table_cases();
    eligibility_cases();
    pass_cases();
    layout_cases();
    trace_cases();
    if (g_fail) { fprintf(stderr, "%d of %d checks failed\n", g_fail, g_checked); return 1; }
    printf("batch plan ok (%d checks, %d descriptors routed)\n", g_checked, g_routed);
    return 0;
}
