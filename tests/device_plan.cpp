// CPU harness of tests/test_device_plan.py: the planning step of the device-resident driver (abpoa_amd/csrc/msa_device_plan.cpp) on synthetic read-length lists,
// and the typed switch accessors of engine_options.cpp.  No GPU, no HIP runtime call; built with -fsanitize=undefined,address.
// The expected routing is what DESIGN.md section 1 and section 4.7 document (w = b + f * length; wide row loop for 40 <= w <= 215 -- 343 in the long-read form
// --; local row loop up to 575 columns; ragged sets: spread over max(64, longest / 8) becomes extra columns; linear gaps on the narrow loop only ...).
// Every planned job is also held against the kernels' per-alignment routing rule (abpoa_amd/csrc/routing.h): routing_checks below.
// Only plan fields that do not depend on lds_fixed_bytes_dp / _bt are asserted: the two values below are stand-ins for the kernels' own.
#include <algorithm>
#include <atomic>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <thread>
#include <vector>
#include "engine_options.h"
#include "msa_device_plan.h"
#include "routing.h"

// (the snapshot a set_option replaces is left alone on purpose -- engine_options.h -- so the leak check would report every switch this harness flips)
extern "C" const char *__asan_default_options() { return "detect_leaks=0"; }

namespace abpoa_hip {
int lds_fixed_bytes_dp() { return 1024; }
int lds_fixed_bytes_bt() { return 2048; }
}  // namespace abpoa_hip
using namespace abpoa_hip;

static int g_fail = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "FAILED %s:%d [%s] %s\n", __FILE__, __LINE__, g_case.c_str(), #cond); g_fail++; } } while (0)
static std::string g_case;

struct Sets {      // read-sets by lengths alone: the plan never looks at a base
    std::vector<std::vector<int32_t>> lens; std::vector<abpoa_hip_readset_t> rs;
    void add(std::vector<int32_t> l) { lens.push_back(std::move(l)); }
    void uniform(int n_sets, int n_reads, int len) { for (int s = 0; s < n_sets; ++s) add(std::vector<int32_t>((size_t)n_reads, len)); }
    const abpoa_hip_readset_t *get() {
        rs.resize(lens.size());
        for (size_t s = 0; s < lens.size(); ++s) { rs[s].n_reads = (int)lens[s].size(); rs[s].seqs = nullptr; rs[s].lens = lens[s].data(); rs[s].weights = nullptr; }
        return rs.data();
    }
    int n() const { return (int)lens.size(); }
};

static std::vector<int32_t> g_mat;
static abpoa_hip_scoring_t scoring(int gap_mode, int align_mode = ABPOA_HIP_GLOBAL_MODE, int m = 5) {      // the reference's defaults: 2 / -4, 4 + 2 k, 24 + k, -b 10 -f 0.01
    abpoa_hip_scoring_t sc;
    g_mat.assign((size_t)m * m, -4); for (int i = 0; i < m; ++i) g_mat[(size_t)i * m + i] = 2;
    sc.m = m; sc.mat = g_mat.data(); sc.max_mat = 2; sc.min_mis = 4;
    sc.gap_open1 = gap_mode == ABPOA_HIP_LINEAR_GAP ? 0 : 4; sc.gap_ext1 = 2;
    sc.gap_open2 = gap_mode == ABPOA_HIP_CONVEX_GAP ? 24 : 0; sc.gap_ext2 = gap_mode == ABPOA_HIP_CONVEX_GAP ? 1 : 0;
    sc.align_mode = align_mode; sc.gap_mode = gap_mode; sc.wb = 10; sc.wf = 0.01f; sc.zdrop = 0; sc.ret_cigar = 1; sc.rev_cigar = 0;
    return sc;
}

// The plan's job-level answers against the per-alignment rule of the kernels (routing.h): the launch's DevBatch as msa_device.cpp fill_dev_batch builds it, and
// for every set and every read length in it the round's AlnDesc as poa_bodies.h poa_prepare_body builds it, at the score widths of the first round (three graph
// rows) and of the set's node slots.  A job that the driver would hand back to the host (final_lds_plan fails, no fast row loop in the final plan) has no launch.
// known_e: sets for which (e) is a known disagreement of today's rules (LOG.md); it is asserted as such, so that a fix has to come here
static int g_routed = 0;
static void routing_checks(const DevicePlan &P, Sets &S, const std::vector<int> &known_e = {}) {
    const abpoa_hip_scoring_t *sc = &P.sc;
    DevBatch b; memset(&b, 0, sizeof(b)); b.n = S.n(); b.m = sc->m;
    if (final_lds_plan(P, S.n(), S.get(), b)) return;
    if (!P.local && !P.general && !fast_loop_fits(b.lds, P.max_qlen)) return;
    set_job_fields(b, *sc); b.dir_mode = P.dir ? (P.dir_wide ? 2 : 1) : 0; b.dbg = 0;
    CHECK(P.set_wide.size() == P.ps.size() && P.set_dir.size() == P.ps.size());
    bool all_local = true, any_wide = false;
    for (int s = 0; s < S.n(); ++s) {
        int longest = 0; for (int l : S.lens[s]) longest = std::max(longest, l);
        any_wide |= P.set_wide[s] != 0;
        for (int qlen : S.lens[s]) for (int n_rows : {3, (int)P.ps[s].node_cap}) {
            AlnDesc d; memset(&d, 0, sizeof(d));
            d.n_rows = n_rows; d.qlen = qlen; d.bits = abpoa_hip_score_bits(sc, n_rows, qlen, &d.inf_min);
            d.w = sc->wb < 0 ? qlen : sc->wb + (int)(sc->wf * (float)qlen);
            d.flags = P.general ? 0 : ALN_FAST_OK; d.pad0 = P.ps[s].band_extra;
            const bool nar = for_narrow_kernel(b, d), wid = for_wide_kernel(b, d), loc = for_local_kernel(b, d), gen = for_general_kernel(b, d);
            CHECK((int)nar + (int)wid + (int)loc + (int)gen == 1);                          // (a)
            CHECK(for_tail_kernel(b, d) == (nar || wid || loc));
            CHECK(gen == P.general);                               // (b), (c): no kernel is launched for a general alignment of a fast job
            all_local &= loc;
            if (b.lds.narrow_off) CHECK(!nar);                                              // (f)
            if (b.lds.wide_on == 0) CHECK(!wid);
            if (P.rounds_possible) CHECK(rounds_takes(b, d.flags, d.w) && nar);             // (g)
            if (qlen == longest) {                                                        // (e): what size_arenas sized the set's arena for
                const bool known = std::find(known_e.begin(), known_e.end(), s) != known_e.end();
                const bool agree = takes_wide(b, d) == (P.set_wide[s] != 0) && takes_dir(b, d) == (P.set_dir[s] != 0);
                CHECK(agree != known);
            }
            d.flags = ALN_SKIP; CHECK(!for_general_kernel(b, d));
            g_routed++;
        }
    }
    CHECK(P.fast_local == all_local);                                                       // (d)
    CHECK(P.any_wide_set == any_wide);
}

// One case: the plan's documented answer, then the same job with one switch set (what: 'd' NODIR -> no direction words, the choice of kernels untouched;
// 'w' NOWIDE -> empty wide range; 'l' WIDE_LO=30 -> the range starts at 30, for jobs that have a wide loop; 'g' DEVICE_GENERAL -> the general kernel), then
// the switch reset: the first answer must come back.  Every case names at least one switch.
template <typename F>
static void run_case(const char *name, const abpoa_hip_scoring_t &sc, Sets &S, double node_factor, unsigned flags, bool force_general, const char *what, F expect,
                     const std::vector<int> &known_e = {}) {
    g_case = name;
    const DevicePlan B = plan_device_job(&sc, S.n(), S.get(), node_factor, flags, force_general); expect(B); CHECK((int)B.ps.size() == S.n());
    routing_checks(B, S, known_e);
    CHECK(*what != 0);
    for (const char *c = what; *c; ++c) {
        g_case = std::string(name) + " + switch " + *c;
        const char *sw = *c == 'd' ? "ABPOA_HIP_NODIR" : *c == 'w' ? "ABPOA_HIP_NOWIDE" : *c == 'l' ? "ABPOA_HIP_WIDE_LO" : "ABPOA_HIP_DEVICE_GENERAL";
        CHECK(set_option(sw, *c == 'l' ? "30" : "1") == 0);
        const DevicePlan P = plan_device_job(&sc, S.n(), S.get(), node_factor, flags, force_general);
        if (*c == 'd') CHECK(!P.dir && P.general == B.general && P.fast_local == B.fast_local && P.lin_fast == B.lin_fast);
        if (*c == 'w') CHECK(P.wide_hi < P.wide_lo && !P.any_wide_set && P.general == B.general && P.dir == B.dir);
        if (*c == 'l') CHECK(P.wide_lo == 30);
        if (*c == 'g') CHECK(P.general && !P.dir && !P.fast_local && !P.lin_fast && !P.rounds_possible);
        routing_checks(P, S, *c == 'g' ? std::vector<int>() : known_e);
        CHECK(set_option(sw, nullptr) == 0);
        g_case = std::string(name) + " after reset of switch " + *c;
        const DevicePlan Q = plan_device_job(&sc, S.n(), S.get(), node_factor, flags, force_general); expect(Q);
        routing_checks(Q, S, known_e);
    }
}

static void plan_cases() {
    const unsigned CONS = ABPOA_HIP_OUT_CONS;
    {   Sets S; S.uniform(8, 6, 1000); const abpoa_hip_scoring_t sc = scoring(ABPOA_HIP_AFFINE_GAP);
        int32_t inf; CHECK(abpoa_hip_score_bits(&sc, 3 * 1000 + 1026, 1000, &inf) == 16);
        run_case("1 kb affine", sc, S, 3.0, CONS, false, "dg", [](const DevicePlan &P) {
            CHECK(P.w_max == 20 && !P.general && P.dir && P.rounds_possible && !P.any_wide_set && !P.lin_fast && !P.fast_local && P.max_extra == 0);
            CHECK(P.wide_lo == 40 && P.wide_hi == 215 && P.CW == 4 && P.DB == 2 && !P.roomy && P.in_cap == POA_IN_CAP && P.out_cap == POA_OUT_CAP); });
        run_case("1 kb affine -s", sc, S, 3.0, CONS | ABPOA_HIP_AMB_STRAND, false, "g", [](const DevicePlan &P) { CHECK(!P.general && !P.dir && !P.rounds_possible && P.amb); });
        const abpoa_hip_scoring_t se = scoring(ABPOA_HIP_AFFINE_GAP, ABPOA_HIP_EXTEND_MODE);
        run_case("1 kb affine extend", se, S, 3.0, CONS, false, "g", [](const DevicePlan &P) { CHECK(!P.general && !P.dir && !P.rounds_possible); });
        run_case("1 kb affine forced general", sc, S, 3.0, CONS, true, "dwg", [](const DevicePlan &P) {
            CHECK(P.general && !P.dir && !P.fast_local && !P.lin_fast && !P.rounds_possible && P.wide_hi < P.wide_lo && !P.any_wide_set && P.max_extra == 0); });
        abpoa_hip_scoring_t su = sc; su.wb = -1;
        run_case("1 kb affine no band", su, S, 3.0, CONS, false, "dw", [](const DevicePlan &P) { CHECK(P.general && P.unbanded && !P.dir); });
    }
    {   Sets S; S.uniform(4, 4, 10000); const abpoa_hip_scoring_t sc = scoring(ABPOA_HIP_AFFINE_GAP);
        run_case("10 kb affine", sc, S, 3.0, CONS, false, "wlg", [](const DevicePlan &P) {
            CHECK(P.w_max == 110 && !P.general && P.wide_lo == 40 && P.wide_hi == 215 && P.wfr_cols == 448 && P.any_wide_set && !P.rounds_possible);
            for (const PoaSet &s : P.ps) CHECK(s.band_extra == 0); });
    }
    {   Sets S; S.uniform(2, 3, 26000); const abpoa_hip_scoring_t sc = scoring(ABPOA_HIP_CONVEX_GAP);
        run_case("26 kb convex", sc, S, 3.0, CONS, false, "w", [](const DevicePlan &P) {
            CHECK(P.w_max == 270 && !P.general && P.wfr_cols == 704 && P.wide_hi == 343 && P.any_wide_set && P.CW == 8 && P.DB == 4); });
    }
    {   Sets S; S.uniform(8, 6, 1000); abpoa_hip_scoring_t sc = scoring(ABPOA_HIP_LINEAR_GAP);
        run_case("linear e 2", sc, S, 3.0, CONS, false, "g", [](const DevicePlan &P) { CHECK(!P.general && P.lin_fast && !P.dir && P.rounds_possible && P.CW == 2); });
        sc.gap_ext1 = 0;
        run_case("linear e 0", sc, S, 3.0, CONS, false, "wg", [](const DevicePlan &P) { CHECK(P.general && !P.lin_fast && !P.rounds_possible); });
        sc.gap_ext1 = 2; Sets L; L.uniform(4, 4, 4000);
        run_case("linear 4 kb", sc, L, 3.0, CONS, false, "wg", [](const DevicePlan &P) { CHECK(P.w_max == 50 && P.general && !P.lin_fast); });
    }
    {   Sets S; S.uniform(1, 30, 500); const abpoa_hip_scoring_t sc = scoring(ABPOA_HIP_AFFINE_GAP, ABPOA_HIP_LOCAL_MODE, 27);
        run_case("local 500 aa", sc, S, 3.0, CONS, false, "g", [](const DevicePlan &P) {
            CHECK(P.local && P.sc.wb == -1 && !P.general && P.fast_local && P.wide_on == 0 && P.wide_hi < P.wide_lo && !P.dir && !P.rounds_possible && P.aln_cap == 26); });
        Sets L; L.uniform(1, 30, 700);
        run_case("local 700 aa", sc, L, 3.0, CONS, false, "dg", [](const DevicePlan &P) { CHECK(P.general && !P.fast_local); });
    }
    {   Sets S; S.uniform(3, 3, 1000); S.add({1000, 1000, 600}); S.add({1000, 900}); const abpoa_hip_scoring_t sc = scoring(ABPOA_HIP_AFFINE_GAP);
        run_case("ragged set", sc, S, 3.0, CONS, false, "d", [](const DevicePlan &P) {
            CHECK(!P.general && P.extra[0] == 0 && P.extra[1] == 0 && P.extra[2] == 0 && P.extra[3] == 400 && P.extra[4] == 0 && P.max_extra == 400 && !P.rounds_possible);
            CHECK(P.ps[3].band_extra == 400 && P.ps[4].band_extra == 0); }, {3});      // (set 3: the disagreement of "ragged set, routed past 40" below)
    }
    {   Sets S; S.uniform(2, 20, 1000); const abpoa_hip_scoring_t sc = scoring(ABPOA_HIP_AFFINE_GAP);
        run_case("last pass, 20 reads", sc, S, 4096.0, CONS, false, "dwg", [](const DevicePlan &P) { CHECK(P.roomy && P.in_cap == 21 && P.out_cap == 21 && !P.dir && !P.rounds_possible); });
        Sets T; T.uniform(2, 6, 1000);
        run_case("last pass, 6 reads", sc, T, 4096.0, CONS, false, "wg", [](const DevicePlan &P) { CHECK(P.roomy && P.in_cap == POA_IN_CAP && P.out_cap == POA_OUT_CAP); });
        Sets U; U.uniform(1, 400, 1000);
        run_case("last pass, 400 reads", sc, U, 4096.0, CONS, false, "wg", [](const DevicePlan &P) { CHECK(P.in_cap == 250 && P.out_cap == 250 && !P.dir); });
    }
}

// The edges of the routing rules (-b 10 -f 0.01: w = 10 + length / 100), each through run_case and so through routing_checks
static void routing_cases() {
    const unsigned CONS = ABPOA_HIP_OUT_CONS;
    const abpoa_hip_scoring_t aff = scoring(ABPOA_HIP_AFFINE_GAP), lin = scoring(ABPOA_HIP_LINEAR_GAP);
    {   Sets A; A.uniform(3, 4, 2900); Sets B; B.uniform(3, 4, 3000);      // the wide loop's first band half-width
        run_case("w 39", aff, A, 3.0, CONS, false, "dwg", [](const DevicePlan &P) { CHECK(P.w_max == 39 && !P.general && !P.any_wide_set && P.rounds_possible); });
        run_case("w 40", aff, B, 3.0, CONS, false, "dwlg", [](const DevicePlan &P) { CHECK(P.w_max == 40 && !P.general && P.any_wide_set && !P.rounds_possible); });
        run_case("linear w 39", lin, A, 3.0, CONS, false, "wg", [](const DevicePlan &P) { CHECK(P.w_max == 39 && !P.general && P.lin_fast && P.rounds_possible); });
        run_case("linear w 40", lin, B, 3.0, CONS, false, "wg", [](const DevicePlan &P) { CHECK(P.w_max == 40 && P.general && !P.lin_fast); });
    }
    {   Sets A; A.uniform(2, 3, 20500); Sets B; B.uniform(2, 3, 20600);      // the last one of the 448-column ring; the long-read form goes on to 343
        run_case("w 215", aff, A, 3.0, CONS, false, "wg", [](const DevicePlan &P) { CHECK(P.w_max == 215 && !P.general && P.any_wide_set && P.wide_hi == 343); });
        run_case("w 216", aff, B, 3.0, CONS, false, "wg", [](const DevicePlan &P) { CHECK(P.w_max == 216 && !P.general && P.any_wide_set && P.wide_hi == 343); });
        CHECK(set_option("ABPOA_HIP_NOXL", "1") == 0);
        run_case("w 215, no long-read form", aff, A, 3.0, CONS, false, "wg", [](const DevicePlan &P) { CHECK(!P.general && P.any_wide_set && P.wide_hi == 215 && P.wfr_cols == 448); });
        run_case("w 216, no long-read form", aff, B, 3.0, CONS, false, "wg", [](const DevicePlan &P) { CHECK(!P.general && !P.any_wide_set && P.wide_hi == 215); });
        CHECK(set_option("ABPOA_HIP_NOXL", nullptr) == 0);
    }
    {   const abpoa_hip_scoring_t loc = scoring(ABPOA_HIP_AFFINE_GAP, ABPOA_HIP_LOCAL_MODE, 27);      // the local loop's 576 columns
        Sets A; A.uniform(2, 5, 575); Sets B; B.uniform(2, 5, 576);
        run_case("local 575", loc, A, 3.0, CONS, false, "g", [](const DevicePlan &P) { CHECK(!P.general && P.fast_local); });
        run_case("local 576", loc, B, 3.0, CONS, false, "g", [](const DevicePlan &P) { CHECK(P.general && !P.fast_local); });
    }
    {   Sets S; S.uniform(2, 3, 1000); S.add({1000, 1000, 600});      // a ragged set: w = 20 of its long reads, 220 with half of its 400 extra columns
        // KNOWN DISAGREEMENT (LOG.md, the routing round): the plan takes the wide range from an estimate without the extra columns (120 columns: the 448-column
        // ring, band half-widths up to 215), the launch's final plan counts them (520 columns: the long-read ring, up to 343).  size_arenas sizes set 2 for the
        // narrow loop and direction words; on the device its alignments take the wide loop, which in dir_mode 1 writes score records.
        run_case("ragged set, routed past 40", aff, S, 3.0, CONS, false, "d", [](const DevicePlan &P) {
            CHECK(!P.general && P.extra[2] == 400 && P.route[2] == 400 && P.weff_hi == 220 && P.ps[2].band_extra == 400 && !P.set_wide[0] && !P.set_wide[1]);
            CHECK(P.wide_hi == 215 && !P.set_wide[2]); }, {2});
    }
    {   Sets S; S.add({3000, 2900}); S.add({3000, 2900, 2950});      // one set, both loops: its longest read takes the wide one, its shortest the narrow one
        run_case("wide and narrow reads in a set", aff, S, 3.0, CONS, false, "dwg", [](const DevicePlan &P) {
            CHECK(!P.general && P.max_extra == 0 && P.any_wide_set && P.set_wide[0] && P.set_wide[1] && !P.rounds_possible); });
    }
    CHECK(g_routed > 1000);
}

static void accessor_cases() {
    g_case = "accessors";
    CHECK(!opt_set("ABPOA_HIP_NO_SUCH_SWITCH") && !opt_on("ABPOA_HIP_NO_SUCH_SWITCH") && opt_int("ABPOA_HIP_NO_SUCH_SWITCH", 7) == 7);
    CHECK(set_option("ABPOA_HIP_NO_SUCH_SWITCH", "1") != 0);
    CHECK(set_option("ABPOA_HIP_VERBOSE", "0") == 0);
    CHECK(opt_set("ABPOA_HIP_VERBOSE") && !opt_on("ABPOA_HIP_VERBOSE") && opt_int("ABPOA_HIP_VERBOSE", 7) == 0);
    CHECK(set_option("ABPOA_HIP_VERBOSE", nullptr) == 0 && !opt_set("ABPOA_HIP_VERBOSE") && opt_int("ABPOA_HIP_VERBOSE", 7) == 7);
    CHECK(set_option("ABPOA_HIP_WIDE_LO", "30") == 0 && opt_on("ABPOA_HIP_WIDE_LO") && opt_int("ABPOA_HIP_WIDE_LO", 0) == 30 && set_option("ABPOA_HIP_WIDE_LO", nullptr) == 0);
    // another thread sets and resets a switch while this one reads it: every read sees one snapshot -- unset (the default) or "5"
    std::atomic<bool> stop{false};
    std::thread flip([&] { for (int i = 0; !stop.load(); ++i) set_option("ABPOA_HIP_RING_ROWS", (i & 1) ? nullptr : "5"); });
    int bad = 0;
    for (int i = 0; i < 100000; ++i) { const int v = opt_int("ABPOA_HIP_RING_ROWS", -1); (void)opt_on("ABPOA_HIP_RING_ROWS"); if (v != -1 && v != 5) bad++; }
    stop.store(true); flip.join();
    CHECK(bad == 0);
    CHECK(set_option("ABPOA_HIP_RING_ROWS", nullptr) == 0 && !opt_set("ABPOA_HIP_RING_ROWS"));
}

int main() {
    // (the harness owns every switch it tests: nothing inherited from the environment)
    for (const char *sw : {"ABPOA_HIP_NODIR", "ABPOA_HIP_NOWIDE", "ABPOA_HIP_WIDE_LO", "ABPOA_HIP_DEVICE_GENERAL", "ABPOA_HIP_NOFAST", "ABPOA_HIP_NOXL",
                           "ABPOA_HIP_RING_ROWS", "ABPOA_HIP_DIR_WIDE", "ABPOA_HIP_EXTRA_ROUTE_MIN", "ABPOA_HIP_ARENA_PCT", "ABPOA_HIP_VERBOSE"}) unsetenv(sw);
    plan_cases();
    routing_cases();
    accessor_cases();
    if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
    printf("device plan ok (%d descriptors routed)\n", g_routed);
    return 0;
}
